"""Every structurally different way of lt_scatter.hip to a hit, driven on purpose and shown to have run.

The triangle scatter reaches a hit through the in-workgroup round robin, through the slice queue of heavy workgroups
or the big-triangle queue (both k_sc_rest), through bins holding one ray, several (LT_GRID_MULTI) or none, through the
first or the second triangle of a lane (LT_SC_T2), under the single-scan or the batch caps.  Each case below builds an
input for one of them, compares all five images bit for bit with the brute-force oracle (and the LBVH strategy on the
same input), and asserts from the kernel's own counters -- candidate bins / triangle tests of a count=True render,
queue lengths from lt_debug_scatter_queues -- that the path was taken: a case whose condition does not hold is a wrong
input, not a pass.  The ray set's bin grid (k_rs_fit / k_rs_keys: nb_az, nb_el, dev_az, dev_el) is read back through
lt_debug_rayset_params and held against a float64 restatement.  Counters observed: profiles/scatter_paths/README.md."""
import ctypes as C
import functools
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from lidar_transfer_amd.laserscan import create_rays
from lidar_transfer_amd.synth import synth_scene

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_trace_gpu import _adversarial_soup, _assert_bits  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("tri", "range", "endpoints", "endcolors", "endrem")
ORIGINS = ((0.0, 0.0, 0.0), (0.37, -0.21, 0.13))
ORIGINS_B = ((0.0, 0.0, 0.0), (0.3, -0.2, 0.1))
BUDGET = 2.8e7  # triangles x rays per oracle call (the oracle does ~1e8 tests a second)


def _define(name):
    """A constant of lt_scatter.hip, from the source."""
    with open(os.path.join(ROOT, "lidar_transfer_amd", "csrc", "lt_scatter.hip")) as f:
        m = re.search(r"^#define %s\s+([0-9.e+-]+)f?\b" % name, f.read(), re.M)
    return float(m.group(1))


LT_SC_T = int(_define("LT_SC_T"))
LT_SC_BIG = int(_define("LT_SC_BIG"))
LT_SC_CAP_SINGLE = int(_define("LT_SC_CAP_SINGLE"))
LT_SC_CAP_BATCH = int(_define("LT_SC_CAP_BATCH"))
LT_BIN_SLACK = _define("LT_BIN_SLACK")
MAX_COLS, MAX_ROWS = 8192, 4096  # the bin grid's limits (lt_rayset_create_dev)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _attrs(rng, n_verts):
    return rng.integers(0, 256, (n_verts, 3)).astype(np.int32), rng.uniform(0, 1, n_verts).astype(np.float32)


def _soup_of(tri, rng):
    v = np.ascontiguousarray(tri.reshape(-1, 3).astype(np.float32))
    f = np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)
    return (v, f) + _attrs(rng, v.shape[0])


def _facing(centre, u, w, radius, rng):
    """triangles [n, 3, 3] around `centre` in the plane spanned by the unit vectors u, w; circumradius `radius`"""
    ang = rng.uniform(0, 2 * np.pi, centre.shape[0])[:, None] + np.arange(3)[None] * (2 * np.pi / 3)
    return centre[:, None] + radius[:, None, None] * (np.cos(ang)[..., None] * u[:, None] + np.sin(ang)[..., None] * w[:, None])


@functools.lru_cache(maxsize=None)
def _tiles(n, origin=ORIGINS[0]):
    """n small triangles, each centred on its own ray of a 4-row grid (seen from `origin`), 0.2 pixel pitches in radius,
    3-8 m away, faces dealt to rays by a seeded permutation; the last column repeats the first and stays unused.
    -> mesh, rays, H, ray_of [n]"""
    H, W = 4, -(-n // 4) + 1
    rays = create_rays(10.0, -10.0, H, W)
    rng = np.random.default_rng(1000 + n)
    usable = (np.arange(H)[:, None] * W + np.arange(W - 1)[None]).reshape(-1)
    ray_of = rng.permutation(usable)[:n]
    d = rays[ray_of].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = rng.uniform(3.0, 8.0, n)
    pitch = min(2 * np.pi / (W - 1), np.deg2rad(20.0) / (H - 1))
    u = np.cross(d, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    tri = _facing(np.asarray(origin, np.float32).astype(np.float64) + d * dist[:, None], u, np.cross(d, u), 0.2 * pitch * dist, rng)
    return _soup_of(tri, rng), rays, H, ray_of


@functools.lru_cache(maxsize=None)
def _lowpoly():
    """33 triangles tens of metres across: the ground (horizontal, pierced by the vertical axis: every azimuth, thousands
    of bins, all LT_SC_PARTS waves) and two octagonal rings of walls.  Every one of them is 'big'."""
    tris = [[(-60.0, -40.0, -1.7), (60.0, -40.0, -1.7), (0.0, 70.0, -1.7)]]
    for ring, (R, z0, z1) in enumerate([(20.0, -1.7, 12.0), (45.0, -1.7, 30.0)]):
        for k in range(8):
            a0, a1 = 2 * np.pi * (k + 0.3 * ring) / 8, 2 * np.pi * (k + 1 + 0.3 * ring) / 8
            p0, p1 = (R * np.cos(a0), R * np.sin(a0)), (R * np.cos(a1), R * np.sin(a1))
            tris.append([p0 + (z0,), p1 + (z0,), p1 + (z1,)])
            tris.append([p0 + (z0,), p1 + (z1,), p0 + (z1,)])
    H, W = 64, 1024
    return _soup_of(np.array(tris, np.float64), np.random.default_rng(2)), create_rays(10.0, -30.0, H, W), H


@functools.lru_cache(maxsize=None)
def _slice_scene():
    """900 medium triangles (three blocks: 448 + 448 + 4) 1.5-3 m from the sensor, each 0.11-0.14 rad across: between
    about 100 and 300 bins of a 32 x 1024 grid, none above LT_SC_BIG -- some 60 000 candidates per full block."""
    n, H, W, up, down = 900, 32, 1024, 3.0, -25.0
    rng = np.random.default_rng(7)
    az, el = rng.uniform(-np.pi, np.pi, n), np.deg2rad(rng.uniform(down + 3, up - 3, n))
    dist, half = rng.uniform(1.5, 3.0, n), rng.uniform(0.055, 0.07, n)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    u = np.stack([-np.sin(az), np.cos(az), np.zeros(n)], 1)
    tri = _facing(d * dist[:, None], u, np.cross(d, u), half * dist, rng)
    return _soup_of(tri, rng), create_rays(up, down, H, W), H


@functools.lru_cache(maxsize=None)
def _soup(seed, n):
    return _adversarial_soup(np.random.default_rng(seed), n)


@functools.lru_cache(maxsize=None)
def _shared_direction_grid():
    """case 5a: a sensor grid in which a third of the rays are scaled copies of other rays (the stress tool's draw)"""
    H, W = 16, 301
    rng = np.random.default_rng(51)
    rays = create_rays(15.0, -15.0, H, W)
    idx = rng.integers(0, rays.shape[0], size=rays.shape[0] // 3)
    rays[idx] = rays[rng.integers(0, rays.shape[0], size=idx.size)] * rng.uniform(0.5, 3.0, (idx.size, 1)).astype(np.float32)
    return _soup(52, 2500), rays, H


def _angles_to_rays(el, az):
    return np.stack([np.cos(el)[:, None] * np.cos(az)[None], np.cos(el)[:, None] * np.sin(az)[None],
                     np.sin(el)[:, None] * np.ones(az.size)[None]], -1).reshape(-1, 3).astype(np.float32)


def _seamless(H, W, up=15.0, down=-15.0):
    """W columns over [-pi, pi) with a random phase: no duplicated seam column"""
    az = -np.pi + 2 * np.pi * (np.arange(W) + np.random.default_rng(W).random()) / W
    return _angles_to_rays(np.deg2rad(np.linspace(up, down, H)), az)


def _two_blocks(H, W, up=2.0, down=-24.8):
    """two beam blocks with different spacing (HDL-64 style): rows are not equidistant"""
    el = np.deg2rad(np.concatenate([np.linspace(up, (up + down) / 2, H - H // 2, endpoint=False),
                                    np.linspace((up + down) / 2, down, H // 2)]))[:H]
    return _angles_to_rays(el, np.linspace(np.pi, -np.pi, W))


def _jittered(H, W):
    rays = create_rays(15.0, -15.0, H, W)
    return (rays + np.random.default_rng(71).normal(size=rays.shape).astype(np.float32) * 1e-3).astype(np.float32)


# name -> (H, W, layout, rays()).  layout: "inclusive" = first and last column coincide ([-pi, pi] inclusively, what
# create_rays makes), "seamless" = W distinct columns over [-pi, pi).
RAYSETS = {
    # case 6: beyond the bin grid's 4096 rows / 8192 columns, and the 13-bit column field at its limit
    "rows5000x3": (5000, 3, "inclusive", lambda: create_rays(15.0, -25.0, 5000, 3)),
    "rows4097x1": (4097, 1, "inclusive", lambda: create_rays(15.0, -25.0, 4097, 1)),
    "cols2x10000": (2, 10000, "inclusive", lambda: create_rays(2.0, -12.0, 2, 10000)),
    "cols1x8192": (1, 8192, "inclusive", lambda: create_rays(-3.0, -3.0, 1, 8192)),
    "cols1x8193": (1, 8193, "inclusive", lambda: create_rays(-3.0, -3.0, 1, 8193)),
    "cols1x8191": (1, 8191, "inclusive", lambda: create_rays(-3.0, -3.0, 1, 8191)),
    # case 7: azimuth and elevation layouts
    **{"seamless%d" % W: (16, W, "seamless", functools.partial(_seamless, 16, W)) for W in (4, 5, 301, 1024)},
    **{"inclusive%d" % W: (16, W, "inclusive", functools.partial(create_rays, 15.0, -15.0, 16, W)) for W in (4, 5, 301, 1024)},
    "two_blocks": (64, 256, "inclusive", functools.partial(_two_blocks, 64, 256)),
    "jittered": (16, 301, "inclusive", functools.partial(_jittered, 16, 301)),
    "fov89": (32, 256, "inclusive", functools.partial(create_rays, 89.0, -89.0, 32, 256)),
}
BEYOND = ("rows5000x3", "rows4097x1", "cols2x10000", "cols1x8193")  # more rays than bins along one axis
CASE6 = ("rows5000x3", "rows4097x1", "cols2x10000", "cols1x8192", "cols1x8193", "cols1x8191")
CASE7 = tuple(k for k in RAYSETS if k not in CASE6)


def _expected_nb_az(W, layout):
    """k_rs_fit / k_rs_keys: an inclusive grid of W >= 5 columns has W - 1 distinct azimuths and gets W - 1 columns --
    while W - 1 <= 8192: beyond the column field neither candidate (8192, 8191) fits the rays, and 8192 stays."""
    if layout == "inclusive" and 5 <= W <= MAX_COLS + 1:
        return W - 1
    return min(W, MAX_COLS)


EMPTY_MESH = (np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((3, 3), np.int32), np.zeros(3, np.float32))


# ---- device side ----------------------------------------------------------------------------------------------------
def _queues(sc):
    """(n_large, n_slices) of the scene's last count=True render"""
    lib = sc._lib
    lib.lt_debug_scatter_queues.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.lt_debug_scatter_queues.restype = C.c_int
    qs = (C.c_int * 2)()
    assert lib.lt_debug_scatter_queues(sc._h, qs) == 0
    return int(qs[0]), int(qs[1])


def _dev_mesh(mesh):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0)) for x in mesh]


def _np(out):
    return {k: (x.cpu().numpy() if hasattr(x, "cpu") else x) for k, x in out.items()}


def _cast(mesh, rays, origin, H, lbvh=True):
    """count=True scatter render + its queue lengths, and the LBVH strategy on the same input"""
    import torch
    from lidar_transfer_amd.raytracer import RaySet, Scene
    sc = Scene(0)
    t = _dev_mesh(mesh)
    sc.set_mesh(*t)
    trays = torch.from_numpy(np.ascontiguousarray(rays)).to(torch.device("cuda", 0))
    rs = RaySet(trays, H)
    a = _np(sc.render(rs, origin, count=True))
    q = _queues(sc)
    b = None
    if lbvh:
        sc.build()
        b = _np(sc.trace(trays, origin, H))
    torch.cuda.synchronize()
    rs.close()
    sc.close()
    return a, b, q


_REF = {}


def _reference(oracle, key, mesh, rays, origin, H):
    """the brute-force oracle's images, computed once per input and left unchanged"""
    if key not in _REF:
        ref = oracle.oracle_trace(rays, np.asarray(origin, np.float32), *mesh, H, mode=oracle.MODE_BRUTE, norm=oracle.NORM_SSE_TABLE)
        for k in KEYS:
            ref[k].setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _check(oracle, key, mesh, rays, origin, H):
    """both strategies against the oracle on all five outputs -> (scatter outputs, oracle images, (n_large, n_slices))"""
    assert mesh[1].shape[0] * (rays.shape[0] // H * H) <= 3e7
    a, b, q = _cast(mesh, rays, origin, H)
    ref = _reference(oracle, key, mesh, rays, origin, H)
    st = a["stats"]
    print("PATHS %s origin=%s: tris=%d rays=%d n_large=%d n_slices=%d nodes_visited=%d tris_tested=%d hits=%d" % (
        key, origin, mesh[1].shape[0], rays.shape[0], q[0], q[1], st["nodes_visited"], st["tris_tested"], st["n_hits"]))
    for k in KEYS:
        _assert_bits(a[k], ref[k], f"scatter {k} {key} origin={origin}")
        _assert_bits(b[k], ref[k], f"lbvh {k} {key} origin={origin}")
    assert st["n_hits"] == int((ref["tri"] >= 0).sum())
    return a, ref, q


# ---- case 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 447, 448, 449, 703, 704, 705, 895, 896, 897, 1344, 1345])
def test_every_slot_of_a_block_wins_its_own_ray(oracle, n, origin):
    """Block boundaries: n = the edges of a wave, of the lanes' first triangles, of LT_SC_T, and of the second-triangle
    lanes of the last block.  Every face is the winner of the ray it was built on, so a slot that is dropped, read
    twice or numbered wrongly changes the tri image."""
    mesh, rays, H, ray_of = _tiles(n, origin)
    a, ref, (n_large, n_slices) = _check(oracle, ("tiles", n, origin), mesh, rays, origin, H)
    assert np.array_equal(ref["tri"][ray_of], np.arange(n)), "the input is wrong: a face does not win its ray in the oracle"
    assert np.array_equal(a["tri"], ref["tri"])
    assert n_large == 0 and n_slices == 0
    assert a["stats"]["nodes_visited"] >= n  # every triangle has at least its own bin


# ---- case 2 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", ORIGINS)
def test_big_triangle_queue(oracle, origin):
    mesh, rays, H = _lowpoly()
    a, ref, (n_large, n_slices) = _check(oracle, ("lowpoly", origin), mesh, rays, origin, H)
    assert n_large >= 1 and n_slices == 0
    assert n_large == mesh[1].shape[0]  # every triangle of this scene covers more than LT_SC_BIG bins
    assert a["stats"]["nodes_visited"] > n_large * LT_SC_BIG
    assert int((ref["tri"] >= 0).sum()) > rays.shape[0] // 2
    assert int((ref["tri"] == 0).sum()) > 1024  # the pierced ground triangle is seen at every azimuth


# ---- case 3 ---------------------------------------------------------------------------------------------------------
def test_slice_queue_under_the_default_cap(oracle):
    mesh, rays, H = _slice_scene()
    a, ref, (n_large, n_slices) = _check(oracle, ("slices",), mesh, rays, ORIGINS[0], H)
    blocks = -(-mesh[1].shape[0] // LT_SC_T)
    assert n_large == 0 and n_slices > 0
    assert a["stats"]["nodes_visited"] > LT_SC_CAP_SINGLE * blocks  # work really was deferred
    assert int((ref["tri"] >= 0).sum()) > rays.shape[0] // 4


# ---- case 4 ---------------------------------------------------------------------------------------------------------
def _forced_cases():
    """name -> (mesh, rays, H, origin, has a block of more than one candidate)"""
    out = {}
    for n in (449, 897):
        mesh, rays, H, _ = _tiles(n)
        out["tiles%d" % n] = (mesh, rays, H, ORIGINS[0], True)
    mesh, rays, H = _lowpoly()
    out["lowpoly"] = (mesh, rays, H, ORIGINS[1], False)  # every triangle is big: its blocks have no candidates of their own
    mesh, rays, H = _slice_scene()
    out["slices"] = (mesh, rays, H, ORIGINS[0], True)
    out["soup"] = (_soup(41, 2500), create_rays(15.0, -15.0, 16, 301), 16, ORIGINS[1], True)
    return out


_CHILD = """
import ctypes as C, json, sys, numpy as np, torch
sys.path.insert(0, {root!r})
from lidar_transfer_amd.raytracer import RaySet, Scene
g = np.load({npz!r})
dev = torch.device("cuda", 0)
res = {{}}
for name in {names!r}:
    sc = Scene(0); t = [torch.from_numpy(g[name + "__" + k]).to(dev) for k in ("v", "f", "c", "r")]; sc.set_mesh(*t)
    H = int(g[name + "__H"]); origin = tuple(float(x) for x in g[name + "__origin"])
    rs = RaySet(torch.from_numpy(g[name + "__rays"]).to(dev), H)
    a = sc.render(rs, origin, count=True)
    qs = (C.c_int * 2)()
    sc._lib.lt_debug_scatter_queues.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    assert sc._lib.lt_debug_scatter_queues(sc._h, qs) == 0
    b = Scene.render_batch([sc], [rs], [origin])[0]
    torch.cuda.synchronize()
    for o in (a, b):
        for k in {keys!r}:
            assert np.array_equal(o[k].cpu().numpy().reshape(-1).view(np.int32), g[name + "__out_" + k].reshape(-1).view(np.int32)), (name, k)
    res[name] = [int(qs[0]), int(qs[1]), int(a["stats"]["nodes_visited"]), int(a["stats"]["tris_tested"])]
    rs.close(); sc.close()
print("FORCED_OK " + json.dumps(res))
"""


@pytest.mark.parametrize("setting", ["cap1_rest1", "cap64_rest3", "cap_huge"])
def test_slice_queue_forced_in_a_child_process(oracle, tmp_path, setting):
    """LIDARHIP_SC_CAP / LIDARHIP_SC_REST_BLOCKS (read once per process, hence the child) push every block through the
    slice queue, or nothing: the images are those of this process, which are the oracle's."""
    env_of = {"cap1_rest1": dict(LIDARHIP_SC_CAP="1", LIDARHIP_SC_REST_BLOCKS="1"),
              "cap64_rest3": dict(LIDARHIP_SC_CAP="64", LIDARHIP_SC_REST_BLOCKS="3"),
              "cap_huge": dict(LIDARHIP_SC_CAP="100000000")}[setting]
    assert "LIDARHIP_SC_CAP" not in os.environ and "LIDARHIP_SC_REST_BLOCKS" not in os.environ
    cases = _forced_cases()
    arrays, default = {}, {}
    for name, (mesh, rays, H, origin, _) in cases.items():
        a, b, q = _cast(mesh, rays, origin, H, lbvh=False)
        ref = _reference(oracle, ("forced", name), mesh, rays, origin, H)
        for k in KEYS:
            _assert_bits(a[k], ref[k], f"scatter {k} {name}")
            arrays[name + "__out_" + k] = a[k]
        default[name] = q
        for k, x in zip(("v", "f", "c", "r"), mesh):
            arrays[name + "__" + k] = x
        arrays[name + "__rays"], arrays[name + "__H"], arrays[name + "__origin"] = rays, np.int32(H), np.asarray(origin, np.float64)
    np.savez(tmp_path / "forced.npz", **arrays)
    code = _CHILD.format(root=ROOT, npz=str(tmp_path / "forced.npz"), names=list(cases), keys=KEYS)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env_of), timeout=300)
    assert res.returncode == 0 and "FORCED_OK" in res.stdout, res.stdout + res.stderr
    forced = json.loads(res.stdout.split("FORCED_OK ", 1)[1])
    print("PATHS forced %s: default (n_large, n_slices) %s; child [n_large, n_slices, nodes_visited, tris_tested] %s" % (setting, default, forced))
    for name, (_, _, _, _, has_block) in cases.items():
        assert forced[name][0] == default[name][0]  # the big queue does not depend on the cap
        if setting == "cap_huge":
            assert forced[name][1] == 0
        elif setting == "cap1_rest1":
            if has_block:
                assert forced[name][1] > default[name][1], name
            else:
                assert forced[name][1] == default[name][1] == 0, name
        else:
            assert forced[name][1] >= default[name][1], name


# ---- case 5 ---------------------------------------------------------------------------------------------------------
def test_bins_with_several_rays_on_a_sensor_grid(oracle):
    """A single-ray or empty bin contributes at most one triangle test per candidate: more tests than candidates can only
    come from LT_GRID_MULTI bins."""
    mesh, rays, H = _shared_direction_grid()
    for origin in ORIGINS_B:
        a, ref, q = _check(oracle, ("shared", origin), mesh, rays, origin, H)
        assert a["stats"]["tris_tested"] > a["stats"]["nodes_visited"]
        assert a["stats"]["n_hits"] > 0


def test_one_bin_holds_every_ray(oracle):
    H = W = 64
    d = np.array([0.6, -0.3, -0.2], np.float32)
    d /= np.linalg.norm(d)
    rays = np.tile(d, (H * W, 1)).astype(np.float32)
    rays[1::2] *= np.float32(2.5)  # an unnormalised copy
    rng = np.random.default_rng(53)
    v, f, c, r = _adversarial_soup(rng, 300)
    on_ray = _facing(d.astype(np.float64)[None] * rng.uniform(2.0, 40.0, 12)[:, None], np.tile([[0.4472136, 0.8944272, 0.0]], (12, 1)),
                     np.tile(np.cross(d.astype(np.float64), [0.4472136, 0.8944272, 0.0])[None], (12, 1)), rng.uniform(0.05, 3.0, 12), rng)
    v = np.concatenate([v, on_ray.reshape(-1, 3).astype(np.float32)])
    mesh = (v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)) + _attrs(rng, v.shape[0])
    for origin in ORIGINS_B:
        a, ref, q = _check(oracle, ("one_bin", origin), mesh, rays, origin, H)
        assert a["stats"]["tris_tested"] > a["stats"]["nodes_visited"]
        assert a["stats"]["tris_tested"] >= H * W  # a candidate of that bin tests every ray
    assert int((_REF[("one_bin", ORIGINS_B[0])]["tri"] >= 0).sum()) == H * W  # (the triangles on the ray, seen from where they were built)


def test_random_directions_leave_many_bins_empty(oracle):
    """H x W random directions in the upper hemisphere and one straight down: the rows below the horizon are empty bins
    (LT_GRID_EMPTY), and a soup lying mostly below the sensor visits them -- candidates that cost no triangle test.  (The
    rays above share their bins, so fewer tests than candidates means that empty bins were visited.)"""
    H, W = 8, 512
    rng = np.random.default_rng(54)
    rays = rng.normal(size=(H * W, 3)).astype(np.float32)
    rays[:, 2] = np.abs(rays[:, 2])
    rays[:6] = [[0, 0, 1], [0, 0, -1], [1, 0, 0.01], [-1, 0, 0.01], [0, 1, 0.01], [0, -1, 0.01]]
    v, f, c, r = _soup(55, 2500)
    mesh = ((v - np.array([0, 0, 3], np.float32)).astype(np.float32), f, c, r)
    for origin in ORIGINS_B:
        a, ref, q = _check(oracle, ("random_dirs", origin), mesh, rays, origin, H)
        assert a["stats"]["tris_tested"] < a["stats"]["nodes_visited"]
        assert a["stats"]["n_hits"] > 100


# ---- cases 6 and 7 --------------------------------------------------------------------------------------------------
def _soup_for(name):
    H, W = RAYSETS[name][:2]
    return _soup(60 + sorted(RAYSETS).index(name), int(min(2500, BUDGET // (H * W))))


@pytest.mark.parametrize("name", CASE6)
def test_shapes_beyond_the_bin_grid(oracle, name):
    """More rows than the grid's 4096, more columns than its 8192 (the 13-bit column field of S.pre), and the W - 1 fit
    at the limit.  Along the clamped axis every bin holds a ray and some hold two: more tests than candidates."""
    H, W, _, make = RAYSETS[name]
    rays, mesh = make(), _soup_for(name)
    for origin in ORIGINS_B:
        a, ref, q = _check(oracle, (name, origin), mesh, rays, origin, H)
        assert a["stats"]["n_hits"] > 0
        if name in BEYOND:
            assert a["stats"]["tris_tested"] > a["stats"]["nodes_visited"]


@pytest.mark.parametrize("name", CASE7)
def test_azimuth_and_elevation_layouts(oracle, name):
    """Seamless and inclusive azimuth grids on either side of the nb_az >= 5 / nb_az < 4 branches, rows that are not
    equidistant, a jittered grid, and elevations beyond +-45 degrees (the general path of f_atan_pair, rays next to the
    vertical axis)."""
    H, W, _, make = RAYSETS[name]
    rays, mesh = make(), _soup_for(name)
    for origin in ORIGINS_B:
        a, ref, q = _check(oracle, (name, origin), mesh, rays, origin, H)
        assert a["stats"]["n_hits"] > 0
        if RAYSETS[name][2] == "seamless":  # W distinct azimuths on W columns, H rows: exactly one ray in every bin
            assert a["stats"]["tris_tested"] == a["stats"]["nodes_visited"]
        elif name.startswith("inclusive"):  # the seam column's bins hold two rays, every other bin one
            assert a["stats"]["tris_tested"] > a["stats"]["nodes_visited"]


# ---- case 8 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [(1e3, -2e3, 5.0), (1e5, 1e5, 0.0)])
def test_far_origins(oracle, origin):
    """Scene and sensor moved far from the coordinate origin: vertex - origin cancels in float32, as in the reference."""
    v, f, c, r = synth_scene(5, 3000)
    v = (v + np.asarray(origin, np.float32)).astype(np.float32)
    H, W = 16, 256
    a, ref, q = _check(oracle, ("far", origin), (v, f, c, r), create_rays(3.0, -25.0, H, W), origin, H)
    assert a["stats"]["n_hits"] > 0


# ---- case 9 ---------------------------------------------------------------------------------------------------------
def test_no_state_survives_between_renders(oracle):
    """One scene renders a scene that fills the big queue, one that fills the slice queue, an empty mesh and a small mesh
    in a row: the cells and both queues must be back to empty each time."""
    import torch
    from lidar_transfer_amd.raytracer import RaySet, Scene
    dev = torch.device("cuda", 0)
    sc = Scene(0)
    keep = []

    def render(mesh, rays, H, origin, count):
        t = _dev_mesh(mesh)
        keep.append(t)
        sc.set_mesh(*t)
        rs = RaySet(torch.from_numpy(rays).to(dev), H)
        out = _np(sc.render(rs, origin, count=count))
        q = _queues(sc) if count else None
        rs.close()
        return out, q

    mesh, rays, H = _lowpoly()
    a, q = render(mesh, rays, H, ORIGINS[0], True)
    assert q[0] >= 1 and np.array_equal(a["tri"], _reference(oracle, ("lowpoly", ORIGINS[0]), mesh, rays, ORIGINS[0], H)["tri"])
    mesh, rays, H = _slice_scene()
    a, q = render(mesh, rays, H, ORIGINS[0], True)
    assert q[1] > 0 and np.array_equal(a["tri"], _reference(oracle, ("slices",), mesh, rays, ORIGINS[0], H)["tri"])
    empty = EMPTY_MESH
    a, q = render(empty, rays, H, ORIGINS[0], False)  # the slice scene's rays: their cells were just used
    assert (a["tri"] == -1).all()
    for k in ("range", "endpoints", "endcolors", "endrem"):
        assert not a[k].view(np.int32).any(), k
    mesh, rays, H, ray_of = _tiles(705)
    a, q = render(mesh, rays, H, ORIGINS[0], True)
    ref = _reference(oracle, ("tiles", 705, ORIGINS[0]), mesh, rays, ORIGINS[0], H)
    assert q == (0, 0)
    for k in KEYS:
        _assert_bits(a[k], ref[k], f"after the queues were used: {k}")
    assert a["stats"]["n_hits"] == int((ref["tri"] >= 0).sum())
    sc.close()


# ---- case 10 --------------------------------------------------------------------------------------------------------
def test_batch_groups_equal_their_single_renders():
    """Groups of 8 scans through lt_scene_render_batch_dev (LT_SC_CAP_BATCH, LT_SC_REST_BLOCKS_BATCH): tile meshes, the big
    queue, the slice queue (a block beyond the batch cap), multi-ray bins, an empty mesh first / in the middle / last, and
    a ray set without rays."""
    import torch
    from lidar_transfer_amd.raytracer import RaySet, Scene
    dev = torch.device("cuda", 0)
    empty = EMPTY_MESH

    def scan(name):
        if isinstance(name, int):
            mesh, rays, H, _ = _tiles(name)
        elif name == "lowpoly":
            mesh, rays, H = _lowpoly()
        elif name == "slices":
            mesh, rays, H = _slice_scene()
        elif name == "shared":
            mesh, rays, H = _shared_direction_grid()
        elif name == "empty":
            mesh, rays, H = empty, create_rays(3.0, -25.0, 16, 64), 16
        else:  # "no_rays"
            mesh, rays, H = _tiles(64)[0], np.zeros((0, 3), np.float32), 4
        return mesh, rays, H

    # a block of the slice scene exceeds the batch cap
    mesh, rays, H = _slice_scene()
    a, _, q = _cast(mesh, rays, ORIGINS[0], H, lbvh=False)
    assert a["stats"]["nodes_visited"] / -(-mesh[1].shape[0] // LT_SC_T) > LT_SC_CAP_BATCH
    groups = [["empty", 1, 449, "lowpoly", "slices", "shared", "no_rays", 705],
              [897, "lowpoly", "slices", "empty", "shared", 1345, 64, 257],
              ["slices", 448, "shared", "lowpoly", "no_rays", 896, 1344, "empty"]]
    for g, group in enumerate(groups):
        scenes, raysets, origins, singles, keep = [], [], [], [], []
        for i, name in enumerate(group):
            mesh, rays, H = scan(name)
            sc = Scene(0)
            t = _dev_mesh(mesh)
            keep.append(t)
            sc.set_mesh(*t)
            rs = RaySet(torch.from_numpy(rays).to(dev), H)
            origin = ORIGINS[(g + i) % 2] if name in ("lowpoly", "shared") else ORIGINS[0]
            singles.append({k: x.clone() for k, x in sc.render(rs, origin).items()})
            scenes.append(sc); raysets.append(rs); origins.append(origin)
        outs = Scene.render_batch(scenes, raysets, origins)
        torch.cuda.synchronize()
        for name, s, o in zip(group, singles, outs):
            for k in KEYS:
                assert o[k].shape == s[k].shape and torch.equal(o[k].view(torch.int32), s[k].view(torch.int32)), (g, name, k)
            if name == "empty":
                assert bool((o["tri"] == -1).all()) and not bool(o["range"].view(torch.int32).any())
            elif name != "no_rays":
                assert int((o["tri"] >= 0).sum()) > 0, (g, name)
        for rs, sc in zip(raysets, scenes):
            rs.close(); sc.close()


# ---- part B: the ray set's bin grid against a float64 restatement ---------------------------------------------------
def _rayset_params(rs):
    lib = rs._lib
    lib.lt_debug_rayset_params.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.lt_debug_rayset_params.restype = C.c_int
    nb, p = (C.c_int * 2)(), (C.c_float * 6)()
    assert lib.lt_debug_rayset_params(rs._h, nb, p) == 0
    return dict(nb_az=int(nb[0]), nb_el=int(nb[1]), az_scale=float(p[0]), az_off=float(p[1]), el_lo=float(p[2]),
                el_scale=float(p[3]), dev_az=float(p[4]), dev_el=float(p[5]))


def _rayset_params_f64(dirs, H, W):
    """k_rs_dirs' angles, k_rs_fit's choice of the azimuth grid and k_rs_keys' grid and deviations, in float64, from the
    product's normalised float32 directions"""
    d = dirs.astype(np.float64)
    phi, th = np.arctan2(d[:, 1], d[:, 0]), np.arctan2(d[:, 2], np.hypot(d[:, 0], d[:, 1]))

    def az_grid(K):
        scale = K / (2 * np.pi)
        x0 = (phi[0] + np.pi) * scale
        off = x0 - np.floor(x0 + 0.5)
        x = (phi + np.pi) * scale - off
        return scale, off, float(np.abs(x - np.floor(x + 0.5)).max())

    nb0 = min(max(W, 1), MAX_COLS)
    fit = [az_grid(nb0)[2], az_grid(nb0 - 1)[2] if nb0 - 1 >= 1 else 0.0]
    nb_az = nb0 - 1 if (nb0 >= 5 and fit[1] + 0.01 < fit[0]) else nb0
    az_scale, az_off, dev_az = az_grid(nb_az)
    nb_el = min(H, MAX_ROWS)
    lo, hi = float(th.min()), float(th.max())
    el_scale = (nb_el - 1) / (hi - lo) if (nb_el > 1 and hi > lo) else 0.0
    y = (th - lo) * el_scale
    dev_el = float(np.abs(y - np.clip(np.floor(y + 0.5), 0, nb_el - 1)).max())
    return dict(nb_az=nb_az, nb_el=nb_el, az_scale=az_scale, az_off=az_off, el_lo=lo, el_scale=el_scale, dev_az=dev_az,
                dev_el=dev_el, fit=fit)


def _sensor_raysets():
    from lidar_transfer_amd.config import load_sensor
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "config", "*.yaml"))):
        if os.path.basename(path).startswith("approach_"):
            continue
        s = load_sensor(path)
        out["config/" + os.path.basename(path)] = (s.H, s.W, "inclusive", s.create_rays)
    return out


SENSORS = ("config/hdl64_1024.yaml", "config/hdl64_2048.yaml", "config/os128_2048.yaml", "config/vlp32_1024.yaml")


@pytest.mark.parametrize("name", CASE6 + CASE7 + SENSORS)
def test_rayset_grid_and_deviations_against_float64(oracle, name):
    """dev_az / dev_el are what makes a triangle's candidate rectangle sound: measured too small, a triangle skips a
    column whose ray it hits.  They may differ from the float64 figure by the float rounding of a grid coordinate, which
    is what LT_BIN_SLACK budgets for -- not by more."""
    import torch
    from lidar_transfer_amd.raytracer import RaySet
    H, W, layout, make = (RAYSETS[name] if name in RAYSETS else _sensor_raysets()[name])
    rays = make()
    assert rays.shape[0] == H * W
    rs = RaySet(torch.from_numpy(rays).to(torch.device("cuda", 0)), H)
    got = _rayset_params(rs)
    rs.close()
    want = _rayset_params_f64(oracle.normalize_rays(rays, oracle.NORM_SSE_TABLE), H, W)
    print("RAYSET %s: %dx%d nb_az=%d nb_el=%d dev_az device %.6f float64 %.6f (diff %+.2e) dev_el device %.6f float64 %.6f (diff %+.2e) fit %s" % (
        name, H, W, got["nb_az"], got["nb_el"], got["dev_az"], want["dev_az"], got["dev_az"] - want["dev_az"],
        got["dev_el"], want["dev_el"], got["dev_el"] - want["dev_el"], ["%.4f" % x for x in want["fit"]]))
    assert got["nb_az"] == _expected_nb_az(W, layout) == want["nb_az"]
    assert got["nb_el"] == min(H, MAX_ROWS) == want["nb_el"]
    assert abs(got["dev_az"] - want["dev_az"]) <= LT_BIN_SLACK
    assert abs(got["dev_el"] - want["dev_el"]) <= LT_BIN_SLACK
    assert 0.0 <= got["dev_az"] <= 0.5 + LT_BIN_SLACK and 0.0 <= got["dev_el"] <= 0.5 + LT_BIN_SLACK
    assert abs(got["az_scale"] - want["az_scale"]) <= 1e-6 * want["az_scale"]
    assert abs(got["el_lo"] - want["el_lo"]) <= 1e-6
