"""Phase B of the triangle scatter (sc_round_robin in lt_scatter.hip) at the shapes where its block loop can go wrong.

A lane takes its candidates in blocks of U = LT_SC_PB rounds: U searches in lockstep, U grid loads back to back, U
triangle tests, and only then the block's atomicMins (the hits wait in registers).  What can go wrong is keyed on the
block: a last block with 1 .. U live sub-rounds, a sub-round that only some waves or some lanes have, several deferred
hits of one lane on the same cell, a slice that starts and ends inside a block, and single-ray, multi-ray and empty bins
inside one block.

Every input is a LATTICE mesh on a 32 x 257 sensor grid (32 x 256 bins, one ray per bin): a "single" is a small triangle
around one ray (one candidate bin, hit by that ray), a "quad" a triangle around 2 x 2 ray centres (four candidate bins).
With at most LT_SC_T faces the mesh is one workgroup, the candidates of face f follow those of face f - 1, and the
kernel's own counters say whether the shape was built: K = candidate bins (nodes_visited of a count=True render) must
equal singles + 4 quads exactly, the queues (lt_debug_scatter_queues) must be what the case names -- a case whose
condition does not hold is a wrong input, not a pass.  All five images are compared bit for bit with the brute-force
oracle through test_scatter_paths_gpu._check.  Counters observed: profiles/sc_phaseb/README.md."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from lidar_transfer_amd.laserscan import create_rays

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_scatter_paths_gpu import (KEYS, LT_SC_CAP_SINGLE, LT_SC_T, ORIGINS, ROOT, _assert_bits, _attrs, _cast, _check,  # noqa: E402
                                    _define, _reference, _slice_scene)

pytestmark = pytest.mark.gpu
U = int(_define("LT_SC_PB"))
SLICE = int(_define("LT_SC_SLICE"))
NT = 256  # lanes of a workgroup = candidates of a round
H, W = 32, 257
UP, DOWN = 10.0, -10.0
LAST_PLATE = (8, 100, 16, 17)  # rows 8 .. 23, columns 100 .. 116: a triangle of more than 256 bins (K beyond the cap)


# ---- the lattice ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid():
    """rays of the sensor grid and the azimuth / elevation of every bin centre [H, W - 1] (the last column repeats the first)"""
    rays = create_rays(UP, DOWN, H, W)
    d = rays.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    az = np.arctan2(d[:, 1], d[:, 0]).reshape(H, W)
    el = np.arcsin(d[:, 2]).reshape(H, W)
    return rays, az, el


def _point(az, el, dist):
    return dist * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])


def _plate(r0, c0, nr, nc, dist):
    """a triangle whose angular bounding box holds the ray centres of rows r0 .. r0 + nr - 1, columns c0 .. c0 + nc - 1 and
    ends 0.2 pitches beyond them: the apex above the middle, so a 1 x 1 plate is hit by its ray"""
    _, az, el = _grid()
    pa, pe = abs(az[0, 2] - az[0, 1]), abs(el[1, 1] - el[0, 1])
    a = np.sort(az[r0, c0:c0 + nc])
    e = np.sort(el[r0:r0 + nr, c0])
    a_lo, a_hi, e_lo, e_hi = a[0] - 0.2 * pa, a[-1] + 0.2 * pa, e[0] - 0.2 * pe, e[-1] + 0.2 * pe
    return np.stack([_point(a_lo, e_lo, dist), _point(a_hi, e_lo, dist), _point(0.5 * (a_lo + a_hi), e_hi, dist)])


class _Sites:
    """2 x 2 blocks of bins in a seeded order (none touching the seam columns, none inside LAST_PLATE): a block hosts one
    quad or up to four singles"""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        r0, c0, nr, nc = LAST_PLATE
        blocks = [(r, c) for r in range(0, H, 2) for c in range(2, W - 3, 2)
                  if not (r0 - 2 < r < r0 + nr and c0 - 2 < c < c0 + nc)]
        self.blocks = [blocks[i] for i in rng.permutation(len(blocks))]
        self.cells = []
        self.rng = rng

    def quad(self):
        return self.blocks.pop()

    def cell(self):
        if not self.cells:
            r, c = self.blocks.pop()
            self.cells = [(r, c), (r, c + 1), (r + 1, c), (r + 1, c + 1)]
        return self.cells.pop()

    def dist(self):
        return float(self.rng.uniform(3.0, 8.0))


class _Mesh:
    """faces in order; cand[f] = first candidate of face f while every plate has exactly its nr x nc bins"""

    def __init__(self, seed):
        self.sites = _Sites(seed)
        self.tris, self.cells, self.k = [], [], 0

    def add(self, r0, c0, nr=1, nc=1, dist=None):
        self.tris.append(_plate(r0, c0, nr, nc, self.sites.dist() if dist is None else dist))
        self.cells.append((r0, c0, nr, nc))
        self.k += nr * nc
        return len(self.tris) - 1

    def fill_to(self, k):
        """quads, then singles, until the next face's first candidate is k"""
        gap = k - self.k
        assert gap >= 0
        for _ in range(gap // 4):
            self.add(*self.sites.quad(), 2, 2)
        for _ in range(gap % 4):
            self.add(*self.sites.cell())

    def mesh(self):
        assert 0 < len(self.tris) <= LT_SC_T, len(self.tris)  # one workgroup
        v = np.ascontiguousarray(np.array(self.tris).reshape(-1, 3).astype(np.float32))
        f = np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)
        return (v, f) + _attrs(np.random.default_rng(len(self.tris)), v.shape[0])


@functools.lru_cache(maxsize=None)
def _lattice(k, last_plate_bins=0):
    """one workgroup with k candidates; last_plate_bins > 0: the last face is LAST_PLATE, taken to have that many bins"""
    m = _Mesh(5000 + k)
    if last_plate_bins:
        m.fill_to(k - last_plate_bins)
        m.add(*LAST_PLATE, dist=9.0)
        m.k = k
    else:
        m.fill_to(k)
    return m.mesh()


# ---- rounds per workgroup -------------------------------------------------------------------------------------------
def _round_counts():
    """K for ceil(K / 256) = 1, 2, U, U + 1, 2U, 2U + 1 with K mod 256 = 1, 63 .. 65, 255, 0"""
    ks = set()
    for r in sorted({1, 2, U, U + 1, 2 * U, 2 * U + 1}):
        for m in (1, 63, 64, 65, 255, 256):
            ks.add((r - 1) * NT + m)
    return sorted(ks)


@pytest.mark.parametrize("k", _round_counts())
def test_rounds_of_one_workgroup(oracle, k):
    """K kept candidates = ceil(K / 256) rounds: a last block of 1 .. U live sub-rounds, a last sub-round that one wave
    has partly (K mod 256 = 1, 63, 65, 255), that whole waves have not (64), or that is full (0)."""
    rays = _grid()[0]
    plate = 0
    if k > LT_SC_CAP_SINGLE:
        # beyond the cap a workgroup keeps everything only if its LAST triangle crosses the cap: a plate of > 256 bins
        # whose exact count the kernel's bounds decide -- measured once, then the filler is cut to fit
        r0, c0, nr, nc = LAST_PLATE
        plate = nr * nc
        assert k <= LT_SC_CAP_SINGLE - 1 + plate, "LT_SC_PB too deep for a single workgroup under the single-scan cap"
        a, _, q = _cast(_lattice(k, plate), rays, ORIGINS[0], H, lbvh=False)
        plate += int(a["stats"]["nodes_visited"]) - k
    mesh = _lattice(k, plate)
    a, ref, (n_large, n_slices) = _check(oracle, ("phaseb_rounds", k), mesh, rays, ORIGINS[0], H)
    st = a["stats"]
    print("PHASEB rounds K=%d: faces=%d rounds=%d last=%d candidates=%d tests=%d hits=%d" % (
        k, mesh[1].shape[0], -(-k // NT), k % NT, st["nodes_visited"], st["tris_tested"], st["n_hits"]))
    assert n_large == 0 and n_slices == 0
    assert st["nodes_visited"] == k, "the input is wrong: not the K it names"
    assert st["tris_tested"] >= k  # one ray per bin away from the seam column
    assert st["n_hits"] > 0


def test_workgroup_without_candidates(oracle):
    """K = 0: every triangle lies above the field of view"""
    rng = np.random.default_rng(3)
    tri = np.array([[[x, y, 30.0], [x + 0.1, y, 30.0], [x, y + 0.1, 30.0]] for x, y in rng.uniform(1.0, 2.0, (70, 2))])
    v = np.ascontiguousarray(tri.reshape(-1, 3).astype(np.float32))
    mesh = (v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)) + _attrs(rng, v.shape[0])
    a, ref, q = _check(oracle, ("phaseb_k0",), mesh, _grid()[0], ORIGINS[0], H)
    assert q == (0, 0) and a["stats"]["nodes_visited"] == 0 and a["stats"]["n_hits"] == 0


# ---- many hits per lane and cell ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stacks(order):
    """Three rays with a stack of 2U + 1 parallel singles each.  Stack s sits on lane L_s: its tiles are the candidates
    L_s + 256 r for r = 0 .. 2U - 1 -- ONE lane, all U sub-rounds of its first two blocks, U deferred hits on one cell in
    each -- and L_s + 1 (the neighbouring lane, same wave, same round as the first).  order = +1: the faces come near to
    far, -1: far to near.  -> mesh, cells of the stacks, {cell: nearest face}"""
    m = _Mesh(77 + order)
    lanes = (5, 70, 201)  # three different waves
    cells = [m.sites.cell() for _ in lanes]
    want = []
    for s, lane in enumerate(lanes):
        want += [(lane + NT * r, s) for r in range(2 * U)] + [(lane + 1, s)]
    want.sort()
    depth = {s: 0 for s in range(len(lanes))}
    faces = {s: [] for s in range(len(lanes))}
    for k, s in want:
        m.fill_to(k)
        i = depth[s] if order > 0 else 2 * U - depth[s]
        faces[s].append((3.0 + 0.5 * i, m.add(*cells[s], dist=3.0 + 0.5 * i)))
        depth[s] += 1
    nearest = {cells[s]: min(faces[s])[1] for s in faces}
    return m.mesh(), m.k, nearest


@pytest.mark.parametrize("order", [1, -1], ids=["near_to_far", "far_to_near"])
def test_stacks_of_hits_on_one_cell(oracle, order):
    """The nearest tile of a stack wins whichever lane, sub-round and block holds it: the U hits one lane keeps back in a
    block go to the same cell, and the next block's go there after them."""
    mesh, k, nearest = _stacks(order)
    rays = _grid()[0]
    a, ref, q = _check(oracle, ("phaseb_stacks", order), mesh, rays, ORIGINS[0], H)
    assert q == (0, 0) and k <= LT_SC_CAP_SINGLE
    assert a["stats"]["nodes_visited"] == k, "the input is wrong: a face is not where its lane and round were meant"
    for (r, c), face in nearest.items():
        assert ref["tri"][r * W + c] == face, "the input is wrong: the oracle's winner is not the nearest tile"
        assert a["tri"][r * W + c] == face


# ---- single-ray, multi-ray and empty bins inside one block ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed():
    """Some rays are replaced by scaled copies of others: the copied ray's bin holds two rays (LT_GRID_MULTI), the replaced
    ray's bin none.  Lanes 9, 100 and 190 meet a single-ray, a multi-ray and an empty bin in the U sub-rounds of one block
    (a different order each); more pairs lie under the filler.  -> mesh, rays, K, expected triangle tests"""
    m = _Mesh(91)
    rays = _grid()[0].copy()
    per_bin = np.ones((H, W - 1), np.int64)
    per_bin[:, 0] = 2  # the seam column holds the first and the last ray of a row

    def pair():
        (rm, cm), (re, ce) = m.sites.cell(), m.sites.cell()
        rays[re * W + ce] = rays[rm * W + cm] * np.float32(1.75)
        per_bin[rm, cm] += 1
        per_bin[re, ce] -= 1
        return (rm, cm), (re, ce)

    kinds = ["single", "multi", "empty"]
    want = []
    for i, lane in enumerate((9, 100, 190)):
        multi, empty = pair()
        cell_of = dict(single=m.sites.cell(), multi=multi, empty=empty)
        for u in range(max(U, 2)):
            want.append((lane + NT * u, cell_of[kinds[(i + u) % 3]]))
    for i in range(24):  # under the filler: quads over blocks with a multi-ray bin, and over every third emptied one
        r, c = m.sites.quad()
        r2, c2 = m.sites.quad()
        rays[r2 * W + c2] = rays[r * W + c] * np.float32(0.6)
        per_bin[r, c] += 1
        per_bin[r2, c2] -= 1
        want.append((None, (r, c, 2, 2)))
        if i % 3 == 0:
            want.append((None, (r2, c2, 2, 2)))
    placed = sorted([w for w in want if w[0] is not None])
    loose = [w[1] for w in want if w[0] is None]
    for k, cell in placed:
        while loose and m.k + 4 <= k:
            m.add(*loose.pop())
        m.fill_to(k)
        m.add(*cell)
    for plate in loose:
        m.add(*plate)
    tests = sum(int(per_bin[r0:r0 + nr, c0:c0 + nc].sum()) for r0, c0, nr, nc in m.cells)
    return m.mesh(), rays, m.k, tests


def test_single_multi_and_empty_bins_in_one_block(oracle):
    mesh, rays, k, tests = _mixed()
    a, ref, q = _check(oracle, ("phaseb_mixed",), mesh, rays, ORIGINS[0], H)
    st = a["stats"]
    print("PHASEB mixed: K=%d candidates=%d tests=%d (expected %d) hits=%d" % (k, st["nodes_visited"], st["tris_tested"], tests, st["n_hits"]))
    assert q == (0, 0)
    assert st["nodes_visited"] == k, "the input is wrong: a face is not where its lane and round were meant"
    assert st["tris_tested"] == tests  # 0 for an empty bin, 1 for a single ray, 2 for the copied ray's bin
    assert tests > k  # (more multi-ray than empty bins are visited: the sum cannot come out right by visiting neither)


# ---- slices and wide addressing: child processes --------------------------------------------------------------------
_CHILD = """
import ctypes as C, json, sys, numpy as np, torch
sys.path.insert(0, {root!r})
from lidar_transfer_amd.raytracer import RaySet, Scene
g = np.load({npz!r})
dev = torch.device("cuda", 0)
names = {names!r}
res, scenes, raysets, origins, keep = {{}}, [], [], [], []
for name in names:
    sc = Scene(0); t = [torch.from_numpy(g[name + "__" + k]).to(dev) for k in ("v", "f", "c", "r")]; sc.set_mesh(*t)
    Hn = int(g[name + "__H"]); origin = tuple(float(x) for x in g[name + "__origin"])
    rs = RaySet(torch.from_numpy(g[name + "__rays"]).to(dev), Hn)
    a = sc.render(rs, origin, count=True)
    qs = (C.c_int * 2)()
    sc._lib.lt_debug_scatter_queues.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    assert sc._lib.lt_debug_scatter_queues(sc._h, qs) == 0
    torch.cuda.synchronize()
    for k in {keys!r}:
        assert np.array_equal(a[k].cpu().numpy().reshape(-1).view(np.int32), g[name + "__out_" + k].reshape(-1).view(np.int32)), ("single", name, k)
    res[name] = [int(qs[0]), int(qs[1]), int(a["stats"]["nodes_visited"]), int(a["stats"]["tris_tested"])]
    scenes.append(sc); raysets.append(rs); origins.append(origin); keep.append(t)
outs = Scene.render_batch(scenes, raysets, origins)
torch.cuda.synchronize()
for name, o in zip(names, outs):
    for k in {keys!r}:
        assert np.array_equal(o[k].cpu().numpy().reshape(-1).view(np.int32), g[name + "__out_" + k].reshape(-1).view(np.int32)), ("batch", name, k)
for rs, sc in zip(raysets, scenes):
    rs.close(); sc.close()
print("PHASEB_OK " + json.dumps(res))
"""


def _in_child(oracle, tmp_path, cases, env):
    """Render every case alone (count=True) and all of them as one batch in a child process under `env`; the images must be
    this process's, which are the oracle's.  -> {name: [n_large, n_slices, candidates, tests]} of the child"""
    for name in env:
        assert name not in os.environ
    arrays = {}
    for name, (mesh, rays, Hn, origin) in cases.items():
        a, _, _ = _cast(mesh, rays, origin, Hn, lbvh=False)
        ref = _reference(oracle, ("phaseb_child", name), mesh, rays, origin, Hn)
        for k in KEYS:
            _assert_bits(a[k], ref[k], f"scatter {k} {name}")
            arrays[name + "__out_" + k] = a[k]
        for k, x in zip(("v", "f", "c", "r"), mesh):
            arrays[name + "__" + k] = x
        arrays[name + "__rays"], arrays[name + "__H"], arrays[name + "__origin"] = rays, np.int32(Hn), np.asarray(origin, np.float64)
    np.savez(tmp_path / "phaseb.npz", **arrays)
    code = _CHILD.format(root=ROOT, npz=str(tmp_path / "phaseb.npz"), names=list(cases), keys=KEYS)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)
    assert res.returncode == 0 and "PHASEB_OK" in res.stdout, res.stdout + res.stderr
    out = json.loads(res.stdout.split("PHASEB_OK ", 1)[1])
    print("PHASEB child %s: [n_large, n_slices, candidates, tests] %s" % (env, out))
    return out


def test_slices_start_and_end_inside_a_block(oracle, tmp_path):
    """LIDARHIP_SC_CAP = 300 (read once per process: a child): a lattice workgroup keeps the faces that start below
    candidate 300 -- quads: it ends at 300 .. 303, inside the second round of its first block -- and queues the rest in
    slices of LT_SC_SLICE from there: every slice starts and ends off the multiples of 256 and of 256 U, the last one ends
    with the workgroup.  A single-scan render of each input and a batch of the two (and the slice scene of the existing
    file, many workgroups)."""
    cap = 300
    k_a, k_b = 5 * NT + 37, 2 * NT + 130
    cases = {"lattice_a": (_lattice(k_a), _grid()[0], H, ORIGINS[0]), "lattice_b": (_lattice(k_b), _grid()[0], H, ORIGINS[0])}
    mesh, rays, Hs = _slice_scene()
    cases["slices"] = (mesh, rays, Hs, ORIGINS[0])
    got = _in_child(oracle, tmp_path, cases, dict(LIDARHIP_SC_CAP=str(cap)))
    for name, k in (("lattice_a", k_a), ("lattice_b", k_b)):
        n_large, n_slices, cand, tests = got[name]
        # kept = the end of the face holding candidate `cap` - 1 or crossing it: the lattice starts with quads
        kept = min(x for x in range(cap, cap + 4) if x % 4 == 0)
        assert kept % NT != 0 and (kept + SLICE) % (NT * U) != 0 and (k - kept) % SLICE != 0
        assert n_large == 0 and n_slices == -(-(k - kept) // SLICE), name
        assert cand == k, name  # k_sc_tris and k_sc_rest together visit every candidate once
    assert got["slices"][1] > 0


def test_wide_addressing(oracle, tmp_path):
    """the 64-bit addressing variants (LIDARHIP_FORCE_WIDE, read once per process) on a full last block, a last block of
    one sub-round and the mixed bins"""
    k_full, k_one = 2 * U * NT - 3, U * NT + 65
    mesh, rays, k_mixed, tests = _mixed()
    cases = {"full": (_lattice(k_full), _grid()[0], H, ORIGINS[0]), "one": (_lattice(k_one), _grid()[0], H, ORIGINS[0]),
             "mixed": (mesh, rays, H, ORIGINS[0])}
    got = _in_child(oracle, tmp_path, cases, dict(LIDARHIP_FORCE_WIDE="1"))
    assert got["full"][:3] == [0, 0, k_full] and got["one"][:3] == [0, 0, k_one]
    assert got["mixed"] == [0, 0, k_mixed, tests]
