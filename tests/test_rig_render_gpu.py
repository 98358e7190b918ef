"""lt_scene_render_rig_dev (Scene.render_rig) against what defines it: successive lt_scene_render_dev calls on the same
scene.  Every image of every sensor is a view into its own sentinel-filled buffer with guard elements in front and
behind (tests/writeback_cases.py), and the WHOLE buffers are compared as int32 bits: no tolerance anywhere.

A case asserts that every sensor that can has both hits and misses, so that the equality says something: a ray set of one
ray has one or the other, and an empty mesh has no hit; those are the only exceptions."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import writeback_cases as wc  # noqa: E402
from test_render_writeback_gpu import Padded  # noqa: E402

from lidar_transfer_amd.laserscan import create_rays  # noqa: E402
from lidar_transfer_amd.synth import synth_scene  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LT_SC_BIG = 512
LT_ERR_INVALID_ARG = -1


# ---- sensors ----------------------------------------------------------------------------------------------------------
SECTOR = (20.0, 120.0)
TABLE = np.array([6.0, 2.0, -3.0, -6.0, -9.0, -13.0, -18.0, -24.0])


def _posed(H, W):
    """a 16-row sensor yawed by 30 and pitched by 5 degrees: its rows are no rows of the world frame"""
    y, p = np.deg2rad(30.0), np.deg2rad(5.0)
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    return np.ascontiguousarray((create_rays(3.0, -25.0, H, W).astype(np.float64) @ (Rz @ Ry).T).astype(np.float32))


# name -> (rays, H, grid)
@functools.lru_cache(maxsize=None)
def _sensor(name):
    from lidar_transfer_amd.raytracer import sector_grid
    return {
        "one": lambda: (create_rays(-12.0, -12.0, 1, 1), 1, None),
        "small": lambda: (create_rays(10.0, -10.0, 3, 65), 3, None),
        "mid": lambda: (create_rays(10.0, -30.0, 16, 64), 16, None),
        "sector": lambda: (create_rays(5.0, -25.0, 16, 96, sector=SECTOR), 16, sector_grid(96, SECTOR)),
        "table": lambda: (create_rays(0.0, 0.0, 8, 128, beam_table=TABLE), 8, None),
        "posed": lambda: (_posed(16, 128), 16, None),
        # the growth case: more rays than any of the above
        "wide": lambda: (create_rays(12.0, -28.0, 32, 256), 32, None),
    }[name]()


ORIGINS = ((0.0, 0.0, 0.0), (0.37, -0.21, 0.13), (1.2, 0.1, -0.4), (-0.8, 0.6, 0.3), (0.05, -1.1, 0.2), (0.6, 0.6, -0.2),
           (-0.3, -0.4, 0.45), (0.9, -0.7, 0.0))
# the rigs of K = 1, 2, 3, 8 sensors; the same ray set twice in K = 2 and K = 8, every origin distinct
RIGS = {1: ("mid",), 2: ("mid", "mid"), 3: ("sector", "table", "posed"),
        8: ("one", "small", "mid", "sector", "table", "posed", "small", "mid")}
BIG_RIG = ("mid", "sector", "table", "posed")   # more than LT_SC_BIG bins each: a near-field triangle can be big for all


# ---- meshes -----------------------------------------------------------------------------------------------------------
def _frozen(mesh):
    for a in mesh:
        a.setflags(write=False)
    return mesh


@functools.lru_cache(maxsize=None)
def _street(n=None):
    """synth_scene with a few thousand faces; n: that many of its faces, dealt by a seeded permutation"""
    v, f, c, r = synth_scene(3, 3000)
    if n is not None:
        f = np.ascontiguousarray(f[np.random.default_rng(n).permutation(f.shape[0])[:n]])
    return _frozen((v, f, c, r))


@functools.lru_cache(maxsize=None)
def _ground():
    """ONE horizontal triangle under every sensor, 16 m and more to its edges: every azimuth of every row that looks down by
    more than some 7 degrees hits it, no ray that looks up does -- and it covers more than LT_SC_BIG bins of every sensor
    that has that many"""
    v = np.array([[-30.0, -20.0, -1.7], [30.0, -20.0, -1.7], [0.0, 35.0, -1.7]], np.float32)
    rng = np.random.default_rng(5)
    return _frozen((v, np.array([[0, 1, 2]], np.int32), rng.integers(0, 256, (3, 3)).astype(np.int32),
                    rng.uniform(0, 1, 3).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def _near_field():
    """the street with the ground triangle in front of its faces, and a second one a metre higher behind them"""
    v, f, c, r = _street()
    gv, gf, gc, gr = _ground()
    n = v.shape[0]
    hi = gv + np.array([0, 0, 1.0], np.float32)
    return _frozen((np.ascontiguousarray(np.concatenate([v, gv, hi])),
                    np.ascontiguousarray(np.concatenate([gf + n, f, gf + n + 3])),
                    np.ascontiguousarray(np.concatenate([c, gc, gc])), np.ascontiguousarray(np.concatenate([r, gr, gr]))))


@functools.lru_cache(maxsize=None)
def _bad_index():
    v, f, c, r = _street()
    f = f.copy()
    f[700, 1] = v.shape[0] + 5   # in the second block of LT_SC_T faces
    return _frozen((v, f, c, r))


def _mesh(n):
    if n == 0:
        return wc.empty_mesh()
    return _ground() if n == 1 else _street(n)


# ---- device side ------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(x):
    import torch
    return torch.from_numpy(np.array(x)).to(_dev())


_RAYSETS = {}


def _rayset(name):
    """one RaySet per sensor for the whole module: a ray set is read-only and shared"""
    from lidar_transfer_amd.raytracer import RaySet
    if name not in _RAYSETS:
        rays, H, grid = _sensor(name)
        _RAYSETS[name] = RaySet(_up(rays), H, grid=grid)
        assert _RAYSETS[name].n_rays == rays.shape[0]
    return _RAYSETS[name]


def _queues(sc):
    lib = sc._lib
    lib.lt_debug_scatter_queues.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.lt_debug_scatter_queues.restype = C.c_int
    qs = (C.c_int * 2)()
    assert lib.lt_debug_scatter_queues(sc._h, qs) == 0
    return int(qs[0]), int(qs[1])


class Fixture:
    """a scene with a mesh, and the padded buffers of a rig of sensors: one set per sensor and kind of colour image"""

    def __init__(self, mesh, names, origins=None, scene=None):
        from lidar_transfer_amd.raytracer import Scene
        self.sc = scene if scene is not None else Scene(0)
        self.own = scene is None
        self.set_mesh(mesh)
        self.set_rig(names, origins)

    def set_mesh(self, mesh):
        self.mesh = mesh
        self.mesh_t = [_up(x) for x in mesh]
        self.sc.set_mesh(*self.mesh_t)

    def set_rig(self, names, origins=None):
        self.names = tuple(names)
        self.origins = tuple(origins) if origins is not None else ORIGINS[:len(self.names)]
        assert len(set(self.origins)) == len(self.origins)
        self.rs = [_rayset(n) for n in self.names]
        self.pads = [{lab: Padded(r.n_rays, lab) for lab in (False, True)} for r in self.rs]

    def singles(self, write_misses, label_image, ptrs, stream=None):
        """successive renders, sensor by sensor -> the whole buffers of every sensor"""
        for i, r in enumerate(self.rs):
            out = self.pads[i][label_image].arm(ptrs[i])
            self.sc.render(r, self.origins[i], out=out, write_misses=write_misses, label_image=label_image, stream=stream)
        return [p[label_image].read() for p in self.pads]

    def rig(self, write_misses, label_image, ptrs, stream=None):
        outs = [self.pads[i][label_image].arm(ptrs[i]) for i in range(len(self.rs))]
        self.sc.render_rig(self.rs, self.origins, outs=outs, write_misses=write_misses, label_image=label_image, stream=stream)
        return [p[label_image].read() for p in self.pads]

    def hits(self):
        """per sensor: the tri image of its own single render"""
        return [self.sc.render(r, self.origins[i])["tri"].cpu().numpy() for i, r in enumerate(self.rs)]

    def assert_hits_and_misses(self):
        for name, tri in zip(self.names, self.hits()):
            if tri.size > 1 and self.mesh[1].shape[0] > 0:
                assert (tri >= 0).any() and (tri < 0).any(), f"sensor {name}: {int((tri >= 0).sum())} hits of {tri.size} rays"

    def compare(self, write_misses=True, label_image=False, ptrs=None, stream=None, what=""):
        ptrs = ptrs if ptrs is not None else [wc.KEYS] * len(self.rs)
        want = self.singles(write_misses, label_image, ptrs, stream)
        got = self.rig(write_misses, label_image, ptrs, stream)
        diff = []
        for i, name in enumerate(self.names):
            # (the sentinel must still stand wherever a single render leaves it: the two share the armed buffers' layout)
            for k in wc.KEYS:
                g, w = got[i][k], want[i][k]
                if not np.array_equal(g, w):
                    bad = np.flatnonzero(g != w)
                    diff.append(f"{what} sensor {i} ({name}) {k} write_misses={write_misses} label_image={label_image} "
                                f"ptrs={','.join(ptrs[i]) or 'none'}: {bad.size} elements differ, first at {bad[0]}: "
                                f"got {g[bad[0]]:#x} expected {w[bad[0]]:#x}")
        assert not diff, "\n".join(diff)

    def close(self):
        if self.own:
            self.sc.close()


# ---- 1: K = 1, 2, 3, 8 on a street scene ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", sorted(RIGS))
def test_rig_equals_successive_renders(K):
    """ray sets of different shapes in one rig (one ray, 3 x 65, 16 x 64, a 120 degree sector on its own grid, a beam table, a
    posed set), distinct origins, the same ray set twice; with and without the misses and the label image"""
    fx = Fixture(_street(), RIGS[K])
    try:
        fx.assert_hits_and_misses()
        for write_misses, label_image in wc.FLAGS:
            fx.compare(write_misses, label_image, what=f"K={K}")
        fx.sc.status()
    finally:
        fx.close()


# ---- 2: the block edges of LT_SC_T ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 447, 448, 449, 897])
def test_block_edges(n):
    fx = Fixture(_mesh(n), RIGS[8])
    try:
        assert fx.mesh[1].shape[0] == n
        fx.assert_hits_and_misses()
        for write_misses, label_image in ((True, False), (False, True)):
            fx.compare(write_misses, label_image, what=f"{n} faces")
        fx.sc.status()
    finally:
        fx.close()


# ---- 3: big triangles, a bad index ------------------------------------------------------------------------------------------
def test_near_field_triangle_is_big_for_every_sensor():
    """the big-triangle queue of every sensor's own slot: a sensor's own LT_TRACE_COUNT render says that it is used"""
    fx = Fixture(_near_field(), BIG_RIG)
    try:
        fx.assert_hits_and_misses()
        for i, r in enumerate(fx.rs):
            fx.sc.render(r, fx.origins[i], count=True)
            n_large, _ = _queues(fx.sc)
            assert n_large >= 1, (fx.names[i], n_large)
        for write_misses, label_image in wc.FLAGS:
            fx.compare(write_misses, label_image, what="near field")
        fx.sc.status()
    finally:
        fx.close()


def test_bad_index_is_reported_as_by_the_single_path():
    from lidar_transfer_amd import _lib
    fx = Fixture(_bad_index(), RIGS[3])
    try:
        fx.assert_hits_and_misses()
        with pytest.raises(RuntimeError) as single:
            fx.sc.status()
        want = fx.singles(True, False, [wc.KEYS] * 3)
        with pytest.raises(RuntimeError):
            fx.sc.status()
        got = fx.rig(True, False, [wc.KEYS] * 3)
        with pytest.raises(RuntimeError) as rig:
            fx.sc.status()
        assert str(rig.value) == str(single.value)
        for g, w in zip(got, want):
            for k in wc.KEYS:
                assert np.array_equal(g[k], w[k]), k
        # the healthy mesh on the same scene: the report is gone, as after a single render
        fx.set_mesh(_street())
        fx.compare(what="after the bad index")
        fx.sc.status()
    finally:
        fx.close()


# ---- 4: the slice queue, forced in a child process ---------------------------------------------------------------------------
_CHILD = """
import ctypes as C, json, sys, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_rig_render_gpu as t
fx = t.Fixture(t._street(), t.RIGS[8])
fx.assert_hits_and_misses()
slices = []
for i, r in enumerate(fx.rs):
    fx.sc.render(r, fx.origins[i], count=True)
    slices.append(t._queues(fx.sc)[1])
for write_misses, label_image in t.wc.FLAGS:
    fx.compare(write_misses, label_image, what="forced slices")
got = fx.rig(True, False, [t.wc.KEYS] * 8)
np.savez({npz!r}, **{{"%d_%s" % (i, k): g[k] for i, g in enumerate(got) for k in t.wc.KEYS}})
fx.sc.status()
print("FORCED_OK " + json.dumps(slices))
"""


def test_slice_queue_forced_in_a_child_process(tmp_path):
    """LIDARHIP_SC_CAP=1 (read once per process, hence the child): every block with two candidates or more goes through
    the slice queue of its sensor's slot.  The child compares rig and successive renders under that cap, and its rig images
    are those of this process under the default cap."""
    assert "LIDARHIP_SC_CAP" not in os.environ and "LIDARHIP_SC_REST_BLOCKS" not in os.environ
    fx = Fixture(_street(), RIGS[8])
    try:
        here = fx.rig(True, False, [wc.KEYS] * 8)
    finally:
        fx.close()
    npz = str(tmp_path / "child.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), npz=npz)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, LIDARHIP_SC_CAP="1", LIDARHIP_SC_REST_BLOCKS="3"))
    assert res.returncode == 0 and "FORCED_OK" in res.stdout, res.stdout + res.stderr
    slices = json.loads(res.stdout.split("FORCED_OK ", 1)[1])
    for name, n in zip(RIGS[8], slices):
        assert name == "one" or n > 0, (name, slices)
    child = np.load(npz)
    for i, g in enumerate(here):
        for k in wc.KEYS:
            assert np.array_equal(child["%d_%s" % (i, k)], g[k]), (i, k)


# ---- 5: NULL images ---------------------------------------------------------------------------------------------------------
def test_every_subset_of_null_images():
    """every sensor of a rig of three with every subset of the five pointers, the three of a call always different ones;
    then whole arrays NULL: no sensor wants that image"""
    fx = Fixture(_street(), RIGS[3])
    try:
        fx.assert_hits_and_misses()
        n = len(wc.SUBSETS)
        for s in range(n):
            ptrs = [wc.SUBSETS[(s + 4 * i) % n] for i in range(3)]
            for write_misses, label_image in ((True, False), (False, True)):
                fx.compare(write_misses, label_image, ptrs=ptrs, what=f"subsets {s}")
        for keys in wc.SUBSETS:
            fx.compare(True, False, ptrs=[keys] * 3, what="whole arrays NULL")
        fx.compare(what="after the render that wrote nothing")
        fx.sc.status()
    finally:
        fx.close()


# ---- 6: state ---------------------------------------------------------------------------------------------------------------
def test_rig_single_rig_on_one_scene():
    """cells and queues are armed again after every call, whichever wrote them: rig, single renders of other sensors on
    another mesh, rig"""
    fx = Fixture(_near_field(), RIGS[8])
    try:
        fx.compare(what="first rig")
        fx.set_mesh(_street(449))
        for name, origin in (("wide", ORIGINS[3]), ("small", ORIGINS[0])):
            fx.sc.render(_rayset(name), origin, write_misses=False)
        fx.compare(False, True, what="second rig")
        fx.set_mesh(_near_field())
        fx.compare(what="third rig")
        fx.sc.status()
    finally:
        fx.close()


def test_rig_after_mesh_and_ray_counts_have_grown():
    """a scene whose slots were sized for a small mesh and small sensors, then a larger mesh and larger sensors in the same
    slots: the images are those of a fresh scene"""
    grown = Fixture(_street(447), ("small", "one", "small"))
    fresh = None
    try:
        grown.compare(what="small")
        grown.set_mesh(_near_field())
        grown.set_rig(("mid", "wide", "posed", "wide"))
        grown.assert_hits_and_misses()
        grown.compare(what="grown")
        got = grown.rig(True, False, [wc.KEYS] * 4)
        fresh = Fixture(_near_field(), ("mid", "wide", "posed", "wide"))
        want = fresh.rig(True, False, [wc.KEYS] * 4)
        for g, w in zip(got, want):
            for k in wc.KEYS:
                assert np.array_equal(g[k], w[k]), k
        grown.sc.status()
    finally:
        grown.close()
        if fresh is not None:
            fresh.close()


def test_side_stream():
    import torch
    fx = Fixture(_street(), RIGS[3])
    try:
        side = torch.cuda.Stream(_dev())
        torch.cuda.synchronize()
        with torch.cuda.stream(side):   # (the buffers are armed on the stream the renders run on)
            fx.compare(stream=side, what="side stream")
            fx.compare(False, True, stream=side, what="side stream")
        fx.compare(what="default stream after it")
        fx.sc.status()
    finally:
        fx.close()


# ---- 7: what is refused -----------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    """n_sensors > 8 and < 0, a NULL ray set, LT_TRACE_COUNT, and a ray set on another device.  The last needs a second GPU: on
    a machine with one it is NOT exercised, and that branch of lt_scene_render_rig_dev stays unverified there."""
    import torch
    from lidar_transfer_amd import _lib
    from lidar_transfer_amd.raytracer import RaySet
    fx = Fixture(_street(), RIGS[2])
    try:
        lib, vp = fx.sc._lib, C.c_void_p
        rs = _rayset("mid")
        org = (C.c_float * 27)()

        def call(n, handles, flags=0):
            arr = (vp * max(len(handles), 1))(*handles)
            return lib.lt_scene_render_rig_dev(fx.sc._h, n, arr, org, None, None, None, None, None, flags, None)

        assert call(9, [rs._h] * 9) == LT_ERR_INVALID_ARG and b"n_sensors=9" in lib.lt_last_error()
        assert call(-1, [rs._h]) == LT_ERR_INVALID_ARG and b"n_sensors=-1" in lib.lt_last_error()
        assert call(3, [rs._h, None, rs._h]) == LT_ERR_INVALID_ARG and b"sensor 1: NULL rayset" in lib.lt_last_error()
        assert call(2, [rs._h] * 2, _lib.LT_TRACE_COUNT) == LT_ERR_INVALID_ARG and b"LT_TRACE_COUNT" in lib.lt_last_error()
        assert call(0, []) == 0
        with pytest.raises(RuntimeError):
            fx.sc.render_rig([rs] * 9, [ORIGINS[0]] * 9, outs=[{}] * 9)
        with pytest.raises(ValueError):
            fx.sc.render_rig([rs] * 2, [ORIGINS[0]])
        if torch.cuda.device_count() > 1:   # another device: only where there is one
            other = RaySet(torch.from_numpy(np.array(_sensor("small")[0])).to(torch.device("cuda", 1)), 3)
            try:
                assert call(2, [rs._h, other._h]) == LT_ERR_INVALID_ARG and b"rayset on device 1" in lib.lt_last_error()
            finally:
                other.close()
        # nothing was started and nothing is left behind
        fx.compare(what="after the refusals")
        fx.sc.status()
    finally:
        fx.close()
