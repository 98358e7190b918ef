"""The write-back of a render held to its contract in every variant: k_sc_resolve (lt_scatter.hip; single scans and
lt_scene_render_batch_dev), trace_writeback (lt_trace.hip) and lt_ctrace on the inputs of tests/writeback_cases.py.

Every output is a view at its own 16-byte phase into a larger buffer filled with a sentinel, and the WHOLE buffer is
compared, as int32 bits, with what writeback_cases.expected makes of the brute-force oracle's images: hits, misses
(written with write_misses, the caller's bytes without), the rays beyond W * H, the bytes in front of and behind the
view, and the buffers whose pointer was not passed.  The one exception to the bits: a cell whose expected remission is
NaN is held to isnan.  What was observed, and which single edits of the kernels these tests catch:
profiles/render_writeback/README.md."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import writeback_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu
STRATEGIES = ("scatter", "lbvh")


# ---- references: computed once per input, left unchanged --------------------------------------------------------------
_CASES = {}


def _case(oracle, kind, shape, offset=0):
    """kind "tiles" / "edges" / "wall" / "empty" at shape (H, W, extra) -> dict(mesh, rays [H * W + extra, 3], H, n, ref, hit)"""
    key = (kind, shape, offset)
    if key not in _CASES:
        H, W, extra = shape
        if kind in ("tiles", "edges"):
            mesh, rays, _ = wc.tiles(H, W, wc.seed_of(shape) + offset, kind == "edges")
        elif kind == "wall":
            mesh, rays = wc.wall(H, W)
        else:
            mesh, rays = wc.empty_mesh(), wc.tiles(H, W, wc.seed_of(shape))[1]
        rays = wc.with_extra(rays, extra)
        ref = wc.reference(oracle, mesh, rays, H, H * W)
        hit = ref["tri"] >= 0
        hit.setflags(write=False)
        _CASES[key] = dict(mesh=mesh, rays=rays, H=H, n=H * W, extra=extra, ref=ref, hit=hit, name=f"{kind} {H}x{W}+{extra}")
    return _CASES[key]


# ---- device side ------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(x):
    import torch
    return torch.from_numpy(np.array(x)).to(_dev())   # (a copy: the cases' arrays are read-only)


class Padded:
    """the five sentinel-filled device buffers of one scan and the views into them that a variant passes"""

    def __init__(self, R, label_image):
        import torch
        self.R, self.label_image = R, label_image
        self.layout = wc.layout(R, label_image)
        self.buf = {k: torch.empty(total, dtype=torch.int32, device=_dev()) for k, (_, _, _, total) in self.layout.items()}

    def arm(self, ptrs):
        import torch
        out = {}
        for k, (lead, count, shape, _) in self.layout.items():
            self.buf[k].fill_(wc.SENTINEL)
            if k in ptrs:
                v = self.buf[k][lead:lead + count]
                out[k] = (v if k in ("endcolors", "tri") else v.view(torch.float32)).view(shape)
                assert out[k].is_contiguous() and (count == 0 or out[k].data_ptr() == self.buf[k].data_ptr() + 4 * lead)
        return out

    def read(self):
        import torch
        torch.cuda.synchronize()
        return {k: b.cpu().numpy() for k, b in self.buf.items()}


class Rig:
    """one scene with the case's mesh (LBVH built), its ray set and its rays on the device"""

    def __init__(self, case, grid=None):
        from lidar_transfer_amd.raytracer import RaySet, Scene
        self.case = case
        self.sc = Scene(0)
        self.mesh_t = [_up(x) for x in case["mesh"]]
        self.sc.set_mesh(*self.mesh_t)
        self.rays_t = _up(case["rays"])
        self.rs = RaySet(self.rays_t, case["H"], grid=grid)
        assert self.rs.n_rays == case["n"]
        self.sc.build()
        self.pads = {}

    def pad(self, label_image):
        if label_image not in self.pads:
            self.pads[label_image] = Padded(self.case["n"] + self.case["extra"], label_image)
        return self.pads[label_image]

    def cast(self, strategy, variant, count=False):
        """-> (the five whole buffers after the cast, stats or None)"""
        pad = self.pad(variant.label_image)
        out = pad.arm(variant.ptrs)
        kw = dict(out=out, write_misses=variant.write_misses, label_image=variant.label_image, count=count)
        if strategy == "scatter":
            res = self.sc.render(self.rs, wc.ORIGIN, **kw)
        else:
            res = self.sc.trace(self.rays_t, wc.ORIGIN, self.case["H"], **kw)
        return pad.read(), res.get("stats")

    def check(self, strategy, variant, count=False):
        got, stats = self.cast(strategy, variant, count)
        want = wc.expected(self.case["ref"], self.case["hit"], variant)
        what = f"{self.case['name']} {strategy}{' count' if count else ''} write_misses={variant.write_misses} " \
               f"label_image={variant.label_image} ptrs={','.join(variant.ptrs) or 'none'}"
        diff = wc.differences(got, want, what)
        assert not diff, "\n".join(diff)
        self.sc.status()
        return stats

    def queues(self):
        lib = self.sc._lib
        lib.lt_debug_scatter_queues.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        lib.lt_debug_scatter_queues.restype = C.c_int
        qs = (C.c_int * 2)()
        assert lib.lt_debug_scatter_queues(self.sc._h, qs) == 0
        return int(qs[0]), int(qs[1])

    def close(self):
        self.rs.close()
        self.sc.close()


def _paths_line(rig, stats):
    c = rig.case
    q = rig.queues()
    print("PATHS %s: tris=%d rays=%d(+%d) resolve_blocks=%d n_large=%d n_slices=%d nodes_visited=%d tris_tested=%d hits=%d" % (
        c["name"], c["mesh"][1].shape[0], c["n"], c["extra"], -(-c["n"] // 256), q[0], q[1], stats["nodes_visited"],
        stats["tris_tested"], stats["n_hits"]))
    return q


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", wc.SHAPES)
def test_flags_at_every_shape(oracle, shape):
    """write_misses x label_image with all five pointers, both strategies, and both instantiations of k_sc_resolve: the
    counting one also has to count the oracle's hits, partial last wave included"""
    case = _case(oracle, "tiles", shape)
    rig = Rig(case)
    try:
        n_hits = int(case["hit"].sum())
        for write_misses, label_image in wc.FLAGS:
            variant = wc.Variant(write_misses, label_image, wc.KEYS, case["extra"])
            for strategy in STRATEGIES:
                rig.check(strategy, variant)
                stats = rig.check(strategy, variant, count=True)
                assert stats["n_hits"] == n_hits, (strategy, variant, stats["n_hits"], n_hits)
                assert stats["n_rays"] == case["n"]
                if strategy == "scatter" and write_misses and not label_image:
                    assert _paths_line(rig, stats) == (0, 0)
    finally:
        rig.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", wc.SUBSET_SHAPES)
def test_pointer_subsets(oracle, shape):
    """Any of the five pointers may be NULL (include/lidarhip.h): what is passed is written as if all were, what is not
    keeps every byte.  After the render with no pointer at all the cells must be armed again: a render of ANOTHER mesh on
    the same scene (same face count) equals its own oracle."""
    case, other = _case(oracle, "tiles", shape), _case(oracle, "tiles", shape, offset=100)
    rig = Rig(case)
    try:
        for ptrs in wc.SUBSETS:
            for write_misses, label_image in wc.FLAGS:
                for strategy in STRATEGIES:
                    rig.check(strategy, wc.Variant(write_misses, label_image, ptrs, 0))
        none = wc.Variant(True, False, (), 0)
        full = wc.Variant(True, False, wc.KEYS, 0)
        for count in (False, True):
            stats = rig.check("scatter", none, count=count)   # nothing written ...
            assert not count or stats["n_hits"] == int(case["hit"].sum())
            rig.case = other
            other_t = [_up(x) for x in other["mesh"]]
            rig.sc.set_mesh(*other_t)
            rig.check("scatter", full)                         # ... and nothing left behind
            rig.case = case
            rig.sc.set_mesh(*rig.mesh_t)
            rig.check("scatter", full)
    finally:
        rig.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", wc.SUBSET_SHAPES)
@pytest.mark.parametrize("kind", ["wall", "empty"])
def test_all_hits_and_all_misses(oracle, kind, shape):
    """One triangle that every ray hits -- on the sector's own bin grid it covers more than LT_SC_BIG bins at 7 x 73 and
    goes through the big-triangle queue of k_sc_rest -- and the empty mesh (no k_sc_tris launch at all), which, hits only,
    leaves every byte of every buffer untouched."""
    from lidar_transfer_amd.raytracer import sector_grid
    case = _case(oracle, kind, shape)
    H, W, _ = shape
    assert case["hit"].all() if kind == "wall" else not case["hit"].any()
    rig = Rig(case, grid=sector_grid(W, wc.WALL_SECTOR) if kind == "wall" else None)
    try:
        for write_misses, label_image in wc.FLAGS:
            variant = wc.Variant(write_misses, label_image, wc.KEYS, 0)
            if kind == "empty" and not write_misses:
                want = wc.expected(case["ref"], case["hit"], variant)
                assert all((b == wc.SENTINEL).all() for b in want.values())
            for strategy in STRATEGIES:
                rig.check(strategy, variant)
            stats = rig.check("scatter", variant, count=True)
            assert stats["n_hits"] == int(case["hit"].sum())
            if write_misses and not label_image:
                n_large, n_slices = _paths_line(rig, stats)
                # 168 degrees of a grid of 4 W columns x H rows: 137 x 7 bins at 7 x 73, above LT_SC_BIG = 512; 1 x 65 has
                # 260 bins in all and cannot get there
                assert (n_large, n_slices) == ((1, 0) if (kind == "wall" and H == 7) else (0, 0))
    finally:
        rig.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def test_value_edges(oracle):
    """Remissions whose mean is a denormal, -0, an overflow, +inf or NaN, and the colours at the ends of the int32 range:
    the device's division, conversions and order of the sum against the oracle's."""
    case = _case(oracle, "edges", wc.EDGE_SHAPE)
    assert int(np.isnan(case["ref"]["endrem"]).sum()) >= 1
    rig = Rig(case)
    try:
        for write_misses, label_image in wc.FLAGS:
            for strategy in STRATEGIES:
                rig.check(strategy, wc.Variant(write_misses, label_image, wc.KEYS, 0))
    finally:
        rig.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", range(len(wc.BATCH_GROUPS)))
def test_batch_groups(oracle, g):
    """lt_scene_render_batch_dev on the padded views: every scan of a group with its own pointer subset, ray counts that put
    a scan's first resolve workgroup behind a full and behind a ragged last workgroup of its neighbour, a ray set without
    rays and an empty mesh inside the groups of 8.  Every scan's buffers equal those of its own single-scan variant."""
    import torch
    from lidar_transfer_amd.raytracer import RaySet, Scene
    group = wc.BATCH_GROUPS[g]
    scans = []
    try:
        for i, s in enumerate(group):
            if s == "no_rays":
                case = dict(_case(oracle, "tiles", (1, 65, 0)), rays=np.zeros((0, 3), np.float32), H=wc.NO_RAYS_H, n=0, extra=0,
                            name="no rays")
                case["ref"] = {k: x[:0] for k, x in case["ref"].items() if k in wc.KEYS}
                case["hit"] = np.zeros(0, bool)
            else:
                case = _case(oracle, "empty", wc.EMPTY_SHAPE) if s == "empty" else _case(oracle, "tiles", s)
            sc = Scene(0)
            mesh_t = [_up(x) for x in case["mesh"]]
            sc.set_mesh(*mesh_t)
            rs = RaySet(_up(case["rays"]), case["H"])
            assert rs.n_rays == case["n"]
            R = case["n"] + case["extra"]
            scans.append(dict(case=case, sc=sc, rs=rs, mesh_t=mesh_t, ptrs=wc.batch_subset(g, i),
                              pads={lab: Padded(R, lab) for lab in (False, True)}))
        for write_misses, label_image in wc.FLAGS:
            outs = [s["pads"][label_image].arm(s["ptrs"]) for s in scans]
            Scene.render_batch([s["sc"] for s in scans], [s["rs"] for s in scans], [wc.ORIGIN] * len(scans), outs=outs,
                               write_misses=write_misses, label_image=label_image)
            torch.cuda.synchronize()
            diff = []
            for i, s in enumerate(scans):
                variant = wc.Variant(write_misses, label_image, s["ptrs"], s["case"]["extra"])
                want = wc.expected(s["case"]["ref"], s["case"]["hit"], variant)
                diff += wc.differences(s["pads"][label_image].read(), want,
                                       f"group {g} scan {i} ({s['case']['name']}) write_misses={write_misses} "
                                       f"label_image={label_image} ptrs={','.join(s['ptrs']) or 'none'}")
                s["sc"].status()
            assert not diff, "\n".join(diff)
    finally:
        for s in scans:
            s["rs"].close()
            s["sc"].close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_ctrace_keeps_the_callers_bytes_where_nothing_was_hit(oracle, monkeypatch, strategy):
    """lt_ctrace always renders hits only (RayTracer.cpp:73): on host arrays that hold the sentinel, hits equal the oracle
    and every other byte -- misses, and the guards around the five flat arrays -- is the caller's.  LIDARHIP_STRATEGY is
    read on every call."""
    from lidar_transfer_amd.raytracer import C_Trace
    if strategy == "lbvh":
        monkeypatch.setenv("LIDARHIP_STRATEGY", "lbvh")
    else:
        monkeypatch.delenv("LIDARHIP_STRATEGY", raising=False)
    # (the smaller mesh first: a cell left behind by a broken resolve would then name a face that the next mesh has too)
    for shape in wc.SUBSET_SHAPES:
        case = _case(oracle, "tiles", shape)
        H, W, _ = shape
        v, f, c, r = (np.array(x).reshape(-1) for x in case["mesh"])
        variant = wc.Variant(False, False, wc.KEYS, 0)
        want = wc.expected(case["ref"], case["hit"], variant)
        for with_tri in (True, False):
            bufs = wc.buffers(case["n"], False)
            views = {}
            for k, (lead, count, _, _) in wc.layout(case["n"], False).items():
                views[k] = bufs[k][lead:lead + count] if k in ("endcolors", "tri") else bufs[k][lead:lead + count].view(np.float32)
            C_Trace(np.array(case["rays"]).reshape(-1), np.asarray(wc.ORIGIN, np.float32), v, f, c, r, views["endpoints"],
                    views["endcolors"], views["range"], views["endrem"], H, W, tri_image=views["tri"] if with_tri else None)
            if not with_tri:
                want = dict(want, tri=np.full_like(want["tri"], wc.SENTINEL))
            diff = wc.differences(bufs, want, f"lt_ctrace {strategy} {case['name']} tri={with_tri}")
            assert not diff, "\n".join(diff)
