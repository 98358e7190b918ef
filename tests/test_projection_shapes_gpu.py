"""`lt_range_projection_dev`, `lt_range_projection` and `lt_range_projection_batch_dev` (csrc/lt_project.hip) called through the
C ABI into sentinel-filled buffers with guards, against the numpy restatement of tests/projection_cases.py (pinned without a
GPU by tests/test_projection_cases_cpu.py): at every wave and block seam of the compaction with constructed keep patterns, at
the seams of the batch's prefix, bounds fold and cloud groups, at ragged image shapes, on constructed edge points and on
float64 depths sharing one float32 bucket, with every output NULL in turn, and with the workspaces stale, regrown and shared
by threads.

What "equals" means here.  float32 clouds: EVERY output bit for bit, no cell or point exempt (the generators keep float32
points away from the rounding midpoints where two float64 math libraries could round differently: projection_cases.guard).
float64 clouds: every image, every integer output, the kept points and their depths bit for bit; `proj_xf` / `proj_yf`, which
carry the library's float64 `atan2` / `asin`, to the bound derived in projection_cases.tol_xf / tol_yf (one ulp of the yaw
scaled by W / (2 pi) resp. one ulp of the pitch scaled by H / fov, plus the ulps of the result's own operations) -- see
`check_xf_yf`."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024
LT_OK, LT_ERR_INVALID_ARG = 0, -1
LT_PROJ_REMOVE, LT_PROJ_NEW = 1, 2
_SIGNED = {4: np.int32, 8: np.int64}
FU, FD = pc.FOV
#: (name, elements per point, bytes per element -- None: the cloud's dtype) in the order of the C signature
PER_POINT = (("points_kept", 3, None), ("rem_kept", 1, 4), ("label_kept", 1, 4), ("depth", 1, None), ("proj_x", 1, 4),
             ("proj_y", 1, 4), ("proj_xf", 1, None), ("proj_yf", 1, None))
IMAGES = (("idx", 1), ("range", 1), ("xyz", 3), ("rem", 1), ("label", 1), ("color", 3), ("mask", 1))
#: lt_proj_images in the order of the struct: (name, elements per cell, bytes -- None: the cloud's dtype), then n_kept and bnds
BATCH_IMAGES = (("idx", 1, 4), ("range", 1, 4), ("xyz", 3, 4), ("rem", 1, 4), ("label", 1, 4), ("color", 3, 4), ("mask", 1, 4),
                ("label_folded", 1, 4), ("proj_x", 1, 4), ("proj_y", 1, 4), ("proj_xf", 1, None), ("proj_yf", 1, None))
BATCH_ALL = tuple(n for n, _, _ in BATCH_IMAGES) + ("n_kept", "bnds")
NEEDS_PREFIX = ("idx", "mask", "proj_x", "proj_y", "proj_xf", "proj_yf", "n_kept")
#: the largest |device - host| of a float64 proj_xf / proj_yf seen in this process, in units of the derived bound
WORST = {"xf": (0.0, 0.0), "yf": (0.0, 0.0)}   # (share of the bound, in ulps of the value)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print(f"\nfloat64 proj_xf / proj_yf, largest |device - host| (share of the derived bound, ulps of the value): {WORST}")


def _lib():
    from lidar_transfer_amd import _lib as L
    return L.load()


def _device():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _up(a):
    """host array -> device tensor (never empty: a NULL data pointer is an argument error of its own)"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.size == 0:
        a = np.zeros(4, a.dtype)
    return torch.from_numpy(a).to(_device())


def _sent(itemsize):
    return pc.SENT32 if itemsize == 4 else pc.SENT64


class Guarded:
    """n elements of `itemsize` bytes filled with a sentinel, 1024 more on both sides; .host() checks the guards"""

    def __init__(self, n, itemsize):
        import torch
        self.n, self.dtype = n, _SIGNED[itemsize]
        self.sent = int(np.array([_sent(itemsize)], {4: np.uint32, 8: np.uint64}[itemsize]).view(self.dtype)[0])
        self.t = torch.full((n + 2 * GUARD,), self.sent, dtype={4: torch.int32, 8: torch.int64}[itemsize], device=_device())
        self.ptr = self.t.data_ptr() + GUARD * itemsize

    def host(self):
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == self.sent).all() and (h[GUARD + self.n:] == self.sent).all(), "guard overwritten"
        return h[GUARD:GUARD + self.n]


class HostGuarded:
    """the same in host memory, for the host-pointer twin"""

    def __init__(self, n, itemsize):
        self.n, self.dtype = n, _SIGNED[itemsize]
        self.sent = int(np.array([_sent(itemsize)], {4: np.uint32, 8: np.uint64}[itemsize]).view(self.dtype)[0])
        self.a = np.full(n + 2 * GUARD, self.sent, self.dtype)
        self.ptr = self.a.ctypes.data + GUARD * itemsize

    def host(self):
        h = self.a
        assert (h[:GUARD] == self.sent).all() and (h[GUARD + self.n:] == self.sent).all(), "guard overwritten"
        return h[GUARD:GUARD + self.n].copy()


def _stream_ptr(stream):
    import torch
    torch.cuda.current_stream().synchronize()          # inputs and sentinels are in place before a side stream reads them
    return C.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)


def _sync(stream):
    import torch
    (stream if stream is not None else torch.cuda.current_stream()).synchronize()


@pytest.fixture(params=["current stream", "side stream"])
def stream(request):
    import torch
    if request.param == "current stream":
        return None
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    return s


def _flags(new, remove):
    return (LT_PROJ_NEW if new else 0) | (LT_PROJ_REMOVE if remove else 0)


_LUT_DEV = {}


def _lut_dev():
    key = _device().index
    if key not in _LUT_DEV:
        _LUT_DEV[key] = _up(pc.lut().reshape(-1))
    return _LUT_DEV[key]


_WANT = {}


def want_of(key, pts, rem, lab, H, W, new, remove, beams=None, use_lut=True):
    """the restatement of a cloud, computed once per (case, variant) and shared by the tests; never modified"""
    k = (key, H, W, new, remove, beams is not None, rem is None, lab is None, use_lut)
    if k not in _WANT:
        _WANT[k] = pc.restate(pts, rem, lab, H, W, FU, FD, beams=beams, remove=remove, new=new, lut=pc.lut() if use_lut else None)
    return _WANT[k]


# ---- the single-cloud call ----------------------------------------------------------------------------------------------------
def call_single(pts, rem, lab, H, W, new, remove, beams=None, stream=None, null=(), use_lut=True, host=False, expect=LT_OK,
                override=None):
    """one lt_range_projection_dev (``host``: lt_range_projection) call; returns name -> the WHOLE output buffer as integers
    (per-point outputs: n rows), "n_kept" and "rc".  ``null``: names of outputs (or "rem_in" / "label_in") passed as NULL;
    ``override``: positional arguments replaced by index (the invalid-argument cases)."""
    lib = _lib()
    n, es, cells = len(pts), pts.dtype.itemsize, H * W
    G = HostGuarded if host else Guarded
    if host:
        ins = [np.ascontiguousarray(pts.reshape(-1)), None if rem is None else np.ascontiguousarray(rem),
               None if lab is None else np.ascontiguousarray(lab)]
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        lut = pc.lut() if use_lut else None
    else:
        ins = [_up(pts.reshape(-1)), None if rem is None else _up(rem), None if lab is None else _up(lab)]
        ptr = lambda t: None if t is None else t.data_ptr()    # noqa: E731
        lut = _lut_dev() if use_lut else None
    bufs = {name: G(n * width, isz or es) for name, width, isz in PER_POINT}
    bufs.update({name: G(cells * width, 4) for name, width in IMAGES})
    p = lambda name: None if name in null else bufs[name].ptr  # noqa: E731
    b = None if beams is None else np.ascontiguousarray(beams, np.float64)
    r_init, m_init, x_init = pc.default_inits(new)
    kept = C.c_int(-7)
    args = [ptr(ins[0]), int(pts.dtype == np.float64), None if "rem_in" in null else ptr(ins[1]),
            None if "label_in" in null else ptr(ins[2]), n, FU, FD, H, W, None if b is None else b.ctypes.data,
            0 if b is None else len(b), _flags(new, remove), ptr(lut), pc.LUT_LEN if use_lut else 0] + \
           [p(name) for name, _, _ in PER_POINT] + [p(name) for name, _ in IMAGES] + [r_init, m_init, x_init, C.byref(kept)]
    if not host:
        args.append(_stream_ptr(stream))
    for k, v in (override or {}).items():
        args[k] = v
    rc = (lib.lt_range_projection if host else lib.lt_range_projection_dev)(*args)
    assert rc == expect, (rc, lib.lt_last_error())
    if not host:
        _sync(stream)
    out = {name: bufs[name].host() for name in bufs}
    out.update(n_kept=kept.value, rc=rc)
    return out


def check_xf_yf(got_bits, want, H, W, which, tag):
    """float64 `proj_xf` / `proj_yf` of a device against the host's restatement.

    They carry the math library's float64 `atan2` / `asin`, which two libraries may round differently in the last place; every
    other operation is IEEE.  The bound is derived, not measured (projection_cases.tol_xf / tol_yf): one ulp of the yaw
    (<= spacing(pi)) scaled by W / (2 pi), resp. one ulp of the pitch (<= spacing(pi / 2)) scaled by H / fov, plus one ulp per
    rounding of the result's own operations at the magnitude they have once scaled to the image.  With the legacy `beams`
    model the pitch is a table entry and `proj_yf` is exact all the same.
    Measured on an MI355X over every case of this file (the module prints the figures when it is done): the largest
    |device - host| was 0.59 of the bound for `proj_xf` (3 ulps of the value, W = 2048) and 0.14 of the bound for `proj_yf`
    (24 ulps of a value next to 0, where an ulp of the value is far below the ulp of the pitch that the bound scales)."""
    got = got_bits.view(np.float64)
    with np.errstate(invalid="ignore"):
        dev = np.where(got_bits == want.view(np.int64), 0.0, np.abs(got - want))
    tol = pc.tol_xf(W) if which == "xf" else pc.tol_yf(H, pc.FOV)
    worst = float(dev.max()) if dev.size else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        ulps = float(np.nan_to_num(dev / np.spacing(np.abs(want))).max()) if dev.size else 0.0
    WORST[which] = max(WORST[which], (worst / tol, ulps))
    assert not np.isnan(dev).any() and worst <= tol, (tag, which, worst, tol)


def check_single(got, want, pts, H, W, null=(), tag=None, has_rem=True, has_label=True):
    """every output of one single-cloud call against the restatement; rows beyond n_kept and NULL outputs hold the sentinel"""
    es, k = pts.dtype.itemsize, want["n_kept"]
    assert got["n_kept"] == k, (tag, got["n_kept"], k)
    exp = dict(points_kept=want["points_kept"].reshape(-1), rem_kept=want["rem_kept"] if has_rem else None,
               label_kept=want["label_kept"] if has_label else None, depth=want["depth"], proj_x=want["proj_x"],
               proj_y=want["proj_y"], proj_xf=want["proj_xf"], proj_yf=want["proj_yf"])
    for name, width, isz in PER_POINT:
        buf, sz = got[name], isz or es
        sentinel = int(np.array([_sent(sz)], {4: np.uint32, 8: np.uint64}[sz]).view(_SIGNED[sz])[0])
        if name in null or exp[name] is None:
            assert (buf == sentinel).all(), (tag, name, "written though NULL / without its input")
            continue
        w = np.ascontiguousarray(exp[name])
        assert w.dtype.itemsize == sz, (name, w.dtype)
        if sz == 8 and name in ("proj_xf", "proj_yf"):
            check_xf_yf(buf[:k], w, H, W, name[-2:], tag)
        else:
            assert np.array_equal(buf[:k * width], w.view(_SIGNED[sz])), (tag, name, int((buf[:k * width] != w.view(_SIGNED[sz])).sum()))
        assert (buf[k * width:] == sentinel).all(), (tag, name, "rows beyond n_kept were written")
    s32 = int(np.array([pc.SENT32], np.uint32).view(np.int32)[0])
    for name, width in IMAGES:
        buf = got[name]
        if name in null:
            assert (buf == s32).all(), (tag, name)
            continue
        w = np.ascontiguousarray(want[name]).reshape(-1)
        assert np.array_equal(buf, w.view(np.int32)), (tag, name, int((buf != w.view(np.int32)).sum()))


def run_single(key, pts, rem, lab, H, W, new, remove, beams=None, stream=None, **kw):
    want = want_of(key, pts, rem, lab, H, W, new, remove, beams)
    got = call_single(pts, rem, lab, H, W, new, remove, beams, stream, **kw)
    check_single(got, want, pts, H, W, tag=(key, H, W, new, remove, beams is not None))
    return got, want


@pytest.mark.parametrize("new,remove", pc.VARIANTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_sizes_with_keep_patterns_at_every_seam(dtype, new, remove, stream):
    H, W = pc.SIZES_SHAPE
    seen = {"first": set(), "last": set(), 63: set(), 64: set(), 255: set(), 256: set()}
    for n in pc.SIZES:
        pts, rem, lab, keep = pc.size_case(n, dtype, remove)
        _, want = run_single(("size", n, dtype), pts, rem, lab, H, W, new, remove, None, stream)
        assert np.array_equal(want["kept"], keep), n            # the pattern is what the projection keeps
        if n:
            seen["first"].add(bool(keep[0])), seen["last"].add(bool(keep[-1]))
        for s in (63, 64, 255, 256):
            if n > s + 1:
                seen[s].add(bool(keep[s]))
    assert all(v == {True, False} for v in seen.values()), seen   # both ends and both sides of a wave and a block seam, in and out
    assert {65535, 65536, 65537} <= set(pc.SIZES)                 # 255 | 256 | 257 blocks of the per-point kernels
    # the compaction numbers the kept points with k_pb_prefix, whose share per thread goes from one wave to two at 256 waves:
    # the clouds of test_batch_sizes_across_the_prefix_and_fold_seams (and their restatements), one call each
    big = pc.big_batch_case(dtype, remove)[:4]
    assert [len(c[0]) for c in big] == [16383, 16384, 16385, 16448]
    for k, (pts, rem, lab) in enumerate(big):
        got, _ = run_single((("big", dtype, remove), k), pts, rem, lab, H, W, new, remove, None, stream)
        assert 0 < got["n_kept"] < len(pts)


@pytest.mark.parametrize("new,remove", pc.VARIANTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_image_shapes(dtype, new, remove, stream):
    zero = new or remove                                           # (old without `remove` divides by depth 0: not an input)
    for H, W in pc.SHAPES:
        pts, rem, lab = pc.shape_case(H, W, dtype, zero)
        assert len(pts) == (5000 if (H, W) == (64, 2048) else 700)
        run_single(("shape", dtype, zero), pts, rem, lab, H, W, new, remove, None, stream)
    H, W = 16, 301
    pts, rem, lab = pc.shape_case(H, W, dtype, zero)
    run_single(("shape", dtype, zero), pts, rem, lab, H, W, new, remove, pc.LEGACY_BEAMS, stream)   # the legacy `beams` model


def _edge_inputs(H, W, dtype, new, remove):
    pts, rem, lab, pairs = pc.edge_case(H, W, dtype)
    if not (new or remove):                                        # depth 0 stays out of the old variant without `remove`
        ok = pc.project_points(pts, H, W, FU, FD)["depth"] != 0
        pts, rem, lab = np.ascontiguousarray(pts[ok]), rem[ok], lab[ok]
    return pts, rem, lab, pairs


@pytest.mark.parametrize("new,remove", pc.VARIANTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_edge_points_and_bucket_cases(dtype, new, remove):
    for H, W in pc.SHAPES:
        pts, rem, lab, pairs = _edge_inputs(H, W, dtype, new, remove)
        assert len(pairs) >= 2 and np.isnan(pts).any() and np.isinf(pts).any()
        run_single(("edge", dtype), pts, rem, lab, H, W, new, remove)
    if dtype == np.float64:                                        # several depths of one float32 bucket exist in float64 only
        H, W = pc.SIZES_SHAPE
        orders = set()
        for c in pc.bucket_case_list(H, W):
            if c["place"] == "spread":
                continue                                           # (the batch runs those)
            run_single(("bucket", c["name"], c["place"]), c["points"], c["rem"], c["label"], H, W, new, remove)
            orders.add(c["name"])
        assert orders == set(pc.BUCKET_ORDERS)


def test_single_null_subsets():
    H, W = pc.SIZES_SHAPE
    names = [n for n, _, _ in PER_POINT] + [n for n, _ in IMAGES]
    for dtype, new, remove in ((np.float32, True, True), (np.float64, False, True)):
        pts, rem, lab = pc.shape_case(H, W, dtype, True)
        want = want_of(("shape", dtype, True), pts, rem, lab, H, W, new, remove)
        assert (want["label"].view(np.uint32) >= pc.LUT_LEN).any()                 # a label beyond the table: colour 0
        beyond = want["label"].view(np.uint32) >= pc.LUT_LEN
        assert (want["color"][beyond] == 0).all() and (want["color"][~beyond & (want["idx"] >= 0)] != 0).any()
        subsets = [tuple(m for m in names if m != only) for only in names]           # each optional output alone
        subsets += [tuple(n for n, _, _ in PER_POINT), tuple(n for n, _ in IMAGES), tuple(names)]
        for null in subsets:
            got = call_single(pts, rem, lab, H, W, new, remove, null=null)
            check_single(got, want, pts, H, W, null=null, tag=(dtype, null))
        # without remissions / labels / colour table: their images hold the initial value / 0, the compacted copies stay untouched
        w2 = want_of(("shape", dtype, True, "bare"), pts, None, None, H, W, new, remove, use_lut=False)
        got = call_single(pts, rem, lab, H, W, new, remove, null=("rem_in", "label_in"), use_lut=False)
        check_single(got, w2, pts, H, W, tag=(dtype, "no rem / label / lut"), has_rem=False, has_label=False)
        assert (w2["rem"] == -1).all() and (w2["label"] == 0).all() and (w2["color"] == 0).all()


def test_single_host_pointer_twin_gives_the_same_bytes():
    H, W = pc.SIZES_SHAPE
    cases = [(np.float32, True, True, pc.size_case(513, np.float32, True)[:3]), (np.float64, False, True, pc.shape_case(H, W, np.float64, True)),
             (np.float64, True, False, _edge_inputs(H, W, np.float64, True, False)[:3])]
    for dtype, new, remove, (pts, rem, lab) in cases:
        dev = call_single(pts, rem, lab, H, W, new, remove)
        hst = call_single(pts, rem, lab, H, W, new, remove, host=True)
        for name in dev:
            assert np.array_equal(dev[name], hst[name]), (dtype, new, remove, name)
        check_single(hst, pc.restate(pts, rem, lab, H, W, FU, FD, remove=remove, new=new, lut=pc.lut()), pts, H, W, tag="host")


def _workspace_steps(dtype, zero):
    steps = [(H, W, pc.shape_case(H, W, dtype, zero, seed=s + 1, n=n)) for s, (H, W, n) in enumerate(pc.WORKSPACE_STEPS)]
    sizes = [len(c[0]) for _, _, c in steps]
    assert [s[:2] for s in steps[:4]] == [(4, 64), (64, 2048), (3, 85), (64, 2048)]    # small -> large -> small -> large
    assert sizes[4] >= 40 * max(sizes[:4]) and steps[5][:2] == steps[0][:2]            # regrown, then the first case again
    return steps


def _workspace_child(dtype):
    """a fresh process: the process-wide workspace starts unallocated, is regrown by the second and by the fifth call, and every
    call must equal the restatement -- a key left in a cell of an earlier, larger image would show in the next one"""
    for new, remove in pc.VARIANTS:
        for step, (H, W, (pts, rem, lab)) in enumerate(_workspace_steps(dtype, new or remove)):
            run_single(("ws", step, dtype, new or remove), pts, rem, lab, H, W, new, remove)
    print("workspace ok", WORST)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_single_workspace_shape_sequence_and_regrowth_in_a_fresh_process(dtype):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "workspace", dtype], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "workspace ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout[-300:])


def test_single_from_two_threads_on_their_own_streams():
    """two host threads, each with a stream, an image shape and clouds of its own, 20 calls each: every result equals the
    restatement.  The workspace is one per process; the call serialises on it."""
    import torch
    jobs = [((4, 64), np.float32, True, True), ((64, 2048), np.float64, True, False)]
    cases = {t: [pc.shape_case(H, W, dtype, True, seed=j + 1, n=900 + 700 * j) for j in range(2)]
             for t, ((H, W), dtype, _, _) in enumerate(jobs)}
    wants = {(t, j): want_of(("thr", t, j), *cases[t][j], *jobs[t][0], jobs[t][2], jobs[t][3]) for t in range(2) for j in range(2)}
    streams = [torch.cuda.Stream() for _ in range(2)]
    _lut_dev()
    torch.cuda.synchronize()
    results, errors = {}, []

    def work(t):
        try:
            (H, W), _, new, remove = jobs[t]
            for rep in range(20):
                results[(t, rep)] = call_single(*cases[t][rep % 2], H, W, new, remove, stream=streams[t])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert len(results) == 40
    for (t, rep), got in results.items():
        check_single(got, wants[(t, rep % 2)], cases[t][rep % 2][0], *jobs[t][0], tag=("thread", t, rep))


def test_single_arguments():
    """what the entry point refuses before it launches anything: the error code, the message, and untouched outputs"""
    lib = _lib()
    H, W = 4, 64
    pts, rem, lab = pc.shape_case(H, W, np.float32, True)
    s32 = int(np.array([pc.SENT32], np.uint32).view(np.int32)[0])
    beams = np.zeros(1025)
    for override in ({4: -1}, {7: 0}, {7: -3}, {8: 0}, {0: None}, {10: 1025, 9: beams.ctypes.data}, {10: -1}, {10: 4, 9: None}):
        got = call_single(pts, rem, lab, H, W, True, True, expect=LT_ERR_INVALID_ARG, override=override)
        assert b"lt_range_projection" in lib.lt_last_error(), override
        assert got["n_kept"] == -7 and all((got[name] == s32).all() for name, _ in IMAGES), override
    got = call_single(pts, rem, lab, H, W, True, True, host=True, expect=LT_ERR_INVALID_ARG, override={4: -1})
    assert b"lt_range_projection" in lib.lt_last_error() and got["n_kept"] == -7
    got = call_single(pts[:0], rem[:0], lab[:0], H, W, True, True, override={0: None})      # n = 0 with NULL points: empty images
    check_single(got, pc.restate(pts[:0], rem[:0], lab[:0], H, W, FU, FD, lut=pc.lut()), pts[:0], H, W, tag="n = 0")


# ---- the batched call ---------------------------------------------------------------------------------------------------------
def launch_shape(outs_per_cloud):
    """which of the three launch sequences lt_range_projection_batch_dev takes for a group of clouds with these outputs:
    "prefix" (k_pb_prefix), "bnds" (k_pb_bnds alone), "none" (neither)"""
    if any(o in NEEDS_PREFIX for outs in outs_per_cloud for o in outs):
        return "prefix"
    return "bnds" if any("bnds" in outs for outs in outs_per_cloud) else "none"


class Projector:
    def __init__(self):
        self.h = C.c_void_p()
        assert _lib().lt_projector_create(C.byref(self.h), -1) == LT_OK, _lib().lt_last_error()

    def close(self):
        assert _lib().lt_projector_destroy(self.h) == LT_OK
        self.h = None


def call_batch(pj, clouds, H, W, new, remove, outs, beams=None, stream=None, use_lut=True, expect=LT_OK, null_empty=False):
    """one lt_range_projection_batch_dev call; ``outs``: one tuple of output names for all clouds, or a list of one tuple per
    cloud.  Returns a list of name -> the whole buffer as integers (names not asked for are absent)."""
    from lidar_transfer_amd._lib import Cloud, ProjImages
    lib = _lib()
    nc = len(clouds)
    outs = [tuple(outs)] * nc if (not outs or isinstance(outs[0], str)) else [tuple(o) for o in outs]
    dtype = clouds[0][0].dtype if nc else np.dtype(np.float32)
    es, cells = dtype.itemsize, H * W
    carr, oarr = (Cloud * max(nc, 1))(), (ProjImages * max(nc, 1))()
    hold, bufs = [], []
    for k, (pts, rem, lab) in enumerate(clouds):
        assert pts.dtype == dtype
        if len(pts) == 0 and null_empty:
            carr[k].points, carr[k].rem, carr[k].label, carr[k].n = None, None, None, 0
        else:
            d = [_up(pts.reshape(-1)), None if rem is None else _up(rem), None if lab is None else _up(lab)]
            hold.append(d)
            carr[k].points, carr[k].n = d[0].data_ptr(), len(pts)
            carr[k].rem = None if d[1] is None else d[1].data_ptr()
            carr[k].label = None if d[2] is None else d[2].data_ptr()
        b = {}
        for name, width, isz in BATCH_IMAGES:
            if name in outs[k]:
                b[name] = Guarded(cells * width, isz or es)
        if "n_kept" in outs[k]:
            b["n_kept"] = Guarded(1, 4)
        if "bnds" in outs[k]:
            b["bnds"] = Guarded(6, 8)
        for name in BATCH_ALL:
            setattr(oarr[k], name, b[name].ptr if name in b else None)
        bufs.append(b)
    bm = None if beams is None else np.ascontiguousarray(beams, np.float64)
    r_init, m_init, x_init = pc.default_inits(new)
    rc = lib.lt_range_projection_batch_dev(pj.h, nc, carr, int(dtype == np.float64), FU, FD, H, W,
                                           None if bm is None else bm.ctypes.data, 0 if bm is None else len(bm), _flags(new, remove),
                                           _lut_dev().data_ptr() if use_lut else None, pc.LUT_LEN if use_lut else 0, oarr,
                                           r_init, m_init, x_init, _stream_ptr(stream))
    assert rc == expect, (rc, lib.lt_last_error())
    _sync(stream)
    return [{name: g.host() for name, g in b.items()} for b in bufs]


_BATCH_TO_WANT = dict(proj_x="img_px", proj_y="img_py", proj_xf="img_xf", proj_yf="img_yf")


def check_batch(got, want, dtype, H, W, tag):
    """the images of ONE cloud of a batched call against the restatement of that cloud alone"""
    for name, buf in got.items():
        if name == "n_kept":
            assert buf[0] == want["n_kept"], (tag, name, buf[0], want["n_kept"])
        elif name == "bnds":
            b = buf.view(np.float64)                            # by value (a zero's sign is not part of a bound)
            assert np.array_equal(b, want["bnds"]), (tag, name, b, want["bnds"])
            if want["n_kept"] == 0:
                assert b.tolist() == [np.inf, -np.inf] * 3, (tag, b)
        else:
            w = np.ascontiguousarray(want[_BATCH_TO_WANT.get(name, name)]).reshape(-1)
            if dtype == np.float64 and name in ("proj_xf", "proj_yf"):
                check_xf_yf(buf, w, H, W, name[-2:], (tag, name))
            else:
                assert w.dtype.itemsize == buf.dtype.itemsize, (name, w.dtype)
                assert np.array_equal(buf, w.view(buf.dtype)), (tag, name, int((buf != w.view(buf.dtype)).sum()))


def run_batch(pj, key, clouds, H, W, new, remove, outs, beams=None, stream=None, use_lut=True, **kw):
    got = call_batch(pj, clouds, H, W, new, remove, outs, beams, stream, use_lut=use_lut, **kw)
    for k, (g, (pts, rem, lab)) in enumerate(zip(got, clouds)):
        want = want_of((key, k), pts, rem, lab, H, W, new, remove, beams, use_lut)
        check_batch(g, want, pts.dtype, H, W, (key, k, len(pts), new, remove))
    return got


@pytest.fixture
def pj():
    p = Projector()
    yield p
    p.close()


@pytest.mark.parametrize("new,remove", pc.VARIANTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_cloud_counts_across_the_groups_of_eight(dtype, new, remove, pj):
    """1, 7, 8, 9, 16 and 17 clouds: every image of every cloud against the restatement of that cloud alone"""
    H, W = pc.SIZES_SHAPE
    zero = new or remove
    assert {c > 8 for c in pc.BATCH_COUNTS} == {True, False} and max(pc.BATCH_COUNTS) > 16
    for count in pc.BATCH_COUNTS:
        clouds = pc.batch_case(count, dtype, remove, zero)
        assert len(clouds) == count
        if count > 1:
            sizes = [len(c[0]) for c in clouds]
            assert sizes[0] == sizes[count // 2] == sizes[-1] == 0 and sizes[2] == 1
            dropped = want_of((("count", count, dtype, remove, zero), 1), *clouds[1], H, W, new, remove)
            assert sizes[1] > 0 and dropped["n_kept"] == 0       # a cloud all of whose points are dropped
        run_batch(pj, ("count", count, dtype, remove, zero), clouds, H, W, new, remove, BATCH_ALL)
    # the special clouds alone, as calls of one cloud; an empty cloud may have NULL pointers
    special = pc.batch_case(7, dtype, remove, zero)
    for k in (0, 1, 2):
        run_batch(pj, ("count", 7, dtype, remove, zero, "alone", k), [special[k]], H, W, new, remove, BATCH_ALL, null_empty=True)


@pytest.mark.parametrize("new", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_sizes_across_the_prefix_and_fold_seams(dtype, new, pj):
    """16383 | 16384 | 16385 points: k_pb_prefix's share per thread goes from one wave to two at 256 waves; 16448 = 257 waves;
    65537 points = 257 blocks: pb_fold_bounds loops past 64 blocks (and 16385 points are 65 of them)"""
    H, W = pc.SIZES_SHAPE
    assert {n for n in pc.BATCH_BIG if (n + 63) // 64 <= 256} and {n for n in pc.BATCH_BIG if (n + 63) // 64 > 256}
    assert min((n + 255) // 256 for n in pc.BATCH_BIG) == 64 and sorted((n + 255) // 256 for n in pc.BATCH_BIG)[1] == 64 \
        and max((n + 255) // 256 for n in pc.BATCH_BIG) > 256 and 16385 in pc.BATCH_BIG
    for remove in (True, False):
        clouds = pc.big_batch_case(dtype, remove)
        assert [len(c[0]) for c in clouds] == list(pc.BATCH_BIG)
        outs = ("idx", "n_kept", "proj_x", "proj_y", "proj_xf", "proj_yf", "bnds")
        got = run_batch(pj, ("big", dtype, remove), clouds, H, W, new, remove, outs)
        for g, (pts, _, _) in zip(got, clouds):
            assert 0 < g["n_kept"][0] < len(pts)


@pytest.mark.parametrize("new,remove", pc.VARIANTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_output_subsets_take_all_three_launch_shapes(dtype, new, remove, pj, stream):
    H, W = pc.SIZES_SHAPE
    zero = new or remove
    clouds = pc.batch_case(9, dtype, remove, zero)
    key = ("count", 9, dtype, remove, zero)
    deform = ("range", "rem", "label_folded")                    # what lt_deform_scan_dev asks for
    shapes = set()
    for outs in (("idx", "range"), ("bnds",), deform, deform + ("bnds",), ("n_kept",), ("mask",), ("proj_xf",), ("xyz", "color", "label"),
                 ()):
        shapes.add(launch_shape([outs] * 9))
        run_batch(pj, key, clouds, H, W, new, remove, outs)
    assert shapes == {"prefix", "bnds", "none"}
    # a mixed group: one cloud wants idx, its neighbour only range, the next only its bounds, the next nothing at all
    mixed = [(("idx",), ("range",), ("bnds",), ())[k % 4] for k in range(9)]
    assert launch_shape(mixed[:8]) == "prefix" and launch_shape(mixed[8:]) == "prefix"
    run_batch(pj, key, clouds, H, W, new, remove, mixed, None, stream)
    mixed = [(("range",), ("bnds", "rem"))[k % 2] for k in range(8)] + [("idx",)]
    assert launch_shape(mixed[:8]) == "bnds" and launch_shape(mixed[8:]) == "prefix"
    run_batch(pj, key, clouds, H, W, new, remove, mixed)
    # and everything at once after all that, without remissions, labels and a colour table
    bare = tuple((p, None, None) for p, _, _ in clouds)
    run_batch(pj, key + ("bare",), bare, H, W, new, remove, BATCH_ALL, None, stream, use_lut=False)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_workspace_shape_sequence_and_regrowth_on_one_projector(dtype, pj):
    """ONE projector through small -> large -> small -> large image shapes, a regrowth and the first case again, in every
    variant in turn (old float64 allocates `dmin` on its first use: before and after the regrowth), with a legacy `beams` call
    between two calls without it (the table is cached per projector)"""
    order = ((False, True), (True, True), (True, False), (False, False)) if dtype == np.float64 else pc.VARIANTS
    for rnd, (new, remove) in enumerate(order):
        zero = new or remove
        steps = _workspace_steps(dtype, zero)
        for step, (H, W, cloud) in enumerate(steps):
            if rnd >= 2 and step == 4:
                continue                                           # (the projector has been regrown by then)
            other = steps[(step + 2) % 4][2]                       # a second cloud of another size in the same call
            other = tuple(a[:300] for a in other)
            beams = pc.LEGACY_BEAMS if step in (1, 3) else None
            run_batch(pj, ("ws", step, dtype, zero), [cloud, other], H, W, new, remove, BATCH_ALL, beams)


@pytest.mark.parametrize("new,remove", pc.VARIANTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_edge_points_and_bucket_cases(dtype, new, remove, pj):
    for H, W in pc.SHAPES:
        pts, rem, lab, pairs = _edge_inputs(H, W, dtype, new, remove)
        bulk = pc.shape_case(H, W, dtype, new or remove)
        run_batch(pj, ("edge", H, W, dtype), [(pts, rem, lab), bulk], H, W, new, remove, BATCH_ALL)
    if dtype == np.float64:
        H, W = pc.SIZES_SHAPE
        cases = pc.bucket_case_list(H, W)
        spread = [c for c in cases if c["place"] == "spread" and len(c["at"]) >= 2]
        assert {c["name"] for c in spread} == set(pc.BUCKET_ORDERS) - {"lt_alone"}
        for c in spread:                                           # the competing points in different waves and blocks
            assert len(set((c["at"] // 64).tolist())) == len(c["at"]) and len(set((c["at"] // 256).tolist())) >= 2
        for a in range(0, len(cases), 8):
            group = cases[a:a + 8]
            run_batch(pj, ("bucket", a), [(c["points"], c["rem"], c["label"]) for c in group], H, W, new, remove, BATCH_ALL)


def test_batch_arguments(pj):
    from lidar_transfer_amd._lib import Cloud, ProjImages
    lib = _lib()
    H, W = 4, 64
    pts, rem, lab = pc.shape_case(H, W, np.float32, True)
    d = _up(pts.reshape(-1))
    s32 = int(np.array([pc.SENT32], np.uint32).view(np.int32)[0])
    img = Guarded(H * W, 4)
    carr, oarr = (Cloud * 2)(), (ProjImages * 2)()
    oarr[0].range = img.ptr
    beams = np.zeros(1025)

    def call(n0=len(pts), n1=0, p0=d.data_ptr(), h=H, nb=0, handle=pj.h, nc=2):
        carr[0].points, carr[0].n, carr[1].points, carr[1].n = p0, n0, None, n1
        return lib.lt_range_projection_batch_dev(handle, nc, carr, 0, FU, FD, h, W, beams.ctypes.data if nb else None, nb, 3, None, 0,
                                                 oarr, 0.0, -1.0, 0.0, _stream_ptr(None))

    for kw in (dict(n0=-1), dict(n1=-2), dict(p0=None), dict(h=0), dict(nb=1025), dict(handle=None), dict(nc=-1)):
        assert call(**kw) == LT_ERR_INVALID_ARG, kw
        assert b"lt_range_projection_batch_dev" in lib.lt_last_error(), kw
    _sync(None)
    assert (img.host() == s32).all()                              # refused before anything ran
    assert call() == LT_OK
    _sync(None)
    want = pc.restate(pts, None, None, H, W, FU, FD)
    assert np.array_equal(img.host(), want["range"].view(np.int32))
    assert call(nc=0) == LT_OK                                   # no cloud at all: nothing to do


if __name__ == "__main__":
    if sys.argv[1:2] == ["workspace"]:
        sys.path.insert(0, ROOT)
        _workspace_child({"float32": np.float32, "float64": np.float64}[sys.argv[2]])
