"""`lt_reverse_projection_dev`, `lt_pack_scan_dev` and `lt_compare_dev` (csrc/lt_post.hip) called through the C ABI into
sentinel-filled buffers with guards, against the numpy restatements of tests/post_cases.py (pinned without a GPU by
tests/test_post_cpu.py): at the wave, block and chunk seams of the packer and with its process-wide block counts stale,
regrown and shared by threads; at ragged image shapes, edge coordinates and empty cells of the reverse projection; with
non-power-of-two label tables, constructed waves, garbage in the accumulators and NULL outputs of the comparison."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024
LT_OK, LT_ERR_INVALID_ARG = 0, -1
_SIGNED = {4: np.int32, 8: np.int64}


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


class Guarded:
    """n elements of `itemsize` bytes filled with `sentinel`, 1024 more on both sides; .host() checks the guards"""

    def __init__(self, n, itemsize, sentinel):
        import torch
        self.n, self.dtype = n, _SIGNED[itemsize]
        self.sent = int(np.array([sentinel], {4: np.uint32, 8: np.uint64}[itemsize]).view(self.dtype)[0])
        self.t = torch.full((n + 2 * GUARD,), self.sent, dtype={4: torch.int32, 8: torch.int64}[itemsize], device=_device())
        self.ptr = self.t.data_ptr() + GUARD * itemsize

    def host(self):
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == self.sent).all() and (h[GUARD + self.n:] == self.sent).all(), "guard overwritten"
        return h[GUARD:GUARD + self.n]


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


# ---- pack -------------------------------------------------------------------------------------------------------------------
def call_pack(case, stream=None):
    """one lt_pack_scan_dev call; returns (rc, n_out, bin bits [n, 4] uint32, label [n] uint32) -- the WHOLE output buffers"""
    pts = case["points"]
    n = len(pts)
    d = [_up(pts.reshape(-1)), _up(case["rem"]), _up(case["label"])]
    di = _up(case["index"]) if case["index"] is not None else None
    ob, ol = Guarded(4 * n, 4, pc.SENT_F32), Guarded(n, 4, pc.SENT_U32)
    kept = C.c_int(-7)
    rc = _lib().lt_pack_scan_dev(d[0].data_ptr(), int(pts.dtype == np.float64), d[1].data_ptr(), d[2].data_ptr(),
                                 di.data_ptr() if di is not None else None, n, ob.ptr, ol.ptr, C.byref(kept), _stream_ptr(stream))
    return rc, kept.value, ob.host().view(np.uint32).reshape(n, 4), ol.host().view(np.uint32)


def check_pack(res, case, tag):
    rc, n_out, b, l = res
    wb, wl = pc.restate_pack(case["points"], case["label"], case["rem"], case["index"])
    assert rc == LT_OK, tag
    assert n_out == len(wl) == int(case["keep"].sum()), (tag, n_out, len(wl))
    assert np.array_equal(b[:n_out], wb.view(np.uint32)), tag
    assert np.array_equal(l[:n_out], wl), tag
    assert (b[n_out:] == pc.SENT_F32).all() and (l[n_out:] == pc.SENT_U32).all(), (tag, "rows beyond n_out were written")


def _mixed_keep(n):
    """what the size tests keep: a random 60 % with both ends and every block seam forced in or out in turn"""
    k = np.random.default_rng(n).random(n) < 0.6
    k[0], k[-1] = True, True
    seam = np.arange(pc.BLOCK, n, pc.BLOCK)
    k[seam] = (seam // pc.BLOCK) % 2 == 0
    k[seam - 1] = (seam // pc.BLOCK) % 3 != 0
    return k


@pytest.mark.parametrize("with_index", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pack_at_every_block_count_and_ragged_tail(dtype, with_index, stream):
    for n in pc.PACK_SIZES:
        case = pc.pack_case(n, dtype, _mixed_keep(n), with_index)
        check_pack(call_pack(case, stream), case, (n, np.dtype(dtype).name, with_index))


@pytest.mark.parametrize("pattern", pc.KEEP_PATTERNS)
@pytest.mark.parametrize("nb", [65, 2049])
def test_pack_keep_patterns_at_the_wave_block_and_chunk_seams(nb, pattern, stream):
    n = pc.BLOCK * (nb - 1) + 1
    keep = pc.keep_pattern(pattern, n)
    for dtype, with_index in ((np.float32, False), (np.float64, True), (np.float32, True), (np.float64, False)):
        case = pc.pack_case(n, dtype, keep, with_index)
        check_pack(call_pack(case, stream), case, (nb, pattern, np.dtype(dtype).name, with_index))


@pytest.mark.parametrize("with_index", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pack_value_edges(dtype, with_index, stream):
    """the keep rule in the points' dtype, float64 -> float32 at a tie and into the denormals, NaN, labels up to 0x7fffffff and
    with bit 31, index 0 / -1 / INT_MAX"""
    case = pc.pack_value_edges(dtype, with_index)
    check_pack(call_pack(case, stream), case, (np.dtype(dtype).name, with_index))


def test_pack_smaller_calls_run_over_stale_block_counts(stream):
    for nb, pattern in ((2049, "all"), (1, "all"), (1025, "one_per_block"), (64, "odd_waves"), (2049, "none"), (2, "last")):
        n = pc.BLOCK * (nb - 1) + 1
        case = pc.pack_case(n, np.float32, pc.keep_pattern(pattern, n), False)
        check_pack(call_pack(case, stream), case, (nb, pattern))


def test_pack_from_four_threads_on_their_own_streams():
    """four host threads, each with a stream and inputs of its own, three sizes each (one of them past a turn of the chunk
    loop): every result is the serial one.  The block counts are one buffer per process; the call serialises on it."""
    import torch
    sizes = [(pc.BLOCK * 1024 + 1, 257, pc.BLOCK * 64 + 1), (63, pc.BLOCK * 1024 + 1, 65), (pc.BLOCK * 62 + 1, 1, pc.BLOCK * 2048 + 1),
             (256, pc.BLOCK * 1022 + 1, 255)]
    cases = {(t, j): pc.pack_case(n, (np.float32, np.float64)[(t + j) % 2], pc.keep_pattern(pc.KEEP_PATTERNS[(3 * t + j) % 10], n, seed=t),
                                  bool((t + j) % 3 == 0), seed=10 + t)
             for t, ns in enumerate(sizes) for j, n in enumerate(ns)}
    serial = {k: call_pack(c) for k, c in cases.items()}
    for k, c in cases.items():
        check_pack(serial[k], c, ("serial", k))
    streams = [torch.cuda.Stream() for _ in range(4)]
    torch.cuda.synchronize()
    results, errors = {}, []

    def work(t):
        try:
            for rep in range(2):
                for j in range(3):
                    results[(t, j, rep)] = call_pack(cases[(t, j)], streams[t])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert len(results) == 24
    for (t, j, rep), got in results.items():
        want = serial[(t, j)]
        assert got[0] == LT_OK and got[1] == want[1], (t, j, rep)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), (t, j, rep)


def _regrow_child():
    """a fresh process: the first call sizes the block counts for 2 blocks (2 * 2 + 1024 entries), the second needs 2049 + 2"""
    for n, pattern in ((257, "all"), (pc.BLOCK * 2048 + 1, "random50"), (257, "one_per_block"), (pc.BLOCK * 2048 + 1, "seam_chunk")):
        assert n <= 257 or (n + 255) // 256 + 2 > 2 * 2 + 1024
        case = pc.pack_case(n, np.float64, pc.keep_pattern(pattern, n), True)
        check_pack(call_pack(case), case, (n, pattern))
    print("regrow ok")


def test_pack_regrows_its_block_counts_in_a_fresh_process():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "regrow"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "regrow ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_pack_arguments():
    lib = _lib()
    case = pc.pack_case(0, np.float32)
    rc, n_out, b, l = call_pack(case)                         # n = 0: LT_OK, nothing counted, nothing written (guards checked)
    assert rc == LT_OK and n_out == 0 and b.shape == (0, 4)
    case = pc.pack_case(300, np.float32)
    d = [_up(case["points"].reshape(-1)), _up(case["rem"]), _up(case["label"])]
    ob, ol = Guarded(1200, 4, pc.SENT_F32), Guarded(300, 4, pc.SENT_U32)
    kept = C.c_int(-7)
    good = [d[0].data_ptr(), 0, d[1].data_ptr(), d[2].data_ptr(), None, 300, ob.ptr, ol.ptr, C.byref(kept), _stream_ptr(None)]
    bad = list(good)
    bad[5] = -1
    assert lib.lt_pack_scan_dev(*bad) == LT_ERR_INVALID_ARG and b"lt_pack_scan_dev" in lib.lt_last_error()
    for k in (0, 2, 3, 6, 7):                                 # every required pointer in turn
        bad = list(good)
        bad[k] = None
        assert lib.lt_pack_scan_dev(*bad) == LT_ERR_INVALID_ARG, k
    assert (ob.host().view(np.uint32) == pc.SENT_F32).all() and (ol.host().view(np.uint32) == pc.SENT_U32).all()
    assert lib.lt_pack_scan_dev(*good) == LT_OK and kept.value == 300
    good[8] = None                                            # n_out is optional
    assert lib.lt_pack_scan_dev(*good) == LT_OK
    nothing = [None, 0, None, None, None, 0, None, None, C.byref(kept), None]
    assert lib.lt_pack_scan_dev(*nothing) == LT_OK and kept.value == 0


# ---- reverse projection -----------------------------------------------------------------------------------------------------
def call_reverse(r, px, py, fov, stream=None):
    H, W = r.shape
    d = [_up(r.reshape(-1)), _up(px.reshape(-1)), _up(py.reshape(-1))]
    out = Guarded(3 * H * W, 8, pc.SENT_F64)
    rc = _lib().lt_reverse_projection_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), int(px.dtype == np.float64),
                                          float(fov[0]), float(fov[1]), H, W, out.ptr, _stream_ptr(stream))
    assert rc == LT_OK
    _sync(stream)
    return out.host().view(np.float64).reshape(-1, 3)


def check_reverse(got, r, px, py, fov, what, capsys):
    """rtol = atol = 1e-13: the bound tests/test_post_gpu.py holds the same kernel to (two float64 math libraries), kept, not
    derived; float32 bits equal wherever the restatement is not near a float32 tie.  Prints the largest relative difference."""
    want = pc.restate_reverse(r, px, py, *fov)
    assert not (got.view(np.uint64) == pc.SENT_F64).any(), what
    with np.errstate(all="ignore"):
        rel = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == want, 0.0, np.inf))
    near = pc.near_f32_tie(want)
    b_got, b_want = got.astype(np.float32).view(np.uint32), want.astype(np.float32).view(np.uint32)
    with capsys.disabled():
        print(f"\nreverse {what}: largest relative difference {rel.max():.1e}, largest absolute "
              f"{np.abs(got - want)[np.abs(want) < 1e3].max():.1e} (below 1e3), near a tie {int(near.sum())} of {want.size}, "
              f"float32 differing elsewhere {int((b_got != b_want)[~near].sum())}", end="")
    assert np.allclose(got, want, rtol=1e-13, atol=1e-13), what
    assert np.array_equal(b_got[~near], b_want[~near]), what


@pytest.mark.parametrize("float_coords", [False, True])
@pytest.mark.parametrize("shape", pc.REVERSE_SHAPES)
def test_reverse_projection_at_ragged_shapes_and_four_fields_of_view(shape, float_coords, capsys):
    for fov in pc.REVERSE_FOVS:
        r, px, py, what = pc.reverse_case(*shape, fov, float_coords)
        check_reverse(call_reverse(r, px, py, fov), r, px, py, fov, what, capsys)


def test_reverse_projection_on_a_side_stream(capsys):
    import torch
    s = torch.cuda.Stream()
    for float_coords in (False, True):
        r, px, py, what = pc.reverse_case(16, 301, (3.0, -25.0), float_coords)
        check_reverse(call_reverse(r, px, py, (3.0, -25.0), s), r, px, py, (3.0, -25.0), what + " side stream", capsys)


def test_reverse_projection_arguments():
    lib = _lib()
    r, px, py, _ = pc.reverse_case(3, 85, (3.0, -25.0), False)
    d = [_up(r.reshape(-1)), _up(px.reshape(-1)), _up(py.reshape(-1))]
    out = Guarded(3 * 255, 8, pc.SENT_F64)
    good = [d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 3.0, -25.0, 3, 85, out.ptr, _stream_ptr(None)]
    for k, v in ((6, 0), (6, -1), (7, 0), (0, None), (1, None), (2, None), (8, None)):
        bad = list(good)
        bad[k] = v
        assert lib.lt_reverse_projection_dev(*bad) == LT_ERR_INVALID_ARG, k
        assert b"lt_reverse_projection_dev" in lib.lt_last_error()
    _sync(None)
    assert (out.host().view(np.uint64) == pc.SENT_F64).all()


# ---- compare ----------------------------------------------------------------------------------------------------------------
_IN = ("src_label", "src_color", "tgt_label", "src_range", "tgt_range", "src_rem", "tgt_rem")
_OPT = ("range_diff", "rem_diff", "src_masked", "tgt_masked")


def call_compare(c, null=(), stream=None, expect=LT_OK, no_rem=False):
    """one lt_compare_dev call; conf and sq_sum hold garbage before it (the call has to zero them), the images sentinels"""
    n, nl = len(c["src_label"]), c["n_labels"]
    d = {k: _up(np.asarray(c[k]).reshape(-1)) for k in _IN}
    conf, sq = Guarded(max(nl, 0) ** 2, 8, pc.SENT_U64), Guarded(1, 8, pc.SENT_F64)
    img = {k: Guarded(n, 4, pc.SENT_F32 if k.endswith("diff") else pc.SENT_U32) for k in _OPT}
    p = lambda k: None if k in null else img[k].ptr                                   # noqa: E731
    rem = (None, None) if no_rem else (d["src_rem"].data_ptr(), d["tgt_rem"].data_ptr())
    rc = _lib().lt_compare_dev(d["src_label"].data_ptr(), d["src_color"].data_ptr(), d["tgt_label"].data_ptr(),
                               d["src_range"].data_ptr(), d["tgt_range"].data_ptr(), rem[0], rem[1], n, nl, conf.ptr,
                               p("range_diff"), p("rem_diff"), p("src_masked"), p("tgt_masked"), sq.ptr, _stream_ptr(stream))
    assert rc == expect
    _sync(stream)
    out = dict(conf=conf.host().view(np.uint64).reshape((nl, nl) if nl > 0 else (0, 0)), sq_sum=float(sq.host().view(np.float64)[0]))
    out.update({k: img[k].host().view(np.uint32) for k in _OPT})
    return out


def check_compare(got, c, null=(), tag=None):
    tag = tag or c["what"]
    n = len(c["src_label"])
    w = pc.restate_compare_arrays(*[c[k] for k in _IN], n_labels=c["n_labels"])
    assert np.array_equal(got["conf"].astype(np.int64), w["conf"]) and (got["conf"] < 2 ** 62).all(), tag
    want = dict(range_diff=w["range_diff"].view(np.uint32), rem_diff=w["rem_diff"].view(np.uint32),
                src_masked=w["source_label"].view(np.uint32), tgt_masked=w["target_label"].view(np.uint32))
    for k in _OPT:
        if k in null:
            assert (got[k] == (pc.SENT_F32 if k.endswith("diff") else pc.SENT_U32)).all(), (tag, k)
        else:
            assert np.array_equal(got[k], want[k]), (tag, k)
    # non-negative doubles: any order of adding n of them is within (n - 1) * 2^-53 of the exact sum, relative
    assert abs(got["sq_sum"] - w["sq_exact"]) <= n * 2.0 ** -52 * w["sq_exact"], (tag, got["sq_sum"], w["sq_exact"])
    if n <= pc.BLOCK:                                        # one workgroup, one atomic onto zero: the fixed tree, bit for bit
        assert np.float64(got["sq_sum"]).view(np.int64) == np.float64(pc.block_tree_sum(w["range_diff"])).view(np.int64), tag
    return w


@pytest.mark.parametrize("n_labels", pc.COMPARE_NLABELS)
def test_compare_sizes_and_label_tables(n_labels):
    for n in pc.COMPARE_SIZES:
        c = pc.compare_random(n, n_labels)
        check_compare(call_compare(c), c)


@pytest.mark.parametrize("n_labels", [20, 64, 300])
def test_compare_constructed_waves(n_labels):
    import torch
    c = pc.compare_waves(n_labels)
    w = check_compare(call_compare(c), c)
    assert w["conf"][0, 0] == 128 + 192            # the genuine (0, 0) cells and the black ones; no uncounted lane among them
    check_compare(call_compare(c, stream=torch.cuda.Stream()), c, tag=c["what"] + " side stream")
    # every kind of wave alone as well (one workgroup: the sum in its fixed order)
    for b, kind in enumerate(c["kinds"]):
        one = {k: np.asarray(c[k])[b * pc.BLOCK:(b + 1) * pc.BLOCK] for k in _IN}
        one.update(n_labels=n_labels, what=f"{kind} n_labels={n_labels}")
        check_compare(call_compare(one), one)


@pytest.mark.parametrize("case", ["random255", "waves"])
def test_compare_with_optional_outputs_null(case):
    c = pc.compare_random(255, 20, seed=3) if case == "random255" else pc.compare_waves(20)
    full = call_compare(c)
    check_compare(full, c)
    for null in [(k,) for k in _OPT] + [_OPT]:
        got = call_compare(c, null=null)
        check_compare(got, c, null=null, tag=(case, null))
        for k in ("conf",) + tuple(k for k in _OPT if k not in null):
            assert np.array_equal(got[k], full[k]), (case, null, k)
        if case == "random255":
            assert got["sq_sum"] == full["sq_sum"]
    got = call_compare(c, null=("rem_diff",), no_rem=True)            # without remissions when nobody asks for their difference
    check_compare(got, c, null=("rem_diff",), tag=(case, "no remissions"))


def test_compare_arguments():
    c = pc.compare_random(257, 20)
    got = call_compare(c, expect=LT_ERR_INVALID_ARG, no_rem=True)     # rem_diff asked for, remissions missing
    assert b"lt_compare_dev" in _lib().lt_last_error()
    assert (got["conf"] == pc.SENT_U64).all() and (got["rem_diff"] == pc.SENT_F32).all()       # refused before anything ran
    call_compare(dict(c, n_labels=0), expect=LT_ERR_INVALID_ARG)
    call_compare(dict(c, n_labels=-3), expect=LT_ERR_INVALID_ARG)
    empty = {k: np.zeros((0, 3) if k == "src_color" else 0, np.asarray(c[k]).dtype) for k in _IN}
    got = call_compare(dict(empty, n_labels=20))                      # n = 0: the accumulators are zeroed all the same
    assert (got["conf"] == 0).all() and np.float64(got["sq_sum"]).view(np.int64) == 0


if __name__ == "__main__":
    if sys.argv[1:] == ["regrow"]:
        sys.path.insert(0, ROOT)
        _regrow_child()
