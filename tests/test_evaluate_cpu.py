"""The contracts of `lt_source_scan_dev` and `lt_compare_record_dev` (include/lidarhip.h) restated in numpy, and what keeps the
restatements honest without a GPU: the source image against the pinned restatement of the reference's
`do_range_projection` (oracle/projection.py, method "old") on the eight raw scans of golden F17, the record + the shared host
tail `post.confusion_metrics` against the pinned restatement of `compare()` (oracle/compare.py).
tests/test_evaluate_gpu.py compares the kernels with the functions below bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_ingest_cpu as cpu  # noqa: E402
import test_ingest_shapes_cpu as gen  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = (32, 512, 3.0, -25.0)            # golden F17's source sensor
IGNORE = [0, 1]
# make_golden_ingest.COLOR_DICT
COLOR_DICT = {0: [0, 0, 0], 10: [245, 150, 100], 40: [255, 0, 255], 48: [75, 0, 75], 50: [0, 200, 255], 70: [0, 175, 0],
              80: [150, 240, 255], 1: [0, 0, 255], 252: [245, 150, 100], 253: [200, 40, 255]}


def color_lut(color_dict):
    """SemLaserScan.__init__ (laserscan.py:547-555)"""
    lut = np.zeros((max(color_dict) + 1 + 100, 3), np.float32)
    for k, v in color_dict.items():
        lut[k] = np.array(v, np.float32) / 255.0
    return lut


# ---- contract (a): rules 1-5 of lt_source_scan_dev ---------------------------------------------------------------------------
def restate_source(xyzr, label, ignore, H, W, fov_up, fov_down, lut):
    """dict(range, rem, label, black, bad_labels, index).  float32 arithmetic; the transcendental functions are the correctly
    rounded float32 values (float64 evaluation rounded once), as the library computes them."""
    f32 = np.float32
    l = (np.asarray(label, np.uint32) & 0xFFFF).astype(np.int64)                       # rule 1
    bad = int((l >= len(lut)).sum())
    keep = ~np.isin(l, ignore)                                                         # rule 2
    raw_index = np.flatnonzero(keep)
    x, y, z = (np.ascontiguousarray(xyzr[keep, k], f32) for k in range(3))             # rule 3
    fu, fd = fov_up / 180.0 * np.pi, fov_down / 180.0 * np.pi
    afd, fov, pi = f32(abs(fd)), f32(abs(fd) + abs(fu)), f32(np.pi)
    with np.errstate(all="ignore"):
        depth = np.sqrt((x * x + y * y) + z * z)
        yaw = -np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(f32)
        pitch = np.arcsin((z / depth).astype(np.float64)).astype(f32)
        px = f32(0.5) * (yaw / pi + f32(1.0))
        py = f32(1.0) - (pitch + afd) / fov
        ok = (depth != 0) & (py >= 0) & (py <= 1) & ~np.isnan(depth) & ~np.isnan(px) & ~np.isnan(py)
        cx = np.clip(np.floor(px * f32(W)), 0, W - 1)
        cy = np.clip(np.floor(py * f32(H)), 0, H - 1)
    assert depth.dtype == px.dtype == py.dtype == f32
    cell = (cy[ok].astype(np.int64) * W + cx[ok].astype(np.int64))
    d, who = depth[ok], raw_index[ok]
    order = np.lexsort((who, d))                                                       # rule 4: nearest, lowest index
    first = np.unique(cell[order], return_index=True)[1]
    win = order[first]
    index = np.full(H * W, -1, np.int64)
    index[cell[win]] = who[win]
    own = index >= 0
    rng, rem, lab = np.full(H * W, -1, f32), np.full(H * W, -1, f32), np.zeros(H * W, np.int32)
    rng[cell[win]] = d[win]
    rem[own] = np.asarray(xyzr, f32)[index[own], 3]
    lab[own] = l[index[own]]
    col = np.zeros((H * W, 3), np.float64)
    inside = own & (lab < len(lut))
    col[inside] = lut[lab[inside]]
    black = (col.sum(1) == 0).astype(np.uint8)                                          # rule 5
    return dict(range=rng.reshape(H, W), rem=rem.reshape(H, W), label=lab.reshape(H, W), black=black.reshape(H, W),
                bad_labels=bad, index=index.reshape(H, W))


# ---- contract (b): rules 1-3 of lt_compare_record_dev -------------------------------------------------------------------------
def fixed_order_sum(d2):
    """rule 3, in the order the kernels add: 256 cells per workgroup -- a butterfly over the 64 lanes of each wave, the four
    waves as (w0 + w1) + (w2 + w3) -- then thread t of the last kernel adds partials t, t + 256, ... in turn, and a halving
    tree over the 256 threads"""
    v = np.asarray(d2, np.float32).reshape(-1).astype(np.float64)
    nb = (len(v) + 255) // 256
    v = np.concatenate([v, np.zeros(nb * 256 - len(v))]).reshape(nb, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    part = (v[:, 0, 0] + v[:, 1, 0]) + (v[:, 2, 0] + v[:, 3, 0])
    acc = np.zeros(256)
    for b0 in range(0, nb, 256):
        chunk = part[b0:b0 + 256]
        acc[:len(chunk)] += chunk
    for o in (128, 64, 32, 16, 8, 4, 2, 1):
        acc[:o] = acc[:o] + acc[o:2 * o]
    return float(acc[0])


def restate_compare(src_label, src_black, tgt_label, src_range, tgt_range, n_labels=512, max_present=64):
    """dict(status, present, counts [P, P] (target, source), sq_sum, n_cells)"""
    sl, tl = np.array(src_label, np.int64).reshape(-1), np.array(tgt_label, np.int64).reshape(-1)
    black = np.asarray(src_black).reshape(-1) != 0
    sl[black] = 0
    tl[black] = 0
    bg = sl == 0
    tl[bg] = 0
    sr = np.where(bg, np.float32(0), np.asarray(src_range, np.float32).reshape(-1))
    tr = np.where(bg, np.float32(0), np.asarray(tgt_range, np.float32).reshape(-1))
    d = (sr - tr).astype(np.float32)
    out = dict(sq_sum=fixed_order_sum(d * d), n_cells=len(sl), sl=sl, tl=tl, bg=bg)
    if ((sl < 0) | (sl >= n_labels) | (tl < 0) | (tl >= n_labels)).any():
        return dict(out, status=2, present=np.zeros(0, np.int64), counts=np.zeros((0, 0), np.int64))
    present = np.union1d(sl, tl)
    if len(present) > max_present:
        return dict(out, status=1, present=present, counts=np.zeros((0, 0), np.int64))
    counts = np.zeros((len(present), len(present)), np.int64)
    np.add.at(counts, (np.searchsorted(present, tl), np.searchsorted(present, sl)), 1)
    return dict(out, status=0, present=present, counts=counts)


def random_images(seed, H, W, values, agree=0.8):
    rng = np.random.default_rng(seed)
    vals = np.asarray(values, np.int32)
    sl = rng.choice(vals, (H, W)).astype(np.int32)
    tl = np.where(rng.random((H, W)) < agree, sl, rng.choice(vals, (H, W))).astype(np.int32)
    black = (rng.random((H, W)) < 0.1).astype(np.uint8)
    sr, tr = rng.uniform(0, 80, (H, W)).astype(np.float32), rng.uniform(0, 80, (H, W)).astype(np.float32)
    return sl, black, tl, sr, tr


# ---- tests ----------------------------------------------------------------------------------------------------------------
def test_source_restatement_equals_the_pinned_projection_on_the_f17_scans():
    """rules 1-5 against oracle.projection.range_projection(method="old", remove=True) -- the restatement of the reference's
    do_range_projection pinned by goldens F6 / F9 -- on the file bytes of F17: same winner per cell (the oracle numbers the
    KEPT points, rule 4 says the raw index orders them alike), same range bits, remissions, labels; black = the colour sum"""
    from oracle import projection as op
    g = cpu.gold()
    H, W, fu, fd = SOURCE
    lut = color_lut(COLOR_DICT)
    for k, (xyzr, label) in enumerate(cpu.raw_scans(g)):
        got = restate_source(xyzr, label, IGNORE, H, W, fu, fd, lut)
        l = label & 0xFFFF
        keep = ~np.isin(l, IGNORE)
        want = op.range_projection(xyzr[keep, :3], xyzr[keep, 3], H, W, fu, fd, remove=True, method="old")
        kept_raw = np.flatnonzero(keep)[want["kept"]]
        widx = np.where(want["index"] >= 0, kept_raw[np.maximum(want["index"], 0)], -1)
        assert np.array_equal(got["index"], widx), k
        assert np.array_equal(got["range"].view(np.int32), want["range"].view(np.int32)), k
        assert np.array_equal(got["rem"].view(np.int32), want["remission"].view(np.int32)), k
        wl, wc = op.label_projection(want["index"], l[keep][want["kept"]], lut)
        assert np.array_equal(got["label"], wl) and np.array_equal(got["black"] != 0, wc.sum(2) == 0), k
        assert got["bad_labels"] == 0 and (got["index"] >= 0).sum() > 1500 and 0 < got["black"].sum() < H * W
        assert not np.isin(got["label"][got["index"] >= 0], IGNORE).any()


def test_source_restatement_edge_inputs():
    lut = color_lut(COLOR_DICT)
    H, W, fu, fd = 8, 32, 3.0, -25.0
    empty = restate_source(np.zeros((0, 4), np.float32), np.zeros(0, np.uint32), IGNORE, H, W, fu, fd, lut)
    assert (empty["range"] == -1).all() and (empty["rem"] == -1).all() and (empty["label"] == 0).all() and empty["black"].all()
    one = restate_source(np.array([[5, 0, -0.5, 0.25]], np.float32), np.array([(7 << 16) | 40], np.uint32), IGNORE, H, W, fu, fd, lut)
    assert (one["index"] >= 0).sum() == 1 and one["label"].max() == 40 and one["black"].sum() == H * W - 1
    two = restate_source(np.array([[5, 0, -0.5, 0.25], [5, 0, -0.5, 0.75]], np.float32), np.array([40, 50], np.uint32), IGNORE,
                         H, W, fu, fd, lut)
    assert two["label"].max() == 40 and two["rem"].max() == 0.25                      # equal depths: the lower index
    out = restate_source(np.array([[5, 0, -0.5, 0.25]], np.float32), np.array([9999], np.uint32), IGNORE, H, W, fu, fd, lut)
    assert out["bad_labels"] == 1 and out["black"].all() and out["label"].max() == 9999


@pytest.mark.parametrize("seed", range(4))
def test_record_restatement_and_the_shared_tail_equal_the_pinned_compare(seed):
    """`restate_compare` + `post.confusion_metrics` against oracle.compare.compare (pinned to the reference by golden F7):
    m_iou / m_acc / iou within 1e-12, MSE within 1e-6 * MSE + 1e-9 (the reference sums in float32 pairwise)"""
    from lidar_transfer_amd.post import confusion_metrics
    from oracle.compare import compare as ocompare
    H, W = 16, 256
    sl, black, tl, sr, tr = random_images(200 + seed, H, W, [0, 1, 10, 40, 48, 50, 70, 259])
    color = np.where(black[:, :, None] != 0, 0.0, 0.5) * np.ones((H, W, 3))
    want = ocompare(sl, color, tl, sr, tr, sr, tr, nclasses=20)
    r = restate_compare(sl, black, tl, sr, tr)
    assert r["status"] == 0 and int(r["counts"].sum()) == H * W
    final, m_iou, m_acc, iou = confusion_metrics(r["present"], r["counts"], 20)
    assert abs(m_iou - want["m_iou"]) < 1e-12 and abs(m_acc - want["m_acc"]) < 1e-12 and np.allclose(iou, want["iou"], atol=1e-12)
    mse = r["sq_sum"] / r["n_cells"]
    assert abs(mse - float(want["MSE"])) < 1e-6 * float(want["MSE"]) + 1e-9
    assert abs(r["sq_sum"] - float(want["range_diff"].astype(np.float64).sum())) < 1e-9 * r["sq_sum"]


def test_record_restatement_statuses_and_the_tails_index_error():
    from lidar_transfer_amd.post import confusion_metrics
    H, W = 16, 128
    sl, black, tl, sr, tr = random_images(7, H, W, list(range(1, 66)), agree=0.5)
    black[:] = 0
    sl[0, :65] = np.arange(1, 66)                                     # 65 values + nothing else needed
    assert restate_compare(sl, black, tl, sr, tr)["status"] == 1
    sl2 = np.where(sl > 64, 64, sl)
    tl2 = np.where(tl > 64, 64, tl)
    sl2[0, 0] = 0
    r = restate_compare(sl2, black, tl2, sr, tr)                       # 0 .. 64 with the background: 65 again
    assert r["status"] == 1
    tl3 = tl2.copy()
    tl3[3, 3] = 512
    sl3 = np.where(sl2 == 0, 1, sl2)
    assert restate_compare(sl3, black, tl3, sr, tr)["status"] == 2 and restate_compare(sl3, black, -tl3, sr, tr)["status"] == 2
    with pytest.raises(IndexError):
        confusion_metrics(np.arange(30), np.ones((30, 30), np.int64), 20)


def test_header_compiles_as_c_and_the_new_structs_match_their_mirrors(tmp_path):
    from lidar_transfer_amd import _lib
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lidarhip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %d %d %d\\n", sizeof(lt_source_images), sizeof(lt_compare_record),\n'
                   '         offsetof(lt_compare_record, sq_sum), offsetof(lt_compare_record, present),\n'
                   '         offsetof(lt_compare_record, counts), LT_COMPARE_MAX_PRESENT, LT_COMPARE_MAX_NLABELS, LT_ABI_VERSION);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    R = _lib.CompareRecord
    assert got == [ctypes.sizeof(_lib.SourceImages), ctypes.sizeof(R), R.sq_sum.offset, R.present.offset, R.counts.offset,
                   _lib.LT_COMPARE_MAX_PRESENT, _lib.LT_COMPARE_MAX_NLABELS, _lib.LT_ABI_VERSION]
    assert _lib.LT_ABI_VERSION >= 8


def test_new_entry_points_reject_bad_arguments_before_any_device_work():
    import ctypes as C
    from lidar_transfer_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    for bad in (0, 100, 257, 4096):
        assert lib.lt_evaluator_create(C.byref(h), bad, 0) == -1 and b"multiple of 256" in lib.lt_last_error()
    rs, im = _lib.RawScan(None, None, 10), _lib.SourceImages()
    dummy = C.c_void_p(256)   # (never dereferenced: every call below is refused before its first launch)
    assert lib.lt_source_scan_dev(None, C.byref(rs), None, 0, 3.0, -25.0, 8, 8, None, 0, C.byref(im), None) == -1
    assert lib.lt_source_scan_dev(dummy, C.byref(rs), None, 0, 3.0, -25.0, 8, 8, None, 0, C.byref(im), None) == -1   # n = 10, no buffers
    rs.n = 0
    assert lib.lt_source_scan_dev(dummy, C.byref(rs), (C.c_int * 1)(70000), 1, 3.0, -25.0, 8, 8, None, 0, C.byref(im), None) == -1
    assert b"65535" in lib.lt_last_error()
    assert lib.lt_source_scan_dev(dummy, C.byref(rs), None, 0, 3.0, -25.0, 0, 8, None, 0, C.byref(im), None) == -1
    assert lib.lt_compare_record_dev(dummy, dummy, dummy, dummy, dummy, dummy, 0, None, dummy, None) == -1
    assert lib.lt_compare_record_dev(dummy, dummy, None, dummy, dummy, dummy, 64, None, dummy, None) == -1
