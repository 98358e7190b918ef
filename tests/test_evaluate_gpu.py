"""`lt_source_scan_dev` and `lt_compare_record_dev` (csrc/lt_evaluate.hip) against the numpy restatements of their contracts
(tests/test_evaluate_cpu.py, which pins those to the restated reference without a GPU) -- bit for bit: on the eight raw scans
of golden F17, at the deployment shape (a 120 k-point scan into 64 x 2048, 64 x 2048 images with 30 classes; generators of
tests/test_ingest_shapes_cpu.py) and at the edge shapes.  Source images are written into sentinel-filled buffers with guards."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_evaluate_cpu as ev  # noqa: E402
import test_ingest_cpu as cpu  # noqa: E402
import test_ingest_shapes_cpu as gen  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 1024
BIG = (64, 2048, 3.0, -25.0)


def big_lut():
    """360 rows like a color_map whose largest key is 259: seeded colours, classes 0 and 13 black; 65535 lies outside"""
    lut = np.random.default_rng(3).uniform(0.1, 1.0, (360, 3)).astype(np.float32)
    lut[[0, 13]] = 0
    return lut


def call_source(e, xyzr, label, H, W):
    """one lt_source_scan_dev call on sentinel-filled, guarded buffers; returns host images + the guards"""
    import torch
    from lidar_transfer_amd import _lib
    dev = e.device
    n = len(label)
    x = torch.from_numpy(np.ascontiguousarray(xyzr, np.float32).reshape(-1, 4)).to(dev) if n else torch.zeros((1, 4), device=dev)
    l = torch.from_numpy(np.ascontiguousarray(label, np.uint32).view(np.int32)).to(dev) if n else torch.zeros(1, dtype=torch.int32, device=dev)
    cells = H * W
    bufs = dict(range=torch.full((cells + 2 * GUARD,), gen.SENT_F32, dtype=torch.int32, device=dev),
                rem=torch.full((cells + 2 * GUARD,), gen.SENT_F32, dtype=torch.int32, device=dev),
                label=torch.full((cells + 2 * GUARD,), -1515870811, dtype=torch.int32, device=dev),
                black=torch.full((cells + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev),
                bad_labels=torch.full((1 + 2 * GUARD,), -1515870811, dtype=torch.int32, device=dev))
    rs = _lib.RawScan(x.data_ptr() if n else None, l.data_ptr() if n else None, n)
    im = _lib.SourceImages(*[bufs[k].data_ptr() + GUARD * bufs[k].element_size() for k in ("range", "rem", "label", "black", "bad_labels")])
    st = torch.cuda.current_stream(dev)
    rc = e._lib.lt_source_scan_dev(e._h, C.byref(rs), e._ign, len(e.ignore), e.fov_up, e.fov_down, H, W, e.lut.data_ptr(),
                                   int(e.lut.shape[0]), C.byref(im), C.c_void_p(st.cuda_stream))
    assert rc == 0, e._lib.lt_last_error()
    st.synchronize()
    out = {}
    for k, t in bufs.items():
        h = t.cpu().numpy()
        m = 1 if k == "bad_labels" else cells
        out[k] = h[GUARD:GUARD + m]
        assert (h[:GUARD] == h[0]).all() and (h[GUARD + m:] == h[0]).all() and h[0] in (gen.SENT_F32, -1515870811, 0xA5), k   # guards untouched
    return out


def check_source(got, want, H, W, tag):
    assert np.array_equal(got["range"], want["range"].reshape(-1).view(np.int32)), tag
    assert np.array_equal(got["rem"], want["rem"].reshape(-1).view(np.int32)), tag
    assert np.array_equal(got["label"], want["label"].reshape(-1)), tag
    assert np.array_equal(got["black"], want["black"].reshape(-1)), tag
    assert int(got["bad_labels"][0]) == want["bad_labels"], tag


def _evaluator(source, ignore, lut, **kw):
    from lidar_transfer_amd.evaluate import Evaluator
    return Evaluator(source, ignore, lut, **kw)


def test_source_scan_of_the_f17_scans_equals_the_restatement_in_both_class_list_forms():
    g = cpu.gold()
    H, W, fu, fd = ev.SOURCE
    lut = ev.color_lut(ev.COLOR_DICT)
    long_list = [0, 1] + list(range(300, 319)) + [65535, 50]          # 23 entries: the bitmap form; class 50 is in the scans
    for ignore in (ev.IGNORE, long_list):
        with _evaluator(ev.SOURCE, ignore, lut) as e:
            for k, (xyzr, label) in enumerate(cpu.raw_scans(g)):
                want = ev.restate_source(xyzr, label, ignore, H, W, fu, fd, lut)
                check_source(call_source(e, xyzr, label, H, W), want, H, W, (len(ignore), k))
                if ignore is ev.IGNORE:
                    assert (want["index"] >= 0).sum() > 1500          # (not idle: the figure test_evaluate_cpu.py asserts)
    a = ev.restate_source(*cpu.raw_scans(g)[2], ev.IGNORE, H, W, fu, fd, lut)
    b = ev.restate_source(*cpu.raw_scans(g)[2], long_list, H, W, fu, fd, lut)
    assert (a["label"] == 50).any() and not (b["label"] == 50).any()


def test_source_scan_at_the_deployment_shape_and_the_edge_shapes():
    H, W, fu, fd = BIG
    lut = big_lut()
    inp = gen.deployment_input(17)
    xyzr, label = inp["raw"][0]
    assert 110000 <= len(label) <= 130000 and ((label & 0xFFFF) == 65535).any() and ((label >> 16) > 0).all()
    with _evaluator(BIG, gen.IGNORE, lut) as e:
        want = ev.restate_source(xyzr, label, gen.IGNORE, H, W, fu, fd, lut)
        assert want["bad_labels"] > 1000 and (want["index"] >= 0).sum() > 50000       # labels outside the LUT are counted
        check_source(call_source(e, xyzr, label, H, W), want, H, W, "deployment")
        # the same evaluator on other shapes: empty scan, every point dropped, one point, then the big scan again
        z4, z1 = np.zeros((0, 4), np.float32), np.zeros(0, np.uint32)
        check_source(call_source(e, z4, z1, 16, 64), ev.restate_source(z4, z1, gen.IGNORE, 16, 64, fu, fd, lut), 16, 64, "empty")
        dropped = np.where(np.arange(len(label)) % 2 == 0, np.uint32((5 << 16) | 0), np.uint32((9 << 16) | 1))
        w = ev.restate_source(xyzr, dropped, gen.IGNORE, H, W, fu, fd, lut)
        assert (w["index"] < 0).all()
        check_source(call_source(e, xyzr, dropped, H, W), w, H, W, "all dropped")
        p1, l1 = np.array([[5, 0, -0.5, 0.25]], np.float32), np.array([(7 << 16) | 40], np.uint32)
        w = ev.restate_source(p1, l1, gen.IGNORE, H, W, fu, fd, lut)
        assert (w["index"] >= 0).sum() == 1
        check_source(call_source(e, p1, l1, H, W), w, H, W, "one point")
        check_source(call_source(e, xyzr, label, H, W), want, H, W, "deployment again")
    with _evaluator(BIG, gen.IGNORE_LONG, lut) as e:                       # 65535 is ignored here, but counted all the same
        want = ev.restate_source(xyzr, label, gen.IGNORE_LONG, H, W, fu, fd, lut)
        assert want["bad_labels"] > 1000 and not (want["label"] == 65535).any()
        check_source(call_source(e, xyzr, label, H, W), want, H, W, "long list")


def _compare(e, sl, black, tl, sr, tr):
    import torch
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(e.device)   # noqa: E731
    src = dict(label=d(sl), black=d(black), range=d(sr), bad_labels=torch.zeros(1, dtype=torch.int32, device=e.device))
    return e.compare(src, d(tl), d(tr))


def _check_record(rec, want):
    status, present, counts, sq_sum, n_cells, bad = rec.counts()
    assert status == want["status"] and n_cells == want["n_cells"] and bad == 0
    assert np.float64(sq_sum).view(np.int64) == np.float64(want["sq_sum"]).view(np.int64)       # the fixed order, bit for bit
    if status == 0:
        assert np.array_equal(present, want["present"]) and np.array_equal(counts, want["counts"])
    return rec.raw()


@pytest.mark.parametrize("shape", [(16, 256), (64, 2048), (3, 85)])
def test_compare_record_equals_the_restatement_and_the_pinned_compare(shape):
    """present values, compacted counts and sq_sum exactly; m_iou / m_acc within 1e-12 and MSE within 1e-6 * MSE + 1e-9 of
    oracle.compare (the tolerances of tests/test_post_gpu.py for the same quantities); two runs: bit-identical records"""
    from oracle.compare import compare as ocompare
    H, W = shape
    values = np.r_[gen.CLASSES[gen.CLASSES < 512], 300].astype(np.int32) if shape == (64, 2048) else [0, 1, 10, 40, 48, 50, 70, 259]   # 30 classes
    sl, black, tl, sr, tr = ev.random_images(11, H, W, values)
    want = ev.restate_compare(sl, black, tl, sr, tr)
    assert want["status"] == 0 and len(want["present"]) == len(values)
    with _evaluator((H, W, 3.0, -25.0), [], big_lut()) as e:
        first = bytes(_check_record(_compare(e, sl, black, tl, sr, tr), want))
        other = ev.random_images(12, H, W, [0, 5, 300])                            # the workspace is clean after every call
        _check_record(_compare(e, *other), ev.restate_compare(*other))
        rec = _compare(e, sl, black, tl, sr, tr)
        assert bytes(_check_record(rec, want))[:16 + 8 + 4 * 64] == first[:16 + 8 + 4 * 64]
        P = len(values)
        assert bytes(rec.raw())[280:280 + 4 * P * P] == first[280:280 + 4 * P * P]
        m = rec.metrics(300)
    color = np.where(black[:, :, None] != 0, 0.0, 0.5) * np.ones((H, W, 3))
    o = ocompare(sl, color, tl, sr, tr, sr, tr, nclasses=300)
    assert abs(m["m_iou"] - o["m_iou"]) < 1e-12 and abs(m["m_acc"] - o["m_acc"]) < 1e-12 and np.allclose(m["iou"], o["iou"], atol=1e-12)
    assert abs(m["MSE"] - float(o["MSE"])) < 1e-6 * float(o["MSE"]) + 1e-9


def test_compare_record_statuses_and_errors():
    H, W = 16, 128
    sl, black, tl, sr, tr = ev.random_images(7, H, W, list(range(1, 65)), agree=0.5)
    black[:] = 0
    with _evaluator((H, W, 3.0, -25.0), [], big_lut()) as e:
        w64 = ev.restate_compare(sl, black, tl, sr, tr)
        assert w64["status"] == 0 and len(w64["present"]) == 64                     # exactly 64 values: fits
        _check_record(_compare(e, sl, black, tl, sr, tr), w64)
        sl65 = sl.copy()
        sl65[0, 0] = 65
        w65 = ev.restate_compare(sl65, black, tl, sr, tr)
        assert w65["status"] == 1 and len(w65["present"]) == 65
        rec = _compare(e, sl65, black, tl, sr, tr)
        _check_record(rec, w65)
        with pytest.raises(OverflowError):
            rec.metrics(300)
        for bad in (512, -3):
            tlb = tl.copy()
            tlb[3, 3] = bad
            sl1 = sl.copy()
            sl1[3, 3] = 1
            wb = ev.restate_compare(sl1, black, tlb, sr, tr)
            assert wb["status"] == 2
            _check_record(_compare(e, sl1, black, tlb, sr, tr), wb)
        _check_record(_compare(e, sl, black, tl, sr, tr), w64)                     # and the workspace is clean afterwards
        with pytest.raises(IndexError):
            _compare(e, sl, black, tl, sr, tr).metrics(20)                         # 64 classes, nclasses 20 (np_ioueval.py:47)
        with pytest.raises(ValueError):
            _compare(e, sl[:8], black[:8], tl[:8], sr[:8], tr[:8])


def test_source_scan_into_compare_end_to_end_on_an_f17_scan():
    """the two calls chained on one stream as a sequence runner queues them: the source image of scan 3 against itself shifted
    by one column as the target; a label outside the colour table surfaces as IndexError when the record is collected"""
    import torch
    g = cpu.gold()
    H, W, fu, fd = ev.SOURCE
    lut = ev.color_lut(ev.COLOR_DICT)
    xyzr, label = cpu.raw_scans(g)[3]
    w = ev.restate_source(xyzr, label, ev.IGNORE, H, W, fu, fd, lut)
    tl, tr = np.roll(w["label"], 1, axis=1), np.roll(w["range"], 1, axis=1)
    want = ev.restate_compare(w["label"], w["black"], tl, w["range"], tr)
    with _evaluator(ev.SOURCE, ev.IGNORE, lut) as e:
        dx = torch.from_numpy(xyzr.copy()).cuda()
        dl = torch.from_numpy(label.view(np.int32).copy()).cuda()
        src = e.source_scan(dx, dl)
        rec = e.compare(src, torch.from_numpy(tl.copy()).cuda(), torch.from_numpy(tr.copy()).cuda())
        _check_record(rec, want)
        m = rec.metrics(300)
        assert 0 < m["m_iou"] < 1 and m["MSE"] > 0
        lab2 = label.copy()
        lab2[:5] = (3 << 16) | 9999
        src = e.source_scan(dx, torch.from_numpy(lab2.view(np.int32).copy()).cuda())
        rec = e.compare(src, torch.from_numpy(tl.copy()).cuda(), torch.from_numpy(tr.copy()).cuda())
        assert rec.counts()[5] == 5
        with pytest.raises(IndexError):
            rec.metrics(300)
