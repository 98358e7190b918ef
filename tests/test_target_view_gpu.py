"""`lt_target_view_dev` (csrc/lt_evaluate.hip) and the path from it up to the command line.

1. bit for bit against the merged entry points it is defined by: `lt_ingest_scans_dev` of the one scan with `poses[0] = T`,
   then `lt_range_projection_batch_dev` under the model's flags (without T: the torch-side filter and widening), for six
   target models, two image sizes, five point counts and both class-list forms, on guarded buffers;
2. one evaluator through a sequence of shapes, interleaved with `lt_source_scan_dev`;
3. a render fed back as a raw scan sees itself;
4. `SequenceTransfer(evaluate="target")` and `--evaluate target`.
The clouds, the models and the numpy restatement are tests/target_view_cases.py's (held up without a GPU by
tests/test_target_view_cpu.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import beam_az_cases as ac  # noqa: E402
import beam_cases as bc  # noqa: E402
import target_view_cases as tv  # noqa: E402
import test_evaluate_cpu as ev  # noqa: E402
import test_ingest_cpu as cpu  # noqa: E402
import test_sequence_cpu as sq  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = tv.ROOT
GUARD = 1024
SENT = -1515870811                     # 0xA5A5A5A5
SOURCE = (16, 64, 3.0, -25.0)          # the source sensor of the evaluators here: another size and field of view than any target
MODEL_NAMES = ("linear", "table", "table_az", "sector", "sector_table_az", "one_row")


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _evaluator(ignore, **kw):
    from lidar_transfer_amd.evaluate import Evaluator
    return Evaluator(SOURCE, ignore, tv.LUT, **kw)


def view_struct(m):
    """(lt_view_model of a tests/target_view_cases.py model, what keeps its arrays alive)"""
    from lidar_transfer_amd import _lib
    tm = tv.target_model(m).validate(m["H"], m["fov"], "tests")
    sec = tm.sector_rad if tm.sector_rad is not None else (0.0, 0.0)
    az = tm.azimuth_rad
    return _lib.ViewModel(m["fov"][0], m["fov"][1], m["H"], m["W"], tm.proj_flags, tm.rows_ptr,
                          None if az is None else az.ctypes.data_as(C.c_void_p), float(sec[0]), float(sec[1])), tm


def _raw(xyzr, label):
    """(xyzr, label) on the device; an empty scan gets one unused row (its pointers are not passed)"""
    import torch
    if len(label) == 0:
        return torch.zeros((1, 4), device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    return _up(np.ascontiguousarray(xyzr, np.float32)), _up(np.ascontiguousarray(label, np.uint32).view(np.int32))


def call_view(e, m, T, xyzr, label):
    """one lt_target_view_dev call of evaluator `e` into sentinel-filled, guarded buffers: the host images"""
    import torch
    from lidar_transfer_amd import _lib
    n, cells = len(label), m["H"] * m["W"]
    x, l = _raw(xyzr, label)
    bufs = {k: torch.full((c + 2 * GUARD,), s, dtype=dt, device="cuda")
            for k, c, s, dt in (("range", cells, SENT, torch.int32), ("rem", cells, SENT, torch.int32), ("label", cells, SENT, torch.int32),
                                ("black", cells, 0xA5, torch.uint8), ("bad_labels", 1, SENT, torch.int32))}
    rs = _lib.RawScan(x.data_ptr() if n else None, l.data_ptr() if n else None, n)
    im = _lib.SourceImages(*[bufs[k].data_ptr() + GUARD * bufs[k].element_size() for k in ("range", "rem", "label", "black", "bad_labels")])
    vm, keep = view_struct(m)
    Th = None if T is None else np.ascontiguousarray(T, np.float64).reshape(16)
    st = torch.cuda.current_stream()
    rc = e._lib.lt_target_view_dev(e._h, C.byref(rs), e._ign, len(e.ignore), None if Th is None else Th.ctypes.data_as(C.POINTER(C.c_double)),
                                   C.byref(vm), e.lut.data_ptr(), int(e.lut.shape[0]), C.byref(im), C.c_void_p(st.cuda_stream))
    assert rc == 0, e._lib.lt_last_error()
    st.synchronize()
    out = {}
    for k, t in bufs.items():
        h = t.cpu().numpy()
        c = 1 if k == "bad_labels" else cells
        assert (h[:GUARD] == h[0]).all() and (h[GUARD + c:] == h[0]).all() and h[0] in (SENT, 0xA5), f"guard of {k}"
        out[k] = h[GUARD:GUARD + c]
    H, W = m["H"], m["W"]
    return dict(range=out["range"].view(np.float32).reshape(H, W), rem=out["rem"].view(np.float32).reshape(H, W),
                label=out["label"].reshape(H, W), black=out["black"].reshape(H, W), bad_labels=int(out["bad_labels"][0]))


def oracle_images(pj, m, T, xyzr, label, ignore):
    """the merged entry points: ingest of the one scan with poses[0] = T (no `back`, no `moving`) -- without T the torch-side
    filter and widening -- then the batched projection under the model's flags, without beam angles"""
    import torch
    from lidar_transfer_amd import _lib
    n = len(label)
    if n == 0:
        cloud = (torch.zeros((0, 3), dtype=torch.float64, device="cuda"), torch.zeros(0, device="cuda"),
                 torch.zeros(0, dtype=torch.int32, device="cuda"))
    elif T is None:
        x, l = _raw(xyzr, label)
        l = l & 0xFFFF
        keep = ~torch.isin(l, torch.tensor(ignore, dtype=torch.int32, device="cuda"))
        cloud = (x[keep, :3].to(torch.float64).contiguous(), x[keep, 3].contiguous(), l[keep].contiguous())
    else:
        x, l = _raw(xyzr, label)
        lib = _lib.load()
        pts, rem, lab = (torch.empty((n, 3), dtype=torch.float64, device="cuda"), torch.empty(n, device="cuda"),
                         torch.empty(n, dtype=torch.int32, device="cuda"))
        n_kept = torch.empty(2, dtype=torch.int32, device="cuda")
        work = torch.empty(_lib.ingest_work_ints(n, 1), dtype=torch.int32, device="cuda")
        rs = (_lib.RawScan * 1)(_lib.RawScan(x.data_ptr(), l.data_ptr(), n))
        io = (_lib.IngestOut * 1)(_lib.IngestOut(pts.data_ptr(), rem.data_ptr(), lab.data_ptr()))
        pose = np.ascontiguousarray(T, np.float64).reshape(1, 16)
        ign = (C.c_int * max(len(ignore), 1))(*ignore)
        _lib.check(lib.lt_ingest_scans_dev(1, rs, pose.ctypes.data_as(C.POINTER(C.c_double)), None, ign, len(ignore), None, 0,
                                           _lib.LT_INGEST_MERGED, io, C.c_void_p(n_kept.data_ptr()), C.c_void_p(work.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lt_ingest_scans_dev")
        cloud = (pts, rem, lab)      # (behind the kept points: depth-0 points, which the projection removes)
    o = pj.project([cloud], m["fov"][0], m["fov"][1], m["H"], m["W"], new=True, remove=True, outputs=("range", "rem", "label", "idx"),
                   beam_table=m["table"], sector=m["sector"], beam_azimuth=m["az"])[0]
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def check_view(got, want, xyzr, label, tag):
    has = want["idx"] >= 0
    assert np.array_equal(got["range"] != -1, has), tag                         # empty in one iff empty in the other
    for k in ("range", "rem"):
        assert np.array_equal(got[k][has].view(np.int32), want[k][has].view(np.int32)), (tag, k)
        assert (got[k][~has] == -1).all(), (tag, k)
    assert np.array_equal(got["label"][has], want["label"][has]) and (got["label"][~has] == 0).all(), tag
    lab = got["label"]
    colour = np.where((lab < len(tv.LUT))[..., None], tv.LUT[np.minimum(lab, len(tv.LUT) - 1)], 0).astype(np.float64)
    assert np.array_equal(got["black"] != 0, ~has | (colour.sum(2) == 0)), tag
    assert got["bad_labels"] == int(((np.asarray(label, np.uint32) & 0xFFFF) >= len(tv.LUT)).sum()), tag
    return int(has.sum())


# ---- 1: bit for bit against the merged entry points ---------------------------------------------------------------------------
@pytest.mark.parametrize("mounted", (False, True))
@pytest.mark.parametrize("name", MODEL_NAMES)
def test_view_equals_ingest_and_projection_bit_for_bit(name, mounted):
    from lidar_transfer_amd.laserscan import Projector
    T = tv.mounting() if mounted else None
    pj = Projector()
    filled = {}
    for ignore in (tv.IGNORE_SHORT, tv.IGNORE_LONG):
        with _evaluator(ignore) as e:
            for H, W in tv.SIZES:
                m = tv.models(H, W)[name]
                for n in tv.COUNTS:
                    xyzr, label = tv.cloud(n, 100 + n + 7 * mounted, m["sector"])
                    tag = (name, mounted, H, W, n, len(ignore))
                    want = oracle_images(pj, m, T, xyzr, label, ignore)
                    got = call_view(e, m, T, xyzr, label)
                    filled[tag] = check_view(got, want, xyzr, label, tag)
    pj.close()
    for (H, W), floor in zip(tv.SIZES, (8, 400)):
        if name != "one_row":
            assert all(v >= floor for k, v in filled.items() if k[2:5] == (H, W, 5000)), filled


# ---- 2: one evaluator, many calls -----------------------------------------------------------------------------------------------
def test_one_evaluator_through_shapes_models_and_source_scans_equals_fresh_evaluators():
    """4 x 8, 32 x 171, 4 x 8 again (re-armed keys, grown workspace, the model uploaded only when it changed), every model,
    source scans in between; every result equals that of a fresh evaluator, two equal calls give equal bits"""
    T = tv.mounting()
    steps = [((4, 8), "sector_table_az", True, 257), ((32, 171), "table_az", False, 5000), ((32, 171), "table_az", False, 5000),
             ((4, 8), "sector_table_az", True, 257), ((4, 8), "linear", False, 255), ((32, 171), "sector", True, 5000),
             ((32, 171), "table", True, 5000), ((4, 8), "one_row", False, 257), ((4, 8), "sector_table_az", True, 257)]
    same = lambda a, b: all(np.array_equal(np.asarray(a[k]).view(np.uint8) if isinstance(a[k], np.ndarray) else a[k],   # noqa: E731
                                           np.asarray(b[k]).view(np.uint8) if isinstance(b[k], np.ndarray) else b[k]) for k in a)
    sx, sl = tv.cloud(3000, 77, None)
    H0, W0, fu0, fd0 = SOURCE
    want_src = ev.restate_source(sx, sl, tv.IGNORE_SHORT, H0, W0, fu0, fd0, tv.LUT)
    import torch
    with _evaluator(tv.IGNORE_SHORT) as e:
        prev = None
        for k, ((H, W), name, mounted, n) in enumerate(steps):
            Tk = T if mounted else None
            m = tv.models(H, W)[name]
            xyzr, label = tv.cloud(n, 300 + n, m["sector"])
            got = call_view(e, m, Tk, xyzr, label)
            with _evaluator(tv.IGNORE_SHORT) as fresh:
                assert same(got, call_view(fresh, m, Tk, xyzr, label)), (k, name)
            if prev is not None and steps[k - 1] == steps[k]:
                assert same(got, prev), k
            prev = got
            src = e.source_scan(*_raw(sx, sl))                                    # the keys are shared with the source scan
            torch.cuda.synchronize()
            for key in ("range", "rem", "label", "black"):
                assert np.array_equal(src[key].cpu().numpy().view(np.uint8), want_src[key].view(np.uint8)), (k, key)
            assert int(src["bad_labels"][0]) == want_src["bad_labels"]


# ---- 3: a render sees itself ------------------------------------------------------------------------------------------------------
R_LUT = np.zeros((354, 3), np.float32)
R_LUT[[40, 50, 80]] = [[1.0, 0.0, 1.0], [0.0, 0.8, 1.0], [0.6, 0.9, 1.0]]        # cars (10) are a black class
R_IGNORE = [0, 1, 80]                                                              # poles are removed


@pytest.mark.parametrize("mounted", (False, True))
def test_a_render_fed_back_as_a_raw_scan_sees_itself(mounted):
    """The scene of tests/test_sector_cpu.py (50 000 triangles) rendered by a sector + table + offsets target at 32 x 171; the
    hits between 0.5 m and 20 m -- where 1e-4 m is the round-trip bound of DESIGN 7c / 7d -- go back in as a raw scan, in the
    SOURCE frame, with their labels and remissions.  Every such cell whose label is kept and not black holds its own label
    and its range within 1e-4 m; a cell of the black class holds its label under black = 1 (rule 6), which compare() treats
    as background like an empty cell; every other cell is empty.  The compare record of the render against its own view has
    counts on the diagonal only, m_iou = m_acc = 1, and n_compared is the number of those cells."""
    import torch
    import mount_common as mc
    import test_sector_cpu as stc
    from lidar_transfer_amd.evaluate import Evaluator
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.raytracer import RaySet, Scene
    from lidar_transfer_amd.synth import synth_scene
    H, W = 32, 171
    m = tv.models(H, W)["sector_table_az"]
    T = tv.mounting() if mounted else None
    P = np.linalg.inv(T) if mounted else None
    scn = Scene(0)
    scn.set_mesh(*[_up(x) for x in synth_scene(stc.RENDER_SEED, stc.RENDER_TRIS)])
    rays = create_rays_device(m["fov"][0], m["fov"][1], H, W, rot=P[:3, :3] if mounted else None, beam_table=m["table"],
                              sector=m["sector"], beam_azimuth=m["az"])
    tm = tv.target_model(m)
    rs = RaySet(rays, H, pose=P, grid=tm.grid(W), beam_table=m["table"], sector=m["sector"], beam_azimuth=m["az"])
    out = scn.render(rs, mc.origin_of(P) if mounted else (0.0, 0.0, 0.0), label_image=True)
    torch.cuda.synchronize()
    scn.status()
    tri, rng = out["tri"].cpu().numpy(), out["range"].cpu().numpy()
    lab, rem, end = out["endcolors"].cpu().numpy(), out["endrem"].cpu().numpy(), out["endpoints"].cpu().numpy()
    fed = (tri >= 0) & (rng <= 20.0)                                            # the hits that go back in
    assert fed.sum() > H * W // 4 and (rng[fed] >= 0.5).all() and (rng[fed] <= 20.0).all()
    xyzr = np.concatenate([end[fed], rem[fed, None]], 1).astype(np.float32)    # the SOURCE frame: as rendered
    label = lab[fed].astype(np.uint32) | np.uint32(5 << 16)
    with Evaluator(SOURCE, R_IGNORE, R_LUT, target=(H, W) + m["fov"], target_model=tm, transformation=T) as e:
        view = e.target_view(*_raw(xyzr, label))
        rec = e.compare(view, out["endcolors"].view(H, W), out["range"].view(H, W))
        got = {k: view[k].cpu().numpy().reshape(-1) for k in ("range", "rem", "label", "black")}
        assert int(view["bad_labels"][0]) == 0
        metrics = rec.metrics(20, compared=True)
        status, present, counts, _, n_cells, _ = rec.counts()
    kept = fed & ~np.isin(lab, R_IGNORE)
    black = kept & (R_LUT[np.clip(lab, 0, 353)].sum(1) == 0)
    seen = kept & ~black
    assert seen.sum() > H * W // 8 and black.sum() > 0 and (fed & ~kept).sum() > 0   # (the fixture holds all three kinds)
    for sel, b in ((seen, 0), (black, 1)):                                      # no cell is left out
        assert np.array_equal(got["label"][sel], lab[sel]) and (got["black"][sel] == b).all(), mounted
        assert np.array_equal(got["rem"][sel], rem[sel]), mounted
        err = np.abs(got["range"][sel].astype(np.float64) - rng[sel])
        print(f"\nrender sees itself (mounted: {mounted}, black: {b}): {int(sel.sum())} cells, largest range error {err.max():.3e} m")
        assert err.max() <= 1e-4, mounted
    rest = ~kept
    assert (got["range"][rest] == -1).all() and (got["rem"][rest] == -1).all() and (got["label"][rest] == 0).all() \
        and (got["black"][rest] == 1).all(), mounted
    assert status == 0 and n_cells == H * W and np.array_equal(counts, np.diag(np.diag(counts))), (present, counts)
    assert metrics["m_iou"] == 1.0 and metrics["m_acc"] == 1.0
    assert metrics["n_compared"] == int(seen.sum())
    assert metrics["MSE_compared"] <= 1e-8 and metrics["MSE"] <= metrics["MSE_compared"]
    rs.close()
    scn.close()


# ---- 4: the sequence and the command line -----------------------------------------------------------------------------------------
SEQ_TARGET = (32, 171, bc.VLP32C_FOV[0], bc.VLP32C_FOV[1])
SEQ_AZ = ac.offsets("mixed", 32)


def _target_sensor():
    from lidar_transfer_amd.config import load_sensor
    tH, tW, tfu, tfd = SEQ_TARGET
    return load_sensor(dict(name="VLP-32C table with offsets", fov_up=tfu, fov_down=tfd, beams=tH, angle_res_hor=360.0 / tW,
                            fov_hor=360.0, beam_model="table", beam_angles=[float(x) for x in bc.VLP32C],
                            beam_azimuth_offsets=[float(x) for x in SEQ_AZ]))


def _seq_setup(many_labels=False):
    """the F17 sequence, F18's mergemesh approach with the example mounting; `many_labels`: the scans' kept labels spread over
    70 values of the colour table, more than a compare record holds"""
    g17, g18 = cpu.gold(), sq.gold18()
    a = sq.approach_for(g18, "mergemesh")
    a.transformation = [float(x) for x in tv.mounting().reshape(-1)]
    raw = cpu.raw_scans(g17)
    if many_labels:
        a.color_map = {**ev.COLOR_DICT, **{k: [k, 50, 200] for k in range(100, 170)}}                    # none of them black
        spread = []
        for x, l in raw:
            low = l & 0xFFFF
            moved = np.where(np.isin(low, list(a.ignore) + list(a.moving)), low, 100 + (np.arange(len(l)) % 70)).astype(np.uint32)
            spread.append((x, moved))
        raw = spread
    return g17, g18, a, raw


def _source(g17, raw):
    from lidar_transfer_amd.ingest import SequenceSource
    return SequenceSource(scans=[x for x, _ in raw], labels=[l for _, l in raw], poses=g17["poses"])


def _run(a, raw, g17, out_dir, chains, evaluate, nclasses, indices=None):
    from lidar_transfer_amd.sequence import SequenceTransfer
    src = _source(g17, raw)
    with SequenceTransfer(src, a, ev.SOURCE, _target_sensor(), out_dir=None if out_dir is None else str(out_dir), chains=chains,
                          nclasses=nclasses, evaluate=evaluate) as tr:
        recs = list(tr.run())
        info = dict(evaluate=tr.evaluate, mode=tr.evaluate_mode, mounted=tr.mounted, beam_model=tr.beam_model)
    src.close()
    return recs, info


def _hand_loop(a, raw, g17, nclasses, n_scans):
    """the same scans from the public calls: DeviceDeform.mergemesh, Evaluator.target_view, post.compare on host copies"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.evaluate import Evaluator
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.post import compare
    t = _target_sensor()
    m = t.target_model()
    src = _source(g17, raw)
    ing = ScanIngest(src, a)
    outs = []
    with DeviceDeform(ev.SOURCE, SEQ_TARGET, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=False, transformation=a.mount(),
                      t_beam_table=m.beam_table, t_beam_azimuth=m.beam_azimuth) as dd, \
            Evaluator(ev.SOURCE, a.ignore, a.color_lut(), target=SEQ_TARGET, target_model=m, transformation=a.mount()) as e:
        for idx in a.scan_indices(len(src))[:n_scans]:
            out = dd.deform("mergemesh", ing, idx)
            view = e.target_view(*src.raw(idx))
            torch.cuda.synchronize()
            h = {k: view[k].cpu().numpy() for k in ("range", "rem", "label", "black")}
            color = np.where(h["black"][:, :, None] != 0, 0.0, 1.0) * np.ones((1, 1, 3))
            tl, tr_ = out["label"].cpu().numpy(), out["range"].cpu().numpy()
            c = compare(h["label"], color, tl, h["range"], tr_, h["rem"], out["rem"].cpu().numpy(), nclasses)
            c["n_compared"] = int(((h["black"] == 0) & (h["label"] != 0)).sum())
            c["labels_present"] = len(np.union1d(np.unique(h["label"]), np.unique(tl)))
            outs.append(c)
    src.close()
    return outs


def _close(rec, want, tag):
    assert abs(rec["m_iou"] - want["m_iou"]) < 1e-12 and abs(rec["m_acc"] - want["m_acc"]) < 1e-12, tag
    assert np.allclose(rec["iou"], want["iou"], atol=1e-12), tag
    assert abs(rec["MSE"] - want["MSE"]) <= 1e-9 * want["MSE"] + 1e-12, tag       # (float64 sums in two orders)
    assert rec["n_compared"] == want["n_compared"] > 0, tag
    sq_sum = float(want["range_diff"].astype(np.float64).sum())
    assert abs(rec["MSE_compared"] - sq_sum / want["n_compared"]) <= 1e-9 * sq_sum / want["n_compared"] + 1e-12, tag


def test_sequence_with_a_mounted_table_target_evaluates_through_the_target_view(tmp_path):
    from lidar_transfer_amd.sequence import SequenceTransfer
    g17, g18, a, raw = _seq_setup()
    nc = int(g18["nclasses"])
    r1, i1 = _run(a, raw, g17, tmp_path / "c1", 1, "target", nc)
    r2, i2 = _run(a, raw, g17, tmp_path / "c2", 2, "target", nc)
    r0, i0 = _run(a, raw, g17, tmp_path / "off", 1, False, nc)
    rn, i_none = _run(a, raw, g17, None, 1, None, nc)
    assert i1 == dict(evaluate=True, mode="target", mounted=True, beam_model="table") and i2["mode"] == "target"
    assert i0["evaluate"] is False and i0["mode"] is None and i_none["evaluate"] is False and i_none["mode"] is None
    want = _hand_loop(a, raw, g17, nc, len(r1))
    assert len(r1) == len(r2) == len(r0) == len(want) >= 3
    from lidar_transfer_amd.sequence import output_paths
    for x, y, z, n, w in zip(r1, r2, r0, rn, want):
        idx = x["idx"]
        for k in ("idx", "n_points", "m_iou", "m_acc", "MSE", "n_compared", "MSE_compared"):
            assert x[k] == y[k], (idx, k)                                          # one chain and two: the same bits
        assert np.array_equal(x["iou"], y["iou"])
        _close(x, w, idx)
        assert 0.0 < x["m_iou"] <= 1.0 and x["n_compared"] < SEQ_TARGET[0] * SEQ_TARGET[1]
        for r in (z, n):                                                            # off, and None for such a target: as before
            assert r["m_iou"] is None and r["MSE"] is None and "n_compared" not in r
        for d in ("c1", "c2"):                                                      # the files do not know about the evaluation
            for p, q in zip(output_paths(str(tmp_path / d), "00", idx), output_paths(str(tmp_path / "off"), "00", idx)):
                assert open(p, "rb").read() == open(q, "rb").read() and os.path.getsize(p) > 1000, (d, idx)
    src = _source(g17, raw)
    try:
        with pytest.raises(ValueError, match="mounted|size"):
            SequenceTransfer(src, a, ev.SOURCE, _target_sensor(), evaluate=True)
        with pytest.raises(ValueError, match="evaluate"):
            SequenceTransfer(src, a, ev.SOURCE, _target_sensor(), evaluate="source")
    finally:
        src.close()


def test_a_scan_with_more_label_values_than_a_record_holds_takes_the_fallback_and_agrees():
    g17, g18, a, raw = _seq_setup(many_labels=True)
    nc = len(a.color_map) + 70
    a.batch_interval = 4                                                            # two output scans are enough
    recs, info = _run(a, raw, g17, None, 1, "target", nc)
    want = _hand_loop(a, raw, g17, nc, len(recs))
    assert info["mode"] == "target" and 1 <= len(recs) <= 3
    for r, w in zip(recs, want):
        assert w["labels_present"] > 64, w["labels_present"]                        # the record overflowed
        _close(r, w, r["idx"])


def test_cli_with_evaluate_target_prints_the_three_lines_and_logs_the_keys(tmp_path):
    g17, g18, a, raw = _seq_setup()
    data = tmp_path / "data"
    seq = data / "sequences" / "00"
    (seq / "velodyne").mkdir(parents=True)
    (seq / "labels").mkdir()
    for k, (xyzr, lab) in enumerate(raw):
        xyzr.tofile(seq / "velodyne" / f"{k:06d}.bin")
        lab.tofile(seq / "labels" / f"{k:06d}.label")
    g17["calib_txt"].tofile(seq / "calib.txt")
    g17["poses_txt"].tofile(seq / "poses.txt")
    H, W, fu, fd = ev.SOURCE
    (data / "config.yaml").write_text(f"name: src\nfov_up: {fu}\nfov_down: {fd}\nbeams: {H}\nangle_res_hor: {360.0 / W!r}\nfov_hor: 360.0\n")
    cm = "\n".join(f"  {k}: {list(v)}" for k, v in ev.COLOR_DICT.items())
    cfg = tmp_path / "approach.yaml"
    cfg.write_text(f"adaption: mergemesh\npreserve_float: false\nnumber_of_scans: {a.number_of_scans}\n"
                   f"batch_interval: {a.batch_interval}\nvoxel_size: {a.voxel_size!r}\n"
                   f"voxel_bounds: {[float(x) for x in np.asarray(a.voxel_bounds).reshape(-1)]}\n"
                   f"transformation: {[float(x) for x in a.transformation]}\nignore: {a.ignore}\nmoving: {a.moving}\ncolor_map:\n{cm}\n")
    target = os.path.join(ROOT, "config", "vlp32c_table_az_1024.yaml")
    runs = {}
    for name, more in (("target", ["--evaluate", "target"]), ("auto", ["--one_scan"]), ("off", ["--one_scan", "--evaluate", "off"])):
        log = tmp_path / f"{name}.jsonl"
        res = subprocess.run([sys.executable, "-m", "lidar_transfer_amd", "-d", str(data), "-c", str(cfg), "-s", "00", "-t", target,
                              "--log", str(log)] + more, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-3000:]
        runs[name] = (res.stdout, [json.loads(x) for x in log.read_text().splitlines()])
    so, rows = runs["target"]
    vals = {k: [float(line.split(":", 1)[1]) for line in so.splitlines() if line.startswith(k + ": ")] for k in ("IoU", "Acc", "MSE")}
    scans = rows[:-1]
    assert len(scans) >= 3 and all(len(v) == len(scans) for v in vals.values())
    for k, r in enumerate(scans):
        assert r["evaluate"] == "target" and r["mounted"] is True and r["beam_model"] == "table" and r["beam_azimuth"] is True
        assert vals["IoU"][k] == r["m_iou"] and vals["Acc"][k] == r["m_acc"] and vals["MSE"][k] == r["MSE"]
        assert 0 < r["n_compared"] < 32 * 1024 and r["MSE_compared"] >= r["MSE"] and 0.0 < r["m_iou"] <= 1.0
    for name in ("auto", "off"):                                                    # without the flag: what it was
        so, rows = runs[name]
        assert "IoU:" not in so and "Acc:" not in so and "MSE:" not in so
        assert all(r["m_iou"] is None and "evaluate" not in r and "n_compared" not in r for r in rows[:-1])
    assert runs["auto"][0] == runs["off"][0] and runs["auto"][1] == runs["off"][1]
