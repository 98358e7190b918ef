"""The target sensor's noise model on the GPU.  `lt_noise_model_dev` through the C ABI into sentinel-filled buffers
with guards, bit for bit against the numpy restatement of tests/noise_cases.py (pinned without a GPU by
tests/test_noise_model_cpu.py); then the chains -- `DeviceDeform`, `FusionScanPipeline`, `SequenceTransfer`, the CLI -- against
the same call without the model followed by the restatement on its outputs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import beam_cases as bc  # noqa: E402
import mount_common as mc  # noqa: E402
import noise_cases as nc  # noqa: E402
import test_evaluate_cpu as ev  # noqa: E402
import test_ingest_cpu as cpu  # noqa: E402
import test_mount_gpu as tm  # noqa: E402
import test_return_model_gpu as rg  # noqa: E402
import test_sequence_cpu as sq  # noqa: E402

pytestmark = pytest.mark.gpu
LT_OK, LT_ERR_INVALID_ARG = 0, -1
FILL = rg.FILL
IMAGES = ("endpoints", "endcolors", "range", "endrem", "tri")
EXTRA = ("range_error", "state")
TYPES = dict(endpoints=np.float32, endcolors=np.int32, range=np.float32, endrem=np.float32, tri=np.int32, range_error=np.float32,
             state=np.uint8)
ORIGIN = (1.5, -2.25, 0.75)
Buf, _bits = rg.Buf, rg._bits


def _L():
    from lidar_transfer_amd import _lib
    return _lib


def _args(p):
    return _L().NoiseModelArgs(p["range_sigma"], p["range_sigma_rel"], p["range_resolution"], p["remission_sigma"], p["min_range"],
                               p["max_range"], p["remission_levels"], p["seed"])


def call_noise(case, p, scan, nulls=(), label=True, stream=None, model_args=None, n=None, origin=None):
    """one lt_noise_model_dev call on copies of the case's images; returns (rc, dict of the buffers afterwards)"""
    import torch
    L = _L()
    cells = len(case["tri"])
    n = cells if n is None else n
    bufs = {k: Buf(case[k]) for k in IMAGES if k not in nulls}
    if "range_error" not in nulls:
        bufs["range_error"] = Buf(nbytes=4 * cells)
    if "state" not in nulls:
        bufs["state"] = Buf(nbytes=cells)
    a = model_args if model_args is not None else _args(p)
    o = (C.c_float * 3)(*[float(x) for x in (case["origin"] if origin is None else origin)])
    torch.cuda.current_stream().synchronize()           # the buffers are in place before a side stream reads them
    st = stream if stream is not None else torch.cuda.current_stream()
    ptr = lambda k: bufs[k].ptr if k in bufs else None   # noqa: E731
    ret = L.load().lt_noise_model_dev(o, n, C.byref(a), scan, ptr("endpoints"), ptr("endcolors"), ptr("range"), ptr("endrem"),
                                      ptr("tri"), ptr("range_error"), ptr("state"), L.LT_TRACE_LABEL_IMAGE if label else 0,
                                      C.c_void_p(st.cuda_stream))
    st.synchronize()
    return ret, {k: b.host(TYPES[k]) for k, b in bufs.items()}


def check(case, p, scan, tag, nulls=(), label=True, stream=None):
    """the call equals the restatement bit for bit in every image it was given (the guards are checked by Buf.host); returns the
    restatement"""
    ret, got = call_noise(case, p, scan, nulls, label, stream)
    assert ret == LT_OK, (tag, _L().load().lt_last_error())
    opt = {k: (case[k] if k not in nulls else None) for k in ("endrem", "endpoints", "endcolors")}
    want = nc.restate(p, scan, case["origin"], case["tri"], case["range"], **opt)
    for k in EXTRA + IMAGES:
        if k in nulls:
            continue
        bad = np.nonzero(_bits(got[k]).reshape(-1) != _bits(want[k]).reshape(-1))[0]
        assert bad.size == 0, f"{tag}: {k} differs in {bad.size} elements, first at {bad[0]}: {got[k].reshape(-1)[bad[0]]!r} " \
                              f"against {want[k].reshape(-1)[bad[0]]!r}"
    return want


def _busy(**kw):
    """every part of the model on, and a gate that some of scan_case's ranges (0.5 .. 60 m) leave"""
    p = dict(range_sigma=0.05, range_sigma_rel=0.001, range_resolution=0.002, remission_sigma=0.05, remission_levels=256, seed=11,
             min_range=2.0, max_range=55.0)
    p.update(kw)
    return nc.params(**p)


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", nc.SIZES)
def test_every_cell_count_equals_the_restatement(n):
    case = nc.scan_case(n)
    want = check(case, _busy(), 3, f"n={n}")
    if n >= 255:
        assert min(nc.totals(want["state"])) > 0, nc.totals(want["state"])
    check(case, nc.params(range_sigma=0.02, range_sigma_rel=0.0005, range_resolution=0.002, remission_sigma=0.02, remission_levels=256,
                          seed=1, min_range=1.0, max_range=80.0), 3, f"n={n}, the shipped model")


@pytest.mark.parametrize("null", ["endpoints", "endcolors", "endrem", "range_error", "state", "all five"])
def test_every_optional_pointer_may_be_null(null):
    nulls = ("endpoints", "endcolors", "endrem", "range_error", "state") if null == "all five" else (null,)
    check(nc.scan_case(513), _busy(), 6, f"NULL {null}", nulls=nulls)
    check(nc.scan_case(65), _busy(), 6, f"NULL {null}, 65 cells", nulls=nulls)


@pytest.mark.parametrize("label", [True, False])
def test_both_colour_layouts(label):
    case = nc.scan_case(513, label=label)
    assert case["endcolors"].shape == ((513,) if label else (513, 3))
    want = check(case, _busy(), 4, f"label image {label}", label=label)
    lost = want["state"] == 2
    assert lost.sum() > 5 and not want["endcolors"][lost].any()
    assert np.array_equal(want["endcolors"][~lost], case["endcolors"][~lost])


def test_what_is_no_return_keeps_its_bytes_and_a_lost_return_is_the_full_miss():
    case = nc.scan_case(513)
    ret, got = call_noise(case, _busy(), 9)
    assert ret == LT_OK
    tri, rng = case["tri"], case["range"]
    kinds = dict(miss=(tri < 0) & (rng == 0), tri_alone=(tri < 0) & (rng > 0), range_alone=(tri >= 0) & (rng == 0))
    assert all(m.sum() > 10 for m in kinds.values()), {k: int(m.sum()) for k, m in kinds.items()}
    still = kinds["miss"] | kinds["tri_alone"] | kinds["range_alone"]
    assert (got["state"][still] == 0).all() and (got["state"][~still] != 0).all() and (got["range_error"][still] == 0).all()
    for k in IMAGES:
        a, b = got[k].reshape(513, -1), case[k].reshape(513, -1)
        assert np.array_equal(_bits(a[still]), _bits(b[still])), k
    lost = got["state"] == 2
    assert lost.sum() > 5
    assert (got["tri"][lost] == -1).all() and not got["range"][lost].any() and not got["endrem"][lost].any()
    assert not got["endpoints"].reshape(513, 3)[lost].any() and not got["endcolors"][lost].any() and not got["range_error"][lost].any()
    assert (FILL not in got["state"]) and got["state"].max() == 2


def _cells(rng, rem=None, origin=(0.0, 0.0, 0.0)):
    """hand-made returns along +x from ``origin``"""
    rng = np.asarray(rng, np.float32)
    n = len(rng)
    o = np.asarray(origin, np.float32)
    pts = np.tile(o, (n, 1))
    pts[:, 0] += rng
    return dict(endpoints=pts, endcolors=np.full(n, 7, np.int32), range=rng, tri=np.arange(n, dtype=np.int32),
                endrem=np.full(n, 0.5, np.float32) if rem is None else np.asarray(rem, np.float32), origin=o)


def test_a_cell_exactly_at_the_gate_is_kept_and_a_tie_goes_to_even():
    case = _cells([1.25, 1.75, 1.3, 3.0, 7.5])
    # no jitter, a grid of 0.5: 2.5 -> 2, 3.5 -> 4, 2.6 -> 3, and the gate exactly at the reported 1.0 and 7.5
    want = check(case, nc.params(range_resolution=0.5, min_range=1.0, max_range=7.5), 0, "ties and the gate")
    assert want["range"].tolist() == [1.0, 2.0, 1.5, 3.0, 7.5] and want["state"].tolist() == [1] * 5
    assert want["endpoints"][:, 0].tolist() == [1.0, 2.0, 1.5, 3.0, 7.5]
    assert want["range_error"].tolist() == [-0.25, 0.25, np.float32(1.5) - np.float32(1.3), 0.0, 0.0]
    # one float64 step inside and the two cells at the gate go
    want = check(case, nc.params(range_resolution=0.5, min_range=np.nextafter(1.0, 2.0), max_range=np.nextafter(7.5, 0.0)), 0, "a step inside")
    assert want["state"].tolist() == [2, 1, 1, 1, 2]
    # no grid either: r2 = r, and a gate at r itself keeps the cell
    one = _cells([np.float32(12.345)])
    r = float(one["range"][0])
    assert check(one, nc.params(min_range=r, max_range=r), 0, "r at both ends")["state"].tolist() == [1]


def test_a_huge_sigma_loses_every_return_whose_draw_is_negative():
    case = nc.scan_case(257)
    want = check(case, nc.params(range_sigma=1e9, seed=2), 1, "sigma 1e9")
    z = nc.draws(2, 1, np.arange(257))[0]
    ret = (case["tri"] >= 0) & (case["range"] > 0)
    assert (want["state"][ret & (z < 0)] == 2).all() and (want["state"][ret & (z > 0)] == 1).all()
    assert (ret & (z < 0)).sum() > 50 and (ret & (z > 0)).sum() > 50


@pytest.mark.parametrize("levels", [0, 2, 256])
def test_remission_is_clamped_at_both_ends_and_put_on_its_levels(levels):
    rs = np.random.default_rng(8)
    rem = np.concatenate([rs.uniform(0, 0.05, 100), rs.uniform(0.95, 1, 100), rs.uniform(0, 1, 57)]).astype(np.float32)
    case = _cells(rs.uniform(2, 50, 257), rem)
    want = check(case, nc.params(remission_sigma=0.2, remission_levels=levels, seed=4), 2, f"levels {levels}")
    e = want["endrem"]
    assert (e == 0).sum() > 20 and (e == 1).sum() > 20 and e.min() == 0 and e.max() == 1
    if levels == 2:
        assert set(e.tolist()) == {0.0, 1.0}
    if levels:
        assert np.array_equal(e, (np.rint(e.astype(np.float64) * (levels - 1)) / (levels - 1)).astype(np.float32))
    else:
        assert len(set(e.tolist())) > 100
    assert np.array_equal(_bits(want["range"]), _bits(case["range"]))      # (the range draw has sigma 0)


def test_end_points_are_scaled_about_a_non_zero_origin():
    case = nc.scan_case(513, origin=ORIGIN)
    want = check(case, _busy(min_range=0.0, max_range=np.inf), 5, "origin")
    ok = want["state"] == 1
    assert ok.sum() > 300
    o = np.asarray(ORIGIN, np.float64)
    dist = np.linalg.norm(want["endpoints"][ok].astype(np.float64) - o, axis=1)
    # the made-up scan's end points lie at their range from the origin up to float32 rounding; so do the moved ones
    assert np.abs(dist - want["range"][ok]).max() < 2e-5
    before = case["endpoints"][ok].astype(np.float64) - o
    after = want["endpoints"][ok].astype(np.float64) - o
    cosine = (before * after).sum(1) / (np.linalg.norm(before, axis=1) * np.linalg.norm(after, axis=1))
    assert cosine.min() > 1 - 1e-9                                          # along the ray
    about_zero = nc.restate(_busy(min_range=0.0, max_range=np.inf), 5, (0, 0, 0), case["tri"], case["range"], endpoints=case["endpoints"])
    assert not np.array_equal(about_zero["endpoints"], want["endpoints"])


def test_a_model_of_zeros_leaves_range_and_end_points_bit_identical():
    for origin in ((0.0, 0.0, 0.0), ORIGIN):
        case = nc.scan_case(513, origin=origin)
        want = check(case, nc.params(seed=5), 7, "zeros")
        ret = (case["tri"] >= 0) & (case["range"] > 0)
        assert np.array_equal(want["state"], ret.astype(np.uint8)) and not want["range_error"].any()
        for k in ("range", "endpoints", "endrem", "tri", "endcolors"):
            assert np.array_equal(_bits(want[k]), _bits(case[k])), k


def test_two_scans_and_two_seeds_give_different_patterns():
    case = nc.scan_case(513)
    res = {(seed, scan): check(case, _busy(seed=seed), scan, f"seed {seed} scan {scan}") for seed, scan in ((11, 0), (11, 1), (12, 0))}
    ret = (case["tri"] >= 0) & (case["range"] > 0)
    for other in ((11, 1), (12, 0)):
        same = res[11, 0]["range"][ret] == res[other]["range"][ret]
        assert same.mean() < 0.2, (other, float(same.mean()))
        assert not np.array_equal(res[11, 0]["endrem"], res[other]["endrem"])
    again = check(case, _busy(seed=11), 0, "once more")
    assert np.array_equal(_bits(again["range"]), _bits(res[11, 0]["range"]))


def test_a_side_stream():
    import torch
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    check(nc.scan_case(513), _busy(), 12, "side stream", stream=s)


def test_bad_arguments_are_refused_with_a_message_that_names_the_entry():
    L = _L()
    lib = L.load()
    case = nc.scan_case(64)
    ok = nc.params()
    for tag, kw in (("tri", dict(nulls=("tri",))), ("range", dict(nulls=("range",))), ("n", dict(n=-1)),
                    ("origin nan", dict(origin=(0.0, float("nan"), 0.0))), ("origin inf", dict(origin=(float("inf"), 0.0, 0.0)))):
        ret, got = call_noise(case, ok, 0, **kw)
        assert ret == LT_ERR_INVALID_ARG and b"lt_noise_model_dev" in lib.lt_last_error(), tag
        assert (got["state"] == FILL).all(), tag
    nan, inf = float("nan"), float("inf")
    for tag, a in (("sigma < 0", (-1.0, 0, 0, 0, 0, inf, 0, 0)), ("sigma nan", (nan, 0, 0, 0, 0, inf, 0, 0)), ("sigma inf", (inf, 0, 0, 0, 0, inf, 0, 0)),
                   ("rel < 0", (0, -1e-9, 0, 0, 0, inf, 0, 0)), ("rel nan", (0, nan, 0, 0, 0, inf, 0, 0)), ("res < 0", (0, 0, -0.5, 0, 0, inf, 0, 0)),
                   ("res nan", (0, 0, nan, 0, 0, inf, 0, 0)), ("res inf", (0, 0, inf, 0, 0, inf, 0, 0)), ("rem < 0", (0, 0, 0, -0.1, 0, inf, 0, 0)),
                   ("rem nan", (0, 0, 0, nan, 0, inf, 0, 0)), ("min < 0", (0, 0, 0, 0, -1.0, inf, 0, 0)), ("min > max", (0, 0, 0, 0, 5.0, 4.0, 0, 0)),
                   ("min nan", (0, 0, 0, 0, nan, inf, 0, 0)), ("max nan", (0, 0, 0, 0, 0, nan, 0, 0)), ("one level", (0, 0, 0, 0, 0, inf, 1, 0))):
        ret, got = call_noise(case, ok, 0, model_args=L.NoiseModelArgs(*a))
        assert ret == LT_ERR_INVALID_ARG and b"lt_noise_model_dev" in lib.lt_last_error(), tag
        assert (got["state"] == FILL).all() and np.array_equal(_bits(got["range"]), _bits(case["range"])), tag
    b = Buf(case["tri"])
    a = _args(ok)
    o = (C.c_float * 3)(0, 0, 0)
    assert lib.lt_noise_model_dev(None, 64, C.byref(a), 0, None, None, b.ptr, None, b.ptr, None, None, 0, None) == LT_ERR_INVALID_ARG
    assert lib.lt_noise_model_dev(o, 64, None, 0, None, None, b.ptr, None, b.ptr, None, None, 0, None) == LT_ERR_INVALID_ARG
    assert lib.lt_noise_model_dev(o, 0, C.byref(a), 0, None, None, None, None, None, None, None, 0, None) == LT_OK   # no cells


def test_the_wrapper_is_the_entry_point():
    import torch
    from lidar_transfer_amd import post
    from lidar_transfer_amd.config import NoiseModel, ReturnModel
    case = nc.scan_case(513, origin=ORIGIN)
    m, gate = NoiseModel(0.05, 0.001, 0.004, 0.1, 16, 9), ReturnModel(3.0, 50.0)
    out = {k: torch.from_numpy(case[k]).cuda() for k in IMAGES}
    more = post.noise_model(ORIGIN, m, 17, out, gate=gate)
    torch.cuda.synchronize()
    want = nc.restate(nc.params_of(m, gate), 17, ORIGIN, case["tri"], case["range"], case["endrem"], case["endpoints"], case["endcolors"])
    for k in IMAGES:
        assert np.array_equal(_bits(out[k].cpu().numpy()).reshape(-1), _bits(want[k]).reshape(-1)), k
    assert np.array_equal(more["noise_state"].cpu().numpy(), want["state"]) and more["noise_state"].dtype == torch.uint8
    assert np.array_equal(_bits(more["range_error"].cpu().numpy()), _bits(want["range_error"]))
    assert min(nc.totals(want["state"])) > 0
    only = post.noise_model(ORIGIN, m, 17, dict(tri=torch.from_numpy(case["tri"]).cuda(), range=torch.from_numpy(case["range"]).cuda()),
                            gate=gate, range_error=None)
    assert only["range_error"] is None and np.array_equal(only["noise_state"].cpu().numpy(), want["state"])
    with pytest.raises(ValueError):
        post.noise_model(ORIGIN, m, 17, dict(range=out["range"]))
    with pytest.raises(ValueError):
        post.noise_model(ORIGIN, None, 17, out)
    with pytest.raises(ValueError):
        post.noise_model(ORIGIN, m, 17, out, gate=dict(min_range=1.0))


# ---- the chains -----------------------------------------------------------------------------------------------------------------
SEQ_TARGET = rg.SEQ_TARGET
T_EXAMPLE = tm.T_EXAMPLE
#: a model whose every part shows on the F17 sequence's few metres (its scans' ranges: 1 .. 18 m, the middle half 4.5 .. 8 m)
NOISE_BLOCK = dict(range_sigma=0.05, range_sigma_rel=0.002, range_resolution=0.004, remission_sigma=0.05, remission_levels=64, seed=5)
#: a gate close enough to the returns for the jitter to carry some of them over it
GATE_BLOCK = dict(min_range=4.6, max_range=8.0)


def _noise():
    from lidar_transfer_amd.config import NoiseModel
    return NoiseModel(**NOISE_BLOCK)


def _gate():
    from lidar_transfer_amd.config import ReturnModel
    return ReturnModel(**GATE_BLOCK)


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy().copy() for k in ("range", "rem", "label", "endpoints", "endpoints_scene", "tri", "bin", "label_file",
                                                    "range_error", "noise_state", "drop") if k in out}


def _expect(base, model, gate, scan, origin, T=None):
    """the model restated on a result ``base`` made WITHOUT it (with the same return model, if any): the images, range_error,
    state and the bytes write() packs.  The end points are moved in the scene's frame about the ray origin and go into the
    target's frame afterwards (``T``; a miss stays (0, 0, 0))."""
    import oracle_chain as oc
    w = nc.restate(nc.params_of(model, gate), scan, origin, base["tri"], base["range"].reshape(-1), base["rem"].reshape(-1),
                   base["endpoints_scene"], base["label"].reshape(-1))
    w["endpoints_target"] = w["endpoints"] if T is None else mc.to_frame(w["endpoints"], T, w["tri"])
    w["bin"], w["label_file"] = oc.pack_write(w["endpoints_target"], w["endcolors"], w["endrem"])
    return w


def _check_result(got, w, tag):
    pairs = (("range", "range"), ("rem", "endrem"), ("label", "endcolors"), ("tri", "tri"), ("endpoints_scene", "endpoints"),
             ("endpoints", "endpoints_target"), ("range_error", "range_error"), ("noise_state", "state"))
    for gk, wk in pairs:
        assert np.array_equal(_bits(got[gk]).reshape(-1), _bits(w[wk]).reshape(-1)), (tag, gk)
    if "bin" in got:
        assert got["bin"].tobytes() == w["bin"].tobytes(), (tag, "velodyne bytes")
        assert got["label_file"].view(np.uint32).tobytes() == w["label_file"].astype(np.uint32).tobytes(), (tag, "label bytes")


@pytest.fixture
def noise_calls(monkeypatch):
    """counts the calls of ``post.noise_model`` (the one place ``lt_noise_model_dev`` is called from)"""
    from lidar_transfer_amd import post
    calls = []
    real = post.noise_model
    monkeypatch.setattr(post, "noise_model", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("mounted,gated", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("adaption", ["mesh", "mergemesh"])
def test_device_deform_with_a_model_is_the_plain_call_followed_by_the_restatement(adaption, mounted, gated, noise_calls):
    """``gated``: the sensor has a return model too -- the noise runs behind it and a measured range that leaves its gate is
    lost; ``mounted``: the example mounting and the VLP-32C table -- the ranges are jittered about the target's position in the
    scene and the end points go into its frame afterwards.  Two scans each: mergemesh's first has no geometry to assume and is
    rendered twice, the model runs once."""
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    g17, g18, a, target = tm._seq_setup(adaption, [])
    kw = dict(transformation=T_EXAMPLE, t_beam_table=bc.VLP32C) if mounted else {}
    if mounted:
        target = SEQ_TARGET
    model, gate = _noise(), (_gate() if gated else None)
    if gated:
        kw["returns"] = gate
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    indices = [int(x) for x in a.scan_indices(8)[:2]]
    more = lambda idx: dict(scan_index=idx) if gated else {}   # noqa: E731
    mk = lambda **extra: DeviceDeform(ev.SOURCE, target, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=adaption == "mesh",   # noqa: E731
                                      **kw, **extra)
    with mk() as plain:
        base = []
        for idx in indices:
            out = plain.deform(adaption, ing, idx, **more(idx))
            assert "range_error" not in out and "noise_state" not in out
            base.append(_host(out))
        origin, T = plain.origin, (plain.mount[0] if mounted else None)
    assert noise_calls == [] and (np.any(origin) == mounted)
    with mk(noise=model) as dd:
        assert dd.noise == model and dd.returns == gate
        for idx, b in zip(indices, base):
            got = _host(dd.deform(adaption, ing, idx, scan_index=idx))
            w = _expect(b, model, gate, idx, origin, T)
            tag = f"{adaption}/mounted={mounted}/gated={gated}/scan {idx}"
            _check_result(got, w, tag)
            tot = nc.totals(w["state"])
            print(f"\n{tag}: cells per state {tot}, {w['bin'].shape[0]} points written ({b['bin'].shape[0]} without the model), "
                  f"range error RMS {np.sqrt(np.mean(w['range_error'][w['state'] == 1].astype(np.float64) ** 2)):.4f} m")
            assert tot[1] > 500 and tot[0] > 0 and (tot[2] > 0) == gated, tot
            assert not np.array_equal(got["range"], b["range"]) and not np.array_equal(got["endpoints"], b["endpoints"])
            if gated:
                assert not got["endpoints"][w["state"] == 2].any() and w["bin"].shape[0] < b["bin"].shape[0]
                assert np.array_equal(got["drop"], b["drop"])                # (the return model saw the clean scan)
        mm_stats = dict(dd._mm().stats) if adaption == "mergemesh" else None
        with pytest.raises(ValueError, match="scan_index"):
            dd.deform(adaption, ing, indices[0])
    assert noise_calls == [1, 1]                                             # once per output scan, re-run or not
    if mm_stats is not None:
        assert mm_stats["scans"] == 2 and mm_stats["waited"] + mm_stats["rerun"] >= 1, mm_stats
    src.close()


@pytest.mark.parametrize("chains", [1, 3])
def test_fusion_pipeline_with_one_and_three_scans_in_flight_equals_device_deform(chains):
    """six output scans (the sequence's, then again) with scan_index 40 .. 45 through ``submit_mergemesh`` and ``submit_clouds``
    against one DeviceDeform scan after scan, and -- the same clouds under another scan_index -- another pattern"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.pipeline import FusionScanPipeline
    model, gate = _noise(), _gate()
    g17, g18, a, target = tm._seq_setup("mergemesh", [])
    am = sq.approach_for(g18, "mesh")
    src = tm._source(g17)
    rays = create_rays_device(target[2], target[3], target[0], target[1], device=0)
    order = [int(x) for x in a.scan_indices(8)]
    order = (order * 6)[:6]
    keys = ("range", "endrem", "endcolors", "endpoints", "tri", "range_error", "noise_state", "drop")
    host = lambda r: {k: r[k].cpu().numpy().copy() for k in keys}   # noqa: E731
    names = dict(endrem="rem", endcolors="label")
    for adaption, ap, merged in (("mergemesh", a, True), ("mesh", am, False)):
        ing = ScanIngest(src, ap)
        more = dict(fixed_volume=False) if merged else {}
        fov = (target[2], target[3]) if merged else (ev.SOURCE[2], ev.SOURCE[3])
        with FusionScanPipeline(ap.voxel_bounds.copy(), ap.voxel_size, fov[0], fov[1], rays, target[0], chains=chains, device=0,
                                label_image=True, source_hw=ev.SOURCE[:2], returns=gate, noise=model, **more) as pipe:
            assert pipe.noise == model
            submit = pipe.submit_mergemesh if merged else pipe.submit_clouds
            tickets = []
            for k, idx in enumerate(order):
                clouds = ing.prepare(idx, merged=merged)
                torch.cuda.synchronize()
                tickets.append(submit(clouds, inputs_ready=True, scan_index=40 + k))
            got = [host(pipe.wait(t)) for t in tickets]
        with pytest.raises(ValueError, match="scan_index"):
            with FusionScanPipeline(ap.voxel_bounds.copy(), ap.voxel_size, fov[0], fov[1], rays, target[0], chains=1, device=0,
                                    label_image=True, source_hw=ev.SOURCE[:2], noise=model, **more) as pipe:
                (pipe.submit_mergemesh if merged else pipe.submit_clouds)(ing.prepare(order[0], merged=merged), inputs_ready=True)
        with DeviceDeform(ev.SOURCE, target, ap.voxel_bounds.copy(), ap.voxel_size, mesh_volume=not merged, returns=gate,
                          noise=model) as dd:
            for k, idx in enumerate(order):
                s = getattr(dd, adaption)(ing.prepare(idx, merged=merged), pack=False, scan_index=40 + k)
                torch.cuda.synchronize()
                for key in keys:
                    want = s[names.get(key, key)].cpu().numpy()
                    assert np.array_equal(_bits(got[k][key]).reshape(-1), _bits(want).reshape(-1)), (adaption, chains, k, key)
                assert min(nc.totals(got[k]["noise_state"])) > 0
        again = len(set(order))
        if again < 6:
            assert not np.array_equal(got[0]["range"], got[again]["range"]), "the same clouds under another scan_index: another pattern"
    src.close()


def _target_sensor(noise_block, return_block=None, **kw):
    from lidar_transfer_amd.config import load_sensor
    tH, tW, tfu, tfd = SEQ_TARGET
    cfg = dict(name="VLP-32C table with a noise model", fov_up=tfu, fov_down=tfd, beams=tH, angle_res_hor=360.0 / tW, fov_hor=360.0,
               beam_model="table", beam_angles=[float(x) for x in bc.VLP32C])
    if noise_block is not None:
        cfg["noise_model"] = noise_block
    if return_block is not None:
        cfg["return_model"] = return_block
    cfg.update(kw)
    return load_sensor(cfg)


def _run_sequence(a, target, out_dir, chains, offset=0, **kw):
    from lidar_transfer_amd.sequence import SequenceTransfer
    g17, g18 = cpu.gold(), sq.gold18()
    src = tm._source(g17)
    with SequenceTransfer(src, a, ev.SOURCE, target, out_dir=str(out_dir) if out_dir is not None else None, chains=chains,
                          nclasses=int(g18["nclasses"]), **kw) as tr:
        recs = list(tr.run(offset=offset))
        summary, noise = tr.summary, tr.noise
    src.close()
    return recs, summary, noise


def test_a_sequence_writes_the_restated_files_with_one_chain_and_with_three(tmp_path, noise_calls):
    """the mergemesh sequence with a table target, a gate and a noise model: every file is write() of the restatement on the
    plain chain's scan of that FILE index -- the bytes DeviceDeform.mergemesh packs for it too --; the totals and the RMS are
    the restatement's"""
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.sequence import format_noise_totals
    g17, g18, a, _ = tm._seq_setup("mergemesh", [])
    sensor = _target_sensor(NOISE_BLOCK, GATE_BLOCK)
    model, gate = sensor.noise_model(), sensor.return_model()
    r1, s1, n1 = _run_sequence(a, sensor, tmp_path / "c1", 1)
    assert noise_calls == [1] * len(r1) and s1["mm_stats"]["waited"] + s1["mm_stats"]["rerun"] >= 1   # once per scan, re-runs included
    r3, s3, _ = _run_sequence(a, sensor, tmp_path / "c3", 3)
    assert n1 == model == _noise() and s3["chains"] == 3 and len(noise_calls) == 2 * len(r1)
    indices = [r["idx"] for r in r1]
    assert indices == [r["idx"] for r in r3] == [int(x) for x in a.scan_indices(8)] and len(indices) >= 3
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    total, sq_sum = np.zeros(3, np.int64), 0.0
    n_before = len(noise_calls)
    with DeviceDeform(ev.SOURCE, SEQ_TARGET, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=False, t_beam_table=bc.VLP32C,
                      returns=gate) as plain:
        for rec in r1:
            idx = rec["idx"]
            w = _expect(_host(plain.deform("mergemesh", ing, idx, scan_index=idx)), model, gate, idx, (0.0, 0.0, 0.0))
            total += np.array(nc.totals(w["state"]))
            sq_sum += float((w["range_error"].astype(np.float64) ** 2).sum())
            b1, l1 = tm._read(tmp_path / "c1", idx)
            assert b1 == w["bin"].tobytes(), f"scan {idx}: velodyne file"
            assert l1 == w["label_file"].astype(np.uint32).tobytes(), f"scan {idx}: label file"
            assert rec["n_points"] == w["bin"].shape[0]
            assert (b1, l1) == tm._read(tmp_path / "c3", idx), f"scan {idx}: one chain vs three"
    assert len(noise_calls) == n_before
    src.close()
    assert s1["noise_totals"] == s3["noise_totals"] == total.tolist() and min(total) > 0
    assert int(total.sum()) == len(indices) * SEQ_TARGET[0] * SEQ_TARGET[1]
    rms = float(np.sqrt(sq_sum / total[1]))
    assert abs(s1["range_error_rms"] - rms) <= 1e-9 * rms and abs(s3["range_error_rms"] - rms) <= 1e-9 * rms
    # sigma 0.05 + 0.002 r on 1 .. 18 m, a grid of 4 mm, and the gate takes the largest errors near it: a few centimetres
    assert 0.04 < rms < 0.09, rms
    print("\n" + format_noise_totals(s1["noise_totals"], s1["range_error_rms"]))


def test_a_sequence_started_at_an_offset_writes_the_bytes_of_the_run_from_zero(tmp_path):
    """the draws hang on the scan's FILE index, not on its place in the run.  On the ``mesh`` adaption, whose scans do not
    depend on the ones before them (mergemesh's volume bounds are state that a run from an offset starts afresh)."""
    g17, g18 = cpu.gold(), sq.gold18()
    a = sq.approach_for(g18, "mesh")
    sensor = _target_sensor(NOISE_BLOCK)
    r0, _, _ = _run_sequence(a, sensor, tmp_path / "zero", 1)
    k = 2
    rk, _, _ = _run_sequence(a, sensor, tmp_path / "offset", 1, offset=k)
    first = rk[0]["idx"]
    assert first == int(a.scan_indices(8, k)[0]) and first in [r["idx"] for r in r0][1:]
    for rec in rk:
        assert tm._read(tmp_path / "offset", rec["idx"]) == tm._read(tmp_path / "zero", rec["idx"]), rec["idx"]
    plain, _, _ = _run_sequence(a, _target_sensor(None), tmp_path / "plain", 1, offset=k)
    assert tm._read(tmp_path / "plain", first) != tm._read(tmp_path / "offset", first)


@pytest.mark.parametrize("adaption", ["cp", "mesh", "mergemesh"])
def test_without_the_key_and_with_an_all_default_block_nothing_changes(adaption, noise_calls):
    """no new keys, the bytes of the path without ``noise=``, and the wrapper is never called"""
    import torch
    from lidar_transfer_amd.config import NoiseModel
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    g17, g18, a, target = tm._seq_setup(adaption, [])
    sensors = [_target_sensor(None), _target_sensor({}), _target_sensor(dict(NoiseModel.DEFAULTS)),
               _target_sensor(dict(range_sigma=0.0, range_resolution=0, remission_levels=0))]
    assert all(s.noise_model() is None for s in sensors)
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    res = []
    for kw in ({}, dict(noise=None), dict(noise=sensors[1].noise_model()), dict(noise=NoiseModel())):
        bnds = None if adaption == "cp" else a.voxel_bounds.copy()
        with DeviceDeform(ev.SOURCE, target, bnds, a.voxel_size, mesh_volume=adaption == "mesh", **kw) as dd:
            assert dd.noise is None and not dd._noise
            outs = []
            for idx in a.scan_indices(8)[:2]:
                out = dd.deform(adaption, ing, idx)
                torch.cuda.synchronize()
                assert "range_error" not in out and "noise_state" not in out
                outs.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
            res.append(outs)
    for other in res[1:]:
        for x, y in zip(res[0], other):
            tm._same(x, y, adaption)
    assert res[0][0]["bin"].shape[0] > 100
    src.close()
    assert noise_calls == []


def test_sequences_without_the_key_write_the_bytes_they_wrote(tmp_path, noise_calls):
    g17, g18, a, _ = tm._seq_setup("mergemesh", [])
    r0, s0, n0 = _run_sequence(a, _target_sensor(None), tmp_path / "none", 1)
    r1, s1, n1 = _run_sequence(a, _target_sensor({}), tmp_path / "default", 3)
    r2, s2, _ = _run_sequence(a, SEQ_TARGET, tmp_path / "tuple", 1)      # (a plain tuple has no model; nor the table: other bytes)
    assert n0 is None and n1 is None and noise_calls == []
    for s in (s0, s1, s2):
        assert s["noise_totals"] is None and s["range_error_rms"] is None
    for rec in r0:
        assert tm._read(tmp_path / "none", rec["idx"]) == tm._read(tmp_path / "default", rec["idx"])
        assert "range_error" not in rec and "noise_state" not in rec


def test_the_target_view_is_not_noised_so_its_mse_contains_the_noise(noise_calls):
    """``evaluate="target"``: the noisy output against the clean source scan seen through the target -- the same reference
    image as without the key, a larger squared range difference"""
    g17, g18, a, _ = tm._seq_setup("mergemesh", [])
    big = dict(NOISE_BLOCK, range_sigma=1.0)
    clean, _, _ = _run_sequence(a, _target_sensor(None), None, 1, evaluate="target")
    noisy, s, _ = _run_sequence(a, _target_sensor(big), None, 1, evaluate="target")
    assert len(noise_calls) == len(noisy) == len(clean) >= 3 and s["noise_totals"][1] > 0
    for c, n in zip(clean, noisy):
        assert c["n_compared"] == n["n_compared"] > 0                      # the view is the same image
        print(f"\nscan {c['idx']}: MSE_compared {c['MSE_compared']:.4f} without the key, {n['MSE_compared']:.4f} with range_sigma 1")
        # every compared cell that holds a return gains sigma^2 >= 1 m^2 in expectation; the cross term averages out over
        # the thousands of cells of a scan
        assert n["MSE_compared"] > c["MSE_compared"]


def test_cp_with_a_model_raises():
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.sequence import SequenceTransfer
    model = _noise()
    g17, g18, a, target = tm._seq_setup("cp", [])
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    with DeviceDeform(ev.SOURCE, target, None, noise=model) as dd:
        with pytest.raises(ValueError, match="cp renders no ray"):
            dd.deform("cp", ing, int(a.scan_indices(8)[0]))
        with pytest.raises(ValueError, match="cp renders no ray"):
            dd.cp(ing.prepare(int(a.scan_indices(8)[0]), merged=True))
    with pytest.raises(ValueError, match="cp renders no ray"):
        SequenceTransfer(src, a, ev.SOURCE, _target_sensor(NOISE_BLOCK))
    with pytest.raises(ValueError, match="target sensors only"):
        SequenceTransfer(src, sq.approach_for(g18, "mesh"), _target_sensor(NOISE_BLOCK, beam_model="linear"), SEQ_TARGET)
    with pytest.raises(ValueError, match="NoiseModel"):
        DeviceDeform(ev.SOURCE, target, None, noise=NOISE_BLOCK)
    src.close()


def test_the_cli_closes_with_the_cells_per_state_and_the_rms_and_refuses_cp(tmp_path):
    """the shipped file through ``python -m lidar_transfer_amd`` in a child process: the closing line is the summary's, which the
    log carries; ``cp`` ends with a message and status 1 before any device work"""
    import json
    import subprocess
    from lidar_transfer_amd.sequence import format_noise_totals
    shipped = os.path.join(ROOT, "config", "vlp32c_table_noise_1024.yaml")
    data, cfgs, a = rg._write_dataset(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    log = tmp_path / "log.jsonl"
    base = [sys.executable, "-m", "lidar_transfer_amd", "-d", str(data), "-s", "00"]
    res = subprocess.run(base + ["-c", str(cfgs["mergemesh"]), "-t", shipped, "-w", "-p", str(out), "--log", str(log), "--one_scan"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    rows = [json.loads(x) for x in log.read_text().splitlines()]
    summary = rows[-1]["summary"]
    tot, rms = summary["noise_totals"], summary["range_error_rms"]
    assert len(rows) == 2 and sum(tot) == 32 * 1024 and tot[1] > 1000 and sum(summary["return_totals"]) == 32 * 1024
    assert tot[1] + tot[2] == summary["return_totals"][0]                  # what the return model kept is what the noise saw
    assert 0.015 < rms < 0.04, rms                                         # 0.02 + 0.0005 r on a few metres, a grid of 2 mm
    lines = [x for x in res.stdout.splitlines() if x.startswith("Noise:")]
    assert lines == [format_noise_totals(tot, rms)], (lines, tot, rms)
    assert [x for x in res.stdout.splitlines() if x.startswith("Returns:")]
    alone = tmp_path / "noise_alone.yaml"                                  # the shipped file without its return model
    text = open(shipped).read()
    alone.write_text(text[:text.index("return_model:")] + text[text.index("noise_model:"):])
    res = subprocess.run(base + ["-c", str(cfgs["cp"]), "-t", str(alone)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 1 and "cp renders no ray" in res.stdout and "noise_model" in res.stdout
