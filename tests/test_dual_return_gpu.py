"""Dual-return target sensors on the GPU.  `lt_echo_resolve_dual_dev` through the C ABI into sentinel-filled
buffers with guards, bit for bit against the numpy restatement of tests/dual_return_cases.py (pinned without a GPU by
tests/test_dual_return_cpu.py) and, for its primary set, against `lt_echo_resolve_dev` itself; a plate in front of a wall end
to end; then the chains -- `DeviceDeform`, `FusionScanPipeline`, `SequenceTransfer`, the CLI -- whose primary results and
leading file bytes are those of the same chain WITHOUT the block and whose second return is the restatement chain: dual
resolve, return and noise models with the xor-ed seed, frame change, packing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import beam_cases as bc  # noqa: E402
import dual_return_cases as dc  # noqa: E402
import echo_cases as ec  # noqa: E402
import mount_common as mc  # noqa: E402
import noise_cases as nc  # noqa: E402
import return_cases as rc  # noqa: E402
import test_echo_model_gpu as eg  # noqa: E402
import test_evaluate_cpu as ev  # noqa: E402
import test_ingest_cpu as cpu  # noqa: E402
import test_mount_gpu as tm  # noqa: E402
import test_return_model_gpu as rg  # noqa: E402
import test_sequence_cpu as sq  # noqa: E402

pytestmark = pytest.mark.gpu
LT_OK, LT_ERR_INVALID_ARG = 0, -1
FILL, Buf, _bits, _same_bits = rg.FILL, rg.Buf, rg._bits, eg._same_bits
OUT1 = eg.OUT                                                       # the primary set, n_echoes included
OUT2 = tuple(k + "2" for k in dc.KEYS)                             # endpoints2 .. fraction2
TYPES = dict(eg.TYPES, **{k + "2": eg.TYPES[k] for k in dc.KEYS})
WIDTH = dict(eg.WIDTH, **{k + "2": eg.WIDTH[k] for k in dc.KEYS})
ORIGIN = eg.ORIGIN
XOR = dc.SECOND_SEED_XOR


def _L():
    from lidar_transfer_amd import _lib
    return _lib


# ---- lt_echo_resolve_dual_dev ------------------------------------------------------------------------------------------------
def call_dual(case, p, second, nulls=(), stream=None, model_args=None, n=None):
    """one lt_echo_resolve_dual_dev call on the case's sub-images; returns (rc, dict of ALL output buffers afterwards, each
    read whole between its guards)"""
    import torch
    cells = case["rays"].shape[0]
    n = cells if n is None else n
    ins = {k: Buf(case[k]) for k in ("rays",) + eg.SUB if k not in nulls}
    outs = {k: Buf(nbytes=WIDTH[k] * cells) for k in OUT1 + OUT2 if k not in nulls}
    a = model_args if model_args is not None else eg._args(p)
    o = (C.c_float * 3)(*[float(x) for x in case["origin"]])
    torch.cuda.current_stream().synchronize()
    st = stream if stream is not None else torch.cuda.current_stream()
    i = lambda k: ins[k].ptr if k in ins else None     # noqa: E731
    q = lambda k: outs[k].ptr if k in outs else None   # noqa: E731
    sec = dc.SECONDS.index(second) if isinstance(second, str) else int(second)
    ret = _L().load().lt_echo_resolve_dual_dev(
        i("rays"), o, n, C.byref(a), sec, i("range"), i("label"), i("rem"), i("tri"), q("endpoints"), q("endcolors"), q("range"),
        q("endrem"), q("tri"), q("n_echoes"), q("fraction"), q("endpoints2"), q("endcolors2"), q("range2"), q("endrem2"), q("tri2"),
        q("fraction2"), C.c_void_p(st.cuda_stream))
    st.synchronize()
    for b in ins.values():
        b.host(np.uint8)                                                   # (the guards of the inputs)
    return ret, {k: b.host(TYPES[k]) for k, b in outs.items()}


def check(case, p, second, tag, nulls=(), stream=None):
    ret, got = call_dual(case, p, second, nulls, stream)
    assert ret == LT_OK, (tag, _L().load().lt_last_error())
    one, two = dc.restate_resolve_dual(p, second, case["rays"], case["origin"], case["range"], case["tri"],
                                       None if "label" in nulls else case["label"], None if "rem" in nulls else case["rem"])
    for k in OUT1:
        if k not in nulls:
            _same_bits(got[k], one[k], f"{tag}: {k}")
    for k in dc.KEYS:
        if k + "2" not in nulls:
            _same_bits(got[k + "2"], two[k], f"{tag}: {k}2")
    return one, two, got


@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("S", [2, 5, 8])
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_random_hit_patterns_resolve_like_the_restatement_under_every_pair(n, S, mode):
    case = ec.resolve_case(n, S)
    off = ec.offsets(0.2, S)
    for second in dc.SECONDS:
        for min_subrays in (1, min(2, S)):
            one, two, _ = check(case, ec.params(off, 0.5, min_subrays, mode), second, f"n={n} S={S} {mode}/{second}/{min_subrays}")
            if n >= 255 and min_subrays == 1 and S >= 5:
                assert (two["tri"] >= 0).mean() > 0.35 and (one["n_echoes"] >= 3).mean() > 0.05


@pytest.mark.parametrize("mode,second", dc.PAIRS)
def test_the_hand_written_cells(mode, second):
    """tests/test_dual_return_cpu.py asserts what each cell must give; here the kernel gives it, about two origins, and on
    the single resolve's hand-written cells as well"""
    for min_subrays in (1, 2):
        for origin in ((0.0, 0.0, 0.0), ORIGIN):
            for cells in (dc.crafted_cells(origin=origin), ec.crafted_cells(origin=origin)):
                check(cells, ec.params(ec.offsets(0.2, 5), 0.5, min_subrays, mode), second, f"{mode}/{second}/{min_subrays}/{origin}")


@pytest.mark.parametrize("S", [2, 5, 8])
def test_the_primary_set_is_what_the_single_resolve_writes(S):
    for n in (1, 257, 1000):
        case = ec.resolve_case(n, S, seed=1, origin=ORIGIN)
        for mode, second in dc.PAIRS:
            for min_subrays in (1, min(2, S)):
                p = ec.params(ec.offsets(0.2, S), 0.5, min_subrays, mode)
                ret1, single = eg.call_resolve(case, p)
                ret2, dual = call_dual(case, p, second)
                assert ret1 == LT_OK and ret2 == LT_OK
                for k in OUT1:
                    assert np.array_equal(_bits(dual[k]), _bits(single[k])), (n, S, mode, second, min_subrays, k)


@pytest.mark.parametrize("null", ["endpoints2", "endcolors2", "endrem2", "fraction2", "all four", "both sets' optional ones"])
def test_every_optional_pointer_of_the_second_set_may_be_null(null):
    nulls = dict([("all four", ("endpoints2", "endcolors2", "endrem2", "fraction2")),
                  ("both sets' optional ones", ("endpoints2", "endcolors2", "endrem2", "fraction2", "endpoints", "endcolors", "endrem",
                                                "n_echoes", "fraction", "label", "rem"))]).get(null, (null,))
    for mode, second in dc.PAIRS:
        check(ec.resolve_case(257, 5, seed=2), ec.params(ec.offsets(0.2, 5), 0.5, 1, mode), second, f"NULL {null}, {mode}/{second}",
              nulls=nulls)
    check(ec.resolve_case(63, 8, seed=2, origin=ORIGIN), ec.params(ec.offsets(0.2, 8)), "last", f"NULL {null}, 63 cells", nulls=nulls)


def test_a_side_stream():
    import torch
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    check(ec.resolve_case(1000, 5, seed=4, origin=ORIGIN), ec.params(ec.offsets(0.2, 5)), "last", "side stream", stream=s)


def test_the_dual_resolve_refuses_bad_arguments_with_a_message_that_names_the_entry():
    lib = _L().load()
    case = ec.resolve_case(63, 5)
    ok = ec.params(ec.offsets(0.2, 5))
    refused = lambda ret: ret == LT_ERR_INVALID_ARG and b"lt_echo_resolve_dual_dev" in lib.lt_last_error()   # noqa: E731
    untouched = lambda got: all((v.view(np.uint8) == FILL).all() for v in got.values())                      # noqa: E731
    for tag, kw in (("range2", dict(nulls=("range2",))), ("tri2", dict(nulls=("tri2",))), ("rays", dict(nulls=("rays",))),
                    ("n", dict(n=-1)), ("second_mode 3", dict(second=3)), ("second_mode -1", dict(second=0xFFFFFFFF))):
        ret, got = call_dual(case, ok, kw.pop("second", "last"), **kw)
        assert refused(ret) and untouched(got), tag
    # (`range` and `tri` name an input and an output each in this harness: the primary's outputs alone)
    b = {k: Buf(case[k]) for k in ("rays",) + eg.SUB}
    o, o2 = Buf(nbytes=4 * 63), Buf(nbytes=4 * 63)
    a = eg._args(ok)
    org = (C.c_float * 3)(0, 0, 0)
    for tag, rng, tri in (("range", None, o.ptr), ("tri", o.ptr, None)):
        ret = lib.lt_echo_resolve_dual_dev(b["rays"].ptr, org, 63, C.byref(a), 2, b["range"].ptr, None, None, b["tri"].ptr, None, None,
                                           rng, None, tri, None, None, None, None, o2.ptr, None, o2.ptr, None, None)
        assert refused(ret), tag
    for tag, bad in eg._bad_models(ok):
        ret, got = call_dual(case, ok, "last", model_args=bad)
        assert refused(ret) and untouched(got), tag
    ret = lib.lt_echo_resolve_dual_dev(b["rays"].ptr, None, 63, C.byref(a), 2, b["range"].ptr, None, None, b["tri"].ptr, None, None,
                                       o.ptr, None, o.ptr, None, None, None, None, o2.ptr, None, o2.ptr, None, None)
    assert refused(ret)                                                       # no origin
    assert lib.lt_echo_resolve_dual_dev(None, org, 0, C.byref(a), 2, *([None] * 17), None) == LT_OK   # no cells
    assert lib.lt_echo_resolve_dual_dev(None, org, 0, C.byref(a), 3, *([None] * 17), None) == LT_ERR_INVALID_ARG


def test_the_wrapper_is_the_entry_point():
    import torch
    from lidar_transfer_amd import post
    from lidar_transfer_amd.config import DualReturn, EchoModel
    n = 1000
    case = ec.resolve_case(n, 5, seed=6, origin=ORIGIN)
    m = EchoModel(0.2, 5, separation=0.4, min_subrays=1, mode="strongest")
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    sub = dict(range=dev(case["range"]), tri=dev(case["tri"]), endcolors=dev(case["label"]), endrem=dev(case["rem"]))
    alloc = lambda: dict(endpoints=torch.empty((n, 3), device="cuda"), endcolors=torch.empty(n, dtype=torch.int32, device="cuda"),   # noqa: E731
                         range=torch.empty(n, device="cuda"), endrem=torch.empty(n, device="cuda"),
                         tri=torch.empty(n, dtype=torch.int32, device="cuda"))
    out, out2 = alloc(), alloc()
    more = post.echo_resolve_dual(dev(case["rays"]), ORIGIN, m, DualReturn("last"), sub, out, out2)
    torch.cuda.synchronize()
    one, two = dc.restate_resolve_dual(ec.params_of(m), "last", case["rays"], ORIGIN, case["range"], case["tri"], case["label"],
                                       case["rem"])
    for k in ("endpoints", "endcolors", "range", "endrem", "tri"):
        _same_bits(out[k].cpu().numpy(), one[k], k)
        _same_bits(out2[k].cpu().numpy(), two[k], k + "2")
    assert np.array_equal(more["n_echoes"].cpu().numpy(), one["n_echoes"])
    _same_bits(more["echo_fraction"].cpu().numpy(), one["fraction"], "echo_fraction")
    _same_bits(more["echo_fraction2"].cpu().numpy(), two["fraction"], "echo_fraction2")
    for bad in (dict(second=DualReturn()), dict(second="last"), dict(out2=dict(range=out2["range"])), dict(model=None)):
        kw = dict(model=m, second=DualReturn("last"), out2=out2)
        kw.update(bad)
        with pytest.raises(ValueError):
            post.echo_resolve_dual(dev(case["rays"]), ORIGIN, kw["model"], kw["second"], sub, out, kw["out2"])


# ---- end to end: a plate in front of a wall ----------------------------------------------------------------------------------
def test_a_plate_edge_gives_the_plate_first_and_the_wall_second():
    import torch
    from lidar_transfer_amd import _chain, post
    from lidar_transfer_amd.config import DualReturn, EchoModel
    from lidar_transfer_amd.laserscan import create_rays
    from lidar_transfer_amd.raytracer import RaySet, Scene
    H, W, S = 8, 64, 5
    n = H * W
    rays_h = create_rays(10.0, -10.0, H, W)
    verts, faces, colors, rem, w0 = ec.edge_scene(rays_h, H, W)
    dev = [torch.from_numpy(x).cuda() for x in (verts, faces, colors, rem)]
    rays = torch.from_numpy(rays_h).cuda()
    origin = (0.0, 0.0, 0.0)
    keys = ("endpoints", "endcolors", "range", "endrem", "tri")
    host = lambda o: {k: o[k].cpu().numpy().copy() for k in keys}   # noqa: E731
    sc = Scene(0)
    sc.set_mesh(*dev)
    plain_set = RaySet(rays, H)
    sub = post.create_subrays(rays, EchoModel(0.2, S))
    sub_set = RaySet(sub, S * H, grid=_chain.Echoes.grid_of(plain_set.grid, H))
    sub_dev = sc.render(sub_set, origin, label_image=True)
    torch.cuda.synchronize()
    sub_out = host(sub_dev)
    res = {}
    for mode, second in (("first", "last"), ("last", "first")):
        m = EchoModel(0.2, S, separation=0.5, mode=mode)
        out, out2 = sc.alloc_outputs(n, label_image=True), sc.alloc_outputs(n, label_image=True)
        more = post.echo_resolve_dual(rays, origin, m, DualReturn(second), sub_dev, out, out2)
        torch.cuda.synchronize()
        one, two = dc.restate_resolve_dual(ec.params_of(m), second, rays_h, origin, sub_out["range"], sub_out["tri"], sub_out["endcolors"],
                                           sub_out["endrem"])
        a, b = host(out), host(out2)
        for k in keys:
            _same_bits(a[k], one[k], f"{mode}/{second}: {k}")
            _same_bits(b[k], two[k], f"{mode}/{second}: {k}2")
        a["n_echoes"] = more["n_echoes"].cpu().numpy()
        res[mode] = (a, b)
    (p, s), (ps, ss) = res["first"], res["last"]
    cells = np.arange(H) * W + w0
    assert (p["n_echoes"][cells] == 2).all()
    assert (np.abs(p["range"][cells] - 5.0) < 0.1).all() and (p["endcolors"][cells] == 7).all()        # the plate
    assert (np.abs(s["range"][cells] - 10.0) < 0.2).all() and (s["endcolors"][cells] == 3).all()       # the wall behind it
    d = np.linalg.norm(s["endpoints"][cells].astype(np.float64), axis=1)
    assert np.abs(d - s["range"][cells]).max() < 1e-5
    two = p["n_echoes"] >= 2
    assert np.array_equal(s["tri"] >= 0, two) and two.sum() >= H and (~two).sum() > n // 2
    for k in keys:                                                      # first and last swapped: the two sets swap there
        assert np.array_equal(_bits(ps[k][two]), _bits(s[k][two])) and np.array_equal(_bits(ss[k][two]), _bits(p[k][two])), k
    sub_set.close()
    plain_set.close()
    sc.close()


# ---- the chains --------------------------------------------------------------------------------------------------------------
SEQ_TARGET, T_EXAMPLE, ECHO_BLOCK, NOISE_BLOCK, GATE_BLOCK = eg.SEQ_TARGET, eg.T_EXAMPLE, eg.ECHO_BLOCK, eg.NOISE_BLOCK, eg.GATE_BLOCK
PRIMARY = ("range", "rem", "label", "endpoints", "endpoints_scene", "tri", "n_echoes", "echo_fraction", "incidence", "drop",
           "range_error", "noise_state")
SECOND = ("range", "rem", "label", "endpoints", "endpoints_scene", "tri", "echo_fraction", "incidence", "drop", "range_error",
          "noise_state")


def _dual(second="last"):
    from lidar_transfer_amd.config import DualReturn
    return DualReturn(second)


@pytest.fixture
def calls(monkeypatch):
    """counts the calls of ``post.echo_resolve_dual``, ``post.echo_resolve`` and ``DeviceDeform._pack`` (the one place each
    entry is called from on a chain)"""
    from lidar_transfer_amd import post
    from lidar_transfer_amd.deform import DeviceDeform
    n = dict(dual=[], single=[], pack=[])
    real_d, real_s, real_p = post.echo_resolve_dual, post.echo_resolve, DeviceDeform._pack
    monkeypatch.setattr(post, "echo_resolve_dual", lambda *a, **k: (n["dual"].append(1), real_d(*a, **k))[1])
    monkeypatch.setattr(post, "echo_resolve", lambda *a, **k: (n["single"].append(1), real_s(*a, **k))[1])
    monkeypatch.setattr(DeviceDeform, "_pack", lambda self, *a, **k: (n["pack"].append(a[5]), real_p(self, *a, **k))[1])
    return n


def _host2(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in out["second"].items() if k in SECOND}


def _expect_second(sub, rays, echo, second, gate, noise, scan, origin, T=None):
    """the second return a chain must give, from the PLAIN chain's render ``sub`` of the sub-ray set (and its mesh): the dual
    resolve restated, the return model and the noise model restated with the xor-ed seed, the frame change, the packing"""
    import oracle_chain as oc
    _, w = dc.restate_resolve_dual(ec.params_of(echo), second.second, rays, origin, sub["range"].reshape(-1), sub["tri"],
                                   sub["label"].reshape(-1), sub["rem"].reshape(-1))
    w["echo_fraction"] = w.pop("fraction")
    xored = lambda p: dict(p, seed=(int(p["seed"]) ^ XOR) & 0xFFFFFFFF)   # noqa: E731
    if gate is not None:
        r = rc.restate(xored(rc.params_of(gate)), scan, rays, sub["mesh"][0], sub["mesh"][1], w["tri"], w["range"], w["endrem"],
                       w["endpoints"], w["endcolors"])
        w.update({k: r[k] for k in ("tri", "range", "endrem", "endpoints", "endcolors", "incidence", "drop")})
    if noise is not None:
        r = nc.restate(xored(nc.params_of(noise, gate)), scan, origin, w["tri"], w["range"], w["endrem"], w["endpoints"], w["endcolors"])
        w.update({k: r[k] for k in ("tri", "range", "endrem", "endpoints", "endcolors", "range_error")})
        w["noise_state"] = r["state"]
    w["endpoints_target"] = w["endpoints"] if T is None else mc.to_frame(w["endpoints"], T, w["tri"])
    w["bin"], w["label_file"] = oc.pack_write(w["endpoints_target"], w["endcolors"], w["endrem"])
    return w


def _check_second(got2, w, tag):
    pairs = [("range", "range"), ("rem", "endrem"), ("label", "endcolors"), ("tri", "tri"), ("endpoints_scene", "endpoints"),
             ("endpoints", "endpoints_target"), ("echo_fraction", "echo_fraction")]
    pairs += [(k, k) for k in ("incidence", "drop", "range_error", "noise_state") if k in w]
    assert set(got2) == {g for g, _ in pairs}, (tag, sorted(got2))
    for gk, wk in pairs:
        _same_bits(got2[gk], w[wk], f"{tag}: second {gk}")


def _check_files(got, single, w, tag):
    """``bin`` / ``label_file``: the single-return chain's bytes, then the restated second returns' packed rows"""
    b, l = got["bin"].tobytes(), got["label_file"].view(np.uint32).tobytes()
    b1, l1 = single["bin"].tobytes(), single["label_file"].view(np.uint32).tobytes()
    assert b[:len(b1)] == b1 and l[:len(l1)] == l1, (tag, "the files' leading bytes")
    assert b[len(b1):] == w["bin"].tobytes() and l[len(l1):] == w["label_file"].astype(np.uint32).tobytes(), (tag, "the files' tail")


@pytest.mark.parametrize("mounted,models", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("adaption", ["mesh", "mergemesh"])
def test_device_deform_adds_the_restated_second_return_and_leaves_the_primary_alone(adaption, mounted, models, calls):
    """three chains side by side, two scans each (mergemesh's first has no geometry to assume: it is rendered again, and the
    resolve runs once, on the render that stands): the PLAIN chain over the sub-rays that the restatements start from, the
    chain with the echo model alone, and the chain with the dual return"""
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    g17, g18, a, target = tm._seq_setup(adaption, [])
    kw = dict(transformation=T_EXAMPLE, t_beam_table=bc.VLP32C) if mounted else {}
    if mounted:
        target = SEQ_TARGET
    echo, second = eg._echo(), _dual("last")
    gate, noise = (eg._gate(), eg._noise()) if models else (None, None)
    if models:
        kw.update(returns=gate, noise=noise)
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    indices = [int(x) for x in a.scan_indices(8)[:2]]
    make = lambda **more: DeviceDeform(ev.SOURCE, target, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=adaption == "mesh",   # noqa: E731
                                       echoes=echo, **kw, **more)
    with make() as d1, make(dual=second) as d2:
        assert d2.dual == second and d1.dual is None
        origin, T = d2.origin, (d2.mount[0] if mounted else None)
        chain, rs, rays = eg._sub_chain(d2, target, a, adaption, mounted)
        with chain:
            for idx in indices:
                tag = f"{adaption}/mounted={mounted}/models={models}/scan {idx}"
                sub = eg._host(chain.deform(adaption, ing, idx), chain.mesh_obj)
                plain = d1.deform(adaption, ing, idx, scan_index=idx)
                single = eg._host(plain)
                before = {k: len(v) for k, v in calls.items()}
                out = d2.deform(adaption, ing, idx, scan_index=idx)
                assert [len(calls[k]) - before[k] for k in ("dual", "single", "pack")] == [1, 0, 1] and calls["pack"][-1] == 2 * d2.n_rays
                got, got2 = eg._host(out), _host2(out)
                assert set(out) - {"second"} == set(plain), tag
                for k in PRIMARY:
                    assert (k in got) == (k in single), (tag, k)
                    if k in got:
                        _same_bits(got[k], single[k], f"{tag}: primary {k}")
                w = _expect_second(sub, rays, echo, second, gate, noise, idx, origin, T)
                _check_second(got2, w, tag)
                _check_files(got, single, w, tag)
                hits = int((w["tri"] >= 0).sum())
                print(f"\n{tag}: {single['bin'].shape[0]} + {w['bin'].shape[0]} points written, {hits} second returns stand")
                assert hits > 20 and w["bin"].shape[0] > 20
            if adaption == "mergemesh":
                stats = dict(d2._mm().stats)
                assert stats["scans"] == 2 and stats["waited"] + stats["rerun"] >= 1, stats
        rs.close()
    src.close()


@pytest.mark.parametrize("chains", [1, 3])
def test_fusion_pipeline_with_one_and_three_scans_in_flight_equals_device_deform(chains, calls):
    """six output scans through ``submit_mergemesh`` and ``submit_clouds`` against one DeviceDeform scan after scan, the second
    return included; and against the pipeline WITHOUT the setting for the primary"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.pipeline import FusionScanPipeline
    echo, gate, noise, second = eg._echo(), eg._gate(), eg._noise(), _dual("first")
    g17, g18, a, target = tm._seq_setup("mergemesh", [])
    am = sq.approach_for(g18, "mesh")
    src = tm._source(g17)
    rays = create_rays_device(target[2], target[3], target[0], target[1], device=0)
    order = ([int(x) for x in a.scan_indices(8)] * 6)[:6]
    keys = ("range", "endrem", "endcolors", "endpoints", "tri", "n_echoes", "echo_fraction", "range_error", "noise_state", "drop",
            "incidence")
    names = dict(endrem="rem", endcolors="label")
    host = lambda r: ({k: r[k].cpu().numpy().copy() for k in keys},   # noqa: E731
                      {k: r["second"][k].cpu().numpy().copy() for k in SECOND} if "second" in r else None)
    for adaption, ap, merged in (("mergemesh", a, True), ("mesh", am, False)):
        ing = ScanIngest(src, ap)
        more = dict(fixed_volume=False) if merged else {}
        fov = (target[2], target[3]) if merged else (ev.SOURCE[2], ev.SOURCE[3])
        got = {}
        for dual in (second, None):
            n_dual = len(calls["dual"])
            with FusionScanPipeline(ap.voxel_bounds.copy(), ap.voxel_size, fov[0], fov[1], rays, target[0], chains=chains, device=0,
                                    label_image=True, source_hw=ev.SOURCE[:2], returns=gate, noise=noise, echoes=echo, dual=dual,
                                    **more) as pipe:
                assert pipe.dual == dual
                submit = pipe.submit_mergemesh if merged else pipe.submit_clouds
                tickets = []
                for k, idx in enumerate(order):
                    clouds = ing.prepare(idx, merged=merged)
                    torch.cuda.synchronize()
                    tickets.append(submit(clouds, inputs_ready=True, scan_index=40 + k))
                got[dual is not None] = [host(pipe.wait(t)) for t in tickets]
            assert len(calls["dual"]) - n_dual == (len(order) if dual is not None else 0)
        with DeviceDeform(ev.SOURCE, target, ap.voxel_bounds.copy(), ap.voxel_size, mesh_volume=not merged, returns=gate,
                          noise=noise, echoes=echo, dual=second) as dd:
            for k, idx in enumerate(order):
                s = getattr(dd, adaption)(ing.prepare(idx, merged=merged), pack=False, scan_index=40 + k)
                torch.cuda.synchronize()
                tag = f"{adaption}/{chains} chains/scan {k}"
                assert got[False][k][1] is None
                for key in keys:
                    _same_bits(got[True][k][0][key], s[names.get(key, key)].cpu().numpy(), f"{tag}: {key}")
                    _same_bits(got[True][k][0][key], got[False][k][0][key], f"{tag}: {key} against the pipeline without the setting")
                for key in SECOND:
                    _same_bits(got[True][k][1][key], s["second"][key].cpu().numpy(), f"{tag}: second {key}")
                assert (got[True][k][1]["tri"] >= 0).sum() > 5
    src.close()


def _sensor(dual_block, **kw):
    more = {} if dual_block is None else dict(dual_return=dual_block)
    return eg._target_sensor(ECHO_BLOCK, GATE_BLOCK, NOISE_BLOCK, **more, **kw)


def _run_sequence(a, target, out_dir, chains):
    from lidar_transfer_amd.sequence import SequenceTransfer
    g17, g18 = cpu.gold(), sq.gold18()
    src = tm._source(g17)
    with SequenceTransfer(src, a, ev.SOURCE, target, out_dir=str(out_dir), chains=chains, nclasses=int(g18["nclasses"])) as tr:
        recs = list(tr.run())
        summary, dual = tr.summary, tr.dual
    src.close()
    return recs, summary, dual


def test_a_sequence_writes_the_single_return_files_followed_by_the_restated_tail(tmp_path, calls):
    """the mergemesh sequence with a table target, an echo model, a gate, a noise model and ``second: last``, with one chain
    and with three: every file is the file of the same run WITHOUT the block followed by write() of the restated second
    returns of that FILE index; ``second_returns`` is the restatement's count"""
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    g17, g18, a, _ = tm._seq_setup("mergemesh", [])
    sensor = _sensor(dict(second="last"))
    echo, gate, noise, second = sensor.echo_model(), sensor.return_model(), sensor.noise_model(), sensor.dual_return()
    r0, s0, d0 = _run_sequence(a, _sensor(None), tmp_path / "single", 1)
    assert d0 is None and s0["second_returns"] is None and calls["dual"] == [] and len(calls["single"]) == len(r0)
    r1, s1, d1 = _run_sequence(a, sensor, tmp_path / "c1", 1)
    assert d1 == second == _dual("last") and len(calls["dual"]) == len(r1) and len(calls["single"]) == len(r0)
    assert calls["pack"][-len(r1):] == [2 * SEQ_TARGET[0] * SEQ_TARGET[1]] * len(r1) and len(calls["pack"]) == 2 * len(r1)
    r3, s3, _ = _run_sequence(a, sensor, tmp_path / "c3", 3)
    assert s3["chains"] == 3 and len(calls["dual"]) == 2 * len(r1)
    indices = [r["idx"] for r in r1]
    assert indices == [r["idx"] for r in r3] == [r["idx"] for r in r0] == [int(x) for x in a.scan_indices(8)] and len(indices) >= 3
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    with DeviceDeform(ev.SOURCE, SEQ_TARGET, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=False, t_beam_table=bc.VLP32C,
                      echoes=echo) as dd:
        chain, rs, rays = eg._sub_chain(dd, SEQ_TARGET, a, "mergemesh", False)
    stand = 0
    with chain:
        for rec0, rec in zip(r0, r1):
            idx = rec["idx"]
            w = _expect_second(eg._host(chain.deform("mergemesh", ing, idx), chain.mesh_obj), rays, echo, second, gate, noise, idx,
                               (0.0, 0.0, 0.0))
            stand += int((w["tri"] >= 0).sum())
            b0, l0 = tm._read(tmp_path / "single", idx)
            b1, l1 = tm._read(tmp_path / "c1", idx)
            assert b1 == b0 + w["bin"].tobytes(), f"scan {idx}: velodyne file"
            assert l1 == l0 + w["label_file"].astype(np.uint32).tobytes(), f"scan {idx}: label file"
            assert rec["n_points"] == len(b1) // 16 == rec0["n_points"] + w["bin"].shape[0]
            print(f"\nscan {idx}: {rec0['n_points']} + {w['bin'].shape[0]} points")
            assert (b1, l1) == tm._read(tmp_path / "c3", idx), f"scan {idx}: one chain vs three"
    rs.close()
    src.close()
    assert s1["second_returns"] == s3["second_returns"] == stand > 0      # (the gate's 4.6 .. 8 m leave few of them standing)
    for k in ("echo_totals", "echo_fraction_mean", "return_totals", "noise_totals", "range_error_rms"):
        assert s1[k] == s0[k], k                                           # (the tallies are the primary's)


@pytest.mark.parametrize("adaption", ["mesh", "mergemesh"])
def test_without_the_key_and_with_second_none_nothing_changes(adaption, calls):
    import torch
    from lidar_transfer_amd.config import DualReturn
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    g17, g18, a, target = tm._seq_setup(adaption, [])
    assert _sensor(dict(second="none")).dual_return() is None and _sensor({}).dual_return() is None
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    res = []
    for kw in ({}, dict(dual=None), dict(dual=DualReturn()), dict(dual=_sensor(dict(second="none")).dual_return())):
        with DeviceDeform(ev.SOURCE, target, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=adaption == "mesh", echoes=eg._echo(),
                          **kw) as dd:
            assert dd.dual is None and not dd._sensing.dual
            outs = []
            for idx in a.scan_indices(8)[:2]:
                out = dd.deform(adaption, ing, idx)
                torch.cuda.synchronize()
                assert "second" not in out
                outs.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
            res.append(outs)
    for other in res[1:]:
        for x, y in zip(res[0], other):
            tm._same(x, y, adaption)
    assert res[0][0]["bin"].shape[0] > 100 and calls["dual"] == [] and len(calls["single"]) == 8
    assert calls["pack"] == [dd.n_rays] * 8
    src.close()


def test_sequences_without_the_key_write_the_bytes_they_wrote(tmp_path, calls):
    g17, g18, a, _ = tm._seq_setup("mergemesh", [])
    r0, s0, d0 = _run_sequence(a, _sensor(None), tmp_path / "none", 1)
    r1, s1, d1 = _run_sequence(a, _sensor(dict(second="none")), tmp_path / "off", 3)
    r2, s2, d2 = _run_sequence(a, _sensor({}), tmp_path / "empty", 1)
    assert d0 is None and d1 is None and d2 is None and calls["dual"] == []
    for rec in r0:
        assert tm._read(tmp_path / "none", rec["idx"]) == tm._read(tmp_path / "off", rec["idx"]) == tm._read(tmp_path / "empty", rec["idx"])
    assert s0["second_returns"] is None and s1["second_returns"] is None and s2["second_returns"] is None


def test_cp_with_the_key_raises():
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.sequence import SequenceTransfer
    g17, g18, a, target = tm._seq_setup("cp", [])
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    with DeviceDeform(ev.SOURCE, target, None, echoes=eg._echo(), dual=_dual()) as dd:
        with pytest.raises(ValueError, match="cp renders no ray.*no echo to choose a second from"):
            dd.deform("cp", ing, int(a.scan_indices(8)[0]))
        with pytest.raises(ValueError, match="dual_return"):
            dd.cp(ing.prepare(int(a.scan_indices(8)[0]), merged=True))
    with pytest.raises(ValueError, match="cp renders no ray"):
        SequenceTransfer(src, a, ev.SOURCE, eg._target_sensor(ECHO_BLOCK, dual_return=dict(second="last")))
    with pytest.raises(ValueError, match="target sensors only"):
        SequenceTransfer(src, sq.approach_for(g18, "mesh"), eg._target_sensor(None, beam_model="linear", dual_return={}), SEQ_TARGET)
    with pytest.raises(ValueError, match="DualReturn"):
        DeviceDeform(ev.SOURCE, target, None, echoes=eg._echo(), dual=dict(second="last"))
    with pytest.raises(ValueError, match="dual= needs echoes="):
        DeviceDeform(ev.SOURCE, target, None, dual=_dual())
    src.close()


def test_the_cli_closes_with_the_second_returns_and_refuses_cp(tmp_path):
    """the shipped file through ``python -m lidar_transfer_amd`` in a child process: ``Second returns: N`` follows the
    ``Echoes:`` line and is the summary's, every row says ``"dual_return": true`` and counts the file's points; ``cp`` ends
    with a message and status 1 before any device work"""
    import json
    import subprocess
    shipped = os.path.join(ROOT, "config", "vlp32c_table_dual_1024.yaml")
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
    n2 = summary["second_returns"]
    assert len(rows) == 2 and rows[0]["dual_return"] is True and rows[0]["echo_model"] is True
    assert isinstance(n2, int) and 0 < n2 < 32 * 1024 and sum(summary["echo_totals"]) == 32 * 1024
    lines = res.stdout.splitlines()
    at = [k for k, x in enumerate(lines) if x.startswith("Echoes:")]
    assert len(at) == 1 and lines[at[0] + 1] == f"Second returns: {n2}" and lines[-1] == f"Second returns: {n2}"
    b, l = tm._read(out, rows[0]["idx"])
    assert rows[0]["n_points"] == len(b) // 16 == len(l) // 4
    res = subprocess.run(base + ["-c", str(cfgs["cp"]), "-t", shipped], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 1 and "cp renders no" in res.stdout
