"""The target sensor's echo model on the GPU.  `lt_create_subrays_dev` and `lt_echo_resolve_dev` through the C ABI
into sentinel-filled buffers with guards, bit for bit against the numpy restatement of tests/echo_cases.py (pinned without a GPU
by tests/test_echo_model_cpu.py); a wall with a plate in front of it end to end; then the chains -- `DeviceDeform`,
`FusionScanPipeline`, `SequenceTransfer`, the CLI -- against the plain chain's render of the sub-ray set followed by the
restatements of the echo, return and noise models."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import beam_cases as bc  # noqa: E402
import echo_cases as ec  # noqa: E402
import mount_common as mc  # noqa: E402
import noise_cases as nc  # noqa: E402
import return_cases as rc  # noqa: E402
import test_evaluate_cpu as ev  # noqa: E402
import test_ingest_cpu as cpu  # noqa: E402
import test_mount_gpu as tm  # noqa: E402
import test_return_model_gpu as rg  # noqa: E402
import test_sequence_cpu as sq  # noqa: E402

pytestmark = pytest.mark.gpu
LT_OK, LT_ERR_INVALID_ARG = 0, -1
FILL = rg.FILL
Buf, _bits = rg.Buf, rg._bits
OUT = ("endpoints", "endcolors", "range", "endrem", "tri", "n_echoes", "fraction")
SUB = ("range", "label", "rem", "tri")
TYPES = dict(endpoints=np.float32, endcolors=np.int32, range=np.float32, endrem=np.float32, tri=np.int32, n_echoes=np.uint8,
             fraction=np.float32)
WIDTH = dict(endpoints=12, endcolors=4, range=4, endrem=4, tri=4, n_echoes=1, fraction=4)
ORIGIN = (1.5, -2.25, 0.75)


def _L():
    from lidar_transfer_amd import _lib
    return _lib


def _args(p):
    a = _L().EchoModelArgs()
    for k, v in enumerate(np.asarray(p["off"], np.float64).ravel()):
        a.off[k] = float(v)
    a.separation, a.n_subrays, a.min_subrays, a.mode, a.reserved = p["separation"], p["S"], p["min_subrays"], p["mode"], 0
    return a


def _same_bits(got, want, tag):
    bad = np.nonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))[0]
    assert bad.size == 0, f"{tag}: differs in {bad.size} elements, first at {bad[0]}: {np.asarray(got).reshape(-1)[bad[0]]!r} " \
                          f"against {np.asarray(want).reshape(-1)[bad[0]]!r}"


# ---- lt_create_subrays_dev ------------------------------------------------------------------------------------------------------
def call_subrays(rays, p, stream=None, n=None, model_args=None, null=()):
    import torch
    cells = rays.shape[0]
    n = cells if n is None else n
    src, dst = Buf(rays), Buf(nbytes=12 * cells * p["S"])
    a = model_args if model_args is not None else _args(p)
    torch.cuda.current_stream().synchronize()
    st = stream if stream is not None else torch.cuda.current_stream()
    ret = _L().load().lt_create_subrays_dev(None if "rays" in null else src.ptr, n, None if "model" in null else C.byref(a),
                                            None if "subrays" in null else dst.ptr, C.c_void_p(st.cuda_stream))
    st.synchronize()
    assert np.array_equal(_bits(src.host(np.float32)), _bits(rays).reshape(-1))       # (the input is read only)
    return ret, dst.host(np.float32, (-1, 3))


@pytest.mark.parametrize("S", [2, 5, 8])
@pytest.mark.parametrize("n", [1, 21, 63, 257])
def test_the_sub_rays_equal_the_restatement_and_plane_zero_is_the_input(n, S):
    rays = ec.ray_case(n)
    if n >= 21:
        assert np.isnan(rays).any() and (~rays.any(1)).any() and (np.abs(rays[:, :2]).max(1) < 1e-37).sum() >= 4
    for divergence in (0.2, 3.0):
        p = ec.params(ec.offsets(divergence, S))
        ret, got = call_subrays(rays, p)
        assert ret == LT_OK, _L().load().lt_last_error()
        _same_bits(got, ec.restate_subrays(rays, p["off"]), f"n={n} S={S} divergence={divergence}")
        assert np.array_equal(_bits(got[:n]), _bits(rays))


def test_the_sub_rays_on_a_side_stream_and_through_the_wrapper():
    import torch
    from lidar_transfer_amd import post
    from lidar_transfer_amd.config import EchoModel
    s = torch.cuda.Stream()
    rays = ec.ray_case(257, seed=3)
    p = ec.params(ec.offsets(0.2, 5))
    ret, got = call_subrays(rays, p, stream=s)
    assert ret == LT_OK
    want = ec.restate_subrays(rays, p["off"])
    _same_bits(got, want, "side stream")
    m = EchoModel(0.2, 5)
    dev = torch.from_numpy(rays).cuda()
    sub = post.create_subrays(dev, m)
    torch.cuda.synchronize()
    assert sub.shape == (5 * 257, 3) and sub.dtype == torch.float32
    _same_bits(sub.cpu().numpy(), want, "post.create_subrays")
    with torch.cuda.stream(s):
        sub = post.create_subrays(dev, m, stream=s)
    s.synchronize()
    _same_bits(sub.cpu().numpy(), want, "post.create_subrays on a side stream")
    with pytest.raises(ValueError):
        post.create_subrays(dev, EchoModel())
    with pytest.raises(ValueError):
        post.create_subrays(dev.double(), m)


def _bad_models(ok):
    nan, inf = float("nan"), float("inf")
    bad = []
    for tag, kw in (("one sub-ray", dict(S=1)), ("nine sub-rays", dict(S=9)), ("no sub-ray", dict(S=0)), ("min 0", dict(min_subrays=0)),
                    ("min > S", dict(min_subrays=ok["S"] + 1)), ("mode 3", dict(mode=3)), ("separation 0", dict(separation=0.0)),
                    ("separation < 0", dict(separation=-1.0)), ("separation nan", dict(separation=nan)),
                    ("separation inf", dict(separation=inf))):
        p = dict(ok, **kw)
        a = _L().EchoModelArgs()
        for k, v in enumerate(np.asarray(ok["off"], np.float64).ravel()):
            a.off[k] = float(v)
        a.separation, a.n_subrays, a.min_subrays, a.mode = p["separation"], p["S"], p["min_subrays"], p["mode"]
        bad.append((tag, a))
    for tag, v in (("offset nan", nan), ("offset inf", inf)):
        a = _args(ok)
        a.off[2 * ok["S"] - 1] = v
        bad.append((tag, a))
    return bad


def test_create_subrays_refuses_bad_arguments_with_a_message_that_names_the_entry():
    lib = _L().load()
    rays = ec.ray_case(63)
    ok = ec.params(ec.offsets(0.2, 5))
    for tag, kw in (("rays", dict(null=("rays",))), ("subrays", dict(null=("subrays",))), ("model", dict(null=("model",))),
                    ("n", dict(n=-1))):
        ret, got = call_subrays(rays, ok, **kw)
        assert ret == LT_ERR_INVALID_ARG and b"lt_create_subrays_dev" in lib.lt_last_error(), tag
        assert (got.view(np.uint8) == FILL).all(), tag
    for tag, a in _bad_models(ok):
        ret, got = call_subrays(rays, ok, model_args=a)
        assert ret == LT_ERR_INVALID_ARG and b"lt_create_subrays_dev" in lib.lt_last_error(), tag
        assert (got.view(np.uint8) == FILL).all(), tag
    a = _args(ok)
    a.off[15] = float("nan")                                              # beyond n_subrays: ignored
    ret, got = call_subrays(rays, ok, model_args=a)
    assert ret == LT_OK
    _same_bits(got, ec.restate_subrays(rays, ok["off"]), "a NaN in an unused slot")
    ret, got = call_subrays(rays, ok, n=0, null=("rays", "subrays"))
    assert ret == LT_OK and (got.view(np.uint8) == FILL).all()            # no cells


# ---- lt_echo_resolve_dev ----------------------------------------------------------------------------------------------------------
def call_resolve(case, p, nulls=(), stream=None, model_args=None, n=None, origin=None):
    """one lt_echo_resolve_dev call on the case's sub-images; returns (rc, dict of the output buffers afterwards)"""
    import torch
    cells = case["rays"].shape[0]
    n = cells if n is None else n
    ins = {k: Buf(case[k]) for k in ("rays",) + SUB if k not in nulls}
    outs = {k: Buf(nbytes=WIDTH[k] * cells) for k in OUT if k not in nulls}
    a = model_args if model_args is not None else _args(p)
    o = None if "origin" in nulls else (C.c_float * 3)(*[float(x) for x in (case["origin"] if origin is None else origin)])
    torch.cuda.current_stream().synchronize()
    st = stream if stream is not None else torch.cuda.current_stream()
    i = lambda k: ins[k].ptr if k in ins else None     # noqa: E731
    q = lambda k: outs[k].ptr if k in outs else None   # noqa: E731
    ret = _L().load().lt_echo_resolve_dev(i("rays"), o, n, None if "model" in nulls else C.byref(a), i("range"), i("label"), i("rem"),
                                          i("tri"), q("endpoints"), q("endcolors"), q("range"), q("endrem"), q("tri"), q("n_echoes"),
                                          q("fraction"), C.c_void_p(st.cuda_stream))
    st.synchronize()
    for k, b in ins.items():
        b.host(np.uint8)                                                   # (the guards of the inputs)
    return ret, {k: b.host(TYPES[k]) for k, b in outs.items()}


def check(case, p, tag, nulls=(), stream=None):
    ret, got = call_resolve(case, p, nulls, stream)
    assert ret == LT_OK, (tag, _L().load().lt_last_error())
    want = ec.restate_resolve(p, case["rays"], case["origin"], case["range"], case["tri"],
                              None if "label" in nulls else case["label"], None if "rem" in nulls else case["rem"])
    for k in OUT:
        if k not in nulls:
            _same_bits(got[k], want[k], f"{tag}: {k}")
    return want


@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("S", [2, 5, 8])
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_random_hit_patterns_resolve_like_the_restatement(n, S, mode):
    case = ec.resolve_case(n, S)
    off = ec.offsets(0.2, S)
    want = check(case, ec.params(off, 0.5, 1, mode), f"n={n} S={S} {mode}")
    check(case, ec.params(off, 0.5, min(2, S), mode), f"n={n} S={S} {mode}, two sub-hits needed")
    check(case, ec.params(off, 0.03, 1, mode), f"n={n} S={S} {mode}, a separation inside the jitter")
    if n >= 255:
        count = np.bincount(want["n_echoes"], minlength=3)
        assert count[0] > 0 and count[1] > 20 and count[2:].sum() > 2, count


@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("min_subrays", [1, 2])
def test_the_hand_written_cells(mode, min_subrays):
    """all misses, one hit, equal t, a gap equal to the separation, a chain longer than it, min_subrays removing the nearest and
    every echo, the ties of `strongest`, first == last, a zero central ray (tests/test_echo_model_cpu.py asserts what each
    must give) -- and about a non-zero origin"""
    for origin in ((0.0, 0.0, 0.0), ORIGIN):
        c = ec.crafted_cells(origin=origin)
        want = check(c, ec.params(ec.offsets(0.2, 5), 0.5, min_subrays, mode), f"{mode}/{min_subrays}/{origin}")
        i = c["names"].index("a gap exactly equal to separation")
        assert want["n_echoes"][i] == (1 if min_subrays <= 2 else 0) and want["range"][i] == 4.25
        i = c["names"].index("a chain of close hits spanning more")
        assert want["n_echoes"][i] == (3 if min_subrays == 1 else 2)
        i = c["names"].index("a zero central ray")
        assert want["tri"][i] == -1 and want["n_echoes"][i] == 1 and not want["endpoints"][i].any()
        hit = want["tri"] >= 0
        d = np.linalg.norm(want["endpoints"][hit].astype(np.float64) - np.asarray(origin), axis=1)
        assert np.abs(d - want["range"][hit]).max() < 2e-6


@pytest.mark.parametrize("null", ["endpoints", "endcolors", "endrem", "n_echoes", "fraction", "label", "rem", "all seven"])
def test_every_optional_pointer_may_be_null(null):
    nulls = ("endpoints", "endcolors", "endrem", "n_echoes", "fraction", "label", "rem") if null == "all seven" else (null,)
    for mode in ec.MODES:
        check(ec.resolve_case(257, 5, seed=2), ec.params(ec.offsets(0.2, 5), 0.5, 1, mode), f"NULL {null}, {mode}", nulls=nulls)
    check(ec.resolve_case(63, 8, seed=2, origin=ORIGIN), ec.params(ec.offsets(0.2, 8)), f"NULL {null}, 63 cells", nulls=nulls)


def test_a_side_stream():
    import torch
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    check(ec.resolve_case(1000, 5, seed=4, origin=ORIGIN), ec.params(ec.offsets(0.2, 5)), "side stream", stream=s)


def test_resolve_refuses_bad_arguments_with_a_message_that_names_the_entry():
    lib = _L().load()
    case = ec.resolve_case(63, 5)
    ok = ec.params(ec.offsets(0.2, 5))
    nan, inf = float("nan"), float("inf")
    for tag, kw in (("rays", dict(nulls=("rays",))), ("sub_range", dict(nulls=("range",))), ("sub_tri", dict(nulls=("tri",))),
                    ("origin", dict(nulls=("origin",))), ("model", dict(nulls=("model",))), ("n", dict(n=-1)),
                    ("origin nan", dict(origin=(0.0, nan, 0.0))), ("origin inf", dict(origin=(inf, 0.0, 0.0)))):
        ret, got = call_resolve(case, ok, **kw)
        assert ret == LT_ERR_INVALID_ARG and b"lt_echo_resolve_dev" in lib.lt_last_error(), tag
        assert all((v.view(np.uint8) == FILL).all() for v in got.values()), tag
    # (`range` and `tri` name an input and an output each in this harness: the outputs alone)
    b = {k: Buf(case[k]) for k in ("rays",) + SUB}
    o = Buf(nbytes=4 * 63)
    a = _args(ok)
    org = (C.c_float * 3)(0, 0, 0)
    for tag, rng, tri in (("range", None, o.ptr), ("tri", o.ptr, None)):
        ret = lib.lt_echo_resolve_dev(b["rays"].ptr, org, 63, C.byref(a), b["range"].ptr, None, None, b["tri"].ptr, None, None, rng,
                                      None, tri, None, None, None)
        assert ret == LT_ERR_INVALID_ARG and b"lt_echo_resolve_dev" in lib.lt_last_error(), tag
    for tag, bad in _bad_models(ok):
        ret, got = call_resolve(case, ok, model_args=bad)
        assert ret == LT_ERR_INVALID_ARG and b"lt_echo_resolve_dev" in lib.lt_last_error(), tag
        assert all((v.view(np.uint8) == FILL).all() for v in got.values()), tag
    assert lib.lt_echo_resolve_dev(None, org, 0, C.byref(a), None, None, None, None, None, None, None, None, None, None, None,
                                   None) == LT_OK                          # no cells


def test_the_wrapper_is_the_entry_point():
    import torch
    from lidar_transfer_amd import post
    from lidar_transfer_amd.config import EchoModel
    case = ec.resolve_case(1000, 5, seed=6, origin=ORIGIN)
    m = EchoModel(0.2, 5, separation=0.4, min_subrays=2, mode="last")
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    sub = dict(range=dev(case["range"]), tri=dev(case["tri"]), endcolors=dev(case["label"]), endrem=dev(case["rem"]))
    out = dict(endpoints=torch.empty((1000, 3), device="cuda"), endcolors=torch.empty(1000, dtype=torch.int32, device="cuda"),
               range=torch.empty(1000, device="cuda"), endrem=torch.empty(1000, device="cuda"),
               tri=torch.empty(1000, dtype=torch.int32, device="cuda"))
    more = post.echo_resolve(dev(case["rays"]), ORIGIN, m, sub, out)
    torch.cuda.synchronize()
    want = ec.restate_resolve(ec.params_of(m), case["rays"], ORIGIN, case["range"], case["tri"], case["label"], case["rem"])
    for k in ("endpoints", "endcolors", "range", "endrem", "tri"):
        _same_bits(out[k].cpu().numpy(), want[k], k)
    assert more["n_echoes"].dtype == torch.uint8 and np.array_equal(more["n_echoes"].cpu().numpy(), want["n_echoes"])
    _same_bits(more["echo_fraction"].cpu().numpy(), want["fraction"], "echo_fraction")
    only = post.echo_resolve(dev(case["rays"]), ORIGIN, m, dict(range=sub["range"], tri=sub["tri"]),
                             dict(range=out["range"], tri=out["tri"]), fraction=None)
    torch.cuda.synchronize()
    assert only["echo_fraction"] is None and np.array_equal(only["n_echoes"].cpu().numpy(), want["n_echoes"])
    with pytest.raises(ValueError):
        post.echo_resolve(dev(case["rays"]), ORIGIN, m, sub, dict(range=out["range"]))
    with pytest.raises(ValueError):
        post.echo_resolve(dev(case["rays"]), ORIGIN, None, sub, out)
    with pytest.raises(ValueError):
        post.echo_resolve(dev(case["rays"]), ORIGIN, m, dict(sub, range=sub["range"][:10]), out)


# ---- end to end: a plate in front of a wall ------------------------------------------------------------------------------------------
def test_a_plate_edge_in_front_of_a_wall_gives_two_echoes_in_its_column():
    import torch
    from lidar_transfer_amd import _chain, post
    from lidar_transfer_amd.config import EchoModel
    from lidar_transfer_amd.laserscan import create_rays
    from lidar_transfer_amd.raytracer import RaySet, Scene
    H, W, S = 8, 64, 5
    n = H * W
    rays_h = create_rays(10.0, -10.0, H, W)
    verts, faces, colors, rem, w0 = ec.edge_scene(rays_h, H, W)
    model = {mode: EchoModel(0.2, S, separation=0.5, mode=mode) for mode in ec.MODES}
    dev = [torch.from_numpy(x).cuda() for x in (verts, faces, colors, rem)]
    rays = torch.from_numpy(rays_h).cuda()
    origin = (0.0, 0.0, 0.0)
    host = lambda o: {k: o[k].cpu().numpy().copy() for k in ("endpoints", "endcolors", "range", "endrem", "tri")}   # noqa: E731
    sc = Scene(0)
    sc.set_mesh(*dev)
    plain_set = RaySet(rays, H)
    plain = host(sc.render(plain_set, origin, label_image=True))
    sub = post.create_subrays(rays, model["first"])
    sub_set = RaySet(sub, S * H, grid=_chain.Echoes.grid_of(plain_set.grid, H))
    sub_dev = sc.render(sub_set, origin, label_image=True)
    torch.cuda.synchronize()
    sub_out = host(sub_dev)
    # 1. plane 0 of the sub-render is the plain render, byte for byte
    for k in plain:
        _same_bits(sub_out[k].reshape(S, -1)[0], plain[k], f"plane 0: {k}")
    # 2. the scatter render of the sub-ray set is build + trace of the same sub-rays
    sc.build()
    traced = host(sc.trace(sub, origin, S * H, label_image=True))
    for k in traced:
        _same_bits(sub_out[k], traced[k], f"render against trace: {k}")
    # ... and with the image's own rule for the taller set, and with the azimuth bins doubled: the grid is a speed choice
    for grid in (None, (2 * (W - 1), H)):
        other = host(sc.render(RaySet(sub, S * H, grid=grid), origin, label_image=True))
        for k in other:
            _same_bits(other[k], sub_out[k], f"grid {grid}: {k}")
    # 3. the resolve of the sub-render is the restatement of it
    res = {}
    for mode, m in model.items():
        out = sc.alloc_outputs(n, label_image=True)
        more = post.echo_resolve(rays, origin, m, sub_dev, out)
        torch.cuda.synchronize()
        want = ec.restate_resolve(ec.params_of(m), rays_h, origin, sub_out["range"], sub_out["tri"], sub_out["endcolors"], sub_out["endrem"])
        got = dict(host(out), n_echoes=more["n_echoes"].cpu().numpy(), fraction=more["echo_fraction"].cpu().numpy())
        for k in OUT:
            _same_bits(got[k], want[k], f"{mode}: {k}")
        res[mode] = got
    # 4. every row's cell in column w0 holds two echoes: three sub-rays (or two, where the central ray grazes the edge) on the
    # plate at about 5 m, the others on the wall at about 10 m
    cells = np.arange(H) * W + w0
    for mode in ec.MODES:
        assert (res[mode]["n_echoes"][cells] == 2).all(), (mode, res[mode]["n_echoes"][cells])
    t = sub_out["range"].reshape(S, n)[:, cells]
    lab = sub_out["endcolors"].reshape(S, n)[:, cells]
    near = (lab == 7).sum(0)
    assert ((near == 3) | (near == 2)).all() and ((lab == 3).sum(0) == S - near).all(), lab
    assert (np.abs(t[lab == 7] - 5.0) < 0.1).all() and (np.abs(t[lab == 3] - 10.0) < 0.2).all()
    first, last = res["first"], res["last"]
    assert (np.abs(first["range"][cells] - 5.0) < 0.1).all() and (first["endcolors"][cells] == 7).all()
    assert (np.abs(last["range"][cells] - 10.0) < 0.2).all() and (last["endcolors"][cells] == 3).all()
    assert np.array_equal(first["fraction"][cells], (near / S).astype(np.float32))
    assert np.array_equal(last["fraction"][cells], ((S - near) / S).astype(np.float32))
    assert np.isin(first["fraction"][cells], np.array([0.6, 0.4], np.float32)).all()
    # the plate returns 0.75 from three sub-rays, the wall 0.25 from two: the plate is the strongest
    assert (res["strongest"]["endcolors"][cells] == 7).all()
    assert np.array_equal(res["strongest"]["endrem"][cells], (near * 0.75 / S).astype(np.float32))
    # a column that sees one surface is the plain render but for the blended range
    one = res["first"]["n_echoes"] == 1
    assert one.sum() > n // 8 and (res["first"]["fraction"][one] == 1).all()
    assert np.array_equal(res["first"]["endcolors"][one], plain["endcolors"][one])
    assert np.array_equal(_bits(res["first"]["endrem"][one]), _bits(plain["endrem"][one]))
    assert np.abs(res["first"]["range"][one] - plain["range"][one]).max() < 1e-3
    # 5. with a separation of 20 m the same cells hold ONE echo whose range lies strictly between the two surfaces
    wide = EchoModel(0.2, S, separation=20.0)
    out = sc.alloc_outputs(n, label_image=True)
    more = post.echo_resolve(rays, origin, wide, sub_dev, out)
    torch.cuda.synchronize()
    r = out["range"].cpu().numpy()[cells]
    assert (more["n_echoes"].cpu().numpy()[cells] == 1).all() and (more["echo_fraction"].cpu().numpy()[cells] == 1).all()
    assert (r > 5.2).all() and (r < 9.8).all(), r
    sub_set.close()
    plain_set.close()
    sc.close()


# ---- the chains -----------------------------------------------------------------------------------------------------------------
SEQ_TARGET = rg.SEQ_TARGET
T_EXAMPLE = tm.T_EXAMPLE
#: a cone wide enough for the F17 sequence's few metres (1 .. 18 m) to hold mixed cells at 32 x 171, a short pulse
ECHO_BLOCK = dict(divergence=1.0, subrays=5, separation=0.3, min_subrays=1, mode="strongest")
NOISE_BLOCK = dict(range_sigma=0.05, range_sigma_rel=0.002, range_resolution=0.004, remission_sigma=0.05, remission_levels=64, seed=5)
GATE_BLOCK = dict(min_range=4.6, max_range=8.0, max_incidence=70.0, drop_rate=0.1, seed=3)


def _echo(**kw):
    from lidar_transfer_amd.config import EchoModel
    return EchoModel(**dict(ECHO_BLOCK, **kw))


def _noise():
    from lidar_transfer_amd.config import NoiseModel
    return NoiseModel(**NOISE_BLOCK)


def _gate():
    from lidar_transfer_amd.config import ReturnModel
    return ReturnModel(**GATE_BLOCK)


@pytest.fixture
def echo_calls(monkeypatch):
    """counts the calls of ``post.echo_resolve`` and ``post.create_subrays`` (the one place each entry is called from)"""
    from lidar_transfer_amd import post
    calls = dict(resolve=[], subrays=[])
    real_r, real_s = post.echo_resolve, post.create_subrays
    monkeypatch.setattr(post, "echo_resolve", lambda *a, **k: (calls["resolve"].append(1), real_r(*a, **k))[1])
    monkeypatch.setattr(post, "create_subrays", lambda *a, **k: (calls["subrays"].append(1), real_s(*a, **k))[1])
    return calls


def _host(out, mesh=None):
    import torch
    torch.cuda.synchronize()
    h = {k: out[k].cpu().numpy().copy() for k in ("range", "rem", "label", "endpoints", "endpoints_scene", "tri", "bin", "label_file",
                                                 "n_echoes", "echo_fraction", "incidence", "drop", "range_error", "noise_state")
         if k in out}
    if mesh is not None:
        h["mesh"] = [t.cpu().numpy().copy() for t in mesh.tensors()]
    return h


def _expect(sub, rays, echo, gate, noise, scan, origin, T=None):
    """what a chain with the models must give, from the PLAIN chain's render ``sub`` of the sub-ray set (and its mesh): the echo
    model restated on it, then the return model, then the noise model, then the frame change and write()'s packing"""
    import oracle_chain as oc
    w = ec.restate_resolve(ec.params_of(echo), rays, origin, sub["range"].reshape(-1), sub["tri"], sub["label"].reshape(-1),
                           sub["rem"].reshape(-1))
    w["echo_fraction"] = w.pop("fraction")
    if gate is not None:
        r = rc.restate(rc.params_of(gate), scan, rays, sub["mesh"][0], sub["mesh"][1], w["tri"], w["range"], w["endrem"], w["endpoints"],
                       w["endcolors"])
        w.update({k: r[k] for k in ("tri", "range", "endrem", "endpoints", "endcolors", "incidence", "drop")})
    if noise is not None:
        r = nc.restate(nc.params_of(noise, gate), scan, origin, w["tri"], w["range"], w["endrem"], w["endpoints"], w["endcolors"])
        w.update({k: r[k] for k in ("tri", "range", "endrem", "endpoints", "endcolors", "range_error")})
        w["noise_state"] = r["state"]
    w["endpoints_target"] = w["endpoints"] if T is None else mc.to_frame(w["endpoints"], T, w["tri"])
    w["bin"], w["label_file"] = oc.pack_write(w["endpoints_target"], w["endcolors"], w["endrem"])
    return w


def _check_result(got, w, tag):
    pairs = [("range", "range"), ("rem", "endrem"), ("label", "endcolors"), ("tri", "tri"), ("endpoints_scene", "endpoints"),
             ("endpoints", "endpoints_target"), ("n_echoes", "n_echoes"), ("echo_fraction", "echo_fraction")]
    pairs += [(k, k) for k in ("incidence", "drop", "range_error", "noise_state") if k in w]
    for gk, wk in pairs:
        _same_bits(got[gk], w[wk], f"{tag}: {gk}")
    if "bin" in got:
        assert got["bin"].tobytes() == w["bin"].tobytes(), (tag, "velodyne bytes")
        assert got["label_file"].view(np.uint32).tobytes() == w["label_file"].astype(np.uint32).tobytes(), (tag, "label bytes")


def _sub_chain(dd, target, a, adaption, mounted):
    """the PLAIN chain (no model) of a target of ``S * t_H`` rows over the sub-rays of ``dd``'s central rays, restated: what the
    echo chain renders, made without any of the echo chain's code but ``lt_create_subrays_dev``"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.raytracer import RaySet
    S = dd.echoes.subrays
    rays = dd.rayset.rays.cpu().numpy()
    want = ec.restate_subrays(rays, dd.echoes.offsets())
    _same_bits(dd._echoes.subrays.cpu().numpy(), want, "the chain's sub-rays")
    sub_rays = torch.from_numpy(want).cuda()
    pose = dd._mounting.P
    rs = RaySet(sub_rays, S * target[0], pose=pose)
    kw = dict(transformation=T_EXAMPLE) if mounted else {}
    chain = DeviceDeform(ev.SOURCE, (S * target[0], target[1], target[2], target[3]), a.voxel_bounds.copy(), a.voxel_size,
                         mesh_volume=adaption == "mesh", rayset=rs, **kw)
    return chain, rs, rays


@pytest.mark.parametrize("mounted,models", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("adaption", ["mesh", "mergemesh"])
def test_device_deform_with_a_model_is_the_sub_render_followed_by_the_restatements(adaption, mounted, models, echo_calls):
    """``models``: the sensor has a return model and a noise model too -- both see the resolved scan, the return model the
    representative's triangle and the CENTRAL rays; ``mounted``: the example mounting and the VLP-32C table.  Two scans each:
    mergemesh's first has no geometry to assume and is rendered twice, the resolve runs once."""
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    g17, g18, a, target = tm._seq_setup(adaption, [])
    kw = dict(transformation=T_EXAMPLE, t_beam_table=bc.VLP32C) if mounted else {}
    if mounted:
        target = SEQ_TARGET
    echo = _echo()
    gate, noise = (_gate(), _noise()) if models else (None, None)
    if models:
        kw.update(returns=gate, noise=noise)
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    indices = [int(x) for x in a.scan_indices(8)[:2]]
    with DeviceDeform(ev.SOURCE, target, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=adaption == "mesh", echoes=echo, **kw) as dd:
        assert dd.echoes == echo and echo_calls["subrays"] == [1]
        origin, T = dd.origin, (dd.mount[0] if mounted else None)
        assert np.any(origin) == mounted
        chain, rs, rays = _sub_chain(dd, target, a, adaption, mounted)
        with chain:
            for idx in indices:
                sub = _host(chain.deform(adaption, ing, idx), chain.mesh_obj)
                assert echo_calls["resolve"] == [1] * indices.index(idx)
                got = _host(dd.deform(adaption, ing, idx, scan_index=idx))
                w = _expect(sub, rays, echo, gate, noise, idx, origin, T)
                tag = f"{adaption}/mounted={mounted}/models={models}/scan {idx}"
                _check_result(got, w, tag)
                count = np.bincount(w["n_echoes"], minlength=3)
                print(f"\n{tag}: cells per number of echoes {count.tolist()}, {w['bin'].shape[0]} points written")
                assert count[0] > 0 and count[1] > 500 and count[2:].sum() > 20, count
                mixed = (w["n_echoes"] >= 2) & (got["tri"] >= 0)
                assert (got["echo_fraction"][mixed] < 1).all() and w["bin"].shape[0] > 50
            if adaption == "mergemesh":
                stats = dict(dd._mm().stats)
                assert stats["scans"] == 2 and stats["waited"] + stats["rerun"] >= 1, stats
        rs.close()
    assert echo_calls["resolve"] == [1, 1] and echo_calls["subrays"] == [1]   # once per output scan, re-run or not
    src.close()


@pytest.mark.parametrize("chains", [1, 3])
def test_fusion_pipeline_with_one_and_three_scans_in_flight_equals_device_deform(chains, echo_calls):
    """six output scans (the sequence's, then again) through ``submit_mergemesh`` and ``submit_clouds`` against one DeviceDeform
    scan after scan; the pipeline makes its sub-rays ONCE, for all its chains"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.pipeline import FusionScanPipeline
    echo, gate, noise = _echo(), _gate(), _noise()
    g17, g18, a, target = tm._seq_setup("mergemesh", [])
    am = sq.approach_for(g18, "mesh")
    src = tm._source(g17)
    rays = create_rays_device(target[2], target[3], target[0], target[1], device=0)
    order = [int(x) for x in a.scan_indices(8)]
    order = (order * 6)[:6]
    keys = ("range", "endrem", "endcolors", "endpoints", "tri", "n_echoes", "echo_fraction", "range_error", "noise_state", "drop")
    host = lambda r: {k: r[k].cpu().numpy().copy() for k in keys}   # noqa: E731
    names = dict(endrem="rem", endcolors="label")
    for adaption, ap, merged in (("mergemesh", a, True), ("mesh", am, False)):
        ing = ScanIngest(src, ap)
        more = dict(fixed_volume=False) if merged else {}
        fov = (target[2], target[3]) if merged else (ev.SOURCE[2], ev.SOURCE[3])
        before = len(echo_calls["subrays"])
        with FusionScanPipeline(ap.voxel_bounds.copy(), ap.voxel_size, fov[0], fov[1], rays, target[0], chains=chains, device=0,
                                label_image=True, source_hw=ev.SOURCE[:2], returns=gate, noise=noise, echoes=echo, **more) as pipe:
            assert pipe.echoes == echo
            submit = pipe.submit_mergemesh if merged else pipe.submit_clouds
            tickets = []
            for k, idx in enumerate(order):
                clouds = ing.prepare(idx, merged=merged)
                torch.cuda.synchronize()
                tickets.append(submit(clouds, inputs_ready=True, scan_index=40 + k))
            got = [host(pipe.wait(t)) for t in tickets]
        assert len(echo_calls["subrays"]) == before + 1
        with pytest.raises(ValueError, match="label_image"):
            FusionScanPipeline(ap.voxel_bounds.copy(), ap.voxel_size, fov[0], fov[1], rays, target[0], chains=1, device=0,
                               source_hw=ev.SOURCE[:2], echoes=echo, **more)
        with DeviceDeform(ev.SOURCE, target, ap.voxel_bounds.copy(), ap.voxel_size, mesh_volume=not merged, returns=gate,
                          noise=noise, echoes=echo) as dd:
            for k, idx in enumerate(order):
                s = getattr(dd, adaption)(ing.prepare(idx, merged=merged), pack=False, scan_index=40 + k)
                torch.cuda.synchronize()
                for key in keys:
                    want = s[names.get(key, key)].cpu().numpy()
                    _same_bits(got[k][key], want, f"{adaption}/{chains} chains/scan {k}: {key}")
                assert (got[k]["n_echoes"] >= 2).sum() > 20
    src.close()


def _target_sensor(echo_block, return_block=None, noise_block=None, **kw):
    from lidar_transfer_amd.config import load_sensor
    tH, tW, tfu, tfd = SEQ_TARGET
    cfg = dict(name="VLP-32C table with an echo model", fov_up=tfu, fov_down=tfd, beams=tH, angle_res_hor=360.0 / tW, fov_hor=360.0,
               beam_model="table", beam_angles=[float(x) for x in bc.VLP32C])
    for key, block in (("echo_model", echo_block), ("return_model", return_block), ("noise_model", noise_block)):
        if block is not None:
            cfg[key] = block
    cfg.update(kw)
    return load_sensor(cfg)


def _run_sequence(a, target, out_dir, chains, **kw):
    from lidar_transfer_amd.sequence import SequenceTransfer
    g17, g18 = cpu.gold(), sq.gold18()
    src = tm._source(g17)
    with SequenceTransfer(src, a, ev.SOURCE, target, out_dir=str(out_dir) if out_dir is not None else None, chains=chains,
                          nclasses=int(g18["nclasses"]), **kw) as tr:
        recs = list(tr.run())
        summary, echoes = tr.summary, tr.echoes
    src.close()
    return recs, summary, echoes


def test_a_sequence_writes_the_restated_files_with_one_chain_and_with_three(tmp_path, echo_calls):
    """the mergemesh sequence with a table target, an echo model, a gate and a noise model: every file is write() of the three
    restatements on the plain chain's sub-render of that FILE index; the totals are the restatement's"""
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.sequence import format_echo_totals
    g17, g18, a, _ = tm._seq_setup("mergemesh", [])
    sensor = _target_sensor(ECHO_BLOCK, GATE_BLOCK, NOISE_BLOCK)
    echo, gate, noise = sensor.echo_model(), sensor.return_model(), sensor.noise_model()
    r1, s1, e1 = _run_sequence(a, sensor, tmp_path / "c1", 1)
    assert echo_calls["resolve"] == [1] * len(r1) and echo_calls["subrays"] == [1]
    assert s1["mm_stats"]["waited"] + s1["mm_stats"]["rerun"] >= 1            # once per scan, re-runs included
    r3, s3, _ = _run_sequence(a, sensor, tmp_path / "c3", 3)
    assert e1 == echo == _echo() and s3["chains"] == 3 and len(echo_calls["resolve"]) == 2 * len(r1)
    assert echo_calls["subrays"] == [1, 1]                                     # three chains, one sub-ray set
    indices = [r["idx"] for r in r1]
    assert indices == [r["idx"] for r in r3] == [int(x) for x in a.scan_indices(8)] and len(indices) >= 3
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    total, share = np.zeros(3, np.int64), 0.0
    with DeviceDeform(ev.SOURCE, SEQ_TARGET, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=False, t_beam_table=bc.VLP32C,
                      echoes=echo) as dd:
        chain, rs, rays = _sub_chain(dd, SEQ_TARGET, a, "mergemesh", False)
    n_before = len(echo_calls["resolve"])
    with chain:
        for rec in r1:
            idx = rec["idx"]
            w = _expect(_host(chain.deform("mergemesh", ing, idx), chain.mesh_obj), rays, echo, gate, noise, idx, (0.0, 0.0, 0.0))
            total += np.bincount(np.minimum(w["n_echoes"], 2), minlength=3)
            share += float(w["echo_fraction"].astype(np.float64).sum())
            b1, l1 = tm._read(tmp_path / "c1", idx)
            assert b1 == w["bin"].tobytes(), f"scan {idx}: velodyne file"
            assert l1 == w["label_file"].astype(np.uint32).tobytes(), f"scan {idx}: label file"
            assert rec["n_points"] == w["bin"].shape[0]
            assert (b1, l1) == tm._read(tmp_path / "c3", idx), f"scan {idx}: one chain vs three"
    rs.close()
    src.close()
    assert len(echo_calls["resolve"]) == n_before
    assert s1["echo_totals"] == s3["echo_totals"] == total.tolist() and min(total) > 0
    assert int(total.sum()) == len(indices) * SEQ_TARGET[0] * SEQ_TARGET[1]
    mean = share / (total[1] + total[2])
    assert abs(s1["echo_fraction_mean"] - mean) <= 1e-9 and abs(s3["echo_fraction_mean"] - mean) <= 1e-9 and 0.5 < mean <= 1.0
    assert s1["return_totals"] is not None and s1["noise_totals"] is not None
    print("\n" + format_echo_totals(s1["echo_totals"], s1["echo_fraction_mean"]))


@pytest.mark.parametrize("adaption", ["cp", "mesh", "mergemesh"])
def test_without_the_key_and_with_a_model_that_is_off_nothing_changes(adaption, echo_calls):
    """no new keys, the bytes of the path without ``echoes=``, and neither wrapper is ever called"""
    import torch
    from lidar_transfer_amd.config import EchoModel
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    g17, g18, a, target = tm._seq_setup(adaption, [])
    sensors = [_target_sensor(None), _target_sensor({}), _target_sensor(dict(EchoModel.DEFAULTS)),
               _target_sensor(dict(divergence=0.2)), _target_sensor(dict(subrays=5, mode="first"))]
    assert all(s.echo_model() is None for s in sensors)
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    res = []
    for kw in ({}, dict(echoes=None), dict(echoes=sensors[1].echo_model()), dict(echoes=EchoModel()), dict(echoes=EchoModel(0.2)),
               dict(echoes=EchoModel(subrays=5))):
        bnds = None if adaption == "cp" else a.voxel_bounds.copy()
        with DeviceDeform(ev.SOURCE, target, bnds, a.voxel_size, mesh_volume=adaption == "mesh", **kw) as dd:
            assert dd.echoes is None and not dd._echoes and dd._echoes.rayset is None
            outs = []
            for idx in a.scan_indices(8)[:2]:
                out = dd.deform(adaption, ing, idx)
                torch.cuda.synchronize()
                assert "n_echoes" not in out and "echo_fraction" not in out
                outs.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
            res.append(outs)
    for other in res[1:]:
        for x, y in zip(res[0], other):
            tm._same(x, y, adaption)
    assert res[0][0]["bin"].shape[0] > 100
    src.close()
    assert echo_calls == dict(resolve=[], subrays=[])


def test_sequences_without_the_key_write_the_bytes_they_wrote(tmp_path, echo_calls):
    g17, g18, a, _ = tm._seq_setup("mergemesh", [])
    r0, s0, e0 = _run_sequence(a, _target_sensor(None), tmp_path / "none", 1)
    r1, s1, e1 = _run_sequence(a, _target_sensor({}), tmp_path / "default", 3)
    r2, s2, _ = _run_sequence(a, SEQ_TARGET, tmp_path / "tuple", 1)       # (a plain tuple has no model)
    assert e0 is None and e1 is None and echo_calls == dict(resolve=[], subrays=[])
    for s in (s0, s1, s2):
        assert s["echo_totals"] is None and s["echo_fraction_mean"] is None
    for rec in r0:
        assert tm._read(tmp_path / "none", rec["idx"]) == tm._read(tmp_path / "default", rec["idx"])
        assert "n_echoes" not in rec and "echo_fraction" not in rec
    with_key, _, _ = _run_sequence(a, _target_sensor(ECHO_BLOCK), tmp_path / "echo", 1)
    assert tm._read(tmp_path / "echo", r0[0]["idx"]) != tm._read(tmp_path / "none", r0[0]["idx"])


def test_cp_with_a_model_raises():
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.sequence import SequenceTransfer
    model = _echo()
    g17, g18, a, target = tm._seq_setup("cp", [])
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    with DeviceDeform(ev.SOURCE, target, None, echoes=model) as dd:
        with pytest.raises(ValueError, match="cp renders no ray"):
            dd.deform("cp", ing, int(a.scan_indices(8)[0]))
        with pytest.raises(ValueError, match="cp renders no ray"):
            dd.cp(ing.prepare(int(a.scan_indices(8)[0]), merged=True))
    with pytest.raises(ValueError, match="cp renders no ray.*echo_model"):
        SequenceTransfer(src, a, ev.SOURCE, _target_sensor(ECHO_BLOCK))
    with pytest.raises(ValueError, match="target sensors only"):
        SequenceTransfer(src, sq.approach_for(g18, "mesh"), _target_sensor(ECHO_BLOCK, beam_model="linear"), SEQ_TARGET)
    with pytest.raises(ValueError, match="EchoModel"):
        DeviceDeform(ev.SOURCE, target, None, echoes=ECHO_BLOCK)
    src.close()


def test_the_cli_closes_with_the_cells_per_number_of_echoes_and_refuses_cp(tmp_path):
    """the shipped file through ``python -m lidar_transfer_amd`` in a child process: the closing line is the summary's, which the
    log carries; every row says ``"echo_model": true``; ``cp`` ends with a message and status 1 before any device work"""
    import json
    import subprocess
    from lidar_transfer_amd.sequence import format_echo_totals
    shipped = os.path.join(ROOT, "config", "vlp32c_table_echo_1024.yaml")
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
    tot, mean = summary["echo_totals"], summary["echo_fraction_mean"]
    assert len(rows) == 2 and rows[0]["echo_model"] is True
    assert sum(tot) == 32 * 1024 and tot[1] > 1000 and 0.5 < mean <= 1.0
    assert sum(summary["return_totals"]) == sum(summary["noise_totals"]) == 32 * 1024
    lines = [x for x in res.stdout.splitlines() if x.startswith("Echoes:")]
    assert lines == [format_echo_totals(tot, mean)], (lines, tot, mean)
    assert [x for x in res.stdout.splitlines() if x.startswith("Returns:")] and [x for x in res.stdout.splitlines() if x.startswith("Noise:")]
    alone = tmp_path / "echo_alone.yaml"                                   # the shipped file with its echo model alone
    text = open(shipped).read()
    alone.write_text(text[:text.index("return_model:")] + text[text.index("echo_model:"):])
    res = subprocess.run(base + ["-c", str(cfgs["cp"]), "-t", str(alone)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 1 and "cp renders no ray" in res.stdout and "echo_model" in res.stdout
