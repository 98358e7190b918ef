"""Dual-return target sensors without a GPU: the ``dual_return`` block and its messages, the sample file, the new
entry in the header and the binding, the numpy restatement of tests/dual_return_cases.py held to ``echo_cases`` and to what
the hand-written cells must give, and a census of the random cases the GPU tests resolve."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import dual_return_cases as dc  # noqa: E402
import echo_cases as ec  # noqa: E402

ECHO = dict(divergence=0.2, subrays=5)


def _sensor(**kw):
    from lidar_transfer_amd.config import load_sensor
    cfg = dict(name="dual", fov_up=10.0, fov_down=-10.0, beams=8, angle_res_hor=360.0 / 64, fov_hor=360.0)
    cfg.update(kw)
    return load_sensor(cfg)


# ---- the block --------------------------------------------------------------------------------------------------------------
def test_the_block_is_validated_by_its_constructor_with_messages_led_by_the_sensor():
    from lidar_transfer_amd.config import DualReturn, _ModelBlock
    assert issubclass(DualReturn, _ModelBlock) and DualReturn.KEY == "dual_return" and DualReturn.DEFAULTS == dict(second="none")
    for second in ("first", "strongest", "last"):
        s = _sensor(echo_model=ECHO, dual_return=dict(second=second))
        d = s.dual_return()
        assert d == DualReturn(second) and d.second == second and d.mode == ec.MODES.index(second) and not d.is_default
    with pytest.raises(ValueError, match=r"sensor 'dual': dual_return has unknown key\(s\) mode"):
        _sensor(echo_model=ECHO, dual_return=dict(mode="last"))
    with pytest.raises(ValueError, match="sensor 'dual': dual_return must be a mapping of second"):
        _sensor(echo_model=ECHO, dual_return="last")
    for bad in ("weakest", 2, None, True, ["last"]):
        with pytest.raises(ValueError, match="sensor 'dual': dual_return second must be one of none, first, strongest, last"):
            _sensor(echo_model=ECHO, dual_return=dict(second=bad))
    with pytest.raises(AttributeError):
        DualReturn("last").second = "first"
    with pytest.raises(ValueError, match="no second_mode"):
        DualReturn().mode


def test_none_is_the_absence_of_the_key():
    from lidar_transfer_amd.config import DualReturn
    assert DualReturn().is_default and DualReturn.of(dict(second="none")) is None and DualReturn.of({}) is None
    assert DualReturn.of(None) is None and DualReturn.of(DualReturn()) is None
    for kw in ({}, dict(dual_return={}), dict(dual_return=dict(second="none")), dict(echo_model=ECHO),
               dict(echo_model=ECHO, dual_return=dict(second="none"))):
        assert _sensor(**kw).dual_return() is None, kw


def test_on_without_an_echo_model_is_refused_at_load_time():
    for kw in ({}, dict(echo_model=dict(divergence=0.2)), dict(echo_model=dict(subrays=5)), dict(echo_model={})):
        with pytest.raises(ValueError, match="^sensor 'dual': .*second return needs an echo_model with a divergence and at "
                                             "least two sub-rays"):
            _sensor(dual_return=dict(second="last"), **kw)


def test_a_source_sensor_with_the_key_is_refused():
    from lidar_transfer_amd.config import refuse_source_models
    with pytest.raises(ValueError, match="source sensor 'dual': dual_return is for target sensors only"):
        refuse_source_models(_sensor(dual_return=dict(second="none")))
    refuse_source_models(_sensor())


def test_the_chain_objects_take_the_setting_and_refuse_what_cannot_be():
    from lidar_transfer_amd import _chain
    from lidar_transfer_amd.config import DualReturn, EchoModel
    echo = EchoModel(**ECHO)
    assert not _chain.Sensing(None, None, None, echo, "t").dual and "second" not in _chain.Sensing(None, None, None, echo, "t").keys
    assert not _chain.Sensing(None, None, None, echo, "t", DualReturn()).dual
    s = _chain.Sensing(None, None, None, echo, "t", DualReturn("last"))
    assert s.dual and s.dual.setting == DualReturn("last") and s.keys == ("n_echoes", "echo_fraction", "second")
    with pytest.raises(ValueError, match="t: dual= needs echoes="):
        _chain.Sensing(None, None, None, None, "t", DualReturn("last"))
    with pytest.raises(ValueError, match="t: dual= takes a lidar_transfer_amd.config.DualReturn"):
        _chain.Sensing(None, None, None, echo, "t", dict(second="last"))
    assert _chain.SECOND_SEED_XOR == dc.SECOND_SEED_XOR == 0x9E3779B9
    assert _chain.CP_REFUSALS["dual"][0] == "dual_return"


def test_the_sample_file_loads():
    from lidar_transfer_amd.config import DualReturn, load_sensor
    dual = load_sensor(os.path.join(ROOT, "config", "vlp32c_table_dual_1024.yaml"))
    echo = load_sensor(os.path.join(ROOT, "config", "vlp32c_table_echo_1024.yaml"))
    assert dual.dual_return() == DualReturn("last") and echo.dual_return() is None
    assert dual.echo_model() == echo.echo_model() and dual.echo_model().mode == "strongest"
    assert dual.return_model() == echo.return_model() and dual.noise_model() == echo.noise_model()
    assert np.array_equal(dual.beam_table(), echo.beam_table()) and (dual.H, dual.W) == (32, 1024)
    text = open(os.path.join(ROOT, "config", "vlp32c_table_dual_1024.yaml")).read()
    assert "not a calibration" in text


# ---- the entry --------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entry_and_the_binding_carries_it():
    from lidar_transfer_amd import _lib
    text = open(os.path.join(ROOT, "include", "lidarhip.h")).read()
    m = re.search(r"int lt_echo_resolve_dual_dev\(([^;]*)\);", text)
    assert m, "include/lidarhip.h does not declare lt_echo_resolve_dual_dev"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 23 and args[4] == "unsigned second_mode" and args[-1] == "void* stream"
    assert [a.split()[-1].lstrip("*") for a in args[-7:-1]] == ["endpoints2", "endcolors2", "range2", "endrem2", "tri2", "fraction2"]
    single = re.search(r"int lt_echo_resolve_dev\(([^;]*)\);", text).group(1)
    assert len(single.split(",")) == 16                                       # (the existing entry keeps its signature)
    assert "lt_echo_resolve_dual_dev" in _lib.SYMBOLS and "lt_echo_resolve_dev" in _lib.SYMBOLS
    assert _lib.LT_ABI_VERSION == 10 and re.search(r"#define LT_ABI_VERSION 10\b", text)
    import ctypes as C
    assert C.sizeof(_lib.EchoModelArgs) == 152


# ---- the restatement --------------------------------------------------------------------------------------------------------
CASES = [(n, S) for S in (5, 8) for n in (255, 257, 1000)]


@pytest.mark.parametrize("min_subrays", [1, 2])
def test_the_primary_of_every_pair_is_the_single_restatement(min_subrays):
    cases = [ec.resolve_case(257, S) for S in (2, 5, 8)] + [dc.crafted_cells(), ec.crafted_cells()]
    for case in cases:
        S = case["range"].size // case["rays"].shape[0]
        for mode, second in dc.PAIRS:
            p = ec.params(ec.offsets(0.2, S), 0.5, min(min_subrays, S), mode)
            one, two = dc.restate_resolve_dual(p, second, case["rays"], case["origin"], case["range"], case["tri"], case["label"],
                                               case["rem"])
            want = ec.restate_resolve(p, case["rays"], case["origin"], case["range"], case["tri"], case["label"], case["rem"])
            for k, v in want.items():
                assert np.array_equal(one[k].view(np.uint8), v.view(np.uint8)), (S, mode, second, k)
            # the second: a hit exactly where two echoes were detected on a ray that is one; never the primary's echo
            ok = (want["n_echoes"] >= 2) & (want["tri"] >= 0)
            assert np.array_equal(two["tri"] >= 0, ok), (S, mode, second)
            assert (two["fraction"][~ok] == 0).all() and (two["range"][~ok] == 0).all() and not two["endpoints"][~ok].any()
            both = (one["fraction"].astype(np.float64) + two["fraction"])[ok]
            assert (both <= 1.0 + 1e-6).all() and (two["range"][ok] != one["range"][ok]).all()
            if (mode, second) in (("first", "last"), ("first", "first"), ("first", "strongest")):
                assert (two["range"][ok] > one["range"][ok]).all()
            if mode == "last":
                assert (two["range"][ok] < one["range"][ok]).all()


def _cell(name, mode, second, min_subrays=1):
    c = dc.crafted_cells()
    i = c["names"].index(name)
    p = ec.params(ec.offsets(0.2, 5), 0.5, min_subrays, mode)
    one, two = dc.restate_resolve_dual(p, second, c["rays"], c["origin"], c["range"], c["tri"], c["label"], c["rem"])
    pick = lambda d: {k: d[k][i] for k in d}   # noqa: E731
    return pick(one), pick(two), i


def test_the_hand_written_cells_give_what_their_names_say():
    f = np.float32
    name = "three echoes, the strongest in the middle"
    one, two, i = _cell(name, "strongest", "first")
    assert one["range"] == f(7.05) and two["range"] == 4.0 and one["n_echoes"] == 3 and two["fraction"] == f(0.2)
    assert _cell(name, "strongest", "last")[1]["range"] == 11.0 and _cell(name, "strongest", "strongest")[1]["range"] == 11.0
    assert _cell(name, "first", "first")[1]["range"] == f(7.05) and _cell(name, "last", "last")[1]["range"] == f(7.05)
    name = "three echoes, the strongest is the last"       # the model's ONE rule: the latest of the others, not the runner-up
    one, two, i = _cell(name, "strongest", "last")
    assert one["range"] == f(11.05) and two["range"] == 7.0 and two["tri"] == 1000 * i + 1 and two["endcolors"] == 100 + 10 * i + 1
    assert _cell(name, "strongest", "first")[1]["range"] == 4.0 and _cell(name, "strongest", "strongest")[1]["range"] == 7.0
    name = "two echoes, min_subrays = 2 removes one"
    for mode, second in dc.PAIRS:
        one, two, _ = _cell(name, mode, second, 2)
        assert one["n_echoes"] == 1 and one["range"] == f(9.05) and two["tri"] == -1 and two["range"] == 0 and two["fraction"] == 0
        one, two, _ = _cell(name, mode, second, 1)
        assert one["n_echoes"] == 2 and two["tri"] >= 0 and {float(one["range"]), float(two["range"])} == {4.0, float(f(9.05))}
        for name2 in ("all sub-hits in one echo", "all misses"):
            one, two, _ = _cell(name2, mode, second)
            assert one["n_echoes"] == (name2 != "all misses") and two["tri"] == -1 and two["fraction"] == 0 and two["endcolors"] == 0
        one, two, _ = _cell("a zero central ray with two echoes", mode, second)
        assert one["n_echoes"] == 2 and one["tri"] == -1 and two["tri"] == -1 and two["range"] == 0 and two["fraction"] == 0
    one, two, _ = _cell("the rest ties on Srem, the count decides", "strongest", "strongest")
    assert one["range"] == f(3.05) and two["range"] == f(9.05) and two["fraction"] == f(0.4) and two["endrem"] == f(0.1)
    one, two, _ = _cell("the rest ties on Srem and the count, the earlier decides", "strongest", "strongest")
    assert one["range"] == f(3.05) and two["range"] == 6.0 and two["endrem"] == f(0.1)
    name = "the second's representative is the centre, the primary's is not"
    one, two, i = _cell(name, "first", "last")
    assert one["tri"] == 1000 * i + 1 and two["tri"] == 1000 * i and two["endcolors"] == 100 + 10 * i
    assert two["range"] == f((np.float64(f(10.0)) + np.float64(f(10.04))) / 2)
    h = np.array([0.6, 0.0, 0.8], f).astype(np.float64)
    h = h / np.sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2])
    assert np.abs(two["endpoints"].astype(np.float64) - h * np.float64(two["range"])).max() < 2e-6   # on the CENTRAL ray


@pytest.mark.parametrize("n,S", CASES)
def test_census_of_the_random_cases(n, S):
    """the GPU tests cannot pass vacuously: the random cases hold cells with two and with three echoes, and cells whose
    strongest echo lies strictly between two others (minima over the six cases: 0.425, 0.067, 8 cells)"""
    m, between = dc.census(ec.params(ec.offsets(0.2, S), 0.5, 1, "strongest"), ec.resolve_case(n, S))
    print(f"\nn={n} S={S}: two or more {np.mean(m >= 2):.3f}, three or more {np.mean(m >= 3):.3f}, strongest between {between}")
    assert np.mean(m >= 2) >= 0.4
    assert np.mean(m >= 3) >= 0.05
    assert between >= 5


# ---- the chain's order, with recording fakes in place of ``post``'s wrappers (as tests/test_chain_cpu.py does) ---------------
@pytest.mark.parametrize("mounted", [False, True])
def test_sensing_owns_the_layout_the_order_and_the_seeds(monkeypatch, mounted):
    import torch

    import test_chain_cpu as cc
    from lidar_transfer_amd import _chain, post, raytracer
    from lidar_transfer_amd.config import DualReturn
    calls = []

    def fake(name, keys):
        def f(*args, **kw):
            calls.append((name, args, kw))
            return {k: object() for k in keys}
        return f
    monkeypatch.setattr(post, "echo_resolve_dual", fake("dual", ("n_echoes", "echo_fraction", "echo_fraction2")))
    monkeypatch.setattr(post, "echo_resolve", fake("single", _chain.Echoes.KEYS))
    monkeypatch.setattr(post, "return_model", fake("return", _chain.Returns.KEYS))
    monkeypatch.setattr(post, "noise_model", fake("noise", _chain.Noise.KEYS))
    monkeypatch.setattr(post, "points_to_frame", fake("frame", ()))
    monkeypatch.setattr(post, "create_subrays", lambda rays, model: rays.repeat(model.subrays, 1))
    monkeypatch.setattr(raytracer, "RaySet", cc._RaySet)
    N, T_H = cc.N, cc.T_H
    returns, noise, echoes = cc._models()
    second = DualReturn("last")
    rays = torch.arange(3 * N, dtype=torch.float32).reshape(N, 3)
    s = _chain.Sensing(cc.MOUNT if mounted else None, returns, noise, echoes, "test", second).bind(rays, T_H)
    assert s.keys == ("incidence", "drop", "range_error", "noise_state", "n_echoes", "echo_fraction", "second")
    out = cc._out()
    given = dict(out)
    rout, sub = s.plan(out, N, "cpu")
    # the layout: the scan's images are plane 0 of allocations of 2 N cells, the render still writes the sub-images
    for k in _chain.OUT_KEYS:
        assert out[k] is not given.get(k) and out[k].shape[0] == N and out[k]._base is not None and out[k]._base.shape[0] == 2 * N
        assert out[k].data_ptr() == out[k]._base.data_ptr() and out[k].is_contiguous()
    assert (rout["endpoints"] is out["endpoints"]) == (not mounted) and all(rout[k] is out[k] for k in _chain.OUT_KEYS[1:])
    assert sub["endpoints"] is None and sub["range"].numel() == cc.S * N
    scene, stream, origin = object(), object(), (0.5, 0.25, -1.0)
    seen = s.finish(out, rout, sub, 7, scene, rays, origin, stream)
    assert [c[0] for c in calls] == ["dual", "return", "return", "noise", "noise"] + (["frame"] if mounted else [])
    (_, a, kw) = calls[0]
    assert a[0] is rays and a[1] == origin and a[2] is echoes and a[3] is second and a[4] is sub and a[5] is rout
    plane1 = a[6]
    for k in _chain.OUT_KEYS:                                   # plane 1 follows plane 0 in the same allocation
        assert plane1[k]._base is rout[k]._base and plane1[k].data_ptr() == rout[k].data_ptr() + rout[k].numel() * 4
    # each model on the primary exactly as without the setting, then on plane 1 with the xor-ed seed
    assert calls[1][1][4] is rout and calls[1][2] == dict(label_image=True, stream=stream)
    assert calls[2][1][4] is plane1 and calls[2][2] == dict(label_image=True, stream=stream, seed_xor=0x9E3779B9)
    assert calls[3][1][3] is rout and "seed_xor" not in calls[3][2] and calls[3][2]["gate"] is returns
    assert calls[4][1][3] is plane1 and calls[4][2]["seed_xor"] == 0x9E3779B9 and calls[4][2]["gate"] is returns
    assert calls[1][1][3] == calls[2][1][3] == calls[3][1][2] == calls[4][1][2] == 7
    sec = seen["second"]
    if mounted:                                                 # ONE frame change over both planes
        (_, a, kw) = calls[5]
        assert a[0] is rout["endpoints"]._base and a[0].shape == (2 * N, 3) and kw["out"] is out["endpoints"]._base
        assert kw["tri"] is rout["tri"]._base and kw["stream"] is stream
        assert sec["endpoints_scene"]._base is rout["endpoints"]._base
    assert set(sec) == {"range", "rem", "label", "endpoints", "endpoints_scene", "tri", "echo_fraction", "incidence", "drop",
                        "range_error", "noise_state", "_planes"}
    assert sec["range"].shape == (T_H, N // T_H) and sec["label"].dtype == torch.int32 and sec["endpoints"].shape == (N, 3)
    assert sec["endpoints"]._base is out["endpoints"]._base and sec["range"]._base is out["range"]._base
    planes = sec["_planes"]                                      # what ONE packing over 2 N cells reads
    assert planes["endpoints"] is out["endpoints"]._base and planes["rem"] is out["endrem"]._base
    assert planes["label"] is out["endcolors"]._base
    assert "echo_fraction2" not in seen and tuple(k for k in seen if k != "second") == (
        "n_echoes", "echo_fraction", "incidence", "drop", "range_error", "noise_state")
