"""The target sensor's echo model without a GPU: the loader (``config.EchoModel``, ``SensorModel.echo_model``), the
offsets table and the geometry of the restated sub-rays, the restatement's own rules on hand-written cells, the analytic
two-plane check of the end-to-end scene, the layout of ``lt_echo_model`` against the header compiled as C, and the command
line's refusal of ``cp``."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import echo_cases as ec  # noqa: E402

SHIPPED = os.path.join(ROOT, "config", "vlp32c_table_echo_1024.yaml")
ON = dict(divergence=0.2, subrays=5)


def _sensor(**kw):
    cfg = dict(name="ech", fov_up=3.0, fov_down=-25.0, beams=16, angle_res_hor=360.0 / 130, fov_hor=360.0)
    cfg.update(kw)
    return cfg


# ---- config ------------------------------------------------------------------------------------------------------------------------
def test_defaults_are_no_model():
    from lidar_transfer_amd.config import EchoModel, load_sensor
    assert load_sensor(_sensor()).echo_model() is None
    assert load_sensor(_sensor(echo_model={})).echo_model() is None
    assert load_sensor(_sensor(echo_model=dict(EchoModel.DEFAULTS))).echo_model() is None
    assert load_sensor(_sensor(echo_model=dict(divergence=0.2))).echo_model() is None             # one ray per cell
    assert load_sensor(_sensor(echo_model=dict(subrays=5, mode="last"))).echo_model() is None      # a beam without a width
    assert load_sensor(_sensor(echo_model=dict(divergence=0, subrays=8, separation=2.0))).echo_model() is None
    assert EchoModel.of(None) is None and EchoModel.of(EchoModel()) is None and EchoModel.of(EchoModel(0.2)) is None
    assert EchoModel.DEFAULTS == dict(divergence=0.0, subrays=1, ring=0.7071, separation=0.5, min_subrays=1, mode="strongest")
    m = load_sensor(_sensor(echo_model=ON)).echo_model()
    assert m is not None and m.fields() == dict(EchoModel.DEFAULTS, **ON)
    with pytest.raises(AttributeError):
        m.subrays = 2
    assert m == EchoModel(0.2, 5) and m != EchoModel(0.2, 5, mode="first") and hash(m) == hash(EchoModel(0.2, 5))
    assert EchoModel.of(m) is m
    # the two other models are what they were
    s = load_sensor(_sensor(echo_model=ON))
    assert s.return_model() is None and s.noise_model() is None


@pytest.mark.parametrize("block", [
    dict(divergence=-0.1), dict(divergence=float("nan")), dict(divergence=float("inf")), dict(divergence="wide"),
    dict(divergence=True), dict(divergence=None), dict(divergence=180.0), dict(subrays=0), dict(subrays=9), dict(subrays=2.0),
    dict(subrays=True), dict(subrays="5"), dict(ring=0.0), dict(ring=-0.5), dict(ring=1.5), dict(ring=float("nan")),
    dict(separation=0.0), dict(separation=-1.0), dict(separation=float("inf")), dict(separation=float("nan")),
    dict(separation="0.5"), dict(subrays=5, min_subrays=0), dict(subrays=5, min_subrays=6), dict(min_subrays=2),
    dict(subrays=5, min_subrays=1.0), dict(mode="loudest"), dict(mode=1), dict(mode=None), dict(rays=5), dict(seed=1),
    [0.2, 5], "gaussian", 0.2])
def test_a_block_that_cannot_be_used_is_refused_at_load_time_by_the_sensors_name(block):
    from lidar_transfer_amd.config import load_sensor
    with pytest.raises(ValueError, match="sensor 'ech'.*echo_model"):
        load_sensor(_sensor(echo_model=block))


def test_a_source_sensor_with_the_key_is_refused():
    from lidar_transfer_amd.config import load_sensor, refuse_source_models
    refuse_source_models(load_sensor(_sensor()))
    for block in (ON, {}):
        with pytest.raises(ValueError, match="source sensor 'ech'.*echo_model.*target"):
            refuse_source_models(load_sensor(_sensor(echo_model=block)))


def test_the_shipped_file_loads_and_is_the_noise_file_plus_the_block():
    from lidar_transfer_amd.config import EchoModel, load_sensor
    s = load_sensor(SHIPPED)
    t = load_sensor(os.path.join(ROOT, "config", "vlp32c_table_noise_1024.yaml"))
    assert s.echo_model() == EchoModel(0.17, 5, 0.7071, 0.5, 1, "strongest") and t.echo_model() is None
    assert s.return_model() == t.return_model() is not None and s.noise_model() == t.noise_model() is not None
    assert s.target_model() == t.target_model()
    assert (s.H, s.W, s.fov_up, s.fov_down) == (t.H, t.W, t.fov_up, t.fov_down) == (32, 1024, 15.0, -25.0)
    assert "not a calibration" in open(SHIPPED).read()


def test_the_struct_is_the_models_fields():
    from lidar_transfer_amd import _lib
    from lidar_transfer_amd.config import EchoModel
    m = EchoModel(0.2, 5, 0.5, 0.75, 2, "last")
    a = m.args()
    off = m.offsets()
    assert list(a.off)[:10] == off.ravel().tolist() and not any(list(a.off)[10:])
    assert (a.separation, a.n_subrays, a.min_subrays, a.mode, a.reserved) == (0.75, 5, 2, _lib.LT_ECHO_LAST, 0)
    assert [EchoModel(0.2, 2, mode=x).args().mode for x in ec.MODES] == [_lib.LT_ECHO_FIRST, _lib.LT_ECHO_STRONGEST, _lib.LT_ECHO_LAST]
    assert EchoModel.MODES == ec.MODES and EchoModel.MAX_SUBRAYS == _lib.LT_ECHO_MAX_SUBRAYS == ec.MAX_SUBRAYS == 8
    p = ec.params_of(m)
    assert np.array_equal(p["off"], off) and (p["S"], p["separation"], p["min_subrays"], p["mode"]) == (5, 0.75, 2, 2)


# ---- offsets -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", range(2, 9))
@pytest.mark.parametrize("divergence,ring", [(0.2, 0.7071), (0.17, 0.7071), (3.0, 1.0), (0.01, 0.25)])
def test_offsets_row_zero_is_zero_and_every_ring_row_lies_at_tan_rho(S, divergence, ring):
    from lidar_transfer_amd.config import EchoModel
    off = EchoModel(divergence, S, ring).offsets()
    assert off.shape == (S, 2) and off.dtype == np.float64 and not off[0].any()
    assert np.array_equal(off, ec.offsets(divergence, S, ring))
    t = np.tan(np.radians(divergence / 2.0 * ring))
    hyp = np.hypot(off[1:, 0], off[1:, 1])
    assert (np.abs(hyp - t) <= np.spacing(t)).all(), (hyp - t) / np.spacing(t)
    # evenly spaced, half a step from the left-pointing axis
    want = 2 * np.pi * np.arange(S - 1) / (S - 1) + np.pi / (S - 1)
    turn = (np.arctan2(off[1:, 1], off[1:, 0]) - want + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(turn).max() < 1e-12


#: level, steep, vertical, not normalised
GEOMETRY_RAYS = np.array([[1, 0, 0], [0.6, 0.8, 0], [-0.3, 0.4, 0.02], [0.05, -0.02, 0.99], [0.01, 0.0, -1.0], [0, 0, 1], [0, 0, -1],
                          [3, -4, 12], [1e-3, 2e-3, 5e-4]], np.float32)


@pytest.mark.parametrize("divergence,S", [(0.2, 5), (0.17, 5), (3.0, 8), (0.2, 2)])
def test_the_angle_between_a_restated_sub_ray_and_its_centre_is_rho(divergence, S):
    """the contract's float64 sub-ray ``h + a u + b v``, ahead of its rounding to float32: rho within 1e-6 relative, for level,
    steep, vertical and non-unit rays"""
    off = ec.offsets(divergence, S)
    h, u, v, dd, _ = ec.frame(GEOMETRY_RAYS)
    rho = np.radians(divergence / 2.0 * 0.7071)
    if (divergence, S) == (0.2, 5):
        assert abs(np.degrees(rho) - 0.07071) < 1e-9
    for a, b in off[1:]:
        s = np.stack([(h[:, 0] + a * u[:, 0]) + b * v[:, 0], (h[:, 1] + a * u[:, 1]) + b * v[:, 1], h[:, 2] + b * v[:, 2]], 1)
        # the angle from the cross product: well conditioned at a tenth of a degree
        ang = np.arctan2(np.linalg.norm(np.cross(h, s), axis=1), (h * s).sum(1))
        assert (np.abs(ang - rho) <= 1e-6 * rho).all(), (ang - rho) / rho
    assert np.allclose((h * u).sum(1), 0, atol=1e-15) and np.allclose((h * v).sum(1), 0, atol=1e-15)
    assert np.allclose(np.linalg.norm(v, axis=1), 1, atol=1e-15) and np.allclose(np.linalg.norm(h, axis=1), 1, atol=1e-15)


@pytest.mark.parametrize("divergence,S", [(0.2, 5), (0.17, 5), (3.0, 8), (0.2, 2)])
def test_the_float32_sub_ray_keeps_the_angle_to_the_precision_of_its_format(divergence, S):
    """what the kernel stores: the same sub-ray rounded to float32.  Each component (at most 1 in size) moves by at most 2^-25,
    the ray by at most sqrt(3) 2^-25 < 2^-23 across itself: the angle holds within 2^-23 / rho relative (1e-4 at 0.07 degrees),
    no closer.  Plane 0 is the input."""
    off = ec.offsets(divergence, S)
    n = len(GEOMETRY_RAYS)
    sub = ec.restate_subrays(GEOMETRY_RAYS, off).reshape(S, n, 3)
    rho = np.radians(divergence / 2.0 * 0.7071)
    c = ec.frame(GEOMETRY_RAYS)[0]
    for k in range(1, S):
        s = sub[k].astype(np.float64)
        ang = np.arctan2(np.linalg.norm(np.cross(c, s), axis=1), (c * s).sum(1))
        assert (np.abs(ang - rho) <= 2.0 ** -23).all(), (k, (ang - rho) / rho)
    assert np.array_equal(sub[0].view(np.uint32), GEOMETRY_RAYS.view(np.uint32))


# ---- the restatement's own rules --------------------------------------------------------------------------------------------------
def test_a_positive_a_turns_a_ray_to_the_left_and_a_positive_b_upwards():
    rays = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0.5, 0.5, 0.2], [-0.3, 0.1, -0.4]], np.float32)
    sub = ec.restate_subrays(rays, [[0, 0], [0.01, 0], [-0.01, 0], [0, 0.01], [0, -0.01]]).reshape(5, -1, 3).astype(np.float64)
    az = lambda d: np.arctan2(d[:, 1], d[:, 0])                                           # noqa: E731
    el = lambda d: np.arctan2(d[:, 2], np.hypot(d[:, 0], d[:, 1]))                        # noqa: E731
    turn = lambda k: (az(sub[k]) - az(sub[0]) + np.pi) % (2 * np.pi) - np.pi               # noqa: E731
    assert (turn(1) > 0).all() and (turn(2) < 0).all()
    assert (el(sub[3]) > el(sub[0])).all() and (el(sub[4]) < el(sub[0])).all()
    assert np.abs(turn(3)).max() < 1e-7 and np.abs(el(sub[1]) - el(sub[0])).max() < 1e-4
    # straight up: u = (1, 0, 0), v = h x u = (0, 1, 0) -- a goes to +x, b to +y
    up = ec.restate_subrays(np.array([[0, 0, 2]], np.float32), [[0, 0], [0.25, 0], [0, 0.25]])
    assert up.tolist() == [[0, 0, 2], [0.25, 0, 1], [0, 0.25, 1]]


def test_plane_zero_and_every_ray_without_a_direction_are_copied():
    rays = ec.ray_case(63)
    off = ec.offsets(0.2, 8)
    sub = ec.restate_subrays(rays, off).reshape(8, 63, 3)
    assert np.array_equal(sub[0].view(np.uint32), rays.view(np.uint32))
    dead = ~(np.abs(rays).sum(1) > 0)                                                      # the zero ray and the NaN row
    assert dead.sum() == 2
    for k in range(1, 8):
        assert np.array_equal(sub[k][dead].view(np.uint32), rays[dead].view(np.uint32))
        assert (sub[k][~dead] != rays[~dead]).any(1).all()


@pytest.mark.parametrize("S", range(2, 9))
def test_a_spot_wholly_on_one_surface_keeps_its_remission_bit_for_bit(S):
    rs = np.random.default_rng(S)
    n = 400
    rem = rs.uniform(0, 1, n).astype(np.float32)
    rem[:4] = [0.0, 1.0, np.float32(1e-40), np.nextafter(np.float32(1), np.float32(0))]
    t = (rs.uniform(2, 50, (1, n)) + rs.uniform(0, 0.05, (S, n))).astype(np.float32)
    rays = np.tile(np.array([[1, 0, 0]], np.float32), (n, 1))
    for mode in ec.MODES:
        out = ec.restate_resolve(ec.params(ec.offsets(0.2, S), mode=mode), rays, (0, 0, 0), t.reshape(-1),
                                 np.zeros(S * n, np.int32), None, np.tile(rem, S))
        assert np.array_equal(out["endrem"].view(np.uint32), rem.view(np.uint32))
        assert (out["fraction"] == 1).all() and (out["n_echoes"] == 1).all()
        assert np.array_equal(out["range"], (t.astype(np.float64).sum(0) / S).astype(np.float32)) or S > 2   # (the sum's order)


def test_the_walk_on_hand_written_cells():
    c = ec.crafted_cells()
    name = c["names"].index
    off = ec.offsets(0.2, 5)
    res = {(mode, m): ec.restate_resolve(ec.params(off, 0.5, m, mode), c["rays"], c["origin"], c["range"], c["tri"], c["label"], c["rem"])
           for mode in ec.MODES for m in (1, 2)}
    f32 = np.float32
    mean = lambda *t: f32(np.sum(np.array(t, f32).astype(np.float64)) / len(t))   # noqa: E731  (exact here: few short sums)
    for mode in ec.MODES:
        r = res[mode, 1]
        i = name("all misses")
        assert (r["n_echoes"][i], r["range"][i], r["tri"][i], r["endcolors"][i], r["endrem"][i], r["fraction"][i]) == (0, 0, -1, 0, 0, 0)
        assert not r["endpoints"][i].any()
        i = name("one hit")
        assert (r["n_echoes"][i], r["range"][i], r["tri"][i], r["endcolors"][i]) == (1, 7.0, 1000 * i + 2, 100 + 10 * i + 2)
        assert r["endrem"][i] == f32(0.5 / 5) and r["fraction"][i] == f32(1 / 5)
        assert np.array_equal(r["endpoints"][i], (np.array([0.6, 0.0, 0.8], f32).astype(np.float64) /
                                                  np.sqrt(np.float64(f32(0.6)) ** 2 + np.float64(f32(0.8)) ** 2) * 7.0).astype(f32))
        i = name("equal t in two sub-rays")                                  # the order goes by k: the representative is k = 1
        assert (r["n_echoes"][i], r["range"][i], r["tri"][i], r["endrem"][i]) == (1, 9.0, 1000 * i + 1, f32(1.0 / 5))
        i = name("a gap exactly equal to separation")                        # strict: one echo
        assert (r["n_echoes"][i], r["range"][i], r["fraction"][i]) == (1, 4.25, f32(2 / 5))
        i = name("first == last")
        assert (r["n_echoes"][i], r["fraction"][i], r["tri"][i]) == (1, 1.0, 1000 * i) and r["endrem"][i] == f32(0.5)
        i = name("a zero central ray")                                       # echoes are counted, the cell is a miss
        assert (r["n_echoes"][i], r["range"][i], r["tri"][i], r["fraction"][i]) == (1, 0, -1, 0) and not r["endpoints"][i].any()
    # the chain 4.0 4.3 4.6 4.9 5.2: every step is closer than 0.5, but 4.6 - 4.0 > 0.5 -- the rule is about the FIRST member
    i = name("a chain of close hits spanning more")
    assert res["first", 1]["n_echoes"][i] == 3
    assert res["first", 1]["range"][i] == mean(4.0, 4.3) and res["last", 1]["range"][i] == f32(5.2)
    assert res["last", 1]["tri"][i] == 1000 * i + 4 and res["first", 1]["tri"][i] == 1000 * i
    assert res["strongest", 1]["range"][i] == mean(4.0, 4.3)                # 1.0 = 1.0 on the sum, 2 = 2 on the count: the earlier
    assert res["first", 2]["n_echoes"][i] == 2 and res["last", 2]["range"][i] == mean(4.6, 4.9)
    i = name("min_subrays removes the nearest")
    assert res["first", 1]["range"][i] == 3.0 and res["first", 1]["n_echoes"][i] == 2
    assert res["first", 2]["range"][i] == mean(8.0, 8.1) and res["first", 2]["n_echoes"][i] == 1
    assert res["first", 2]["tri"][i] == 1000 * i + 2
    i = name("min_subrays removes every echo")
    assert res["strongest", 1]["n_echoes"][i] == 3 and res["strongest", 1]["range"][i] == 3.0      # three equal echoes: the earliest
    for mode in ec.MODES:
        r = res[mode, 2]
        assert (r["n_echoes"][i], r["range"][i], r["tri"][i], r["endcolors"][i], r["fraction"][i]) == (0, 0, -1, 0, 0)
    i = name("strongest ties on the sum")                                    # 0.75 = 0.75: the larger count
    assert res["strongest", 1]["range"][i] == mean(3.0, 3.1) and res["strongest", 1]["fraction"][i] == f32(2 / 5)
    i = name("strongest ties on the sum and the count")                      # the earlier
    assert res["strongest", 1]["range"][i] == 3.0 and res["last", 1]["range"][i] == 7.0
    i = name("the sum decides against the count")
    assert res["strongest", 1]["range"][i] == 7.0 and res["strongest", 1]["tri"][i] == 1000 * i + 3
    assert res["strongest", 2]["range"][i] == mean(3.0, 3.1, 3.2)           # (the single strong hit is not detected)
    i = name("the centre is not the nearest")                                # rep: the smallest k of the echo, not the nearest
    assert res["first", 1]["tri"][i] == 1000 * i + 1 and res["last", 1]["tri"][i] == 1000 * i
    assert res["last", 1]["fraction"][i] == f32(3 / 5) and res["strongest", 1]["tri"][i] == 1000 * i
    assert res["last", 1]["endcolors"][i] == 100 + 10 * i


def test_a_non_zero_origin_moves_the_end_points_and_nothing_else():
    c = ec.crafted_cells()
    p = ec.params(ec.offsets(0.2, 5))
    a = ec.restate_resolve(p, c["rays"], (0, 0, 0), c["range"], c["tri"], c["label"], c["rem"])
    b = ec.restate_resolve(p, c["rays"], (1.5, -2.25, 0.75), c["range"], c["tri"], c["label"], c["rem"])
    hit = a["tri"] >= 0
    for k in ("range", "tri", "endcolors", "endrem", "n_echoes", "fraction"):
        assert np.array_equal(a[k], b[k]), k
    assert np.allclose(b["endpoints"][hit] - a["endpoints"][hit], [1.5, -2.25, 0.75], atol=1e-5) and not b["endpoints"][~hit].any()
    # NULL images read as zeros
    z = ec.restate_resolve(p, c["rays"], (0, 0, 0), c["range"], c["tri"])
    assert not z["endcolors"].any() and not z["endrem"].any() and np.array_equal(z["n_echoes"], a["n_echoes"])


def test_the_random_cases_hold_every_kind_of_cell():
    for S in (2, 5, 8):
        c = ec.resolve_case(1000, S)
        r = ec.restate_resolve(ec.params(ec.offsets(0.2, S), 0.5, 1, "strongest"), c["rays"], c["origin"], c["range"], c["tri"],
                               c["label"], c["rem"])
        count = np.bincount(r["n_echoes"], minlength=4)
        assert count[0] > 0 and count[1] > 100 and count[2] > (20 if S > 2 else 5), count
        first = ec.restate_resolve(ec.params(ec.offsets(0.2, S), 0.5, 1, "first"), c["rays"], c["origin"], c["range"], c["tri"])
        last = ec.restate_resolve(ec.params(ec.offsets(0.2, S), 0.5, 1, "last"), c["rays"], c["origin"], c["range"], c["tri"])
        assert (first["range"] <= last["range"]).all() and (first["range"] < last["range"]).sum() == (r["n_echoes"][r["tri"] >= 0] > 1).sum()


# ---- the end-to-end scene, cast analytically ----------------------------------------------------------------------------------------
def test_every_row_of_the_edge_column_holds_two_echoes_under_an_analytic_caster():
    from lidar_transfer_amd.laserscan import create_rays
    H, W, S = 8, 64, 5
    rays = create_rays(10.0, -10.0, H, W)
    verts, faces, colors, rem, w0 = ec.edge_scene(rays, H, W)
    ye = float(verts[4, 1])
    off = ec.offsets(0.2, S)
    sub = ec.restate_subrays(rays, off)
    t, surf = ec.two_plane_cast(sub, ye)
    n = H * W
    sub_rem = np.where(surf == 1, 0.75, np.where(surf == 0, 0.25, 0.0)).astype(np.float32)
    res = {mode: ec.restate_resolve(ec.params(off, 0.5, 1, mode), rays, (0, 0, 0), t.astype(np.float32), surf.astype(np.int32),
                                    (surf + 1).astype(np.int32), sub_rem) for mode in ec.MODES}
    cells = np.arange(H) * W + w0
    assert (res["first"]["n_echoes"][cells] == 2).all()
    s = surf.reshape(S, n)[:, cells]
    near = (s == 1).sum(0)
    assert ((near == 3) | (near == 2)).all() and ((s == 0).sum(0) == S - near).all()
    tt = t.reshape(S, n)[:, cells]
    assert (np.abs(tt[s == 1] - 5.0) < 0.1).all() and (np.abs(tt[s == 0] - 10.0) < 0.2).all()
    assert (np.abs(res["first"]["range"][cells] - 5.0) < 0.1).all() and (np.abs(res["last"]["range"][cells] - 10.0) < 0.2).all()
    for mode in ("first", "last"):
        assert np.isin(res[mode]["fraction"][cells], np.array([0.6, 0.4], np.float32)).all()
    assert np.allclose(res["first"]["fraction"][cells] + res["last"]["fraction"][cells], 1.0)
    # every other column sees one surface
    others = np.setdiff1d(np.arange(n), np.concatenate([cells, np.arange(H) * W + (W - 1 if w0 == 0 else w0)]))
    assert (res["first"]["n_echoes"][others] <= 1).all()
    # with a separation of 20 m the two surfaces are one echo strictly between them
    one = ec.restate_resolve(ec.params(off, 20.0, 1, "strongest"), rays, (0, 0, 0), t.astype(np.float32), surf.astype(np.int32))
    assert (one["n_echoes"][cells] == 1).all() and (one["range"][cells] > 5.2).all() and (one["range"][cells] < 9.8).all()


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_lt_echo_model_matches_its_mirror(tmp_path):
    from lidar_transfer_amd import _lib
    fields = [f for f, _ in _lib.EchoModelArgs._fields_]
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lidarhip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(lt_echo_model));\n'
                   + "".join(f'  printf(" %zu", offsetof(lt_echo_model, {f}));\n' for f in fields)
                   + '  printf(" %d %u %u %u", LT_ECHO_MAX_SUBRAYS, LT_ECHO_FIRST, LT_ECHO_STRONGEST, LT_ECHO_LAST);\n'
                   + '  printf(" %zu %d\\n", sizeof(lt_noise_model), LT_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    V = _lib.EchoModelArgs
    assert got == [ctypes.sizeof(V)] + [getattr(V, f).offset for f in fields] + \
        [_lib.LT_ECHO_MAX_SUBRAYS, _lib.LT_ECHO_FIRST, _lib.LT_ECHO_STRONGEST, _lib.LT_ECHO_LAST,
         ctypes.sizeof(_lib.NoiseModelArgs), _lib.LT_ABI_VERSION]
    assert ctypes.sizeof(V) == 16 * 8 + 8 + 4 * 4 == 152 and _lib.LT_ABI_VERSION == 10
    assert "lt_create_subrays_dev" in _lib.SYMBOLS and "lt_echo_resolve_dev" in _lib.SYMBOLS


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_the_command_line_refuses_cp_with_the_key_before_any_device_work(tmp_path, capsys):
    from lidar_transfer_amd.__main__ import main
    seq = tmp_path / "data" / "sequences" / "00"
    (seq / "velodyne").mkdir(parents=True)
    (seq / "labels").mkdir()
    (tmp_path / "data" / "config.yaml").write_text("name: src\nfov_up: 3.0\nfov_down: -25.0\nbeams: 16\nangle_res_hor: 2.8125\nfov_hor: 360.0\n")
    text = open(os.path.join(ROOT, "config", "approach_mergemesh.yaml")).read()
    assert 'adaption: "mergemesh"' in text
    cp = tmp_path / "approach_cp.yaml"
    cp.write_text(text.replace('adaption: "mergemesh"', 'adaption: "cp"'))
    alone = tmp_path / "echo_alone.yaml"                                   # the shipped file with its echo model alone
    shipped = open(SHIPPED).read()
    alone.write_text(shipped[:shipped.index("return_model:")] + shipped[shipped.index("echo_model:"):])
    assert main(["-d", str(tmp_path / "data"), "-s", "00", "-c", str(cp), "-t", str(alone)]) == 1
    out = capsys.readouterr().out
    assert "cp renders no ray" in out and "echo_model" in out
    # a source sensor with the key: a message and status 1 as well
    source = tmp_path / "data" / "config.yaml"
    source.write_text(source.read_text() + shipped[shipped.index("echo_model:"):])
    assert main(["-d", str(tmp_path / "data"), "-s", "00", "-c", str(cp)]) == 1
    assert "echo_model is for target sensors only" in capsys.readouterr().out
