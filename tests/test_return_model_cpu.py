"""The target sensor's return model without a GPU: the hash's known answers and its statistics, the numpy restatement's
cosine against the analytic one, and the loader (``config.ReturnModel``, ``SensorModel.return_model``)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import return_cases as rc  # noqa: E402

SHIPPED = os.path.join(ROOT, "config", "vlp32c_table_returns_1024.yaml")


def _sensor(**kw):
    cfg = dict(name="ret", fov_up=3.0, fov_down=-25.0, beams=16, angle_res_hor=360.0 / 130, fov_hor=360.0)
    cfg.update(kw)
    return cfg


def test_the_hash_has_its_known_answers_in_the_restatement_and_in_the_package():
    from lidar_transfer_amd.config import return_hash
    for (seed, scan, i), want in rc.HASH_KNOWN:
        assert int(rc.hash32(seed, scan, i)) == want == return_hash(seed, scan, i), (seed, scan, i)
    i = np.arange(4096)
    assert [int(x) for x in rc.hash32(123456789, 4000000000, i)[:64]] == [return_hash(123456789, 4000000000, k) for k in range(64)]
    # uint32 sums wrap: 2^32 more in any argument changes nothing
    assert np.array_equal(rc.hash32(9, 3, i), rc.hash32(9 + 2 ** 32, 3 + 2 ** 32, i + 2 ** 32))


def test_the_dropped_share_and_the_difference_between_patterns_are_those_of_independent_draws():
    n, thr = 2080, int(0.25 * 2 ** 32)
    pat = {(seed, scan): rc.hash32(seed, scan, np.arange(n)) < np.uint64(thr) for seed in (1, 2) for scan in range(6)}
    shares = [float(pat[1, s].mean()) for s in range(6)]
    print("\ndropped share at drop_rate 0.25, seed 1, scans 0-5:", [round(x, 4) for x in shares])
    assert all(0.22 <= x <= 0.28 for x in shares), shares
    d_scan, d_seed = float((pat[1, 0] != pat[1, 1]).mean()), float((pat[1, 0] != pat[2, 0]).mean())
    print("patterns differ in", round(d_scan, 4), "(scan 0 vs 1) and", round(d_seed, 4), "(seed 1 vs 2) of the cells; independent: 0.375")
    assert 0.30 <= d_scan <= 0.45 and 0.30 <= d_seed <= 0.45


@pytest.mark.parametrize("theta", [0.0, 60.0, 89.9])
def test_the_restated_cosine_is_the_analytic_one_on_tilted_planes(theta):
    v0, v1, v2, d, want = rc.tilted_plane(theta)
    got = rc.cosine64(v0, v1, v2, d)
    err = float(np.abs(got - want).max())
    print(f"\nplane tilted by {theta}: max |restatement - cos(theta)| = {err:.3g}")
    assert err <= 1e-12
    # the contract's inputs are float32: rounding the vertices moves the plane itself (1e-7); against the analytic cosine of
    # the geometry the rounded numbers describe the chain holds the same bound
    f = [a.astype(np.float32) for a in (v0, v1, v2, d)]
    got32 = rc.cosine(*f)
    exact = np.array([rc.exact_cosine(*(a[k] for a in f)) for k in range(len(got32))])
    err32 = float(np.abs(got32 - exact).max())
    print(f"float32 vertices: max |restatement - exact| = {err32:.3g}; the rounding moved the cosine by {float(np.abs(exact - want).max()):.3g}")
    assert err32 <= 1e-12
    assert got.max() <= 1.0 and got32.max() <= 1.0


def test_the_restatement_orders_its_rules_and_leaves_a_cell_at_a_threshold():
    verts = np.array([[5, -1, -1], [5, 1, -1], [5, 0, 1], [5, 0, 1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)           # face 1 is degenerate
    rays = np.tile(np.array([[1, 0, 0]], np.float32), (6, 1))
    tri = np.array([-1, 0, 0, 0, 1, 7], np.int32)
    rng = np.array([0, 5, 0.5, 90, 5, 5], np.float32)
    p = rc.params(min_range=1.0, max_range=80.0, min_cos=0.5, drop_threshold=0)
    out = rc.restate(p, 0, rays, verts, faces, tri, rng, endrem=np.ones(6, np.float32), endpoints=np.ones((6, 3), np.float32),
                     endcolors=np.full(6, 9, np.int32))
    assert out["drop"].tolist() == [1, 0, 2, 3, 4, 1]
    assert out["tri"].tolist() == [-1, 0, -1, -1, -1, 7] and out["range"].tolist() == [0, 5, 0, 0, 0, 5]
    assert out["incidence"].tolist() == [-1, 1, -1, -1, -1, -1] and out["endcolors"].tolist() == [9, 9, 0, 0, 0, 9]
    at = rc.restate(rc.params(min_range=5.0, max_range=5.0, min_cos=1.0), 0, rays, verts, faces, tri[1:2], rng[1:2])
    assert at["drop"].tolist() == [0]
    every = rc.restate(rc.params(drop_threshold=2 ** 32 - 1), 0, rays, verts, faces, tri[1:2], rng[1:2])
    assert every["drop"].tolist() == [5]


def test_defaults_are_no_model():
    from lidar_transfer_amd.config import ReturnModel, load_sensor
    assert load_sensor(_sensor()).return_model() is None
    assert load_sensor(_sensor(return_model={})).return_model() is None
    assert load_sensor(_sensor(return_model=dict(ReturnModel.DEFAULTS))).return_model() is None
    assert load_sensor(_sensor(return_model=dict(min_range=0, max_range=float("inf"), max_incidence=90, remission="none",
                                                 drop_rate=0.0, seed=0))).return_model() is None
    assert ReturnModel.of(None) is None and ReturnModel.of(ReturnModel()) is None
    m = load_sensor(_sensor(return_model=dict(seed=1))).return_model()
    assert m is not None and m.seed == 1 and m.drop_threshold == 0 and m.min_cos == 0.0 and not m.lambert
    with pytest.raises(AttributeError):
        m.seed = 2


def test_the_derived_numbers_are_the_hosts():
    import math

    from lidar_transfer_amd.config import ReturnModel
    m = ReturnModel(1.0, 80.0, 80.0, "lambert", 0.02, 1)
    assert m.min_cos == math.cos(80.0 * math.pi / 180.0) and m.drop_threshold == int(0.02 * 2 ** 32) == 85899345 and m.lambert
    assert ReturnModel(max_incidence=90).min_cos == 0.0
    assert ReturnModel(drop_rate=0.25).drop_threshold == 2 ** 30
    assert ReturnModel(drop_rate=math.nextafter(1.0, 0.0)).drop_threshold < 2 ** 32
    assert ReturnModel(seed=2 ** 32 - 1).seed == 2 ** 32 - 1
    assert m == ReturnModel(1, 80, 80.0, "lambert", 0.02, 1) and m != ReturnModel(1, 80, 80.0, "none", 0.02, 1)
    a = m.args()
    assert (a.min_range, a.max_range, a.min_cos, a.drop_threshold, a.seed, a.flags) == (1.0, 80.0, m.min_cos, 85899345, 1, 1)


@pytest.mark.parametrize("block", [
    dict(min_range=-0.1), dict(min_range=5.0, max_range=4.0), dict(min_range=float("nan")), dict(min_range=float("inf")),
    dict(max_range=float("nan")), dict(max_range=-float("inf")), dict(max_range="far"), dict(max_incidence=0.0),
    dict(max_incidence=90.5), dict(max_incidence=-10), dict(max_incidence=float("nan")), dict(drop_rate=1.0), dict(drop_rate=-0.01),
    dict(drop_rate=float("nan")), dict(seed=-1), dict(seed=2 ** 32), dict(seed=1.5), dict(seed="1"), dict(seed=True),
    dict(remission="cosine"), dict(remission=None), dict(min_range=True), dict(minrange=1.0), [1.0, 80.0], "lambert"])
def test_a_block_that_cannot_be_used_is_refused_at_load_time_by_the_sensors_name(block):
    from lidar_transfer_amd.config import load_sensor
    with pytest.raises(ValueError, match="sensor 'ret'.*return_model"):
        load_sensor(_sensor(return_model=block))


def test_a_source_sensor_with_the_key_is_refused_like_a_source_table():
    from lidar_transfer_amd.config import load_sensor, refuse_source_models
    refuse_source_models(load_sensor(_sensor()))
    for block in (dict(drop_rate=0.1), {}):
        with pytest.raises(ValueError, match="source sensor 'ret'.*return_model.*target"):
            refuse_source_models(load_sensor(_sensor(return_model=block)))


def test_the_shipped_file_loads_and_is_the_table_file_plus_the_block():
    from lidar_transfer_amd.config import ReturnModel, load_sensor
    s = load_sensor(SHIPPED)
    t = load_sensor(os.path.join(ROOT, "config", "vlp32c_table_1024.yaml"))
    assert s.return_model() == ReturnModel(1.0, 80.0, 80.0, "lambert", 0.02, 1) and t.return_model() is None
    assert (s.H, s.W, s.fov_up, s.fov_down) == (t.H, t.W, t.fov_up, t.fov_down) == (32, 1024, 15.0, -25.0)
    assert s.target_model() == t.target_model() and s.beam_table() is not None
    assert "not a calibration" in open(SHIPPED).read()


def test_the_totals_line_names_the_six_codes_in_order():
    from lidar_transfer_amd.sequence import RETURN_CODES, format_return_totals
    assert tuple(RETURN_CODES) == rc.CODES
    line = format_return_totals([6, 5, 4, 3, 2, 1])
    assert line == ("Returns: kept 6, no hit 5, below min_range 4, beyond max_range 3, beyond max_incidence 2, "
                    "dropped at random 1")
