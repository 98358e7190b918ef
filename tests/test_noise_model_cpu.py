"""The target sensor's noise model without a GPU: the pinned vectors of its draws, the statistics of ``z``, the
restatement's own rules on hand-made cells, the loader (``config.NoiseModel``, ``SensorModel.noise_model``) and the layout
of ``lt_noise_model`` against the header compiled as C."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import noise_cases as nc  # noqa: E402
import return_cases as rc  # noqa: E402

SHIPPED = os.path.join(ROOT, "config", "vlp32c_table_noise_1024.yaml")
N_STAT = 1 << 20


def _sensor(**kw):
    cfg = dict(name="noi", fov_up=3.0, fov_down=-25.0, beams=16, angle_res_hor=360.0 / 130, fov_hor=360.0)
    cfg.update(kw)
    return cfg


# ---- vectors ---------------------------------------------------------------------------------------------------------------------
def test_the_pinned_vectors_hold_in_the_restatement_and_with_the_packages_mix():
    from lidar_transfer_amd.config import return_hash, return_hash_mix
    i = np.arange(3)
    assert tuple(int(x) for x in nc.g32(1, 0, i)) == nc.G_KNOWN
    s_range, s_rem = nc.draw_sums(1, 0, i)
    assert tuple(int(x) for x in s_range) == nc.S_RANGE_KNOWN and tuple(int(x) for x in s_rem) == nc.S_REM_KNOWN
    z_range, z_rem = nc.draws(1, 0, i)
    assert tuple(float(x) for x in z_range) == nc.Z_RANGE_KNOWN
    assert tuple(float(x) for x in z_rem) == tuple((s - 393210) / 65536.0 for s in nc.S_REM_KNOWN)
    # the same numbers from Python ints and the package's mix
    m = return_hash_mix
    for k in range(3):
        g = m(m(m(1 ^ 0x6e6f6973) + 0) + k)
        assert g == nc.G_KNOWN[k]
        w = [m(g + j) for j in range(1, 13)]
        assert sum((x & 0xffff) + (x >> 16) for x in w[:6]) == nc.S_RANGE_KNOWN[k]
        assert sum((x & 0xffff) + (x >> 16) for x in w[6:]) == nc.S_REM_KNOWN[k]
    # the dropout hash is what it was, and another stream
    assert return_hash(1, 0, 0) == 0x24009c6d == int(rc.hash32(1, 0, 0)) != nc.G_KNOWN[0]
    # uint32 sums wrap: 2^32 more in any argument changes nothing
    j = np.arange(4096)
    assert np.array_equal(nc.g32(9, 3, j), nc.g32(9 + 2 ** 32, 3 + 2 ** 32, j + 2 ** 32))


def test_z_is_exact_in_float64_and_bounded():
    assert nc.z_of(0) == -393210 / 65536.0 and nc.z_of(12 * 65535) == 393210 / 65536.0 and abs(nc.z_of(0)) < 6
    S = np.arange(0, 12 * 65535 + 1, 977)
    z = nc.z_of(S)
    assert np.array_equal((z * 65536.0).astype(np.int64) + 393210, S)


# ---- statistics ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def z_by_stream():
    i = np.arange(N_STAT)
    return {key: nc.draws(key[0], key[1], i) for key in ((1, 0), (0, 0), (7, 4070), (1, 1))}


@pytest.mark.parametrize("key", [(1, 0), (0, 0), (7, 4070)])
def test_both_draws_have_mean_zero_and_variance_one(z_by_stream, key):
    for name, z in zip(("range", "remission"), z_by_stream[key]):
        mean, var = float(z.mean()), float(z.var())
        print(f"\n(seed, scan) = {key}, {name} draw over 2^20 cells: mean {mean:+.5f}, variance {var:.5f}, max |z| {np.abs(z).max():.3f}")
        assert abs(mean) < 0.005 and abs(var - 1.0) < 0.005
        assert np.abs(z).max() < 6.0


def test_the_draws_are_uncorrelated_between_kinds_neighbours_and_scans(z_by_stream):
    corr = lambda a, b: float(np.corrcoef(a, b)[0, 1])   # noqa: E731
    for key in ((1, 0), (0, 0), (7, 4070)):
        zr, ze = z_by_stream[key]
        c = dict(kinds=corr(zr, ze), range_neighbours=corr(zr[:-1], zr[1:]), remission_neighbours=corr(ze[:-1], ze[1:]))
        print(f"\n(seed, scan) = {key}: " + ", ".join(f"{k} {v:+.5f}" for k, v in c.items()))
        assert all(abs(v) < 0.01 for v in c.values()), c
    for k, name in enumerate(("range", "remission")):
        c = corr(z_by_stream[1, 0][k], z_by_stream[1, 1][k])
        print(f"scan 0 against scan 1, {name} draw: {c:+.5f}")
        assert abs(c) < 0.01


# ---- the restatement's own rules --------------------------------------------------------------------------------------------------
def test_the_restatement_leaves_what_is_no_return_and_writes_the_full_miss():
    tri = np.array([-1, 3, -1, 4, 5], np.int32)
    rng = np.array([0, 0, 7, 10, 1e-3], np.float32)
    pts = np.arange(15, dtype=np.float32).reshape(5, 3) + 1
    rem = np.full(5, 0.5, np.float32)
    col = np.arange(5, dtype=np.int32) + 40
    out = nc.restate(nc.params(range_sigma=0.5, seed=1, min_range=1.0), 0, (0, 0, 0), tri, rng, rem, pts, col)
    assert out["state"].tolist() == [0, 0, 0, 1, 2]
    for k, a in (("tri", tri), ("range", rng), ("endpoints", pts), ("endrem", rem), ("endcolors", col)):
        assert np.array_equal(out[k][:3], a[:3]), k
    assert out["tri"][4] == -1 and out["range"][4] == 0 and not out["endpoints"][4].any() and out["endrem"][4] == 0 \
        and out["endcolors"][4] == 0
    z = nc.draws(1, 0, np.arange(5))[0][3]
    r2 = 10.0 + 0.5 * z
    assert out["range"][3] == np.float32(r2) and out["range_error"][3] == np.float32(r2 - 10.0) and out["range_error"][4] == 0
    assert np.array_equal(out["endpoints"][3], (pts[3].astype(np.float64) * (r2 / 10.0)).astype(np.float32))
    assert out["endcolors"][3] == col[3] and out["tri"][3] == 4 and out["endrem"][3] == rem[3]


def test_the_restatement_rounds_ties_to_even_and_keeps_a_cell_at_the_gate():
    one = lambda **kw: nc.restate(nc.params(**kw), 0, (0, 0, 0), np.array([0], np.int32), np.array([1.25], np.float32))   # noqa: E731
    assert one(range_resolution=0.5)["range"][0] == 1.0                     # 2.5 -> 2
    assert nc.restate(nc.params(range_resolution=0.5), 0, (0, 0, 0), np.array([0], np.int32),
                      np.array([1.75], np.float32))["range"][0] == 2.0      # 3.5 -> 4
    assert one(min_range=1.25, max_range=1.25)["state"][0] == 1
    assert one(min_range=np.nextafter(1.25, 2))["state"][0] == 2 and one(max_range=np.nextafter(1.25, 0))["state"][0] == 2
    assert one(range_sigma=1e9, seed=1)["state"][0] == 2                    # z(1, 0, 0) = -0.976: r2 <= 0
    e = nc.restate(nc.params(remission_levels=2), 0, (0, 0, 0), np.zeros(3, np.int32), np.ones(3, np.float32),
                   endrem=np.array([0.5, 0.49, 0.51], np.float32))["endrem"]
    assert e.tolist() == [0.0, 0.0, 1.0]                                    # rint(0.5) = 0


# ---- config ------------------------------------------------------------------------------------------------------------------------
def test_defaults_are_no_model():
    from lidar_transfer_amd.config import NoiseModel, load_sensor
    assert load_sensor(_sensor()).noise_model() is None
    assert load_sensor(_sensor(noise_model={})).noise_model() is None
    assert load_sensor(_sensor(noise_model=dict(NoiseModel.DEFAULTS))).noise_model() is None
    assert load_sensor(_sensor(noise_model=dict(range_sigma=0, range_sigma_rel=0.0, range_resolution=0, remission_sigma=0.0,
                                                remission_levels=0, seed=0))).noise_model() is None
    assert NoiseModel.of(None) is None and NoiseModel.of(NoiseModel()) is None
    m = load_sensor(_sensor(noise_model=dict(range_sigma=0.02))).noise_model()
    assert m is not None and m.range_sigma == 0.02 and m.remission_levels == 0 and m.seed == 0
    with pytest.raises(AttributeError):
        m.seed = 2
    assert m == NoiseModel(0.02) and m != NoiseModel(0.02, seed=1) and hash(m) == hash(NoiseModel(0.02))
    assert NoiseModel.of(m) is m


def test_the_struct_is_the_models_fields_and_the_return_models_gate():
    from lidar_transfer_amd.config import NoiseModel, ReturnModel
    m = NoiseModel(0.02, 0.0005, 0.002, 0.03, 256, 2 ** 32 - 1)
    a = m.args()
    assert (a.range_sigma, a.range_sigma_rel, a.range_resolution, a.remission_sigma, a.min_range, a.max_range, a.remission_levels,
            a.seed) == (0.02, 0.0005, 0.002, 0.03, 0.0, float("inf"), 256, 2 ** 32 - 1)
    a = m.args(ReturnModel(1.0, 80.0))
    assert (a.min_range, a.max_range) == (1.0, 80.0)
    assert nc.params_of(m, ReturnModel(1.0, 80.0)) == nc.params(0.02, 0.0005, 0.002, 0.03, 256, 2 ** 32 - 1, 1.0, 80.0)
    # the return model is what it was
    assert tuple(ReturnModel.DEFAULTS) == ("min_range", "max_range", "max_incidence", "remission", "drop_rate", "seed")


@pytest.mark.parametrize("block", [
    dict(range_sigma=-0.1), dict(range_sigma=float("nan")), dict(range_sigma=float("inf")), dict(range_sigma="wide"),
    dict(range_sigma=True), dict(range_sigma_rel=-1e-9), dict(range_sigma_rel=float("nan")), dict(range_resolution=-0.002),
    dict(range_resolution=float("inf")), dict(remission_sigma=-0.5), dict(remission_sigma=None), dict(remission_levels=1),
    dict(remission_levels=-2), dict(remission_levels=2.5), dict(remission_levels=256.0), dict(remission_levels=2 ** 32),
    dict(remission_levels=True), dict(seed=-1), dict(seed=2 ** 32), dict(seed=1.5), dict(seed="1"), dict(seed=True),
    dict(sigma=0.02), dict(min_range=1.0), [0.02, 0.0005], "gaussian", 0.02])
def test_a_block_that_cannot_be_used_is_refused_at_load_time_by_the_sensors_name(block):
    from lidar_transfer_amd.config import load_sensor
    with pytest.raises(ValueError, match="sensor 'noi'.*noise_model"):
        load_sensor(_sensor(noise_model=block))


def test_a_source_sensor_with_the_key_is_refused_like_a_source_return_model():
    from lidar_transfer_amd.config import load_sensor, refuse_source_models
    refuse_source_models(load_sensor(_sensor()))
    for block in (dict(range_sigma=0.1), {}):
        with pytest.raises(ValueError, match="source sensor 'noi'.*noise_model.*target"):
            refuse_source_models(load_sensor(_sensor(noise_model=block)))


def test_the_shipped_file_loads_and_is_the_returns_file_plus_the_block():
    from lidar_transfer_amd.config import NoiseModel, load_sensor
    s = load_sensor(SHIPPED)
    t = load_sensor(os.path.join(ROOT, "config", "vlp32c_table_returns_1024.yaml"))
    assert s.noise_model() == NoiseModel(0.02, 0.0005, 0.002, 0.02, 256, 1) and t.noise_model() is None
    assert s.return_model() == t.return_model() is not None and s.target_model() == t.target_model()
    assert (s.H, s.W, s.fov_up, s.fov_down) == (t.H, t.W, t.fov_up, t.fov_down) == (32, 1024, 15.0, -25.0)
    assert "not a calibration" in open(SHIPPED).read()


def test_the_totals_line_names_the_three_states_and_the_rms():
    from lidar_transfer_amd.sequence import NOISE_STATES, format_noise_totals
    assert tuple(NOISE_STATES) == nc.STATES
    assert format_noise_totals([3, 2, 1], 0.0251) == "Noise: untouched 3, noised 2, lost 1, range error RMS 0.025100 m"
    assert format_noise_totals([3, 0, 0], None) == "Noise: untouched 3, noised 0, lost 0, range error RMS n/a"


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_lt_noise_model_matches_its_mirror(tmp_path):
    from lidar_transfer_amd import _lib
    fields = [f for f, _ in _lib.NoiseModelArgs._fields_]
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lidarhip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(lt_noise_model));\n'
                   + "".join(f'  printf(" %zu", offsetof(lt_noise_model, {f}));\n' for f in fields)
                   + '  printf(" %zu %d\\n", sizeof(lt_return_model), LT_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    V = _lib.NoiseModelArgs
    assert got == [ctypes.sizeof(V)] + [getattr(V, f).offset for f in fields] + [ctypes.sizeof(_lib.ReturnModelArgs), _lib.LT_ABI_VERSION]
    assert ctypes.sizeof(V) == 56 and _lib.LT_ABI_VERSION == 10
    assert "lt_noise_model_dev" in _lib.SYMBOLS
