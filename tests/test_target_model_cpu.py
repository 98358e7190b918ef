"""``config.TargetModel``: the one value the device path carries for a target sensor's beam table, sector and azimuth offsets --
its marshalled forms against the ``config`` functions bit for bit, what ``SensorModel.target_model()`` carries for every
shipped sensor file, normalisation and equality, every refusal with the caller's prefix, and the input condition of
tests/test_target_model_gpu.py's cloud."""
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import beam_az_cases as ac  # noqa: E402
import beam_cases as bc  # noqa: E402
import sector_cases as sc  # noqa: E402
import target_model_cases as tc  # noqa: E402


def _shipped(name):
    from lidar_transfer_amd.config import load_sensor
    return load_sensor(os.path.join(ROOT, "config", name))


def _sensor_files():
    import yaml
    out = []
    for p in sorted(glob.glob(os.path.join(ROOT, "config", "*.yaml"))):
        with open(p) as f:
            if "fov_up" in yaml.safe_load(f):                      # (the others are approach files)
                out.append(p)
    return out


# ---- marshalled forms -----------------------------------------------------------------------------------------------------------
def test_the_marshalled_forms_are_the_config_functions_bit_for_bit():
    from lidar_transfer_amd.config import TargetModel, beam_azimuth_radians, beam_rows, sector_radians
    sector = _shipped("front120_64x1024.yaml").sector()
    az = _shipped("vlp32c_table_az_1024.yaml").beam_azimuth()
    assert sector is not None and az is not None and az.shape == (32,)
    for table in (bc.VLP32C, np.array([-3.0])):
        m = TargetModel(beam_table=table)
        Brad, halfw = beam_rows(table)
        H = len(table)
        assert m.rows.dtype == np.float64 and m.rows.shape == (2 * H,) and m.rows.flags.c_contiguous
        assert np.array_equal(m.rows[:H], Brad) and np.array_equal(m.rows[H:], halfw)
        assert m.rows_ptr.value == m.rows.ctypes.data and m.rows is m.rows                 # derived once, kept
        assert m.sector_rad is None and m.azimuth_rad is None
    assert np.array_equal(TargetModel(beam_table=[-3.0]).rows, [-3.0 / 180.0 * np.pi, 0.0])   # H = 1: halfw is 0
    for s in (sector, (190.0, 100.0)):
        m = TargetModel(sector=s)
        assert m.sector_rad.dtype == np.float64 and m.sector_rad.shape == (2,)
        assert np.array_equal(m.sector_rad, np.array(sector_radians(m.sector), np.float64))
        assert m.rows is None and m.rows_ptr is None
    m = TargetModel(sector=(190.0, 100.0))
    assert m.sector == (-170.0, 100.0) and np.array_equal(m.sector_rad, np.array(sector_radians((-170.0, 100.0))))
    assert TargetModel(sector=(-190.0, 100.0)).sector == (170.0, 100.0) and TargetModel(sector=(180.0, 90.0)).sector == (180.0, 90.0)
    m = TargetModel(beam_table=bc.VLP32C, beam_azimuth=az)
    assert m.azimuth_rad.dtype == np.float64 and np.array_equal(m.azimuth_rad, beam_azimuth_radians(az))
    assert np.array_equal(m.beam_azimuth, az) and m.beam_azimuth.dtype == np.float64


def test_the_bin_grid_is_sector_grid_or_none():
    from lidar_transfer_amd.config import TargetModel
    from lidar_transfer_amd.raytracer import sector_grid
    for c, s, W in sc.SECTORS + ((0.0, 1.0, 1024),):               # (the last one meets the cap of 8192 bins)
        assert TargetModel(sector=(c, s)).grid(W) == sector_grid(W, (c, s))
    assert TargetModel(sector=(0.0, 1.0)).grid(1024) == (8192, 0)
    assert TargetModel().grid(1024) is None and TargetModel(beam_table=bc.VLP32C).grid(1024) is None


def test_a_model_does_not_change():
    from lidar_transfer_amd.config import TargetModel
    table = bc.VLP32C.copy()
    m = TargetModel(table, (0.0, 120.0), ac.offsets("mixed", 32))
    table[0] = 0.0                                                 # the caller's array is not the model's
    assert m.beam_table[0] == 15.0
    with pytest.raises(ValueError):
        m.beam_table[0] = 0.0
    with pytest.raises(ValueError):
        m.beam_azimuth[0] = 0.0
    with pytest.raises(AttributeError):
        m.sector = None


# ---- what a sensor file brings --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", _sensor_files(), ids=os.path.basename)
def test_every_shipped_sensor_carries_its_three_accessors_and_the_flags_of_its_keys(path):
    import yaml
    from lidar_transfer_amd import _lib
    from lidar_transfer_amd.config import load_sensor
    s = load_sensor(path)
    m = s.target_model()
    for mine, theirs in ((m.beam_table, s.beam_table()), (m.beam_azimuth, s.beam_azimuth())):
        assert (mine is None) == (theirs is None) and (mine is None or (mine.dtype == np.float64 and np.array_equal(mine, theirs)))
    assert m.sector == s.sector()
    with open(path) as f:
        cfg = yaml.safe_load(f)
    want = (_lib.LT_PROJ_BEAM_ROWS if cfg.get("beam_model") == "table" else 0) | \
        (_lib.LT_PROJ_SECTOR if cfg.get("azimuth_model") == "sector" else 0) | \
        (_lib.LT_PROJ_BEAM_AZIMUTH if any(cfg.get("beam_azimuth_offsets") or ()) else 0)
    assert m.proj_flags == want, (path, m.proj_flags, want)
    assert m == s.target_model() and m.validate(s.H, (s.fov_up, s.fov_down)) is m


def test_the_shipped_files_cover_every_flag():
    from lidar_transfer_amd.config import load_sensor
    flags = {load_sensor(p).target_model().proj_flags for p in _sensor_files()}
    assert {0, 4, 8, 4 | 16} <= flags, flags


# ---- normalisation and equality -------------------------------------------------------------------------------------------------
def test_normalisation_and_equality():
    from lidar_transfer_amd.config import TargetModel
    az = ac.offsets("mixed", 32)
    assert TargetModel(sector=(10, 120)) == TargetModel(sector=[10.0, 120.0]) == TargetModel(sector=np.array([10.0, 120.0]))
    assert TargetModel(sector=np.array([350.0, 120.0])) == TargetModel(sector=(-10.0, 120.0))    # an array means degrees too
    assert TargetModel(bc.VLP32C, None, np.zeros(32)) == TargetModel(bc.VLP32C) == TargetModel(list(bc.VLP32C), None, [-0.0] * 32)
    assert TargetModel(bc.VLP32C, None, np.zeros(32)).beam_azimuth is None
    assert TargetModel() == TargetModel(None, None, None) and TargetModel() != TargetModel(bc.VLP32C) and TargetModel() != 0
    full = TargetModel(bc.VLP32C, (10.0, 120.0), az)
    assert full == TargetModel(bc.VLP32C.tolist(), (10, 120), tuple(az)) and full.difference(full) is None
    other = bc.VLP32C.copy()
    other[7] += 1e-6
    assert full != TargetModel(other, (10.0, 120.0), az) and full.difference(TargetModel(other, (10.0, 120.0), az)) == "beam_table"
    assert full != TargetModel(bc.VLP32C, (10.0, 120.5), az) and full.difference(TargetModel(bc.VLP32C, (10.0, 120.5), az)) == "sector"
    assert full.difference(TargetModel(bc.VLP32C, None, az)) == "sector"
    moved = az.copy()
    moved[3] += 0.1
    assert full != TargetModel(bc.VLP32C, (10.0, 120.0), moved)
    assert full.difference(TargetModel(bc.VLP32C, (10.0, 120.0), moved)) == "beam_azimuth"
    assert full.difference(TargetModel(bc.VLP32C, (10.0, 120.0))) == "beam_azimuth"
    with pytest.raises(TypeError):
        hash(full)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_every_refusal_carries_the_callers_prefix():
    from lidar_transfer_amd.config import TargetModel
    az, fov = ac.offsets("mixed", 32), bc.VLP32C_FOV
    with pytest.raises(ValueError, match="^someone: .*beam_model: table"):
        TargetModel(beam_azimuth=az, who="someone")                # offsets without a table
    with pytest.raises(ValueError, match="table"):
        TargetModel(sector=(0.0, 120.0), beam_azimuth=np.zeros(32))    # (even all-zero ones)
    for span in (0.0, 360.0):
        with pytest.raises(ValueError, match="^someone: .*fov_hor"):
            TargetModel(sector=(0.0, span), who="someone")
    for sector in ((360.5, 90.0), (float("nan"), 90.0), (0.0,), "ab", 5):
        with pytest.raises(ValueError, match="^someone: "):
            TargetModel(sector=sector, who="someone")
    ok = TargetModel(bc.VLP32C, (0.0, 120.0), az)
    assert ok.validate(32, fov, "someone") is ok and ok.validate(32, who="someone") is ok
    nan, far = az.copy(), az.copy()
    nan[4], far[4] = np.nan, 90.5
    out = np.where(np.arange(32) == 0, 16.0, bc.VLP32C)            # one entry outside the field of view
    bad = [(TargetModel(bc.VLP32C[:-1]), "31 beam_angles for 32 beams"),
           (TargetModel(bc.VLP32C, None, az[:-1]), "31 beam_azimuth_offsets for 32 beams"),
           (TargetModel(bc.VLP32C, None, nan), "finite"),
           (TargetModel(bc.VLP32C, None, far), "within \\+-90"),
           (TargetModel(out), "fov_down, fov_up"),
           (TargetModel(bc.VLP32C[::-1]), "neighbouring"),
           (TargetModel(np.where(np.arange(32) == 3, np.inf, bc.VLP32C)), "finite")]
    for m, what in bad:
        with pytest.raises(ValueError, match=f"^someone: .*{what}"):
            m.validate(32, fov, "someone")
    with pytest.raises(ValueError, match="^someone: 31 beam_angles for 32 beams"):       # without a field of view: the counts
        bad[0][0].validate(32, who="someone")
    assert bad[4][0].validate(32, who="someone") is bad[4][0]      # (and nothing about where the beams point)
    assert TargetModel(bc.VLP32C, None, np.where(np.arange(32) == 0, 90.0, az)).validate(32, fov) is not None    # |offset| = 90


def test_a_source_with_all_three_keys_hears_about_the_table_first():
    from lidar_transfer_amd.config import load_sensor, refuse_source_models
    cfg = dict(name="s", fov_up=15.0, fov_down=-25.0, beams=32, angle_res_hor=0.5, fov_hor=120.0, beam_model="table",
               beam_angles=[float(x) for x in bc.VLP32C], azimuth_model="sector", azimuth_center=10.0,
               beam_azimuth_offsets=[float(x) for x in ac.offsets("mixed", 32)])
    with pytest.raises(ValueError, match="beam_model 'table' is for target sensors only"):
        refuse_source_models(load_sensor(dict(cfg)))
    del cfg["beam_model"], cfg["beam_azimuth_offsets"]
    with pytest.raises(ValueError, match="azimuth_model 'sector' is for target sensors only"):
        refuse_source_models(load_sensor(dict(cfg)))
    src = load_sensor(dict(cfg, azimuth_model="full"))
    src.beam_azimuth_offsets = [0.0] * 32                          # (no file loads like this: the key alone is refused)
    with pytest.raises(ValueError, match="beam_azimuth_offsets is for target sensors only"):
        refuse_source_models(src)
    refuse_source_models(load_sensor(dict(cfg, azimuth_model="full")))
    refuse_source_models((32, 1024, 10.0, -30.0))


# ---- the input condition of the GPU test ----------------------------------------------------------------------------------------
def test_no_point_of_the_gpu_tests_cloud_lies_near_a_boundary_and_cells_are_contested():
    """tests/test_target_model_gpu.py compares bit for bit on every cell: that needs a cloud without a point within the slack
    of a row, column or sector boundary (tests/test_sector_gpu.py's rule leaves such cells out; here there is none)"""
    pts, rem, lab = tc.cloud()
    assert pts.dtype == np.float64 and len(pts) == tc.N_POINTS
    for name in ("A", "B"):
        table, sector, az = tc.MODELS[name]
        w = ac.project(pts, rem, lab, table, tc.FOV, az, tc.W, sector)
        assert int(w["near"].sum()) == 0 and int(sc.near_cells(w, tc.W).sum()) == 0, name
        assert int(w["kept"].sum()) > (w["idx"] >= 0).sum() > 0.4 * tc.H * tc.W, name      # more points than cells: z-min at work
    a, b = (ac.project(pts, rem, lab, *tc.MODELS[k][:1], tc.FOV, tc.MODELS[k][2], tc.W, tc.MODELS[k][1]) for k in ("A", "B"))
    assert not np.array_equal(a["range"], b["range"])
