"""Per-beam azimuth offsets of a table target (``beam_azimuth_offsets``) without a GPU: the loader -- pairing
across the sort, every refusal, all-zero, the absence of the key, the shipped file --, the host ``create_rays`` against the
restatement, and the conditions on the inputs of tests/test_beam_az_gpu.py.  Restatements: tests/beam_az_cases.py."""
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
import mount_common as mc  # noqa: E402

#: the ray cases of the GPU test: (name, sensor index in ac.SENSORS, offset set, sector, pose) -- both sets on every geometry
#: but one: a +-90 row on the unposed full circle would put column 0 (180 degrees) on 90 / 270, where x is the residue of a
#: cancellation.
RAY_CASES = tuple((f"{ac.SENSORS[si][0]} {kind} {tag}", si, kind, sector, pose)
                  for si in (0, 2)
                  for tag, kind, sector, pose in (("full", "mixed", None, None), ("seam sector", "ninety", ac.SEAM_SECTOR, None),
                                                  ("seam sector", "mixed", ac.SEAM_SECTOR, None),
                                                  ("posed", "ninety", None, mc.POSE_GENERAL), ("posed", "mixed", None, mc.POSE_GENERAL)))


def _cfg(**kw):
    cfg = dict(name="vlp32c az", fov_up=15.0, fov_down=-25.0, beams=32, angle_res_hor=360.0 / 171, fov_hor=360.0,
               beam_model="table", beam_angles=[float(x) for x in bc.VLP32C])
    cfg.update(kw)
    return cfg


# ---- the loader -----------------------------------------------------------------------------------------------------------------
def test_offsets_stay_paired_with_their_angles_across_the_sort():
    from lidar_transfer_amd.config import load_sensor
    az = ac.offsets("mixed", 32)
    m = load_sensor(_cfg(beam_azimuth_offsets=[float(x) for x in az]))
    assert np.array_equal(m.beam_table(), bc.VLP32C) and m.beam_azimuth().dtype == np.float64
    assert np.array_equal(m.beam_azimuth(), az)
    rng = np.random.default_rng(5)
    for _ in range(4):
        p = rng.permutation(32)
        s = load_sensor(_cfg(beam_angles=[float(x) for x in bc.VLP32C[p]], beam_azimuth_offsets=[float(x) for x in az[p]]))
        assert np.array_equal(s.beam_table(), bc.VLP32C) and np.array_equal(s.beam_azimuth(), az)
        assert s.raw["beam_angles"] == [float(x) for x in bc.VLP32C[p]]          # the file's order is kept
    up = load_sensor(_cfg(beam_angles=[float(x) for x in bc.VLP32C[::-1]], beam_azimuth_offsets=[float(x) for x in az[::-1]]))
    assert np.array_equal(up.beam_azimuth(), az)
    rays = m.create_rays()
    assert np.array_equal(rays.view(np.int32), ac.az_rays(bc.VLP32C, az, 171).view(np.int32))


def test_every_refusal_raises_at_load_time():
    from lidar_transfer_amd.config import load_sensor, refuse_source_beam_azimuth
    az = [float(x) for x in ac.offsets("mixed", 32)]
    for bad in (az[:-1], az + [0.0], [float("nan")] + az[1:], [float("inf")] + az[1:], [90.5] + az[1:], [-91.0] + az[1:],
                ["x"] + az[1:], 1.4):
        with pytest.raises(ValueError):
            load_sensor(_cfg(beam_azimuth_offsets=bad))
    load_sensor(_cfg(beam_azimuth_offsets=[90.0, -90.0] + az[2:]))                   # |offset| = 90 is allowed
    lin = _cfg(beam_azimuth_offsets=az)
    del lin["beam_model"]
    with pytest.raises(ValueError, match="beam_model"):                              # the table is a condition
        load_sensor(lin)
    del lin["beam_angles"]
    with pytest.raises(ValueError):
        load_sensor(lin)
    with pytest.raises(ValueError, match="target"):                                  # a source with the key
        refuse_source_beam_azimuth(load_sensor(_cfg(beam_azimuth_offsets=az)))
    refuse_source_beam_azimuth(load_sensor(_cfg()))
    refuse_source_beam_azimuth((32, 171, 15.0, -25.0))


def test_all_zero_offsets_are_the_absence_of_the_key_and_a_file_without_it_loads_as_before():
    from lidar_transfer_amd.config import SensorModel, load_sensor
    zero = load_sensor(_cfg(beam_azimuth_offsets=[0.0] * 31 + [-0.0]))
    plain = load_sensor(_cfg())
    assert zero.beam_azimuth() is None and plain.beam_azimuth() is None and plain.beam_azimuth_offsets is None
    assert np.array_equal(zero.create_rays().view(np.int32), plain.create_rays().view(np.int32))
    assert plain.as_tuple() == ("vlp32c az", 15.0, -25.0, 32, 171, sorted(float(x) for x in bc.VLP32C))
    # the dataclass as it was constructed before the key existed
    old = SensorModel("vlp32c az", 15.0, -25.0, 32, 360.0 / 171, 360.0, sorted(float(x) for x in bc.VLP32C), raw=_cfg(),
                      beam_model="table")
    assert old == plain and old.beam_azimuth() is None
    shipped = load_sensor(os.path.join(ROOT, "config", "vlp32c_table_1024.yaml"))
    assert shipped.beam_azimuth() is None and np.array_equal(shipped.beam_table(), bc.VLP32C)
    assert np.array_equal(shipped.create_rays().view(np.int32), bc.table_rays(bc.VLP32C, 1024).view(np.int32))


def test_the_shipped_file_loads_with_the_heads_four_values():
    from lidar_transfer_amd.config import beam_azimuth_radians, load_sensor
    m = load_sensor(os.path.join(ROOT, "config", "vlp32c_table_az_1024.yaml"))
    plain = load_sensor(os.path.join(ROOT, "config", "vlp32c_table_1024.yaml"))
    assert (m.H, m.W) == (32, 1024) and np.array_equal(m.beam_table(), plain.beam_table())
    az = m.beam_azimuth()
    assert az.shape == (32,) and set(az.tolist()) == {1.4, -1.4, 4.2, -4.2}
    assert np.array_equal(beam_azimuth_radians(az), az / 180. * np.pi)
    text = open(os.path.join(ROOT, "config", "vlp32c_table_az_1024.yaml")).read()
    assert "ILLUSTRATIVE" in text and "NOT a calibration" in text
    assert round(4.2 / m.angle_res_hor) == 12                                        # twelve columns


# ---- host create_rays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(RAY_CASES)))
def test_host_rays_equal_the_restatement_and_no_component_is_the_residue_of_a_cancellation(case):
    """the host mirror bit for bit (one numpy on both sides); and the condition on the GPU ray cases: no component closer to 0
    than 1e-9 (tests/test_mount_gpu.py's RAY_SENSORS: such a component follows the last bit of a double sin / cos, no rule in
    ulps holds for it) -- but what the plain table's rays hold as well, two well-conditioned values of pi's own rounding:
    y of an unposed ray at exactly 180 degrees, sp * sin(-pi) = 1.2e-16 (the seam, excepted there too; only a zero-offset row
    has it), and z of an unposed beam at 0 degrees, cos(pi / 2) = 6.1e-17, which no offset touches"""
    from lidar_transfer_amd.laserscan import create_rays
    name, si, kind, sector, P = RAY_CASES[case]
    _, table, fov, W = ac.SENSORS[si]
    H = len(table)
    az = ac.offsets(kind, H)
    d = ac.rays_f64(table, az, W, sector)
    got = create_rays(fov[0], fov[1], H, W, beam_table=table, sector=sector, beam_azimuth=az)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), d.astype(np.float32).view(np.int32)), name
    rot = None if P is None else P[:3, :3]
    t = np.abs(ac.turned(d, rot))
    if P is None:
        assert np.array_equal(d[:, 2], bc.rays_f64(table, W)[:, 2])                  # z: the plain table's, whatever the yaw
        t[:, 2] = 1.0
    if P is None and sector is None:
        yaw = (ac.nominal_deg(W)[None, :] - az[:, None]).reshape(-1)
        seam = np.isin(yaw, (180.0, 360.0, 540.0))
        assert (az[:, None] * np.ones(W) == 0.0).reshape(-1)[seam].all()
        t[seam, 1] = 1.0
    assert t.min() >= 1e-9, (name, t.min())
    with pytest.raises(ValueError):
        create_rays(fov[0], fov[1], H, W, beam_azimuth=az)                            # offsets without a table
    with pytest.raises(ValueError):
        create_rays(fov[0], fov[1], H, W, beam_table=table, beam_azimuth=np.r_[az, 0.0])


def test_a_row_without_an_offset_is_the_plain_tables_row():
    az = ac.offsets("mixed", 32)
    a, b = ac.az_rays(bc.VLP32C, az, 171).reshape(32, 171, 3), bc.table_rays(bc.VLP32C, 171).reshape(32, 171, 3)
    zero = az == 0.0
    assert zero.sum() > 8 and np.array_equal(a[zero].view(np.int32), b[zero].view(np.int32)) and not np.array_equal(a[~zero], b[~zero])


# ---- the clouds of the GPU test ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sector", [None, ac.SEAM_SECTOR])
@pytest.mark.parametrize("si", range(len(ac.SENSORS)))
def test_the_seeded_clouds_keep_to_the_cap_and_hold_the_chosen_points(si, sector):
    _, table, fov, W = ac.SENSORS[si]
    H = len(table)
    for kind in ("mixed", "ninety"):
        az = ac.offsets(kind, H)
        for n, dtype, seed in [(n, dt, ac.cloud_seed(si, n, sector)) for n, dt in ac.CLOUDS] + [ac.BATCH_CLOUD]:
            pts, rem, lab, special = ac.seeded_cloud(table, fov, az, n, dtype, seed, sector)
            assert pts.dtype == dtype and pts.shape == (n, 3)
            p = ac.project(pts, rem, lab, table, fov, az, W, sector)
            assert p["near"].sum() <= ac.NEAR_CAP * n, (si, kind, n, int(p["near"].sum()))
            if n == 20000:
                assert (p["idx"] >= 0).sum() >= min(0.3 * H * W, 500) or H * W < 10
            if H < 2 or n < 65:
                continue
            (name, (i, r)), = special.items()
            assert p["kept"][i] and p["row"][i] == r and not p["near"][i], (name, kind)
            other = az.copy()
            other[r] = az[r + 1]                                  # the same point under its neighbour's offset
            q = ac.columns(pts[i:i + 1], [r], other, W, sector)
            if name == "seam":                                    # its own offset carried it across: the far side of the image
                plain = ac.columns(pts[i:i + 1], [r], np.zeros(H), W, None)
                assert abs(float(pts[i, 1])) > 0 and abs(int(p["col"][i]) - int(plain["col"][0])) >= W // 2, (p["col"][i], plain["col"][0])
            else:
                assert p["inside"][i] and not q["inside"][0]


def test_the_restated_column_rule_without_offsets_is_the_tables_and_the_sectors():
    """zero offsets: tests/beam_cases.py's columns on the full circle, tests/sector_cases.py's in a sector, bit for bit"""
    import sector_cases as sc
    table, fov, W = bc.VLP32C, bc.VLP32C_FOV, 171
    for dtype in (np.float32, np.float64):
        pts, rem, lab = bc.seeded_cloud(table, fov, 3000, dtype, 4)
        want = bc.project(pts, rem, lab, table, fov, W)
        got = ac.project(pts, rem, lab, table, fov, np.zeros(32), W)
        for k in ("idx", "range", "proj_x", "proj_y", "proj_xf", "proj_yf", "label", "rem"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        pts, rem, lab = sc.seeded_cloud(ac.SEAM_SECTOR, fov, 3000, dtype, 4)
        want = sc.project(pts, rem, lab, ac.SEAM_SECTOR, W, 32, fov, table)
        got = ac.project(pts, rem, lab, table, fov, np.zeros(32), W, ac.SEAM_SECTOR)
        for k in ("idx", "range", "proj_x", "proj_y", "proj_xf", "proj_yf", "label", "rem"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k


def test_the_restated_round_trip_returns_the_sector_rays():
    """the consequence 7d states, on the host: in a sector a ray's own point projects into its own cell and the int32
    reverse projection returns it (1e-4 m at 17.3 m)"""
    table, fov, W = bc.VLP32C, bc.VLP32C_FOV, 171
    for kind in ("mixed", "ninety"):
        az = ac.offsets(kind, 32)
        pts = (ac.az_rays(table, az, W, ac.SEAM_SECTOR).astype(np.float64) * 17.3).astype(np.float32)
        p = ac.project(pts, None, None, table, fov, az, W, ac.SEAM_SECTOR)
        assert np.array_equal(p["idx"].reshape(-1), np.arange(32 * W)), kind
        back = ac.reverse_projection(p["range"], p["proj_x"], p["proj_y"], table, az, False, ac.SEAM_SECTOR)
        assert np.abs(back - pts.astype(np.float64)).max() <= 1e-4
