"""A target sensor with a horizontal sector (``azimuth_model: sector``), host side: the sensor file's new keys and their
refusals, the host rays, the column contract's defining property (a ray's own direction projects into its own column), and
the conditions on the INPUTS of tests/test_sector_gpu.py (the compiled reference raytracer stays within its culling slack on
the sector rays and they hit the scene; the random clouds hardly touch a column boundary).  Restatements:
tests/sector_cases.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import beam_cases as bc  # noqa: E402
import mount_common as mc  # noqa: E402
import sector_cases as sc  # noqa: E402

SHIPPED = os.path.join(ROOT, "config", "front120_64x1024.yaml")
#: share of a cloud's points near a column boundary that the projection tests may leave out (the issue's bound)
NEAR_CAP = 1e-3
LINEAR_FOV = (2.0, -24.8)
#: (n, dtype) of the GPU projection test's clouds
CLOUDS = ((20000, np.float32), (20000, np.float64), (1, np.float32), (2, np.float64), (65, np.float32), (65, np.float64))


def _cfg(**kw):
    cfg = dict(name="s", fov_up=2.0, fov_down=-24.8, beams=64, angle_res_hor=0.1171875, fov_hor=120, azimuth_model="sector",
               azimuth_center=0)
    cfg.update(kw)
    return {k: v for k, v in cfg.items() if v is not None}


def cloud_seed(si, n):
    return 1000 * si + n % 997


# ---- the loader ---------------------------------------------------------------------------------------------------------------
def test_files_without_the_key_and_full_files_load_as_before():
    import yaml
    from lidar_transfer_amd.config import load_sensor
    from lidar_transfer_amd.laserscan import create_rays
    for name in ("vlp32_1024.yaml", "hdl64_1024.yaml", "hdl64_2048.yaml", "os128_2048.yaml", "vlp32c_table_1024.yaml"):
        path = os.path.join(ROOT, "config", name)
        cfg = yaml.safe_load(open(path))
        assert "azimuth_model" not in cfg and "azimuth_center" not in cfg
        for s in (load_sensor(path), load_sensor(dict(cfg, azimuth_model="full")), load_sensor(dict(cfg, azimuth_model="full", azimuth_center=40))):
            assert s.azimuth_model == "full" and s.sector() is None
            assert s.W == int(cfg["fov_hor"] / cfg["angle_res_hor"]) and s.H == cfg["beams"]
            want = create_rays(s.fov_up, s.fov_down, s.H, s.W, beam_table=s.beam_table())
            assert np.array_equal(s.create_rays().view(np.int32), want.view(np.int32))
    # a file that says fov_hor: 120 without the key keeps the reference's behaviour: a third of the columns over the circle
    s = load_sensor(_cfg(azimuth_model=None, azimuth_center=None))
    assert s.sector() is None and s.W == 1024
    assert np.array_equal(s.create_rays().view(np.int32), create_rays(2.0, -24.8, 64, 1024).view(np.int32))


def test_the_shipped_file_gives_its_sector():
    from lidar_transfer_amd.config import load_sensor, sector_radians
    s = load_sensor(SHIPPED)
    assert (s.azimuth_model, s.H, s.W, s.fov_up, s.fov_down, s.beam_model) == ("sector", 64, 1024, 2.0, -24.8, "linear")
    sec = s.sector()
    assert sec == (0.0, 120.0) and all(type(v) is float for v in sec)
    assert sector_radians(sec) == (-0.0 / 180. * np.pi, 120.0 / 180. * np.pi)
    assert np.array_equal(s.create_rays().view(np.int32), sc.sector_rays(sec, 1024, LINEAR_FOV, 64).view(np.int32))
    # a centre beyond +-180 is the same direction a full turn back; +-180 stay
    assert load_sensor(_cfg(azimuth_center=350)).sector() == (-10.0, 120.0)
    assert load_sensor(_cfg(azimuth_center=-360)).sector() == (0.0, 120.0)
    assert load_sensor(_cfg(azimuth_center=180)).sector() == (180.0, 120.0)
    assert load_sensor(_cfg(azimuth_center=-180.0)).sector() == (-180.0, 120.0)
    both = load_sensor(_cfg(fov_up=15.0, fov_down=-25.0, beams=32, beam_model="table", beam_angles=[float(x) for x in bc.VLP32C]))
    assert both.sector() == (0.0, 120.0) and np.array_equal(both.beam_table(), bc.VLP32C)
    assert np.array_equal(both.create_rays().view(np.int32), sc.sector_rays((0.0, 120.0), 1024, table=bc.VLP32C).view(np.int32))


@pytest.mark.parametrize("name,kw", [
    ("an unknown model", dict(azimuth_model="wedge")),
    ("fov_hor 360", dict(fov_hor=360)),
    ("fov_hor 0", dict(fov_hor=0, angle_res_hor=0.1)),
    ("fov_hor negative", dict(fov_hor=-90.0, angle_res_hor=-0.1)),
    ("fov_hor above 360", dict(fov_hor=400)),
    ("fov_hor nan", dict(fov_hor=float("nan"))),
    ("centre nan", dict(azimuth_center=float("nan"))),
    ("centre inf", dict(azimuth_center=float("inf"))),
    ("centre -inf", dict(azimuth_center=float("-inf"))),
    ("centre beyond 360", dict(azimuth_center=360.5)),
    ("centre not a number", dict(azimuth_center="left")),
])
def test_a_sector_that_cannot_be_used_is_refused_at_load_time(name, kw):
    from lidar_transfer_amd.config import load_sensor
    try:
        load_sensor(_cfg(**kw))
    except ValueError as e:
        assert "'s'" in str(e), e                                # the message names the sensor
    else:
        pytest.fail(f"{name}: loaded")
    load_sensor(_cfg())
    load_sensor(_cfg(fov_hor=359.9))


def test_a_source_sensor_with_a_sector_is_refused():
    from lidar_transfer_amd.config import load_sensor, refuse_source_sector
    with pytest.raises(ValueError, match="target"):
        refuse_source_sector(load_sensor(SHIPPED))
    refuse_source_sector(load_sensor(os.path.join(ROOT, "config", "vlp32_1024.yaml")))
    refuse_source_sector((32, 1024, 10.0, -30.0))


def test_the_cli_refuses_a_source_sector_before_it_touches_the_gpu(tmp_path, capsys):
    import shutil
    from lidar_transfer_amd.__main__ import main
    seq = tmp_path / "sequences" / "00"
    (seq / "velodyne").mkdir(parents=True)
    (seq / "labels").mkdir()
    shutil.copy(SHIPPED, tmp_path / "config.yaml")
    rc = main(["-d", str(tmp_path), "-c", os.path.join(ROOT, "config", "approach_mergemesh.yaml"), "-s", "00"])
    out = capsys.readouterr().out
    assert rc == 1 and "target sensors only" in out and "azimuth_model" in out


# ---- rays -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(sc.SECTORS)))
def test_host_rays_of_a_sector_are_the_restatement_bit_for_bit(si):
    from lidar_transfer_amd.laserscan import create_rays
    c, s, W = sc.SECTORS[si]
    for H in (1, 16):
        got = create_rays(LINEAR_FOV[0], LINEAR_FOV[1], H, W, sector=(c, s))
        assert got.dtype == np.float32 and got.shape == (H * W, 3)
        assert np.array_equal(got.view(np.int32), sc.sector_rays((c, s), W, LINEAR_FOV, H).view(np.int32))
    got = create_rays(bc.VLP32C_FOV[0], bc.VLP32C_FOV[1], 32, W, beam_table=bc.VLP32C, sector=(c, s))
    assert np.array_equal(got.view(np.int32), sc.sector_rays((c, s), W, table=bc.VLP32C).view(np.int32))
    # the geometry: column 0 at the left edge, clockwise, the cells' centres, unit length
    az = np.degrees(np.arctan2(got[:W, 1].astype(np.float64), got[:W, 0].astype(np.float64)))
    want = c + s / 2 - (np.arange(W) + 0.5) * s / W
    assert np.abs((az - want + 180) % 360 - 180).max() < 1e-5
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_no_cell_centre_of_the_ray_sectors_lies_near_a_multiple_of_90_degrees():
    """there a component of the ray is the residue of a cancellation and follows the last bit of the double sin / cos: no rule
    in ulps holds for it on two math libraries (tests/test_mount_gpu.py, RAY_SENSORS)"""
    for c, s, W in sc.RAY_SECTORS:
        y = sc.yaw_deg((c, s), W)
        off = np.abs((y + 45) % 90 - 45)
        assert off.min() > 0.08, (c, s, W, off.min())
    y = sc.yaw_deg(sc.SECTORS[3][:2], sc.SECTORS[3][2])
    assert 90.0 in y                                              # why (-90, 30, 7) is not among them


# ---- the column contract ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("si", range(len(sc.SECTORS)))
def test_every_ray_projects_into_its_own_column(si, dtype):
    c, s, W = sc.SECTORS[si]
    for table, fov, H in ((None, LINEAR_FOV, 16), (bc.VLP32C, bc.VLP32C_FOV, 32)):
        rays = sc.sector_rays((c, s), W, fov, H, table)
        pts = (rays.astype(np.float64) * 17.3).astype(dtype)
        p = sc.project(pts, None, None, (c, s), W, H, fov, table)
        w = np.tile(np.arange(W), H)
        assert p["inside"].all() and np.array_equal(p["col"], w), (c, s, W)
        assert not p["near"].any()                                # a cell's centre is half a cell from its boundaries
        if table is not None:                                     # a ray's point lands in its own row too, and is kept
            assert p["kept"].all() and np.array_equal(p["row"], np.repeat(np.arange(H), W))
            assert np.array_equal(p["idx"].reshape(-1), np.arange(H * W))
        else:
            inner = np.repeat((np.arange(H) > 0) & (np.arange(H) < H - 1), W)
            assert p["kept"][inner].all()
        assert np.array_equal(p["proj_x"][p["idx"] >= 0], w[p["kept"]])


def test_the_clouds_of_the_gpu_projection_test_hardly_touch_a_boundary():
    """the window the GPU projection test leaves out cannot hide a failure: at most 0.1 % of a cloud's points lie within 4 ulp
    of a column boundary or of the sector's edge (the points seeded ON an edge are two), and the mask is not idle: at least
    one float32 point is flagged"""
    seen = {}
    flagged32 = 0
    for si, (c, s, W) in enumerate(sc.SECTORS):
        for table, fov, H in ((None, LINEAR_FOV, 16), (bc.VLP32C, bc.VLP32C_FOV, 32)):
            for n, dtype in CLOUDS:
                pts, rem, lab = sc.seeded_cloud((c, s), fov, n, dtype, cloud_seed(si, n))
                p = sc.project(pts, rem, lab, (c, s), W, H, fov, table)
                near = int(p["near"].sum())
                seen[(si, table is not None, n, np.dtype(dtype).name)] = (near, int(p["kept"].sum()))
                assert near <= NEAR_CAP * n, (si, n, dtype, near)
                if dtype == np.float32:
                    flagged32 += near
                if n == 20000:
                    assert p["kept"].sum() > 0.5 * n * s / 360 * 0.8, (si, int(p["kept"].sum()))
                    assert (~p["inside"]).sum() > 0.3 * n * (1 - s / 360)
    assert flagged32 >= 1
    print(f"\n(near a boundary, kept) per (sector, table, n, dtype): {seen}")


# ---- the grid -------------------------------------------------------------------------------------------------------------------
def test_the_fitted_grid_puts_the_rays_on_bin_centres():
    for c, s, W in sc.SECTORS[:3]:
        nb = int(round(W * 360.0 / s))
        rays = sc.sector_rays((c, s), W, LINEAR_FOV, 4)
        fitted, default = sc.grid_dev_az(rays, W, nb), min(sc.grid_dev_az(rays, W, W), sc.grid_dev_az(rays, W, W - 1))
        assert fitted <= 0.5 * s / 360 + sc.LT_BIN_SLACK, (c, s, W, fitted)
        assert default > 0.25, (c, s, W, default)
    assert sc.grid_dev_az(sc.sector_rays((0.0, 120.0), 256, LINEAR_FOV, 4), 256, 768) <= sc.LT_BIN_SLACK


# ---- the inputs of the GPU render test ----------------------------------------------------------------------------------------
RENDER_SEED, RENDER_TRIS = 1, 50000
#: (name, sector, W, table, (fov_up, fov_down), H, pose)
RENDER_CASES = (("120 x 32 linear", (0.0, 120.0), 256, None, LINEAR_FOV, 32, None),
                ("seam x vlp32c", (170.0, 100.0), 200, bc.VLP32C, bc.VLP32C_FOV, 32, None),
                ("70.4 x 16 at the example pose", (35.0, 70.4), 301, None, (3.0, -25.0), 16, mc.POSE_EXAMPLE))


def test_the_compiled_reference_stays_within_its_culling_slack_on_the_sector_rays(oracle, capfd):
    from lidar_transfer_amd.synth import synth_scene
    if not oracle.ref_available("strict"):
        pytest.skip("oracle/_ref not built (the reference checkout was absent at build time)")
    v, f, c, r = synth_scene(RENDER_SEED, RENDER_TRIS)
    seen = {}
    for name, sector, W, table, fov, H, P in RENDER_CASES:
        rays = sc.sector_rays(sector, W, fov, H, table, None if P is None else P[:3, :3])
        org = np.zeros(3, np.float32) if P is None else mc.origin_of(P)
        ref = oracle.ref_trace(rays, org, v, f, c, r, H, kind="strict")
        capfd.readouterr()  # the reference printf()s
        brute = oracle.oracle_trace(rays, org, v, f, c, r, H, mode=oracle.MODE_BRUTE, norm=oracle.NORM_SSE, nthreads=16)
        differs = np.zeros(H * W, bool)
        for k in ("range", "endrem", "endpoints", "endcolors"):
            a, b = np.ascontiguousarray(ref[k]).view(np.int32), np.ascontiguousarray(brute[k]).view(np.int32)
            differs |= (a != b).reshape(H * W, -1).any(1)
        in_plane = (np.abs(rays) < 1e-7).any(1)
        n = int((differs & ~in_plane).sum())
        seen[name] = (n, int((differs & in_plane).sum()), int((brute["tri"] >= 0).sum()), H * W)
        assert n <= mc.REF_CULL_CAP * H * W, (name, n)
        assert (brute["tri"] >= 0).sum() > 0.3 * H * W, f"{name}: the sensor looks past the scene"
    print(f"\nthe compiled reference differs from MODE_BRUTE at (rays off the in-plane set, in-plane rays, hits, rays) {seen}")
