"""A target sensor with a beam table, host side: the sensor file's new key and its refusals, the host rays, the row rule's
binary search against the argmin it stands for, and the conditions on the INPUTS of tests/test_beam_table_gpu.py (the compiled
reference raytracer stays within its culling slack on the table rays; the random clouds hardly touch a row boundary)."""
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

SHIPPED = os.path.join(ROOT, "config", "vlp32c_table_1024.yaml")
#: share of kept points near a row or keep boundary that the row tests may leave out (the issue's bound)
NEAR_CAP = 1e-4


def _cfg(**kw):
    cfg = dict(name="t", fov_up=15.0, fov_down=-25.0, beams=32, angle_res_hor=0.3515625, fov_hor=360, beam_model="table",
               beam_angles=[float(x) for x in bc.VLP32C])
    cfg.update(kw)
    return {k: v for k, v in cfg.items() if v is not None}


# ---- the loader ---------------------------------------------------------------------------------------------------------------
def test_files_without_the_key_load_as_before():
    from lidar_transfer_amd.config import load_sensor
    for name in ("vlp32_1024.yaml", "hdl64_1024.yaml", "hdl64_2048.yaml", "os128_2048.yaml"):
        import yaml
        path = os.path.join(ROOT, "config", name)
        s = load_sensor(path)
        cfg = yaml.safe_load(open(path))
        assert "beam_model" not in cfg
        assert s.beam_model == "linear" and s.beam_table() is None
        want_beams = sorted(cfg["beam_angles"]) if "beam_angles" in cfg else None     # ascending: the reference's quirk
        assert (s.name, s.fov_up, s.fov_down, s.beams, s.angle_res_hor, s.fov_hor, s.beam_angles) == \
            (cfg["name"], cfg["fov_up"], cfg["fov_down"], cfg["beams"], cfg["angle_res_hor"], cfg["fov_hor"], want_beams)
        assert s.as_tuple() == (s.name, s.fov_up, s.fov_down, s.H, s.W, s.beam_angles)
        from lidar_transfer_amd.laserscan import create_rays
        assert np.array_equal(s.create_rays().view(np.int32), create_rays(s.fov_up, s.fov_down, s.H, s.W).view(np.int32))
    lin = load_sensor(_cfg(beam_model="linear"))
    assert lin.beam_model == "linear" and lin.beam_table() is None and lin.beam_angles == sorted(bc.VLP32C.tolist())


def test_the_shipped_file_gives_its_table_descending():
    from lidar_transfer_amd.config import beam_rows, load_sensor
    s = load_sensor(SHIPPED)
    assert (s.beam_model, s.H, s.W, s.fov_up, s.fov_down) == ("table", 32, 1024, 15.0, -25.0)
    t = s.beam_table()
    assert t.dtype == np.float64 and np.array_equal(t, bc.VLP32C) and np.all(np.diff(t) < 0)
    assert np.array_equal(load_sensor(_cfg(beam_angles=[float(x) for x in bc.VLP32C[::-1]])).beam_table(), bc.VLP32C)
    assert np.abs(np.diff(t)).max() == pytest.approx(25.0 - 15.639)
    Brad, halfw = beam_rows(t)
    wb, wh = bc.rows_of(bc.VLP32C)
    assert np.array_equal(Brad, wb) and np.array_equal(halfw, wh)
    assert halfw[0] == (Brad[0] - Brad[1]) / 2 and halfw[-1] == (Brad[-2] - Brad[-1]) / 2
    assert np.array_equal(s.create_rays().view(np.int32), bc.table_rays(bc.VLP32C, 1024).view(np.int32))
    b1, h1 = beam_rows(np.array([-3.0]))
    assert b1.shape == (1,) and h1[0] == 0.0


@pytest.mark.parametrize("name,kw", [
    ("one angle short", dict(beam_angles=[float(x) for x in bc.VLP32C[:-1]])),
    ("one angle more", dict(beam_angles=[float(x) for x in bc.VLP32C] + [-24.0])),
    ("no angles", dict(beam_angles=None)),
    ("nan", dict(beam_angles=[float("nan")] + [float(x) for x in bc.VLP32C[1:]])),
    ("inf", dict(beam_angles=[float("inf")] + [float(x) for x in bc.VLP32C[1:]])),
    ("90 degrees", dict(fov_up=95.0, beam_angles=[90.0] + [float(x) for x in bc.VLP32C[1:]])),
    ("twice the same", dict(beam_angles=[10.333] + [float(x) for x in bc.VLP32C[1:]])),
    ("closer than 1e-6", dict(beam_angles=[10.333 + 5e-7] + [float(x) for x in bc.VLP32C[1:]])),
    ("above fov_up", dict(fov_up=14.9)),
    ("below fov_down", dict(fov_down=-24.9)),
    ("an unknown model", dict(beam_model="spline")),
])
def test_a_table_that_cannot_be_used_is_refused_at_load_time(name, kw):
    from lidar_transfer_amd.config import load_sensor
    with pytest.raises(ValueError):
        load_sensor(_cfg(**kw))
    load_sensor(_cfg())
    ok = [float(x) for x in bc.VLP32C]
    ok[1] = 15.0 - 1e-6 * 1.5                                    # 1.5e-6 degrees under the first: far enough
    assert load_sensor(_cfg(beam_angles=ok)).beam_table()[1] == ok[1]


def test_a_source_sensor_with_a_table_is_refused():
    from lidar_transfer_amd.config import load_sensor, refuse_source_table
    with pytest.raises(ValueError, match="target"):
        refuse_source_table(load_sensor(SHIPPED))
    refuse_source_table(load_sensor(os.path.join(ROOT, "config", "vlp32_1024.yaml")))
    refuse_source_table((32, 1024, 10.0, -30.0))


def test_the_cli_refuses_a_source_table_before_it_touches_the_gpu(tmp_path, capsys):
    import shutil
    from lidar_transfer_amd.__main__ import main
    seq = tmp_path / "sequences" / "00"
    (seq / "velodyne").mkdir(parents=True)
    (seq / "labels").mkdir()
    shutil.copy(SHIPPED, tmp_path / "config.yaml")
    rc = main(["-d", str(tmp_path), "-c", os.path.join(ROOT, "config", "approach_mergemesh.yaml"), "-s", "00"])
    out = capsys.readouterr().out
    assert rc == 1 and "target sensors only" in out


# ---- rays -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fu,fd,H,W", [(3.0, -25.0, 64, 1024), (10.0, -30.0, 32, 2048), (15.0, -15.0, 16, 301), (0.0, -10.0, 1, 720),
                                       (10.0, -30.0, 32, 1)])
def test_host_rays_of_the_linspace_table_are_create_rays_bit_for_bit(fu, fd, H, W):
    from lidar_transfer_amd.laserscan import create_rays
    base = create_rays(fu, fd, H, W)
    tab = create_rays(fu, fd, H, W, beam_table=np.linspace(fu, fd, H))
    assert tab.dtype == np.float32 and tab.shape == (H * W, 3)
    assert np.array_equal(tab.view(np.int32), base.view(np.int32))
    assert np.array_equal(tab.view(np.int32), bc.table_rays(np.linspace(fu, fd, H), W).view(np.int32))
    with pytest.raises(ValueError):
        create_rays(fu, fd, H, W, beam_table=np.linspace(fu, fd, H + 1))


def test_host_rays_of_the_two_tables_are_the_restatement():
    from lidar_transfer_amd.laserscan import create_rays
    for name, table, fov, W in bc.TABLES:
        got = create_rays(fov[0], fov[1], len(table), W, beam_table=table)
        assert np.array_equal(got.view(np.int32), bc.table_rays(table, W).view(np.int32)), name
        el = np.degrees(np.arcsin(got.astype(np.float64)[::W, 2]))
        assert np.abs(el - table).max() < 1e-5, name


# ---- rows -----------------------------------------------------------------------------------------------------------------------
def _row_tables():
    return [(n, t, f) for n, t, f, _ in bc.TABLES] + list(bc.TINY)


def test_the_binary_search_row_is_the_argmin_row():
    rng = np.random.default_rng(5)
    for name, table, fov in _row_tables():
        Brad, _ = bc.rows_of(table)
        q = rng.uniform(np.radians(fov[1]) - 0.1, np.radians(fov[0]) + 0.1, 1_000_000)
        q[:len(Brad)] = Brad                                                      # on every beam
        q[len(Brad):2 * len(Brad) - 1] = (Brad[:-1] + Brad[1:]) / 2                # midway between neighbours, as rounded
        q[100:200] = np.nextafter(Brad[0], 1.0)
        q32 = q.astype(np.float32).astype(np.float64)                             # the pitches of a float32 cloud
        for qq in (q, q32):
            a, s = bc.argmin_rows(qq, Brad), bc.search_rows(qq, Brad)
            assert np.array_equal(a, s), (name, int((a != s).sum()))
            assert a.min() == 0 and a.max() == len(Brad) - 1


def test_on_a_beam_and_exactly_midway_go_to_the_smaller_row():
    table = np.array([10.0, 2.0, -2.0, -10.0])                # symmetric about 0: z = 0 is exactly midway between rows 1 and 2
    Brad, halfw = bc.rows_of(table)
    assert Brad[1] == -Brad[2]
    for rows in (bc.argmin_rows, bc.search_rows):
        assert np.array_equal(rows(Brad, Brad), [0, 1, 2, 3])
        assert rows(np.array([0.0]), Brad)[0] == 1                       # |0 - B1| == |0 - B2| exactly: the first minimum
        assert rows(np.array([-1e-12]), Brad)[0] == 2 and rows(np.array([1e-12]), Brad)[0] == 1
        assert rows(np.array([-5e-324]), Brad)[0] == 1                   # below the distances' ulp: still the exact tie
    # through the whole restatement: a point in the plane z = 0 lands in row 1 and is kept (exactly halfw away)
    pts = np.array([[10.0, 0.0, 0.0], [5.0, 5.0, 0.0]])
    p = bc.project(pts, np.ones(2, np.float32), np.array([7, 8], np.int32), table, (10.0, -10.0), 16)
    assert p["kept"].all() and np.array_equal(p["row"], [1, 1])
    assert (p["proj_y"][p["idx"] >= 0] == 1).all() and (p["idx"] >= 0).sum() == 2
    # and beyond half a gap outside the outermost beam nothing is kept
    up = np.radians(10.0) + halfw[0] * 1.001
    far = np.array([[np.cos(up), 0.0, np.sin(up)]]) * 10.0
    assert not bc.project(far, None, None, table, (10.0, -10.0), 16)["kept"].any()


def test_the_random_clouds_of_the_gpu_row_test_hardly_touch_a_boundary():
    """the window the GPU row test leaves out cannot hide a failure: at most 1e-4 of the kept points lie within 4 ulp of a
    row or keep boundary (the points seeded ON a boundary are a handful)"""
    seen = {}
    for name, table, fov in _row_tables():
        for dtype in (np.float32, np.float64):
            pts, rem, lab = bc.seeded_cloud(table, fov, 100003, dtype, seed=len(table))
            p = bc.project(pts, rem, lab, table, fov, 64)
            kept = int(p["kept"].sum())
            near = int((p["near"] & p["kept"]).sum())
            seen[(name, np.dtype(dtype).name)] = (near, kept)
            assert kept > 10000, (name, kept)
            assert near <= NEAR_CAP * kept, (name, dtype, near, kept)
    print(f"\n(near a boundary, kept) of 100 003 points: {seen}")


# ---- the inputs of the GPU render test ----------------------------------------------------------------------------------------
# Observed where they were chosen (compiled reference against MODE_BRUTE, both with the host's own RSQRTSS seed): 0 rays off
# the in-plane set in all three cases.
RENDER_SEED, RENDER_TRIS = 1, 50000
RENDER_CASES = (("vlp32c", bc.VLP32C, 1024, None), ("two_block", bc.TWO_BLOCK, 512, None), ("vlp32c at the example pose", bc.VLP32C, 1024, mc.POSE_EXAMPLE))


def test_the_compiled_reference_stays_within_its_culling_slack_on_the_table_rays(oracle, capfd):
    from lidar_transfer_amd.synth import synth_scene
    if not oracle.ref_available("strict"):
        pytest.skip("oracle/_ref not built (the reference checkout was absent at build time)")
    v, f, c, r = synth_scene(RENDER_SEED, RENDER_TRIS)
    seen = {}
    for name, table, W, P in RENDER_CASES:
        H = len(table)
        rays = bc.table_rays(table, W, None if P is None else P[:3, :3])
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
        seen[name] = (n, int((differs & in_plane).sum()), int((brute["tri"] >= 0).sum()))
        assert n <= mc.REF_CULL_CAP * H * W, (name, n)
        assert (brute["tri"] >= 0).sum() > 0.3 * H * W, f"{name}: the sensor looks past the scene"
    print(f"\nthe compiled reference differs from MODE_BRUTE at (rays off the in-plane set, in-plane rays, of hits) {seen}")
