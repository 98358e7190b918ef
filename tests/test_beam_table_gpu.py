"""A target sensor with a beam table (``beam_model: table``), on the device: its rays against ``lt_create_rays_dev`` and the
float64 restatement; a render of the irregular ray set by both strategies against the brute-force oracle and the compiled
reference raytracer; the row and keep rule of ``LT_PROJ_BEAM_ROWS`` against the literal sequential loop; the reverse
projection; ``DeviceDeform`` / ``SequenceTransfer`` / the CLI with a table target against a chain composed here from the
independent pieces of tests/oracle_chain.py on the product's downloaded table rays; and the guard that a target without a
table takes exactly the path it took.  Restatements: tests/beam_cases.py; the conditions on the inputs:
tests/test_beam_table_cpu.py."""
import ctypes as C
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
import test_beam_table_cpu as btc  # noqa: E402
import test_evaluate_cpu as ev  # noqa: E402
import test_ingest_cpu as cpu  # noqa: E402
import test_mount_gpu as tm  # noqa: E402
import test_sequence_cpu as sc  # noqa: E402

pytestmark = pytest.mark.gpu
LT_ERR_INVALID_ARG = -1
T_EXAMPLE = tm.T_EXAMPLE
#: the F17 sequence's target of these tests: the VLP-32C table on 32 x 512 (golden F18's target has the same size)
SEQ_TARGET = (32, 512, bc.VLP32C_FOV[0], bc.VLP32C_FOV[1])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _differs(a, b):
    """element by element: do the bits differ? (any dtype)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.view(u) != b.view(u)


# ---- rays -----------------------------------------------------------------------------------------------------------------------
LINSPACE_SENSORS = ((3.0, -25.0, 64, 1024), (10.0, -30.0, 32, 2048), (15.0, -15.0, 16, 301), (0.0, -10.0, 1, 720),
                    (10.0, -30.0, 32, 1), (3.0, -25.0, 1, 1), (3.0, -25.0, 3, 171)) + tm.RAY_SENSORS
#: the tables of the ray tests: the two sensors and a table of one row (at W = 1 a single ray)
RAY_TABLES = bc.TABLES + (bc.TINY[0] + (1,),)


def test_device_rays_of_the_linspace_table_are_create_rays_bit_for_bit():
    from lidar_transfer_amd.laserscan import create_rays_device
    for fu, fd, H, W in LINSPACE_SENSORS:
        base = create_rays_device(fu, fd, H, W).cpu().numpy()
        tab = create_rays_device(fu, fd, H, W, beam_table=np.linspace(fu, fd, H)).cpu().numpy()
        assert tab.shape == (H * W, 3) and tab.dtype == np.float32
        assert np.array_equal(_bits(tab), _bits(base)), (H, W)
    for fu, fd, H, W in tm.RAY_SENSORS:                        # and with a pose: lt_create_rays_pose_dev's bits
        rot = mc.POSE_GENERAL[:3, :3]
        base = create_rays_device(fu, fd, H, W, rot=rot).cpu().numpy()
        tab = create_rays_device(fu, fd, H, W, rot=rot, beam_table=np.linspace(fu, fd, H)).cpu().numpy()
        assert np.array_equal(_bits(tab), _bits(base)), (H, W)
    with pytest.raises(ValueError):
        create_rays_device(3.0, -25.0, 4, 8, beam_table=np.linspace(3.0, -25.0, 5))


@pytest.mark.parametrize("W", [1, 301, 1024])
def test_device_rays_of_the_two_tables_equal_the_restatement(W):
    from lidar_transfer_amd.laserscan import create_rays_device
    for name, table, fov, _ in RAY_TABLES:
        dev = create_rays_device(fov[0], fov[1], len(table), W, beam_table=table).cpu().numpy()
        n = tm._rays_rule(dev, bc.table_rays(table, W), (name, W))
        assert np.abs(np.linalg.norm(dev.astype(np.float64), axis=1) - 1).max() < 1e-6
        print(f"\n{name} x {W}: {n} of {dev.size} elements not bit-equal to the restatement")


@pytest.mark.parametrize("W", [1, 1023, 1025])
@pytest.mark.parametrize("pose", ["example", "general"])
def test_posed_device_rays_of_the_two_tables_equal_the_restatement(pose, W):
    """W - 1 no multiple of 4: no ray ON a zero of a rotated component (tests/test_mount_gpu.py, RAY_SENSORS); W = 1: the one ray
    at the seam, which every W has, and with the table of one row a launch of a single ray"""
    from lidar_transfer_amd.laserscan import create_rays_device
    rot = dict(mc.RENDER_POSES)[pose][:3, :3]
    for name, table, fov, _ in RAY_TABLES:
        dev = create_rays_device(fov[0], fov[1], len(table), W, rot=rot, beam_table=table).cpu().numpy()
        n = tm._rays_rule(dev, bc.table_rays(table, W, rot), (name, pose, W))
        print(f"\n{name} x {W} at the {pose} pose: {n} of {dev.size} elements not bit-equal to the restatement")


def test_table_rays_without_a_rotation_and_with_the_identity_are_equal_by_value():
    from lidar_transfer_amd.laserscan import create_rays_device
    for name, table, fov, W in bc.TABLES:
        none = create_rays_device(fov[0], fov[1], len(table), W, rot=None, beam_table=table).cpu().numpy()
        eye = create_rays_device(fov[0], fov[1], len(table), W, rot=np.eye(3), beam_table=table).cpu().numpy()
        assert np.array_equal(eye, none), name                  # by value: 0 * x may turn a zero's sign


# ---- render ---------------------------------------------------------------------------------------------------------------------
def _rayset_params(rs):
    lib = rs._lib
    lib.lt_debug_rayset_params.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.lt_debug_rayset_params.restype = C.c_int
    nb, p = (C.c_int * 2)(), (C.c_float * 6)()
    assert lib.lt_debug_rayset_params(rs._h, nb, p) == 0
    return dict(nb_az=int(nb[0]), nb_el=int(nb[1]), el_lo=float(p[2]), el_scale=float(p[3]), dev_az=float(p[4]), dev_el=float(p[5]))


def _render_both(mesh, trays, origin, H):
    """the scatter (with its counters and the ray set's grid) and the LBVH on one mesh"""
    import torch
    from lidar_transfer_amd.raytracer import RaySet, Scene
    dev = torch.device("cuda", 0)
    scn = Scene(0)
    scn.set_mesh(*[torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in mesh])
    rs = RaySet(trays, H)
    prm = _rayset_params(rs)
    a = scn.render(rs, origin, count=True)
    stats = a.pop("stats")
    scn.build()
    b = scn.trace(trays, origin, H)
    torch.cuda.synchronize()
    a = {k: x.cpu().numpy() for k, x in a.items()}
    b = {k: x.cpu().numpy() for k, x in b.items()}
    rs.close()
    scn.close()
    return a, b, prm, stats


@pytest.mark.parametrize("case", range(len(btc.RENDER_CASES)))
def test_render_of_table_rays_equals_brute_force_and_the_compiled_reference(case, capfd):
    """tests/test_beam_table_cpu.py checked the scene and the three ray sets; the rays here are the product's own"""
    import oracle_chain as oc
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.synth import synth_scene
    from oracle import binding as ob
    if not ob.ref_available("strict"):
        pytest.skip("oracle/_ref not built (the reference checkout was absent at build time)")
    name, table, W, P = btc.RENDER_CASES[case]
    H = len(table)
    mesh = synth_scene(btc.RENDER_SEED, btc.RENDER_TRIS)
    rot = None if P is None else P[:3, :3]
    fov = (float(table.max()), float(table.min()))
    trays = create_rays_device(fov[0], fov[1], H, W, rot=rot, beam_table=table)
    rays = trays.cpu().numpy()
    tm._rays_rule(rays, bc.table_rays(table, W, rot), name)
    org = np.zeros(3, np.float32) if P is None else mc.origin_of(P)
    a, b, prm, stats = _render_both(mesh, trays, tuple(float(x) for x in org), H)
    grid_line = f"{name}: posed, dev_el {prm['dev_el']:.3f}"
    # the irregular path is what ran: the uniform elevation grid misses the beams by nearly half a bin, and bins hold several
    el = np.arctan2(rays[::W, 2].astype(np.float64), np.hypot(rays[::W, 0], rays[::W, 1]).astype(np.float64))
    if P is None:
        bins = np.clip(np.floor((el - prm["el_lo"]) * prm["el_scale"] + 0.5), 0, prm["nb_el"] - 1).astype(int)
        per_bin = np.bincount(bins, minlength=prm["nb_el"])
        grid_line = (f"{name}: nb_el {prm['nb_el']} dev_el {prm['dev_el']:.3f} dev_az {prm['dev_az']:.3f}; beams per elevation "
                     f"bin: max {per_bin.max()}, empty {int((per_bin == 0).sum())}; candidate bins {stats['nodes_visited']}, "
                     f"triangle tests {stats['tris_tested']} ({stats['tris_tested'] / (H * W):.1f} per ray)")
        assert prm["nb_el"] == H and prm["dev_el"] > 0.4, prm
        assert per_bin.max() >= 2 and (per_bin == 0).any(), per_bin
    brute = ob.oracle_trace(rays, org, *mesh, H, mode=ob.MODE_BRUTE, norm=ob.NORM_SSE_TABLE, nthreads=oc.THREADS)
    for k in ("tri", "range", "endcolors", "endrem", "endpoints"):
        for tag, got in (("scatter", a), ("lbvh", b)):
            bad = np.nonzero((_bits(got[k]) != _bits(brute[k])).reshape(H * W, -1).any(1))[0]
            assert bad.size == 0, f"{name}: {tag} {k} differs from MODE_BRUTE at {bad.size} rays, first {bad[:5]}"
    ref = tm._reference_trace(rays, org, mesh, H)
    capfd.readouterr()  # the reference printf()s
    same = np.ones(H * W, bool)
    for k in ("range", "endcolors", "endrem", "endpoints"):
        same &= (_bits(ref[k]) == _bits(brute[k])).reshape(H * W, -1).all(1)
    for k in ("range", "endcolors", "endrem", "endpoints"):
        for tag, got in (("scatter", a), ("lbvh", b)):
            assert np.array_equal(_bits(got[k])[same], _bits(ref[k])[same]), f"{name}: {tag} {k} vs the compiled reference"
    hits = int((brute["tri"] >= 0).sum())
    assert hits > 0.3 * H * W
    print("\n" + grid_line)
    print(f"{name}: the reference differs from MODE_BRUTE at {int((~same).sum())} of {H * W} rays (in-plane rays included); {hits} hits")


def test_render_of_two_beams_a_millionth_of_a_degree_apart_equals_brute_force():
    import oracle_chain as oc
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.synth import synth_scene
    from oracle import binding as ob
    table = np.array([-3.0, -3.000001])
    H, W = 2, 1024
    mesh = synth_scene(btc.RENDER_SEED, btc.RENDER_TRIS)
    trays = create_rays_device(-3.0, -3.000001, H, W, beam_table=table)
    rays = trays.cpu().numpy()
    a, b, prm, _ = _render_both(mesh, trays, (0.0, 0.0, 0.0), H)
    print(f"\ntwo beams 1e-6 degrees apart: el_scale {prm['el_scale']:.3g} dev_el {prm['dev_el']:.3f}")
    brute = ob.oracle_trace(rays, np.zeros(3, np.float32), *mesh, H, mode=ob.MODE_BRUTE, norm=ob.NORM_SSE_TABLE, nthreads=oc.THREADS)
    for k in ("tri", "range", "endcolors", "endrem", "endpoints"):
        for tag, got in (("scatter", a), ("lbvh", b)):
            bad = np.nonzero((_bits(got[k]) != _bits(brute[k])).reshape(H * W, -1).any(1))[0]
            assert bad.size == 0, f"{tag} {k} differs from MODE_BRUTE at {bad.size} rays, first {bad[:5]}"
    assert (brute["tri"] >= 0).sum() > 0.5 * H * W


# ---- rows -----------------------------------------------------------------------------------------------------------------------
ROW_KEYS = ("idx", "range", "rem", "label", "proj_x", "proj_y", "proj_yf")
ROW_W = 64
ROW_TABLES = [(n, t, f) for n, t, f, _ in bc.TABLES] + list(bc.TINY)


def _up(cloud):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in cloud)


def _check_rows(got, want, tag, cap=None):
    """bit for bit on every cell no near-boundary point touches; ``cap``: the share of such points the CPU test allows.
    ``proj_xf`` is not among the contract's images: float32 clouds bit for bit (the yaw is the correctly rounded float32 on
    both sides); float64 clouds within 8 ulp of W -- the two float64 ``atan2`` are each within 2 ulp of the true yaw
    (|yaw| <= pi), ``0.5 * (yaw / pi + 1) * W`` carries that as at most 4 ulp(pi) * W / (2 pi) < 1 ulp(W), and its one
    division, one sum and two products add an ulp of the result (<= ulp(W)) each."""
    skip = bc.near_cells(want, ROW_W)
    kept, near = int(want["kept"].sum()), int((want["near"] & want["kept"]).sum())
    bad = {k: int(_differs(got[k].cpu().numpy(), want[k])[~skip].sum()) for k in ROW_KEYS}
    yf_g, yf_w = got["proj_yf"].cpu().numpy(), want["proj_yf"]
    ulps = np.abs(yf_g - yf_w)[~skip] / np.maximum(np.spacing(np.abs(yf_w))[~skip], np.finfo(yf_w.dtype).tiny)
    xf_g, xf_w = got["proj_xf"].cpu().numpy(), want["proj_xf"]
    xf_off = float(np.abs(xf_g - xf_w)[~skip].max() / np.spacing(xf_w.dtype.type(ROW_W)))
    print(f"\nrows {tag}: kept {kept}, near a boundary {near}, cells left out {int(skip.sum())}, cells differing {bad}, "
          f"proj_yf off by at most {ulps.max() if ulps.size else 0:.0f} ulp, proj_xf by {xf_off:.2f} ulp(W)")
    if cap is not None:
        assert near <= cap * kept, (tag, near, kept)
    for k in ROW_KEYS:
        assert bad[k] == 0, (tag, k, bad[k])
    empty = want["idx"] < 0
    for k in ("proj_x", "proj_y", "proj_xf", "proj_yf"):
        assert not got[k].cpu().numpy()[empty & ~skip].any(), (tag, k)      # empty cells hold 0
    if xf_w.dtype == np.float32:
        assert not _differs(xf_g, xf_w)[~skip].any(), tag
    else:
        assert xf_off <= 8, (tag, xf_off)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("ti", range(len(ROW_TABLES)))
def test_projected_rows_equal_the_literal_loop(ti, dtype):
    """float64 clouds: the winner's pitch is the correctly rounded ``asin`` on both sides (``lt_asin_cr`` on the device,
    ``beam_cases.asin_cr`` here) -- the device library's and numpy's own float64 ``asin`` differ in the last place in one
    argument of ten, which is what ``proj_yf`` showed when both sides used their library's."""
    import torch
    from lidar_transfer_amd.laserscan import Projector
    name, table, fov = ROW_TABLES[ti]
    H = len(table)
    outs = ROW_KEYS + ("proj_xf",)
    pj = Projector()
    for n in (1, 255, 257, 100003):
        cloud = bc.seeded_cloud(table, fov, n, dtype, seed=len(table))      # n = 100 003: the clouds the CPU test counted
        want = bc.project(*cloud, table, fov, ROW_W)
        got = pj.project([_up(cloud)], fov[0], fov[1], H, ROW_W, new=True, remove=True, outputs=outs, beam_table=table)[0]
        torch.cuda.synchronize()
        _check_rows(got, want, f"{name} {np.dtype(dtype).name} n={n}", cap=btc.NEAR_CAP if n == 100003 else None)
        if n == 100003:
            assert (want["idx"] >= 0).sum() > 0.5 * H * ROW_W or H > 2
    # two clouds in one batch on a side stream
    c1, c2 = bc.seeded_cloud(table, fov, 257, dtype, seed=3), bc.seeded_cloud(table, fov, 100003, dtype, seed=4)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d1, d2 = _up(c1), _up(c2)
        got = pj.project([d1, d2], fov[0], fov[1], H, ROW_W, new=True, remove=True, outputs=outs, beam_table=table, stream=st)
    st.synchronize()
    _check_rows(got[0], bc.project(*c1, table, fov, ROW_W), f"{name} batch/0")
    _check_rows(got[1], bc.project(*c2, table, fov, ROW_W), f"{name} batch/1")
    pj.close()


def test_on_a_beam_exactly_midway_and_the_dead_zone_on_the_device():
    """no window here: a table symmetric about 0 makes the midway case exact on both sides (z = 0)"""
    import torch
    from lidar_transfer_amd.laserscan import Projector
    table, fov, W = np.array([10.0, 2.0, -2.0, -10.0]), (10.0, -10.0), 16
    Brad, halfw = bc.rows_of(table)
    el = np.array([0.0, 0.0, np.radians(5.0), np.radians(10.0) + halfw[0] * 1.01, 0.0])      # midway x2, dead zone, beyond, depth 0
    az = np.array([0.3, 2.0, -1.0, 1.0, 0.0])
    dist = np.array([10.0, 7.0, 5.0, 5.0, 0.0])
    for dtype in (np.float32, np.float64):
        pts = np.stack([dist * np.cos(el) * np.cos(az), dist * np.cos(el) * np.sin(az), dist * np.sin(el)], 1).astype(dtype)
        pts[:2, 2] = 0.0
        cloud = (pts, np.arange(5, dtype=np.float32), np.arange(5, dtype=np.int32) + 1)
        want = bc.project(*cloud, table, fov, W)
        assert np.array_equal(want["kept"], [True, True, False, False, False]) and np.array_equal(want["row"][:2], [1, 1])
        pj = Projector()
        got = pj.project([_up(cloud)], fov[0], fov[1], 4, W, new=True, remove=True, outputs=ROW_KEYS + ("proj_xf", "n_kept"),
                         beam_table=table)[0]
        torch.cuda.synchronize()
        assert int(got["n_kept"].cpu()[0]) == 2
        for k in ROW_KEYS + ("proj_xf",):
            assert not _differs(got[k].cpu().numpy(), want[k]).any(), (dtype, k)
        assert (got["idx"].cpu().numpy() >= 0).sum() == 2 and (got["proj_y"].cpu().numpy()[got["idx"].cpu().numpy() >= 0] == 1).all()
        pj.close()


def test_the_single_cloud_entry_point_takes_the_flag_too():
    from lidar_transfer_amd import _lib
    from lidar_transfer_amd.config import beam_rows
    lib = _lib.load()
    name, table, fov, _ = bc.TABLES[0]
    H, W = len(table), ROW_W
    pts, rem, lab = bc.seeded_cloud(table, fov, 5000, np.float64, seed=9)
    want = bc.project(pts, rem, lab, table, fov, W)
    tab = np.ascontiguousarray(np.concatenate(beam_rows(table)))
    n = len(pts)
    o = dict(py=np.empty(n, np.int32), yf=np.empty(n, np.float64), idx=np.empty((H, W), np.int32), range=np.empty((H, W), np.float32))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    kept = C.c_int(0)
    flags = _lib.LT_PROJ_BEAM_ROWS | _lib.LT_PROJ_NEW | _lib.LT_PROJ_REMOVE
    args = lambda fl, nb: [vp(pts), 1, vp(rem), vp(lab.view(np.uint32)), n, fov[0], fov[1], H, W, vp(tab), nb, fl, None, 0, None, None, None,   # noqa: E731
                           None, None, vp(o["py"]), None, vp(o["yf"]), vp(o["idx"]), vp(o["range"]), None, None, None, None, None,
                           0.0, -1.0, 0.0, C.byref(kept)]
    assert lib.lt_range_projection(*args(flags, H)) == 0
    k = kept.value
    skip = bc.near_cells(want, W)
    n_near = int(want["near"].sum())
    assert abs(k - int(want["kept"].sum())) <= n_near and k > 3000
    assert not _differs(o["range"], want["range"])[~skip].any()
    occupied = (want["idx"] >= 0) & ~skip                          # (the numbering of the kept points may shift by a near point)
    assert np.array_equal(o["idx"][~skip] >= 0, want["idx"][~skip] >= 0) and occupied.sum() > 1000
    if n_near == 0:
        assert np.array_equal(o["idx"], want["idx"]) and np.array_equal(o["py"][:k], want["row"][want["kept"]])
        assert np.array_equal(o["yf"][:k], want["pitch"][want["kept"]])
    for fl, nb in ((_lib.LT_PROJ_BEAM_ROWS, H), (_lib.LT_PROJ_BEAM_ROWS | _lib.LT_PROJ_NEW, H), (flags, H - 1), (flags, 2 * H)):
        assert lib.lt_range_projection(*args(fl, nb)) == LT_ERR_INVALID_ARG, (fl, nb)
        assert b"LT_PROJ_BEAM_ROWS" in lib.lt_last_error()


def test_any_other_flag_combination_is_refused():
    import torch
    from lidar_transfer_amd import _lib
    from lidar_transfer_amd.config import beam_rows
    from lidar_transfer_amd.laserscan import Projector
    lib = _lib.load()
    name, table, fov, _ = bc.TABLES[0]
    H, W = len(table), ROW_W
    cloud = _up(bc.seeded_cloud(table, fov, 257, np.float32, seed=1))
    pj = Projector()
    for new, remove in ((False, False), (True, False), (False, True)):
        with pytest.raises(RuntimeError, match="LT_PROJ_BEAM_ROWS"):
            pj.project([cloud], fov[0], fov[1], H, W, new=new, remove=remove, beam_table=table)
    tab = np.ascontiguousarray(np.concatenate(beam_rows(table)))
    cl, im = (_lib.Cloud * 1)(), (_lib.ProjImages * 1)()
    rng = torch.empty((H, W), dtype=torch.float32, device="cuda")
    cl[0].points, cl[0].rem, cl[0].label, cl[0].n = cloud[0].data_ptr(), cloud[1].data_ptr(), cloud[2].data_ptr(), 257
    im[0].range = rng.data_ptr()
    good = _lib.LT_PROJ_BEAM_ROWS | _lib.LT_PROJ_NEW | _lib.LT_PROJ_REMOVE
    call = lambda fl, nb, t: lib.lt_range_projection_batch_dev(pj._h, 1, cl, 0, fov[0], fov[1], H, W, t, nb, fl, None, 0, im,   # noqa: E731
                                                               0.0, -1.0, 0.0, None)
    vp = tab.ctypes.data_as(C.c_void_p)
    for fl, nb, t in ((4, H, vp), (4 | 2, H, vp), (4 | 1, H, vp), (good | 8, H, vp), (good, H + 1, vp), (good, 0, None), (good, H, None)):
        assert call(fl, nb, t) == LT_ERR_INVALID_ARG, (fl, nb)
    assert call(good, H, vp) == 0
    torch.cuda.synchronize()
    pj.close()


# ---- reverse projection ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preserve_float", [False, True])
@pytest.mark.parametrize("shape", [(1, 1), (32, 1024), (64, 301)])
def test_reverse_projection_with_a_table_equals_the_float64_restatement(shape, preserve_float):
    """rtol = atol = 1e-13 is tests/test_post_shapes_gpu.py's bound for the linear kernel (two float64 math libraries): kept
    from there, not derived.  The largest relative difference is printed (profiles/beam_table/README.md records it)."""
    import torch
    from lidar_transfer_amd import _lib
    lib = _lib.load()
    H, W = shape
    table = {1: np.array([-3.0]), 32: bc.VLP32C, 64: bc.TWO_BLOCK}[H]
    Brad = bc.rows_of(table)[0]
    rng = np.random.default_rng(H * W)
    r = rng.uniform(0.5, 80.0, (H, W)).astype(np.float32)
    r[rng.random((H, W)) < 0.2] = 0.0
    if preserve_float:
        px = rng.uniform(0, W, (H, W))
        py = rng.uniform(Brad.min() - 0.05, Brad.max() + 0.05, (H, W))
    else:
        px = rng.integers(0, W, (H, W)).astype(np.int32)
        py = rng.integers(0, H, (H, W)).astype(np.int32)
    want = bc.reverse_projection(r, px, py, table, preserve_float)
    d = [torch.from_numpy(a).cuda() for a in (r, px, py, Brad)]
    for stream in (None, torch.cuda.Stream()):
        out = torch.full((H * W + 1, 3), -7.0, dtype=torch.float64, device="cuda")
        st = torch.cuda.current_stream() if stream is None else stream
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        rc = lib.lt_reverse_projection_beams_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), int(preserve_float),
                                                 d[3].data_ptr(), H, W, out.data_ptr(), C.c_void_p(st.cuda_stream))
        assert rc == 0
        st.synchronize()
        got = out.cpu().numpy()
        assert (got[-1] == -7.0).all()                          # nothing past the last cell
        got = got[:-1]
        with np.errstate(all="ignore"):
            rel = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == want, 0.0, np.inf))
        print(f"\nreverse {H}x{W} preserve_float={preserve_float}: largest relative difference {rel.max():.1e}, largest absolute "
              f"{np.abs(got - want).max():.1e}")
        assert np.allclose(got, want, rtol=1e-13, atol=1e-13)
    bad = [d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), int(preserve_float), d[3].data_ptr(), H, W, out.data_ptr(), None]
    for k in (0, 1, 2, 7):
        b = list(bad)
        b[k] = None
        assert lib.lt_reverse_projection_beams_dev(*b) == LT_ERR_INVALID_ARG, k
    if not preserve_float:
        b = list(bad)
        b[4] = None
        assert lib.lt_reverse_projection_beams_dev(*b) == LT_ERR_INVALID_ARG


# ---- chains ---------------------------------------------------------------------------------------------------------------------
def _table_rays_dev(target, table, P=None):
    """the product's table rays, downloaded, after they passed the rays' rule against the restatement"""
    from lidar_transfer_amd.laserscan import create_rays_device
    tH, tW, tfu, tfd = target
    rot = None if P is None else P[:3, :3]
    rays = create_rays_device(tfu, tfd, tH, tW, rot=rot, beam_table=table).cpu().numpy()
    tm._rays_rule(rays, bc.table_rays(table, tW, rot), "table rays of the oracle chain")
    return rays


def _finish(vol, target, rays, P=None, T=None):
    """oracle_chain.finish with the render of the table rays (from the pose ``P`` when the target is mounted)"""
    import oracle_chain as oc
    from oracle import binding as ob
    mesh = vol.mesh()
    tH = target[0]
    org = np.zeros(3, np.float32) if P is None else mc.origin_of(P)
    ref = tm._reference_trace(rays, org, mesh, tH)
    brute = ob.oracle_trace(rays, org, *mesh, tH, mode=ob.MODE_BRUTE, norm=ob.NORM_SSE_TABLE, nthreads=oc.THREADS)
    ref["rays"] = brute["rays"] = rays
    return dict(mesh=mesh, ref=ref, brute=brute, T=None if T is None else np.array(T, np.float64).reshape(4, 4))


def _check_scan(got, want, tag, ties):
    """check_images' rule and TIE_BOUND; the written bytes are write() of the images that rule selects"""
    import oracle_chain as oc
    if want["T"] is not None:
        return tm._check_mounted_scan(got, want, tag, ties)
    g = dict(range=got["range"].cpu().numpy(), label=got["label"].cpu().numpy(), rem=got["rem"].cpu().numpy(),
             endpoints=got["endpoints"].cpu().numpy(), tri=got["tri"].cpu().numpy())
    n = oc.check_images(g, want, tag)
    assert n[0] <= tm.TIE_BOUND * want["ref"]["range"].size, f"{tag}: {n[0]} exact-t tie pixels"
    ties[tag] = n
    want["bin"], want["label_file"] = want["bin_rule"], want["label_file_rule"]
    if "bin" in got:
        assert np.array_equal(got["bin"].cpu().numpy().view(np.uint8), want["bin"].view(np.uint8)), f"{tag}: velodyne bytes"
        assert np.array_equal(got["label_file"].cpu().numpy().view(np.uint32), want["label_file"]), f"{tag}: label bytes"
    assert want["bin"].shape[0] > 100, f"{tag}: the oracle's scan is nearly empty"


@pytest.mark.parametrize("mounted", [False, True])
def test_mesh_with_a_table_target_equals_the_composed_oracle_chain(mounted):
    import oracle_chain as oc
    import pin_cases
    import test_default_chain_gpu as dc
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    tm._need_reference_builds()
    T = T_EXAMPLE if mounted else None
    P = tm._pose_of(T) if mounted else None
    _, src, _, n_scans, bnds, voxel, seeds = pin_cases.deform_mesh_case(0)
    tgt = (32, 256, bc.VLP32C_FOV[0], bc.VLP32C_FOV[1])
    clouds = pin_cases.deform_mesh_clouds(seeds[0], n_scans, src, dc._host_render)
    with DeviceDeform(src, tgt, bnds.copy(), voxel, transformation=T, t_beam_table=bc.VLP32C) as dd:
        assert np.array_equal(dd.rayset.beam_table, bc.VLP32C)
        got = dd.mesh(tm._dev(clouds))
        torch.cuda.synchronize()
        H, W, fu, fd = src
        b = np.array(bnds, copy=True)
        dim, origin = oc.volume_geometry(b, voxel)
        vol = oc.RefVolume(dim, origin, voxel, fu, fd)
        for pts, rem, lab in clouds:
            rng, remi, labi, _ = oc.project(pts, rem, lab, H, W, fu, fd)
            vol.integrate(labi, rng, remi)
        dc._check_volumes(dd.vol.get_volume_tensors(), dict(fields=[t.cpu() for t in vol.fields]), "table")   # fusion: untouched
        want = _finish(vol, tgt, _table_rays_dev(tgt, bc.VLP32C, P), P, T)
        ties = {}
        _check_scan(got, want, f"mesh/table/{mounted}", ties)
        with DeviceDeform(src, tgt, bnds.copy(), voxel, transformation=T) as plain:      # evenly spaced rows: another scan
            base = plain.mesh(tm._dev(clouds))
            torch.cuda.synchronize()
            assert not np.array_equal(base["range"].cpu().numpy(), got["range"].cpu().numpy())
    print(f"\nmesh with a table target (mounted: {mounted}) vs the composed oracle chain: (exact-t tie pixels, in-plane pixels) {ties}")


def _seq_setup(adaption="mergemesh"):
    g17, g18 = cpu.gold(), sc.gold18()
    return g17, g18, sc.approach_for(g18, adaption)


def _target_model():
    from lidar_transfer_amd.config import load_sensor
    tH, tW, tfu, tfd = SEQ_TARGET
    return load_sensor(dict(name="VLP-32C table", fov_up=tfu, fov_down=tfd, beams=tH, angle_res_hor=360.0 / tW, fov_hor=360.0,
                            beam_model="table", beam_angles=[float(x) for x in bc.VLP32C]))


_SEQ_ORACLE = dict(outs=[], bnds=None)


def _oracle_sequence(n):
    """the composed chain over the first ``n`` output scans of the F17 sequence on ONE bounds array, rendered with the table
    rays (cached: the sequence test compares its files with the same scans)"""
    import oracle_chain as oc
    from lidar_transfer_amd.ingest import relative_indices
    g17, g18, a = _seq_setup()
    st = _SEQ_ORACLE
    if st["bnds"] is None:
        st["bnds"] = a.voxel_bounds.copy()
        st["rays"] = _table_rays_dev(SEQ_TARGET, bc.VLP32C)
    raw, poses = cpu.raw_scans(g17), [np.array(p, np.float64) for p in g17["poses"]]
    H, W = ev.SOURCE[0], ev.SOURCE[1]
    tfu, tfd = SEQ_TARGET[2], SEQ_TARGET[3]
    indices = [int(x) for x in a.scan_indices(len(raw))]
    while len(st["outs"]) < n:
        idx = indices[len(st["outs"])]
        slots = [idx + r for r in relative_indices(a.number_of_scans)]
        pts, rem, lab = cpu.restate(raw, poses, slots, np.linalg.inv(poses[idx]), a.ignore, a.moving, merged=True)[0]
        rng, remi, labi, kept = oc.project(pts, rem, lab.astype(np.int64), H, W, tfu, tfd)
        dim, origin, given = oc.mergemesh_bounds(st["bnds"], kept, a.voxel_size)
        vol = oc.RefVolume(dim, origin, a.voxel_size, tfu, tfd)
        vol.integrate(labi, rng, remi)
        w = _finish(vol, SEQ_TARGET, st["rays"])
        w.update(idx=idx, vol_dim=tuple(int(x) for x in dim), bnds_after=st["bnds"].copy())
        st["outs"].append(w)
    return st["outs"][:n]


@pytest.mark.parametrize("source_images", [False, True])
def test_mergemesh_sequence_with_a_table_target_equals_the_composed_oracle_chain(source_images):
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    tm._need_reference_builds()
    g17, g18, a = _seq_setup()
    want = _oracle_sequence(3)
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    b = a.voxel_bounds.copy()
    ties = {}
    with DeviceDeform(ev.SOURCE, SEQ_TARGET, b, a.voxel_size, mesh_volume=False, t_beam_table=bc.VLP32C) as dd:
        for w in want:
            got = dd.deform("mergemesh", ing, w["idx"], source_images=source_images)
            torch.cuda.synchronize()
            tag = f"mm{w['idx']}/{source_images}"
            assert got["vol_dim"] == w["vol_dim"], tag
            assert np.array_equal(np.array(got["vol_bnds_after"]).reshape(3, 2), w["bnds_after"].astype(np.float64)), tag
            _check_scan(got, w, tag, ties)
    src.close()
    print(f"\nmergemesh with a table target vs the composed oracle chain: (exact-t tie pixels, in-plane pixels) {ties}")


@pytest.mark.parametrize("preserve_float", [False, True])
def test_cp_with_a_table_target_writes_the_restatements_bytes(preserve_float):
    """the restated ingest, the literal loop with the row and keep rule, the restated reverse projection and write()"""
    import oracle_chain as oc
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest, relative_indices
    g17, g18, a = _seq_setup("cp")
    raw, poses = cpu.raw_scans(g17), [np.array(p, np.float64) for p in g17["poses"]]
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    tH, tW, tfu, tfd = SEQ_TARGET
    with DeviceDeform(ev.SOURCE, SEQ_TARGET, None, preserve_float=preserve_float, t_beam_table=bc.VLP32C) as dd, \
            DeviceDeform(ev.SOURCE, SEQ_TARGET, None, preserve_float=preserve_float) as plain:
        for idx in a.scan_indices(len(raw))[:2]:
            got = dd.deform("cp", ing, idx)
            base = plain.deform("cp", ing, idx)
            torch.cuda.synchronize()
            slots = [idx + r for r in relative_indices(a.number_of_scans)]
            pts, rem, lab = cpu.restate(raw, poses, slots, np.linalg.inv(poses[idx]), a.ignore, a.moving, merged=True)[0]
            p = bc.project(pts, rem, lab.astype(np.int64), bc.VLP32C, bc.VLP32C_FOV, tW)
            assert not (p["near"] & p["kept"]).any(), "a point of the sequence lies on a row boundary: choose another scan"
            px, py = (p["proj_xf"], p["proj_yf"]) if preserve_float else (p["proj_x"], p["proj_y"])
            back = bc.reverse_projection(p["range"], px, py, bc.VLP32C, preserve_float)
            wb, wl = oc.pack_write(back, p["label"], p["rem"], index=p["idx"])
            assert wb.shape[0] > 100
            assert np.array_equal(got["index"].cpu().numpy(), p["idx"]), idx
            assert np.array_equal(got["label_file"].cpu().numpy().view(np.uint32), wl), f"cp {idx}: label bytes"
            gb = got["bin"].cpu().numpy()
            # float32(x) of two float64 math libraries: bytes equal but where the float64 sits on a float32 rounding boundary
            diff = int((gb.view(np.uint32) != wb.view(np.uint32)).sum())
            print(f"\ncp with a table target, scan {idx}, preserve_float={preserve_float}: {wb.shape[0]} points, {diff} of {wb.size} words differ")
            assert np.array_equal(gb.view(np.uint8), wb.view(np.uint8)), f"cp {idx}: velodyne bytes"
            assert gb.tobytes() != base["bin"].cpu().numpy().tobytes()
    src.close()


def _run_sequence(a, target, out_dir, chains, **kw):
    from lidar_transfer_amd.sequence import SequenceTransfer
    g17, g18 = cpu.gold(), sc.gold18()
    src = tm._source(g17)
    with SequenceTransfer(src, a, ev.SOURCE, target, out_dir=str(out_dir), chains=chains, nclasses=int(g18["nclasses"]), **kw) as tr:
        recs = list(tr.run())
        info = dict(beam_model=tr.beam_model, evaluate=tr.evaluate, summary=tr.summary)
    src.close()
    return recs, info


def test_sequence_with_a_table_target_writes_the_oracles_files(tmp_path):
    from lidar_transfer_amd.sequence import SequenceTransfer
    tm._need_reference_builds()
    g17, g18, a = _seq_setup()
    model = _target_model()
    assert ev.SOURCE[:2] == SEQ_TARGET[:2]                      # (with evenly spaced rows this run would compare)
    r1, i1 = _run_sequence(a, model, tmp_path / "c1", 1)
    assert i1["beam_model"] == "table" and i1["evaluate"] is False and i1["summary"]["beam_model"] == "table"
    r3, i3 = _run_sequence(a, model, tmp_path / "c3", 3)
    assert i3["summary"]["chains"] == 3
    r0, i0 = _run_sequence(a, SEQ_TARGET, tmp_path / "lin", 1)
    assert i0["beam_model"] == "linear" and i0["evaluate"] is True and all(r["m_iou"] is not None for r in r0)
    indices = [r["idx"] for r in r1]
    assert indices == [int(x) for x in a.scan_indices(8)] == [r["idx"] for r in r3] and len(indices) >= 3
    want = _oracle_sequence(len(indices))
    for rec, rec3, w in zip(r1, r3, want):
        idx = rec["idx"]
        for r in (rec, rec3):
            assert r["m_iou"] is None and r["MSE"] is None and not r["skipped"]
            assert np.array_equal(r["bnds_after"], w["bnds_after"].astype(np.float64)), idx
        if "bin" not in w:                                      # (scans the DeviceDeform test did not visit)
            import oracle_chain as oc
            sel = tm._rule_images(w)
            w["bin"], w["label_file"] = oc.pack_write(sel["endpoints"], sel["label"], sel["endrem"])
        b1, l1 = tm._read(tmp_path / "c1", idx)
        assert b1 == w["bin"].tobytes(), f"scan {idx}: velodyne file"
        assert l1 == w["label_file"].astype(np.uint32).tobytes(), f"scan {idx}: label file"
        assert (b1, l1) == tm._read(tmp_path / "c3", idx), f"scan {idx}: one chain vs three"
        assert tm._read(tmp_path / "lin", idx)[0] != b1, f"scan {idx}: the table changed nothing"
    for kw, sensors in ((dict(evaluate=True), (ev.SOURCE, model)), ({}, (model, SEQ_TARGET))):    # compare; a SOURCE with a table
        src = tm._source(g17)
        try:
            with pytest.raises(ValueError):
                SequenceTransfer(src, a, sensors[0], sensors[1], **kw)
        finally:
            src.close()


def test_cli_on_the_shipped_table_file_prints_no_metrics_and_logs_the_beam_model(tmp_path):
    import json
    import subprocess
    g17, g18, a = _seq_setup()
    data = tmp_path / "data"
    seq = data / "sequences" / "00"
    (seq / "velodyne").mkdir(parents=True)
    (seq / "labels").mkdir()
    for k, (xyzr, lab) in enumerate(cpu.raw_scans(g17)):
        xyzr.tofile(seq / "velodyne" / f"{k:06d}.bin")
        lab.tofile(seq / "labels" / f"{k:06d}.label")
    g17["calib_txt"].tofile(seq / "calib.txt")
    g17["poses_txt"].tofile(seq / "poses.txt")
    H, W, fu, fd = 32, 1024, 3.0, -25.0                         # the size of the shipped target: a linear one would compare
    (data / "config.yaml").write_text(f"name: src\nfov_up: {fu}\nfov_down: {fd}\nbeams: {H}\nangle_res_hor: {360.0 / W!r}\nfov_hor: 360.0\n")
    cm = "\n".join(f"  {k}: {list(v)}" for k, v in ev.COLOR_DICT.items())
    cfg = tmp_path / "approach.yaml"
    cfg.write_text(f"adaption: mergemesh\npreserve_float: false\nnumber_of_scans: {a.number_of_scans}\n"
                   f"batch_interval: {a.batch_interval}\nvoxel_size: {a.voxel_size!r}\n"
                   f"voxel_bounds: {[float(x) for x in np.asarray(a.voxel_bounds).reshape(-1)]}\n"
                   f"transformation: []\nignore: {a.ignore}\nmoving: {a.moving}\ncolor_map:\n{cm}\n")
    linear = tmp_path / "linear.yaml"
    linear.write_text("name: lin\nfov_up: 15.0\nfov_down: -25.0\nbeams: 32\nangle_res_hor: 0.3515625\nfov_hor: 360\n")
    outs = {}
    for name, target, more in (("table", os.path.join(ROOT, "config", "vlp32c_table_1024.yaml"), []),
                               ("linear", str(linear), ["--one_scan"])):
        out = tmp_path / f"out_{name}"
        out.mkdir()
        log = tmp_path / f"{name}.jsonl"
        res = subprocess.run([sys.executable, "-m", "lidar_transfer_amd", "-d", str(data), "-c", str(cfg), "-s", "00", "-t", target,
                              "-w", "-p", str(out), "--log", str(log)] + more, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-3000:]
        rows = [json.loads(x) for x in log.read_text().splitlines()]
        outs[name] = (res.stdout, rows, tm._read(out, rows[0]["idx"]))
    so, rows, files = outs["table"]
    assert "IoU:" not in so and "Acc:" not in so and "MSE:" not in so
    assert len(rows) >= 3 and all(r["beam_model"] == "table" and r["m_iou"] is None for r in rows[:-1])
    assert rows[-1]["summary"]["beam_model"] == "table"
    so, rows, files0 = outs["linear"]
    assert "IoU:" in so and all("beam_model" not in r for r in rows[:-1]) and rows[-1]["summary"]["beam_model"] == "linear"
    assert files[0] != files0[0] and len(files[0]) > 1600


# ---- nothing changes without it ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adaption", ["cp", "mesh", "mergemesh"])
def test_a_linear_target_and_a_target_without_the_key_change_nothing(adaption):
    import torch
    from lidar_transfer_amd.config import load_sensor
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    g17, g18, a = _seq_setup(adaption)
    t = g18["target_t"]
    target = (int(t[0]), int(t[1]), float(t[2]), float(t[3]))
    cfg = dict(name="t", fov_up=target[2], fov_down=target[3], beams=target[0], angle_res_hor=360.0 / target[1], fov_hor=360.0)
    models = [load_sensor(dict(cfg)), load_sensor(dict(cfg, beam_model="linear"))]
    assert all((m.H, m.W) == target[:2] and m.beam_table() is None for m in models)
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    res = []
    for kw in ({}, dict(t_beam_table=models[0].beam_table()), dict(t_beam_table=models[1].beam_table())):
        bnds = None if adaption == "cp" else a.voxel_bounds.copy()
        with DeviceDeform(ev.SOURCE, target, bnds, a.voxel_size, mesh_volume=adaption == "mesh", **kw) as dd:
            assert dd.t_beam_table is None and (dd.rayset is None or dd.rayset.beam_table is None)
            outs = []
            for idx in a.scan_indices(8)[:2]:
                out = dd.deform(adaption, ing, idx)
                torch.cuda.synchronize()
                outs.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
            res.append(outs)
    for other in res[1:]:
        for x, y in zip(res[0], other):
            tm._same(x, y, adaption)
    assert res[0][0]["bin"].shape[0] > 100
    src.close()


def test_a_shared_rayset_must_have_been_built_for_the_same_table():
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.raytracer import RaySet
    src, tgt = (16, 64, 3.0, -25.0), (32, 64, 15.0, -25.0)
    bnds = np.array([[-4.0, 4.0], [-4.0, 4.0], [-2.0, 2.0]])
    other_table = bc.VLP32C.copy()
    other_table[5] += 0.01
    mk = lambda t: RaySet(create_rays_device(tgt[2], tgt[3], tgt[0], tgt[1], beam_table=t), tgt[0], beam_table=t)   # noqa: E731
    plain, table, other = mk(None), mk(bc.VLP32C), mk(other_table)
    for rs, t, ok in ((plain, None, True), (plain, bc.VLP32C, False), (table, bc.VLP32C, True), (table, None, False),
                      (other, bc.VLP32C, False), (table, list(bc.VLP32C), True)):
        if ok:
            DeviceDeform(src, tgt, bnds.copy(), 0.25, mesh_volume=False, rayset=rs, t_beam_table=t).close()
        else:
            with pytest.raises(ValueError, match="beam table"):
                DeviceDeform(src, tgt, bnds.copy(), 0.25, mesh_volume=False, rayset=rs, t_beam_table=t)
    for bad in (bc.VLP32C[:-1], bc.VLP32C[::-1], np.where(np.arange(32) == 0, 16.0, bc.VLP32C)):    # count, order, outside the fov
        with pytest.raises(ValueError):
            DeviceDeform(src, tgt, None, t_beam_table=bad)
    for rs in (plain, table, other):
        rs.close()
