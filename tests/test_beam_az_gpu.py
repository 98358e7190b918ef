"""Per-beam azimuth offsets of a table target (``beam_azimuth_offsets``), on the device: its rays against the
float64 restatement; a render of an offset ray set by the scatter and by the LBVH against the brute-force oracle; the column
rule of ``LT_PROJ_BEAM_AZIMUTH`` against the literal sequential loop, on the full circle and in a sector; the reverse
projection; the round trip of a sector's rays; ``DeviceDeform`` / ``SequenceTransfer`` / the CLI with an offset target against
a chain composed here from the independent pieces of tests/oracle_chain.py on the product's downloaded rays; and the guard
that a table target without offsets takes exactly the path it took.  Restatements: tests/beam_az_cases.py; the conditions on
the inputs: tests/test_beam_az_cpu.py."""
import ctypes as C
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
import test_beam_az_cpu as azc  # noqa: E402
import test_beam_table_gpu as btg  # noqa: E402
import test_evaluate_cpu as ev  # noqa: E402
import test_ingest_cpu as cpu  # noqa: E402
import test_mount_gpu as tm  # noqa: E402
import test_sector_cpu as stc  # noqa: E402
import test_sector_gpu as tsg  # noqa: E402
import test_sequence_cpu as sq  # noqa: E402

pytestmark = pytest.mark.gpu
LT_ERR_INVALID_ARG = -1
T_EXAMPLE = tm.T_EXAMPLE
#: the F17 sequence's target of these tests: the VLP-32C table on 32 x 171 with the mixed offsets
SEQ_TARGET = (32, 171, bc.VLP32C_FOV[0], bc.VLP32C_FOV[1])
SEQ_AZ = ac.offsets("mixed", 32)
_bits, _differs, _up = btg._bits, btg._differs, btg._up
dp = C.POINTER(C.c_double)


def _dptr(a):
    return a.ctypes.data_as(dp)


# ---- 1: rays --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(azc.RAY_CASES)))
def test_device_rays_with_offsets_equal_the_restatement(case):
    from lidar_transfer_amd.laserscan import create_rays_device
    name, si, kind, sector, P = azc.RAY_CASES[case]
    _, table, fov, W = ac.SENSORS[si]
    H = len(table)
    rot = None if P is None else P[:3, :3]
    for az in (ac.offsets(kind, H),):                             # (tests/test_beam_az_cpu.py holds the input condition for it)
        dev = create_rays_device(fov[0], fov[1], H, W, rot=rot, beam_table=table, sector=sector, beam_azimuth=az).cpu().numpy()
        assert dev.shape == (H * W, 3) and dev.dtype == np.float32
        n = tm._rays_rule(dev, ac.az_rays(table, az, W, sector, rot), name)
        print(f"\n{name}: {n} of {dev.size} elements not bit-equal to the restatement")
        assert np.abs(np.linalg.norm(dev.astype(np.float64), axis=1) - 1).max() < 1e-6
        plain = create_rays_device(fov[0], fov[1], H, W, rot=rot, beam_table=table, sector=sector).cpu().numpy()
        zero = az == 0.0
        a, b = dev.reshape(H, W, 3), plain.reshape(H, W, 3)
        assert np.array_equal(_bits(a[zero]), _bits(b[zero])), name        # a row without an offset: the table's own bits
        assert zero.all() or not np.array_equal(a[~zero], b[~zero]), name
    with pytest.raises(ValueError):
        create_rays_device(fov[0], fov[1], H, W, beam_azimuth=ac.offsets("mixed", H))          # offsets without a table
    with pytest.raises(ValueError):
        create_rays_device(fov[0], fov[1], H, W, beam_table=table, beam_azimuth=np.full(H, 90.5))


def test_the_ray_entry_point_checks_its_arguments():
    import torch
    from lidar_transfer_amd import _lib
    lib = _lib.load()
    H, W = 32, 8
    out = torch.empty((H * W, 3), dtype=torch.float32, device="cuda")
    b, az = np.ascontiguousarray(bc.VLP32C), ac.offsets("mixed", H)
    sec = np.array([170.0, 100.0])
    good = [_dptr(b), _dptr(az), H, W, _dptr(sec), None, out.data_ptr(), None]
    assert lib.lt_create_rays_beams_az_dev(*good) == 0, lib.lt_last_error()
    nan = az.copy()
    nan[3] = np.nan
    for k, v in ((0, None), (2, 0), (3, 0), (6, None), (1, _dptr(np.full(H, 91.0))), (1, _dptr(nan)),
                 (4, _dptr(np.array([0.0, 360.0]))), (4, _dptr(np.array([400.0, 90.0])))):
        bad = list(good)
        bad[k] = v
        assert lib.lt_create_rays_beams_az_dev(*bad) == LT_ERR_INVALID_ARG, k
    torch.cuda.synchronize()


# ---- 2: render ------------------------------------------------------------------------------------------------------------------
def test_render_of_offset_rays_equals_brute_force():
    """the scatter (on the image's own bin grid) and the LBVH on tests/test_sector_cpu.py's scene; the measured ``dev_az`` of
    the sheared rows is printed (profiles/beam_azimuth/README.md records it at deployment size)"""
    import oracle_chain as oc
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.synth import synth_scene
    from oracle import binding as ob
    _, table, fov, W = ac.SENSORS[2]
    H = len(table)
    az = ac.offsets("mixed", H)
    mesh = synth_scene(stc.RENDER_SEED, stc.RENDER_TRIS)
    trays = create_rays_device(fov[0], fov[1], H, W, beam_table=table, beam_azimuth=az)
    rays = trays.cpu().numpy()
    tm._rays_rule(rays, ac.az_rays(table, az, W), "render rays")
    org = np.zeros(3, np.float32)
    sca, lbvh, prm, st = tsg._render(mesh, trays, (0.0, 0.0, 0.0), H, None, lbvh=True)
    plain = create_rays_device(fov[0], fov[1], H, W, beam_table=table)
    _, _, prm0, st0 = tsg._render(mesh, plain, (0.0, 0.0, 0.0), H, None)
    brute = ob.oracle_trace(rays, org, *mesh, H, mode=ob.MODE_BRUTE, norm=ob.NORM_SSE_TABLE, nthreads=oc.THREADS)
    for tag, got in (("scatter", sca), ("lbvh", lbvh)):
        tsg._assert_brute(got, brute, H * W, f"offset rays: {tag}")
    assert int((brute["tri"] >= 0).sum()) > 0.3 * H * W
    print(f"\n32 x 171 with offsets: nb_az {prm['nb_az']} dev_az {prm['dev_az']:.4f}, candidate bins {st['nodes_visited']}, triangle "
          f"tests {st['tris_tested']} ({st['tris_tested'] / (H * W):.1f} per ray); the plain table: nb_az {prm0['nb_az']} dev_az "
          f"{prm0['dev_az']:.4f}, candidate bins {st0['nodes_visited']}, triangle tests {st0['tris_tested']} "
          f"({st0['tris_tested'] / (H * W):.1f} per ray)")


# ---- 3: projection --------------------------------------------------------------------------------------------------------------
OUTS = tsg.PROJ_KEYS + ("proj_xf", "n_kept")


@pytest.mark.parametrize("sector", [None, ac.SEAM_SECTOR])
@pytest.mark.parametrize("si", range(len(ac.SENSORS)))
def test_projected_columns_with_offsets_equal_the_literal_loop(si, sector):
    """tests/test_sector_gpu.py's rule: bit for bit outside the cells a near-boundary point may touch, ``proj_xf`` within 4 ulp
    of the slack.  The clouds from 65 points on hold a point its row's offset carries across the +-pi seam (full circle), or
    one inside the sector by its own row's offset and outside by its neighbour's (tests/test_beam_az_cpu.py)."""
    import torch
    from lidar_transfer_amd.laserscan import Projector
    name, table, fov, W = ac.SENSORS[si]
    H = len(table)
    pj = Projector()
    for kind in ("mixed", "ninety"):
        az = ac.offsets(kind, H)
        for n, dtype in ac.CLOUDS:
            pts, rem, lab, special = ac.seeded_cloud(table, fov, az, n, dtype, ac.cloud_seed(si, n, sector), sector)
            want = ac.project(pts, rem, lab, table, fov, az, W, sector)
            got = pj.project([_up((pts, rem, lab))], fov[0], fov[1], H, W, new=True, remove=True, outputs=OUTS, beam_table=table,
                             sector=sector, beam_azimuth=az)[0]
            torch.cuda.synchronize()
            tsg._check_projection(got, want, W, n, f"{name} {kind} sector={sector} {np.dtype(dtype).name} n={n}")
            for i, r in special.values():                         # the chosen point is in the image where the restatement put it
                assert want["kept"][i] and int(got["idx"].cpu().numpy()[r, want["col"][i]]) >= 0
            if n == 20000 and H == 32:                            # the offsets moved points: another image than the table's
                base = pj.project([_up((pts, rem, lab))], fov[0], fov[1], H, W, new=True, remove=True, outputs=OUTS,
                                  beam_table=table, sector=sector)[0]
                torch.cuda.synchronize()
                assert not np.array_equal(base["range"].cpu().numpy(), got["range"].cpu().numpy())
    # two clouds in one batch on a side stream
    az = ac.offsets("ninety", H)
    c1 = ac.seeded_cloud(table, fov, az, *ac.BATCH_CLOUD, sector)[:3]
    c2 = ac.seeded_cloud(table, fov, az, 20000, np.float32, ac.cloud_seed(si, 20000, sector), sector)[:3]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d1, d2 = _up(c1), _up(c2)
        got = pj.project([d1, d2], fov[0], fov[1], H, W, new=True, remove=True, outputs=OUTS, beam_table=table, sector=sector,
                         beam_azimuth=az, stream=st)
    st.synchronize()
    for g, cl, tag in ((got[0], c1, "batch/0"), (got[1], c2, "batch/1")):
        tsg._check_projection(g, ac.project(*cl, table, fov, az, W, sector), W, len(cl[0]), tag)   # (asserts the cap as well)
    pj.close()


def test_the_single_cloud_entry_points_take_the_azimuth_flag_too():
    from lidar_transfer_amd import _lib
    from lidar_transfer_amd.config import beam_azimuth_radians, beam_rows, sector_radians
    lib = _lib.load()
    _, table, fov, W = ac.SENSORS[2]
    H = len(table)
    az = ac.offsets("ninety", H)
    az_rad = beam_azimuth_radians(az)
    tab = np.ascontiguousarray(np.concatenate(list(beam_rows(table))))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    A, S, B, N, R = _lib.LT_PROJ_BEAM_AZIMUTH, _lib.LT_PROJ_SECTOR, _lib.LT_PROJ_BEAM_ROWS, _lib.LT_PROJ_NEW, _lib.LT_PROJ_REMOVE
    try:
        for sector in (None, ac.SEAM_SECTOR):
            pts, rem, lab, _ = ac.seeded_cloud(table, fov, az, 5000, np.float64, 9, sector)
            want = ac.project(pts, rem, lab, table, fov, az, W, sector)
            n = len(pts)
            o = dict(px=np.empty(n, np.int32), idx=np.empty((H, W), np.int32), range=np.empty((H, W), np.float32))
            kept = C.c_int(0)
            args = lambda fl, nbm, t: [vp(pts), 1, vp(rem), vp(lab.view(np.uint32)), n, fov[0], fov[1], H, W, t, nbm, fl, None, 0,   # noqa: E731
                                       None, None, None, None, vp(o["px"]), None, None, None, vp(o["idx"]), vp(o["range"]), None,
                                       None, None, None, None, 0.0, -1.0, 0.0, C.byref(kept)]
            flags = A | B | N | R | (S if sector is not None else 0)
            if sector is not None:
                assert lib.lt_range_projection_set_sector(*sector_radians(sector)) == 0
            assert lib.lt_range_projection_set_beam_azimuth(None, 0) == 0
            assert lib.lt_range_projection(*args(flags, H, vp(tab))) == LT_ERR_INVALID_ARG       # no offsets set
            assert b"LT_PROJ_BEAM_AZIMUTH" in lib.lt_last_error()
            for bad in (np.full(H, 2.0), np.r_[az_rad[:-1], np.nan], np.r_[az_rad[:-1], np.inf]):
                assert lib.lt_range_projection_set_beam_azimuth(_dptr(bad), H) == LT_ERR_INVALID_ARG
            assert lib.lt_range_projection_set_beam_azimuth(_dptr(az_rad), 512) == LT_ERR_INVALID_ARG
            assert lib.lt_range_projection_set_beam_azimuth(_dptr(az_rad), H - 1) == 0
            assert lib.lt_range_projection(*args(flags, H, vp(tab))) == LT_ERR_INVALID_ARG       # offsets for another H
            assert lib.lt_range_projection_set_beam_azimuth(_dptr(az_rad), H) == 0
            assert lib.lt_range_projection(*args(flags, H, vp(tab))) == 0, lib.lt_last_error()
            k = kept.value
            skip = tsg.sc.near_cells(want, W)
            n_near = int(want["near"].sum())
            assert abs(k - int(want["kept"].sum())) <= n_near and k > 300
            assert not _differs(o["range"], want["range"])[~skip].any()
            assert np.array_equal(o["idx"][~skip] >= 0, want["idx"][~skip] >= 0) and ((want["idx"] >= 0) & ~skip).sum() > 200
            if k == int(want["kept"].sum()):
                sure = ~want["near"][want["kept"]]
                assert np.array_equal(o["px"][:k][sure], want["col"][want["kept"]][sure])
            # the device entry point itself: the same images, the same refusals at its own boundary
            import torch
            dpts, drem, dlab = _up((pts, rem, lab))
            dr, di = torch.empty((H, W), dtype=torch.float32, device="cuda"), torch.empty((H, W), dtype=torch.int32, device="cuda")
            dargs = lambda fl, nbm, t: [dpts.data_ptr(), 1, drem.data_ptr(), dlab.data_ptr(), n, fov[0], fov[1], H, W, t, nbm, fl, None,   # noqa: E731
                                        0, None, None, None, None, None, None, None, None, di.data_ptr(), dr.data_ptr(), None, None,
                                        None, None, None, 0.0, -1.0, 0.0, C.byref(kept), None]
            assert lib.lt_range_projection_dev(*dargs(flags, H, vp(tab))) == 0, lib.lt_last_error()
            assert kept.value == k and np.array_equal(_bits(dr.cpu().numpy()), _bits(o["range"]))
            assert np.array_equal(di.cpu().numpy(), o["idx"])
            for fl, nb, t in ((A, 0, None), (A | N | R, 0, None), (A | B, H, vp(tab)), (A | B | N, H, vp(tab)), (A | B | R, H, vp(tab)),
                              (flags | 32, H, vp(tab)), (flags, H - 1, vp(tab))):
                assert lib.lt_range_projection(*args(fl, nb, t)) == LT_ERR_INVALID_ARG, fl
                assert b"LT_PROJ_" in lib.lt_last_error()
                assert lib.lt_range_projection_dev(*dargs(fl, nb, t)) == LT_ERR_INVALID_ARG, fl
                assert b"LT_PROJ_" in lib.lt_last_error()
            assert lib.lt_range_projection(*args(flags & ~A, H, vp(tab))) == 0               # and without the flag: the table's own path
    finally:
        assert lib.lt_range_projection_set_beam_azimuth(None, 0) == 0
        assert lib.lt_range_projection_set_sector(0.0, 0.0) == 0


def test_any_other_flag_combination_with_the_azimuth_flag_is_refused():
    import torch
    from lidar_transfer_amd import _lib
    from lidar_transfer_amd.config import beam_azimuth_radians, beam_rows, sector_radians
    from lidar_transfer_amd.laserscan import Projector
    lib = _lib.load()
    _, table, fov, W = ac.SENSORS[2]
    H = len(table)
    az_rad = beam_azimuth_radians(ac.offsets("mixed", H))
    cloud = _up(ac.seeded_cloud(table, fov, ac.offsets("mixed", H), 257, np.float32, 1)[:3])
    pj = Projector()
    for new, remove in ((False, False), (True, False), (False, True)):
        with pytest.raises(RuntimeError, match="LT_PROJ_"):
            pj.project([cloud], fov[0], fov[1], H, W, new=new, remove=remove, beam_table=table, beam_azimuth=ac.offsets("mixed", H))
    with pytest.raises(ValueError):
        pj.project([cloud], fov[0], fov[1], H, W, new=True, remove=True, beam_azimuth=ac.offsets("mixed", H))     # no table
    tab = np.ascontiguousarray(np.concatenate(list(beam_rows(table))))
    cl, im = (_lib.Cloud * 1)(), (_lib.ProjImages * 1)()
    rng = torch.empty((H, W), dtype=torch.float32, device="cuda")
    cl[0].points, cl[0].rem, cl[0].label, cl[0].n = cloud[0].data_ptr(), cloud[1].data_ptr(), cloud[2].data_ptr(), 257
    im[0].range = rng.data_ptr()
    A, S, B, N, R = _lib.LT_PROJ_BEAM_AZIMUTH, _lib.LT_PROJ_SECTOR, _lib.LT_PROJ_BEAM_ROWS, _lib.LT_PROJ_NEW, _lib.LT_PROJ_REMOVE
    vt = tab.ctypes.data_as(C.c_void_p)
    call = lambda p, fl, nb, t: lib.lt_range_projection_batch_dev(p._h, 1, cl, 0, fov[0], fov[1], H, W, t, nb, fl, None, 0, im,   # noqa: E731
                                                                  0.0, -1.0, 0.0, None)
    fresh = Projector()                                            # no offsets were ever set on this one
    assert call(fresh, A | B | N | R, H, vt) == LT_ERR_INVALID_ARG and b"LT_PROJ_BEAM_AZIMUTH" in lib.lt_last_error()
    assert call(fresh, B | N | R, H, vt) == 0
    fresh.close()
    for bad, n in ((np.full(H, 1.6), H), (np.r_[az_rad[:-1], np.nan], H), (az_rad, 512), (az_rad, -1)):
        assert lib.lt_projector_set_beam_azimuth(pj._h, _dptr(np.ascontiguousarray(bad)), n) == LT_ERR_INVALID_ARG, n
    assert lib.lt_projector_set_beam_azimuth(None, _dptr(az_rad), H) == LT_ERR_INVALID_ARG
    assert lib.lt_projector_set_beam_azimuth(pj._h, _dptr(az_rad), H) == 0
    for fl, nb, t in ((A, 0, None), (A | N | R, 0, None), (A | S | N | R, 0, None), (A | B, H, vt), (A | B | N, H, vt), (A | B | R, H, vt),
                      (A | B | N | R | 32, H, vt), (A | B | N | R, H - 1, vt), (A | B | N | R, H, None),
                      (A | B | S | N | R, H, vt)):                  # (the last: no sector was set)
        assert call(pj, fl, nb, t) == LT_ERR_INVALID_ARG, (fl, nb)
    assert call(pj, A | B | N | R, H, vt) == 0
    assert lib.lt_projector_set_sector(pj._h, *sector_radians(ac.SEAM_SECTOR)) == 0
    assert call(pj, A | B | S | N | R, H, vt) == 0
    assert lib.lt_projector_set_beam_azimuth(pj._h, _dptr(az_rad), H - 1) == 0                  # offsets for another H
    assert call(pj, A | B | N | R, H, vt) == LT_ERR_INVALID_ARG
    assert lib.lt_projector_set_beam_azimuth(pj._h, None, 0) == 0                               # cleared: refused again
    assert call(pj, A | B | N | R, H, vt) == LT_ERR_INVALID_ARG
    assert call(pj, B | N | R, H, vt) == 0 and call(pj, B | S | N | R, H, vt) == 0 and call(pj, N | R, 0, None) == 0   # what there was
    torch.cuda.synchronize()
    pj.close()


# ---- 4: reverse projection ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sector", [None, ac.SEAM_SECTOR])
@pytest.mark.parametrize("preserve_float", [False, True])
@pytest.mark.parametrize("shape", [(1, 1), (32, 200)])
def test_reverse_projection_with_offsets_equals_the_float64_restatement(shape, preserve_float, sector):
    """rtol = atol = 1e-13 is tests/test_post_shapes_gpu.py's bound for this kernel (two float64 math libraries): kept from
    there, not derived.  int32 rows outside the table read their nearest end, for the offset as for the angle."""
    import torch
    from lidar_transfer_amd import _lib
    from lidar_transfer_amd.config import beam_azimuth_radians, sector_radians
    lib = _lib.load()
    H, W = shape
    table = np.array([-3.0]) if H == 1 else bc.VLP32C
    Brad = bc.rows_of(table)[0]
    rng = np.random.default_rng(H * W + 11)
    r = rng.uniform(0.5, 80.0, (H, W)).astype(np.float32)
    r[rng.random((H, W)) < 0.2] = 0.0
    if preserve_float:
        px = rng.uniform(0, W, (H, W))
        py = rng.uniform(Brad.min() - 0.05, Brad.max() + 0.05, (H, W))
    else:
        px = rng.integers(0, W, (H, W)).astype(np.int32)
        py = rng.integers(0, H, (H, W)).astype(np.int32)
        if H > 1:
            py[0, :4] = [-1, H, -7, H + 40]                        # outside the table: clamped, never read beside it
    sec = None if sector is None else np.array(sector_radians(sector), np.float64)
    for kind in ("mixed", "ninety"):
        az = ac.offsets(kind, H)
        want = ac.reverse_projection(r, px, py, table, az, preserve_float, sector)
        d = [torch.from_numpy(a).cuda() for a in (r, px, py, Brad, beam_azimuth_radians(az))]
        for stream in (None, torch.cuda.Stream()):
            out = torch.full((H * W + 1, 3), -7.0, dtype=torch.float64, device="cuda")
            st = torch.cuda.current_stream() if stream is None else stream
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream())
            rc = lib.lt_reverse_projection_beams_az_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), int(preserve_float),
                                                        d[3].data_ptr(), d[4].data_ptr(), _dptr(sec) if sec is not None else None,
                                                        H, W, out.data_ptr(), C.c_void_p(st.cuda_stream))
            assert rc == 0, lib.lt_last_error()
            st.synchronize()
            got = out.cpu().numpy()
            assert (got[-1] == -7.0).all()                          # the sentinel row: nothing past the last cell
            got = got[:-1]
            with np.errstate(all="ignore"):
                rel = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == want, 0.0, np.inf))
            print(f"\nreverse {H}x{W} {kind} sector={sector} preserve_float={preserve_float}: largest relative difference "
                  f"{rel.max():.1e}, largest absolute {np.abs(got - want).max():.1e}")
            assert np.allclose(got, want, rtol=1e-13, atol=1e-13)
        if H > 1:                                                  # the offsets moved the points
            base = bc.reverse_projection(r, px, np.clip(py, 0, H - 1) if not preserve_float else py, table, preserve_float) \
                if sector is None else None
            assert base is None or not np.allclose(base, want)
    good = [d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), int(preserve_float), d[3].data_ptr(), d[4].data_ptr(),
            _dptr(sec) if sec is not None else None, H, W, out.data_ptr(), None]
    cases = [(0, None), (1, None), (2, None), (5, None), (9, None), (7, 0), (8, 0), (6, _dptr(np.array([4.0, 1.0]))),
             (6, _dptr(np.array([0.0, 7.0])))]
    if not preserve_float:
        cases.append((4, None))
    for k, v in cases:
        b = list(good)
        b[k] = v
        assert lib.lt_reverse_projection_beams_az_dev(*b) == LT_ERR_INVALID_ARG, k
    torch.cuda.synchronize()


# ---- 5: round trip (sector only) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "ninety"])
@pytest.mark.parametrize("si", range(len(ac.SENSORS)))
def test_the_offset_rays_of_a_sector_come_back_from_the_round_trip(si, kind):
    """The rays x 17.3 m, projected with ``LT_PROJ_BEAM_AZIMUTH | LT_PROJ_SECTOR``, land each in its own cell; the int32
    reverse projection returns the points to 1e-4 m -- the bound and the reasoning of tests/test_sector_gpu.py's round trip: a
    float32 ray at 17.3 m is about 1e-6 m, with margin for the two trigonometric round trips.  (On the full circle the
    reference's left-edge quirk stays: no such claim there.)"""
    import torch
    from lidar_transfer_amd import _lib
    from lidar_transfer_amd.config import beam_azimuth_radians, sector_radians
    from lidar_transfer_amd.laserscan import Projector, create_rays_device
    lib = _lib.load()
    name, table, fov, W = ac.SENSORS[si]
    H = len(table)
    az, sector = ac.offsets(kind, H), ac.SEAM_SECTOR
    rays = create_rays_device(fov[0], fov[1], H, W, beam_table=table, sector=sector, beam_azimuth=az)
    pts = (rays.double() * 17.3).float().contiguous()
    pj = Projector()
    o = pj.project([(pts, None, None)], fov[0], fov[1], H, W, new=True, remove=True, outputs=("idx", "range", "proj_x", "proj_y"),
                   beam_table=table, sector=sector, beam_azimuth=az)[0]
    torch.cuda.synchronize()
    assert np.array_equal(o["idx"].cpu().numpy().reshape(-1), np.arange(H * W)), name          # every ray kept, in its own cell
    assert np.array_equal(o["proj_x"].cpu().numpy(), np.tile(np.arange(W), (H, 1)))
    assert np.array_equal(o["proj_y"].cpu().numpy(), np.repeat(np.arange(H), W).reshape(H, W))
    brad = torch.from_numpy(bc.rows_of(table)[0]).cuda()
    azd = torch.from_numpy(beam_azimuth_radians(az)).cuda()
    sec = np.array(sector_radians(sector), np.float64)
    back = torch.empty((H * W, 3), dtype=torch.float64, device="cuda")
    assert lib.lt_reverse_projection_beams_az_dev(o["range"].data_ptr(), o["proj_x"].data_ptr(), o["proj_y"].data_ptr(), 0,
                                                  brad.data_ptr(), azd.data_ptr(), _dptr(sec), H, W, back.data_ptr(), None) == 0
    torch.cuda.synchronize()
    off = float(np.abs(back.cpu().numpy() - pts.cpu().numpy().astype(np.float64)).max())
    print(f"\nround trip {name} {kind} in {sector}: largest coordinate difference {off:.2e} m over {H * W} rays")
    assert off <= 1e-4, off
    pj.close()


# ---- 6: chains ------------------------------------------------------------------------------------------------------------------
def _az_rays_dev(target, az, P=None):
    """the product's offset rays, downloaded, after they passed the rays' rule against the restatement"""
    from lidar_transfer_amd.laserscan import create_rays_device
    tH, tW, tfu, tfd = target
    rot = None if P is None else P[:3, :3]
    rays = create_rays_device(tfu, tfd, tH, tW, rot=rot, beam_table=bc.VLP32C, beam_azimuth=az).cpu().numpy()
    tm._rays_rule(rays, ac.az_rays(bc.VLP32C, az, tW, None, rot), "offset rays of the oracle chain")
    return rays


@pytest.mark.parametrize("mounted", [False, True])
def test_mesh_with_an_offset_target_equals_the_composed_oracle_chain(mounted):
    import oracle_chain as oc
    import pin_cases
    import test_default_chain_gpu as dc
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    tm._need_reference_builds()
    T = T_EXAMPLE if mounted else None
    P = tm._pose_of(T) if mounted else None
    _, src, _, n_scans, bnds, voxel, seeds = pin_cases.deform_mesh_case(0)
    tgt = SEQ_TARGET
    clouds = pin_cases.deform_mesh_clouds(seeds[0], n_scans, src, dc._host_render)
    with DeviceDeform(src, tgt, bnds.copy(), voxel, transformation=T, t_beam_table=bc.VLP32C, t_beam_azimuth=SEQ_AZ) as dd:
        assert np.array_equal(dd.rayset.beam_azimuth, SEQ_AZ) and np.array_equal(dd.rayset.beam_table, bc.VLP32C)
        got = dd.mesh(tm._dev(clouds))
        torch.cuda.synchronize()
        H, W, fu, fd = src
        b = np.array(bnds, copy=True)
        dim, origin = oc.volume_geometry(b, voxel)
        vol = oc.RefVolume(dim, origin, voxel, fu, fd)
        for pts, rem, lab in clouds:
            rng, remi, labi, _ = oc.project(pts, rem, lab, H, W, fu, fd)
            vol.integrate(labi, rng, remi)
        dc._check_volumes(dd.vol.get_volume_tensors(), dict(fields=[t.cpu() for t in vol.fields]), "offsets")   # fusion: untouched
        want = btg._finish(vol, tgt, _az_rays_dev(tgt, SEQ_AZ, P), P, T)
        ties = {}
        btg._check_scan(got, want, f"mesh/offsets/{mounted}", ties)
        with DeviceDeform(src, tgt, bnds.copy(), voxel, transformation=T, t_beam_table=bc.VLP32C) as plain:   # the table alone: another scan
            base = plain.mesh(tm._dev(clouds))
            torch.cuda.synchronize()
            assert not np.array_equal(base["range"].cpu().numpy(), got["range"].cpu().numpy())
    print(f"\nmesh with an offset target (mounted: {mounted}) vs the composed oracle chain: (exact-t tie pixels, in-plane pixels) {ties}")


def _target_model(**kw):
    from lidar_transfer_amd.config import load_sensor
    tH, tW, tfu, tfd = SEQ_TARGET
    cfg = dict(name="VLP-32C table with offsets", fov_up=tfu, fov_down=tfd, beams=tH, angle_res_hor=360.0 / tW, fov_hor=360.0,
               beam_model="table", beam_angles=[float(x) for x in bc.VLP32C], beam_azimuth_offsets=[float(x) for x in SEQ_AZ])
    cfg.update(kw)
    return load_sensor(cfg)


_SEQ_ORACLE = dict(outs=[], bnds=None)


def _oracle_sequence(n):
    """the composed chain over the first ``n`` output scans of the F17 sequence on ONE bounds array, rendered with the offset
    rays (cached: the sequence test compares its files with the same scans)"""
    import oracle_chain as oc
    from lidar_transfer_amd.ingest import relative_indices
    g17, g18, a = btg._seq_setup()
    st = _SEQ_ORACLE
    if st["bnds"] is None:
        st["bnds"] = a.voxel_bounds.copy()
        st["rays"] = _az_rays_dev(SEQ_TARGET, SEQ_AZ)
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
        w = btg._finish(vol, SEQ_TARGET, st["rays"])
        w.update(idx=idx, vol_dim=tuple(int(x) for x in dim), bnds_after=st["bnds"].copy())
        st["outs"].append(w)
    return st["outs"][:n]


def test_mergemesh_sequence_with_an_offset_target_equals_the_composed_oracle_chain():
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    tm._need_reference_builds()
    g17, g18, a = btg._seq_setup()
    want = _oracle_sequence(3)
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    b = a.voxel_bounds.copy()
    ties = {}
    with DeviceDeform(ev.SOURCE, SEQ_TARGET, b, a.voxel_size, mesh_volume=False, t_beam_table=bc.VLP32C, t_beam_azimuth=SEQ_AZ) as dd:
        for w in want:
            got = dd.deform("mergemesh", ing, w["idx"])
            torch.cuda.synchronize()
            tag = f"mm{w['idx']}"
            assert got["vol_dim"] == w["vol_dim"], tag
            assert np.array_equal(np.array(got["vol_bnds_after"]).reshape(3, 2), w["bnds_after"].astype(np.float64)), tag
            btg._check_scan(got, w, tag, ties)
    src.close()
    print(f"\nmergemesh with an offset target vs the composed oracle chain: (exact-t tie pixels, in-plane pixels) {ties}")


@pytest.mark.parametrize("sector", [None, tsg.SEQ_SECTOR])           # (the sequence's points lie ahead: a sector that holds them)
@pytest.mark.parametrize("preserve_float", [False, True])
def test_cp_with_an_offset_target_writes_the_restatements_bytes(preserve_float, sector):
    """the restated ingest, the literal loop with the column rule, the restated reverse projection and write()"""
    import oracle_chain as oc
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest, relative_indices
    g17, g18, a = btg._seq_setup("cp")
    raw, poses = cpu.raw_scans(g17), [np.array(p, np.float64) for p in g17["poses"]]
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    tH, tW = SEQ_TARGET[:2]
    fov = bc.VLP32C_FOV
    with DeviceDeform(ev.SOURCE, SEQ_TARGET, None, preserve_float=preserve_float, t_beam_table=bc.VLP32C, t_sector=sector,
                      t_beam_azimuth=SEQ_AZ) as dd, \
            DeviceDeform(ev.SOURCE, SEQ_TARGET, None, preserve_float=preserve_float, t_beam_table=bc.VLP32C, t_sector=sector) as plain:
        for idx in a.scan_indices(len(raw))[:2]:
            got = dd.deform("cp", ing, idx)
            base = plain.deform("cp", ing, idx)
            torch.cuda.synchronize()
            slots = [idx + r for r in relative_indices(a.number_of_scans)]
            pts, rem, lab = cpu.restate(raw, poses, slots, np.linalg.inv(poses[idx]), a.ignore, a.moving, merged=True)[0]
            p = ac.project(pts, rem, lab.astype(np.int64), bc.VLP32C, fov, SEQ_AZ, tW, sector)
            assert not p["near"].any(), "a point of the sequence lies on a boundary: choose another scan"
            px, py = (p["proj_xf"], p["proj_yf"]) if preserve_float else (p["proj_x"], p["proj_y"])
            back = ac.reverse_projection(p["range"], px, py, bc.VLP32C, SEQ_AZ, preserve_float, sector)
            wb, wl = oc.pack_write(back, p["label"], p["rem"], index=p["idx"])
            assert wb.shape[0] > 100
            assert np.array_equal(got["index"].cpu().numpy(), p["idx"]), idx
            assert np.array_equal(got["label_file"].cpu().numpy().view(np.uint32), wl), f"cp {idx}: label bytes"
            gb = got["bin"].cpu().numpy()
            diff = int((gb.view(np.uint32) != wb.view(np.uint32)).sum())
            print(f"\ncp with an offset target (sector {sector}), scan {idx}, preserve_float={preserve_float}: {wb.shape[0]} points, "
                  f"{diff} of {wb.size} words differ")
            assert np.array_equal(gb.view(np.uint8), wb.view(np.uint8)), f"cp {idx}: velodyne bytes"
            assert gb.tobytes() != base["bin"].cpu().numpy().tobytes()
    src.close()


def _run_sequence(a, target, out_dir, chains, **kw):
    from lidar_transfer_amd.sequence import SequenceTransfer
    g17, g18 = cpu.gold(), sq.gold18()
    src = tm._source(g17)
    with SequenceTransfer(src, a, ev.SOURCE, target, out_dir=str(out_dir), chains=chains, nclasses=int(g18["nclasses"]), **kw) as tr:
        recs = list(tr.run())
        info = dict(beam_azimuth=tr.beam_azimuth, beam_model=tr.beam_model, evaluate=tr.evaluate, summary=tr.summary)
    src.close()
    return recs, info


def test_sequence_with_an_offset_target_writes_the_oracles_files(tmp_path):
    import oracle_chain as oc
    from lidar_transfer_amd.sequence import SequenceTransfer
    tm._need_reference_builds()
    g17, g18, a = btg._seq_setup()
    model = _target_model()
    assert (model.H, model.W) == SEQ_TARGET[:2] and np.array_equal(model.beam_azimuth(), SEQ_AZ)
    r1, i1 = _run_sequence(a, model, tmp_path / "c1", 1)
    assert np.array_equal(i1["beam_azimuth"], SEQ_AZ) and i1["evaluate"] is False and i1["summary"]["beam_azimuth"] is True
    r3, i3 = _run_sequence(a, model, tmp_path / "c3", 3)
    assert i3["summary"]["chains"] == 3
    r0, i0 = _run_sequence(a, _target_model(beam_azimuth_offsets=[0.0] * 32), tmp_path / "table", 1)
    assert i0["beam_azimuth"] is None and i0["beam_model"] == "table" and i0["summary"]["beam_azimuth"] is False
    indices = [r["idx"] for r in r1]
    assert indices == [int(x) for x in a.scan_indices(8)] == [r["idx"] for r in r3] and len(indices) >= 3
    want = _oracle_sequence(len(indices))
    for rec, rec3, w in zip(r1, r3, want):
        idx = rec["idx"]
        for r in (rec, rec3):
            assert r["m_iou"] is None and r["MSE"] is None and not r["skipped"]
            assert np.array_equal(r["bnds_after"], w["bnds_after"].astype(np.float64)), idx
        if "bin" not in w:                                      # (scans the DeviceDeform test did not visit)
            sel = tm._rule_images(w)
            w["bin"], w["label_file"] = oc.pack_write(sel["endpoints"], sel["label"], sel["endrem"])
        b1, l1 = tm._read(tmp_path / "c1", idx)
        assert b1 == w["bin"].tobytes(), f"scan {idx}: velodyne file"
        assert l1 == w["label_file"].astype(np.uint32).tobytes(), f"scan {idx}: label file"
        assert (b1, l1) == tm._read(tmp_path / "c3", idx), f"scan {idx}: one chain vs three"
        assert tm._read(tmp_path / "table", idx)[0] != b1, f"scan {idx}: the offsets changed nothing"
    src = tm._source(g17)
    try:
        with pytest.raises(ValueError, match="target"):               # a SOURCE with the key
            SequenceTransfer(src, a, model, SEQ_TARGET)
    finally:
        src.close()


def test_cli_on_the_shipped_offset_file_prints_no_metrics_and_logs_the_key(tmp_path):
    import json
    import subprocess
    g17, g18, a = btg._seq_setup()
    data = tmp_path / "data"
    seq = data / "sequences" / "00"
    (seq / "velodyne").mkdir(parents=True)
    (seq / "labels").mkdir()
    for k, (xyzr, lab) in enumerate(cpu.raw_scans(g17)):
        xyzr.tofile(seq / "velodyne" / f"{k:06d}.bin")
        lab.tofile(seq / "labels" / f"{k:06d}.label")
    g17["calib_txt"].tofile(seq / "calib.txt")
    g17["poses_txt"].tofile(seq / "poses.txt")
    H, W, fu, fd = 32, 1024, 3.0, -25.0
    (data / "config.yaml").write_text(f"name: src\nfov_up: {fu}\nfov_down: {fd}\nbeams: {H}\nangle_res_hor: {360.0 / W!r}\nfov_hor: 360.0\n")
    cm = "\n".join(f"  {k}: {list(v)}" for k, v in ev.COLOR_DICT.items())
    cfg = tmp_path / "approach.yaml"
    cfg.write_text(f"adaption: mergemesh\npreserve_float: false\nnumber_of_scans: {a.number_of_scans}\n"
                   f"batch_interval: {a.batch_interval}\nvoxel_size: {a.voxel_size!r}\n"
                   f"voxel_bounds: {[float(x) for x in np.asarray(a.voxel_bounds).reshape(-1)]}\n"
                   f"transformation: []\nignore: {a.ignore}\nmoving: {a.moving}\ncolor_map:\n{cm}\n")
    outs = {}
    for name, target, more in (("az", os.path.join(ROOT, "config", "vlp32c_table_az_1024.yaml"), []),
                               ("table", os.path.join(ROOT, "config", "vlp32c_table_1024.yaml"), ["--one_scan"])):
        out = tmp_path / f"out_{name}"
        out.mkdir()
        log = tmp_path / f"{name}.jsonl"
        res = subprocess.run([sys.executable, "-m", "lidar_transfer_amd", "-d", str(data), "-c", str(cfg), "-s", "00", "-t", target,
                              "-w", "-p", str(out), "--log", str(log)] + more, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-3000:]
        rows = [json.loads(x) for x in log.read_text().splitlines()]
        outs[name] = (res.stdout, rows, tm._read(out, rows[0]["idx"]))
    so, rows, files = outs["az"]
    assert "IoU:" not in so and "Acc:" not in so and "MSE:" not in so
    assert len(rows) >= 3 and all(r["beam_azimuth"] is True and r["beam_model"] == "table" and r["m_iou"] is None for r in rows[:-1])
    assert rows[-1]["summary"]["beam_azimuth"] is True
    so, rows, files0 = outs["table"]
    assert all("beam_azimuth" not in r for r in rows[:-1]) and rows[-1]["summary"]["beam_azimuth"] is False
    assert files[0] != files0[0] and len(files[0]) > 1600
    # the key on the source: refused with a message, status 1
    (data / "config.yaml").write_text(open(os.path.join(ROOT, "config", "vlp32c_table_az_1024.yaml")).read().replace("beam_model: table\n", ""))
    res = subprocess.run([sys.executable, "-m", "lidar_transfer_amd", "-d", str(data), "-c", str(cfg), "-s", "00"], capture_output=True,
                         text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 1 and "beam_azimuth_offsets" in res.stdout


# ---- 7: nothing else moved ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adaption", ["cp", "mesh", "mergemesh"])
def test_a_table_target_without_the_key_and_with_zero_offsets_change_nothing(adaption):
    """the bytes, the ray set's parameters and the kernel path (no offsets reach the projector, the ray kernel or the reverse
    projection) of ``t_beam_table`` alone"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    g17, g18, a = btg._seq_setup(adaption)
    models = [_target_model(beam_azimuth_offsets=None), _target_model(beam_azimuth_offsets=[0.0] * 32),
              _target_model(beam_azimuth_offsets=[-0.0] * 32)]
    assert all(m.beam_azimuth() is None and np.array_equal(m.beam_table(), bc.VLP32C) for m in models)
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    res, params = [], []
    for kw in ({}, dict(t_beam_azimuth=models[0].beam_azimuth()), dict(t_beam_azimuth=models[1].beam_azimuth()),
               dict(t_beam_azimuth=np.zeros(32))):
        bnds = None if adaption == "cp" else a.voxel_bounds.copy()
        with DeviceDeform(ev.SOURCE, SEQ_TARGET, bnds, a.voxel_size, mesh_volume=adaption == "mesh", t_beam_table=bc.VLP32C, **kw) as dd:
            assert dd.t_beam_azimuth is None and dd.t_model.beam_azimuth is None and dd.t_model.azimuth_rad is None \
                and dd._t_az_dev is None
            assert dd.rayset is None or dd.rayset.beam_azimuth is None
            assert getattr(dd.projector, "_beam_az", None) is None
            params.append(None if dd.rayset is None else btg._rayset_params(dd.rayset))
            outs = []
            for idx in a.scan_indices(8)[:2]:
                out = dd.deform(adaption, ing, idx)
                torch.cuda.synchronize()
                outs.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
            assert getattr(dd.projector, "_beam_az", None) is None
            res.append(outs)
    for other, prm in zip(res[1:], params[1:]):
        assert prm == params[0]
        for x, y in zip(res[0], other):
            tm._same(x, y, adaption)
    assert res[0][0]["bin"].shape[0] > 100
    src.close()


def test_a_shared_rayset_must_have_been_built_for_the_same_offsets():
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.raytracer import RaySet
    src, tgt = (16, 64, 3.0, -25.0), (32, 64, 15.0, -25.0)
    bnds = np.array([[-4.0, 4.0], [-4.0, 4.0], [-2.0, 2.0]])
    mixed, ninety = ac.offsets("mixed", 32), ac.offsets("ninety", 32)
    mk = lambda z: RaySet(create_rays_device(tgt[2], tgt[3], tgt[0], tgt[1], beam_table=bc.VLP32C, beam_azimuth=z), tgt[0],   # noqa: E731
                          beam_table=bc.VLP32C, beam_azimuth=z)
    plain, a, b = mk(None), mk(mixed), mk(ninety)
    for rs, z, ok in ((plain, None, True), (plain, mixed, False), (a, mixed, True), (a, None, False), (b, mixed, False),
                      (a, list(mixed), True), (plain, np.zeros(32), True)):
        if ok:
            DeviceDeform(src, tgt, bnds.copy(), 0.25, mesh_volume=False, rayset=rs, t_beam_table=bc.VLP32C, t_beam_azimuth=z).close()
        else:
            with pytest.raises(ValueError, match="azimuth"):
                DeviceDeform(src, tgt, bnds.copy(), 0.25, mesh_volume=False, rayset=rs, t_beam_table=bc.VLP32C, t_beam_azimuth=z)
    for bad in (mixed[:-1], np.where(np.arange(32) == 0, 91.0, mixed), np.where(np.arange(32) == 0, np.nan, mixed)):
        with pytest.raises(ValueError):
            DeviceDeform(src, tgt, None, t_beam_table=bc.VLP32C, t_beam_azimuth=bad)
    with pytest.raises(ValueError):
        DeviceDeform(src, tgt, None, t_beam_azimuth=mixed)            # offsets without a table
    for rs in (plain, a, b):
        rs.close()
