"""The target sensor at a pose of its own (``transformation`` of the approach file), on the device: posed rays and the frame
transform against host restatements in the fixed operation order; a render from the pose against the brute-force oracle and
the compiled reference raytracer; ``DeviceDeform`` / ``SequenceTransfer`` with a mounting against a chain composed here from
the independent pieces of tests/oracle_chain.py (posed render, float64 frame transform); and the identity guard."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mount_common as mc  # noqa: E402
import test_evaluate_cpu as ev  # noqa: E402
import test_ingest_cpu as cpu  # noqa: E402
import test_sequence_cpu as sc  # noqa: E402

pytestmark = pytest.mark.gpu
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
T_EXAMPLE = mc.transformation_of(mc.POSE_EXAMPLE)
T_GENERAL = mc.transformation_of(mc.POSE_GENERAL)
TIE_BOUND = 1e-3      # tests/test_default_chain_gpu.py's bound on exact-t tie pixels


def _pose_of(T):
    """P = inv(T): where the product puts the target sensor (float64, numpy's inverse -- the product's own statement)"""
    return np.linalg.inv(np.array(T, np.float64).reshape(4, 4))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _need_reference_builds():
    from oracle import binding as ob
    if not ob.ref_available("strict"):
        pytest.skip("oracle/_ref/libref_strict.so not built (the reference checkout was absent at build time)")
    if not ob.ref_tsdf_available():
        pytest.skip("oracle/_ref/libref_tsdf_integrate.so not built (the reference checkout or hipcc was absent at build time)")


def _rays_rule(dev, host, tag):
    """tests/test_projection_gpu.py:21-25: every element within 1 ulp(f32), at most 1e-5 of them not bit-equal (the device's
    float64 sin / cos may differ from libm in the last ulp of the double)"""
    diff = np.nonzero(_bits(dev) != _bits(host))
    assert diff[0].size <= 1e-5 * dev.size, (tag, diff[0].size)
    assert np.all(np.abs(_bits(dev).astype(np.int64) - _bits(host).astype(np.int64)) <= 1), tag
    return int(diff[0].size)


# ---- 3: rays --------------------------------------------------------------------------------------------------------------
# Sensors whose grids put no ray ON a zero of a rotated component (W - 1 not a multiple of 4: no azimuth a multiple of 90
# degrees but the seam; no beam at +-5 degrees): there a component is the residue of a cancellation, a few 1e-17, and its
# float32 value follows the last bit of the double sin / cos -- no rule in ulps holds for it on any two math libraries.
RAY_SENSORS = ((3.0, -25.0, 60, 1024), (10.0, -30.0, 32, 2048), (2.0, -24.8, 64, 1024))


def test_rays_without_a_rotation_and_with_the_identity_are_create_rays():
    from lidar_transfer_amd.laserscan import create_rays_device
    for fu, fd, H, W in RAY_SENSORS + ((3.0, -25.0, 64, 1024), (15.0, -15.0, 16, 301), (0.0, -10.0, 1, 720), (10.0, -30.0, 32, 1)):
        base = create_rays_device(fu, fd, H, W).cpu().numpy()
        none = create_rays_device(fu, fd, H, W, rot=None).cpu().numpy()
        eye = create_rays_device(fu, fd, H, W, rot=np.eye(3)).cpu().numpy()
        assert np.array_equal(_bits(none), _bits(base)), (H, W)       # the same kernel
        assert np.array_equal(eye, base), (H, W)                      # by value: 0 * x may turn a zero's sign
        assert base.shape == (H * W, 3) and eye.dtype == np.float32


@pytest.mark.parametrize("name,rot", [("yaw 90", mc.rot_zyx(90.0, 0.0, 0.0)), ("pitch -5", mc.rot_zyx(0.0, -5.0, 0.0)),
                                      ("general", mc.POSE_GENERAL[:3, :3])])
def test_posed_rays_equal_the_float64_restatement(name, rot):
    from lidar_transfer_amd.laserscan import create_rays_device
    for fu, fd, H, W in RAY_SENSORS + ((3.0, -25.0, 1, 1), (3.0, -25.0, 3, 171)):
        dev = create_rays_device(fu, fd, H, W, rot=rot).cpu().numpy()
        host = mc.posed_rays(fu, fd, H, W, rot)
        n = _rays_rule(dev, host, (name, H, W))
        assert np.abs(np.linalg.norm(dev.astype(np.float64), axis=1) - 1).max() < 1e-6
        base = create_rays_device(fu, fd, H, W).cpu().numpy()
        assert not np.array_equal(dev, base)
        print(f"\n{name} {H}x{W}: {n} of {dev.size} elements not bit-equal to the restatement")
    with pytest.raises(ValueError):
        create_rays_device(3.0, -25.0, 4, 8, rot=np.eye(4))


# ---- 4: the frame transform -------------------------------------------------------------------------------------------------
def test_points_to_frame_is_the_elementwise_restatement_bit_for_bit():
    import torch
    from lidar_transfer_amd.post import points_to_frame
    rng = np.random.default_rng(11)
    n = 200000
    p = (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 2, (n, 1))).astype(np.float32)
    p[:8] = [[0, 0, 0], [-0.0, 0.0, -0.0], [1e-45, -1e-45, 1e-40], [1e-39, 2e-39, -3e-39], [1e30, -1e30, 1e30],
             [1e30, 1.0, -1e-30], [-0.0, -0.0, -0.0], [3e38, 3e38, 3e38]]
    tri = np.where(rng.random(n) < 0.2, -1 - rng.integers(0, 3, n), rng.integers(0, 50000, n)).astype(np.int32)
    tri[:8] = [5, 5, 5, 5, 5, 5, -1, 5]
    assert (tri < 0).sum() > 10000
    d, t = torch.from_numpy(p).cuda(), torch.from_numpy(tri).cuda()
    for T in (T_EXAMPLE, T_GENERAL, [1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 3.0, 0, 0, 0, 1]):
        want = mc.to_frame(p, T, tri)
        got = points_to_frame(d, T, tri=t)
        assert got.data_ptr() != d.data_ptr()
        g = got.cpu().numpy()
        assert np.array_equal(_bits(g), _bits(want))
        assert np.array_equal(_bits(g[tri < 0]), _bits(p[tri < 0]))                 # misses: copied, bit for bit
        assert np.array_equal(_bits(points_to_frame(d, T).cpu().numpy()), _bits(mc.to_frame(p, T)))   # no tri: every row
        inplace = d.clone()
        assert points_to_frame(inplace, T, tri=t, out=inplace).data_ptr() == inplace.data_ptr()
        assert np.array_equal(_bits(inplace.cpu().numpy()), _bits(want))
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(p))                     # out of place left the input alone
    # on a side stream, and n not a multiple of the workgroup
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = points_to_frame(d[:777].contiguous(), T_GENERAL, tri=t[:777].contiguous())
    st.synchronize()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(mc.to_frame(p[:777], T_GENERAL, tri[:777])))
    assert points_to_frame(d[:0].contiguous(), T_GENERAL).shape == (0, 3)
    with pytest.raises(ValueError):
        points_to_frame(d.double(), T_GENERAL)


# ---- 5: a render from the pose ----------------------------------------------------------------------------------------------
def _both_strategies(v, f, c, r, trays, origin, H):
    import torch
    from lidar_transfer_amd.raytracer import RaySet, Scene
    dev = torch.device("cuda", 0)
    scn = Scene(0)
    scn.set_mesh(*[torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (v, f, c, r)])
    rs = RaySet(trays, H)
    a = scn.render(rs, origin)
    scn.build()
    b = scn.trace(trays, origin, H)
    torch.cuda.synchronize()
    a = {k: x.cpu().numpy() for k, x in a.items()}
    b = {k: x.cpu().numpy() for k, x in b.items()}
    rs.close()
    scn.close()
    return a, b


def _reference_trace(rays, org, mesh, H):
    """the compiled reference raytracer -- on a host whose RSQRTSS is not the seed table the product replays: its restatement,
    first held to the compiled reference with this host's own seed, then run with the table (tests/oracle_chain.py:171-182)"""
    import oracle_chain as oc
    from oracle import binding as ob
    ref = ob.ref_trace(rays, org, *mesh, H, kind="strict")
    if not oc.host_rsqrt_is_the_table():
        mine = ob.oracle_trace(rays, org, *mesh, H, mode=ob.MODE_REF_BVH, norm=ob.NORM_SSE, nthreads=oc.THREADS)
        for k in ("range", "endrem", "endpoints", "endcolors"):
            assert np.array_equal(_bits(mine[k]), _bits(ref[k])), f"the restated reference raytracer differs from the compiled one in {k}"
        ref = ob.oracle_trace(rays, org, *mesh, H, mode=ob.MODE_REF_BVH, norm=ob.NORM_SSE_TABLE, nthreads=oc.THREADS)
    return ref


def test_render_from_a_pose_equals_brute_force_and_the_compiled_reference(capfd):
    """tests/test_mount_cpu.py chose the scene and the two poses; the rays are the product's own, downloaded"""
    import oracle_chain as oc
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.synth import synth_scene
    from oracle import binding as ob
    if not ob.ref_available("strict"):
        pytest.skip("oracle/_ref not built (the reference checkout was absent at build time)")
    mesh = synth_scene(mc.RENDER_SEED, mc.RENDER_TRIS)
    assert mesh[1].shape[0] >= 200000
    H, W = mc.RENDER_H, mc.RENDER_W
    report = {}
    for name, P in mc.RENDER_POSES:
        trays = create_rays_device(mc.RENDER_FOV[0], mc.RENDER_FOV[1], H, W, rot=P[:3, :3])
        rays = trays.cpu().numpy()
        _rays_rule(rays, mc.posed_rays(mc.RENDER_FOV[0], mc.RENDER_FOV[1], H, W, P[:3, :3]), name)
        org = mc.origin_of(P)
        a, b = _both_strategies(*mesh, trays, tuple(float(x) for x in org), H)
        brute = ob.oracle_trace(rays, org, *mesh, H, mode=ob.MODE_BRUTE, norm=ob.NORM_SSE_TABLE, nthreads=oc.THREADS)
        for k in ("tri", "range", "endcolors", "endrem", "endpoints"):
            for tag, got in (("scatter", a), ("lbvh", b)):
                bad = np.nonzero((_bits(got[k]) != _bits(brute[k])).reshape(H * W, -1).any(1))[0]
                assert bad.size == 0, f"{name}: {tag} {k} differs from MODE_BRUTE at {bad.size} rays, first {bad[:5]}"
        ref = _reference_trace(rays, org, mesh, H)
        capfd.readouterr()  # the reference printf()s
        same = np.ones(H * W, bool)
        for k in ("range", "endcolors", "endrem", "endpoints"):
            same &= (_bits(ref[k]) == _bits(brute[k])).reshape(H * W, -1).all(1)
        n_diff = int((~same).sum())
        assert n_diff <= mc.REF_CULL_CAP * H * W, (name, n_diff)
        for k in ("range", "endcolors", "endrem", "endpoints"):
            for tag, got in (("scatter", a), ("lbvh", b)):
                assert np.array_equal(_bits(got[k])[same], _bits(ref[k])[same]), f"{name}: {tag} {k} vs the compiled reference"
        hits = int((brute["tri"] >= 0).sum())
        assert hits > 0.5 * H * W
        report[name] = (n_diff, hits)
    print(f"\nrender from a pose: (rays where the reference differs from MODE_BRUTE, hits) {report}")


# ---- 6: DeviceDeform with a mounting against the composed oracle chain ------------------------------------------------------
def _device_rays(target, P):
    """the product's posed rays, downloaded, after they passed the rays' rule against the restatement"""
    from lidar_transfer_amd.laserscan import create_rays_device
    tH, tW, tfu, tfd = target
    rays = create_rays_device(tfu, tfd, tH, tW, rot=P[:3, :3]).cpu().numpy()
    _rays_rule(rays, mc.posed_rays(tfu, tfd, tH, tW, P[:3, :3]), "rays of the oracle chain")
    return rays


def _posed_finish(vol, target, P, T, rays):
    """oracle_chain.finish with the render from the pose and write() in the target's frame"""
    import oracle_chain as oc
    from oracle import binding as ob
    mesh = vol.mesh()
    tH = target[0]
    org = mc.origin_of(P)
    ref = _reference_trace(rays, org, mesh, tH)
    brute = ob.oracle_trace(rays, org, *mesh, tH, mode=ob.MODE_BRUTE, norm=ob.NORM_SSE_TABLE, nthreads=oc.THREADS)
    ref["rays"] = brute["rays"] = rays
    return dict(mesh=mesh, ref=ref, brute=brute, T=np.array(T, np.float64).reshape(4, 4))


def _rule_images(want):
    """the images oracle_chain.check_images selects (the reference's; MODE_BRUTE's at exact-t ties and in-plane rays)"""
    ref, brute = want["ref"], want["brute"]
    same = lambda a, b: (_bits(a) == _bits(b)).reshape(len(a), -1).all(1)   # noqa: E731
    keys = ("range", "endrem", "endpoints")
    lab_r, lab_b = ref["endcolors"][:, 2], brute["endcolors"][:, 2]
    ref_is_brute = same(ref["range"], brute["range"]) & (lab_r == lab_b) & same(ref["endrem"], brute["endrem"]) & \
        same(ref["endpoints"], brute["endpoints"])
    in_plane = (np.abs(np.asarray(ref["rays"], np.float32).reshape(-1, 3)) < 1e-7).any(1)
    use_brute = ~ref_is_brute & (same(ref["range"], brute["range"]) | in_plane)
    out = {k: np.where(use_brute.reshape((-1,) + (1,) * (np.asarray(ref[k]).ndim - 1)), brute[k], ref[k]) for k in keys}
    out["label"] = np.where(use_brute, lab_b, lab_r)
    return out


def _check_mounted_scan(got, want, tag, ties):
    """scene-frame images by check_images' rule; the target-frame endpoints = the float64 frame transform of the hits; the
    written bytes = write() of the target-frame points"""
    import oracle_chain as oc
    g = dict(range=got["range"].cpu().numpy(), label=got["label"].cpu().numpy(), rem=got["rem"].cpu().numpy(),
             endpoints=got["endpoints_scene"].cpu().numpy(), tri=got["tri"].cpu().numpy())
    n = oc.check_images(g, want, tag)
    assert n[0] <= TIE_BOUND * want["ref"]["range"].size, f"{tag}: {n[0]} exact-t tie pixels"
    ties[tag] = n
    sel = _rule_images(want)
    ends = mc.to_frame(sel["endpoints"], want["T"], want["brute"]["tri"])
    assert np.array_equal(_bits(got["endpoints"].cpu().numpy()), _bits(ends)), f"{tag}: endpoints in the target's frame"
    miss = want["brute"]["tri"] < 0
    assert not ends[miss].any(), f"{tag}: a miss left (0, 0, 0)"
    want["bin"], want["label_file"] = oc.pack_write(ends, sel["label"], sel["endrem"])
    if "bin" in got:
        assert np.array_equal(got["bin"].cpu().numpy().view(np.uint8), want["bin"].view(np.uint8)), f"{tag}: velodyne bytes"
        assert np.array_equal(got["label_file"].cpu().numpy().view(np.uint32), want["label_file"]), f"{tag}: label bytes"
    assert want["bin"].shape[0] > 100, f"{tag}: the oracle's scan is nearly empty"


def _dev(clouds):
    import torch
    return [(torch.from_numpy(np.ascontiguousarray(p)).cuda(), torch.from_numpy(np.ascontiguousarray(r)).cuda(),
             torch.from_numpy(np.ascontiguousarray(l).astype(np.int32)).cuda()) for p, r, l in clouds]


@pytest.mark.parametrize("pose", ["example", "general"])
def test_mesh_with_a_mounting_equals_the_composed_oracle_chain(pose):
    import oracle_chain as oc
    import pin_cases
    import test_default_chain_gpu as dc
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    _need_reference_builds()
    T = mc.transformation_of(dict(mc.RENDER_POSES)[pose])
    P = _pose_of(T)
    _, src, tgt, n_scans, bnds, voxel, seeds = pin_cases.deform_mesh_case(0)
    clouds = pin_cases.deform_mesh_clouds(seeds[0], n_scans, src, dc._host_render)
    with DeviceDeform(src, tgt, bnds.copy(), voxel, transformation=T) as dd:
        assert dd.origin == tuple(float(x) for x in mc.origin_of(P))
        got = dd.mesh(_dev(clouds))
        torch.cuda.synchronize()
        H, W, fu, fd = src
        b = np.array(bnds, copy=True)
        dim, origin = oc.volume_geometry(b, voxel)
        vol = oc.RefVolume(dim, origin, voxel, fu, fd)
        for pts, rem, lab in clouds:
            rng, remi, labi, _ = oc.project(pts, rem, lab, H, W, fu, fd)
            vol.integrate(labi, rng, remi)
        dc._check_volumes(dd.vol.get_volume_tensors(), dict(fields=[t.cpu() for t in vol.fields]), pose)   # fusion: untouched
        want = _posed_finish(vol, tgt, P, T, _device_rays(tgt, P))
        ties = {}
        _check_mounted_scan(got, want, f"mesh/{pose}", ties)
        # the same clouds without the mounting: another scan
        with DeviceDeform(src, tgt, bnds.copy(), voxel) as plain:
            base = plain.mesh(_dev(clouds))
            torch.cuda.synchronize()
            assert not np.array_equal(base["range"].cpu().numpy(), got["range"].cpu().numpy())
            assert base["endpoints_scene"].data_ptr() == base["endpoints"].data_ptr()
    print(f"\nmesh with the {pose} mounting vs the composed oracle chain: (exact-t tie pixels, in-plane pixels) {ties}")


# the F17 sequence (tests/golden/f17_ingest.npz) with the mergemesh approach of F18 and the example mounting
def _seq_setup(adaption="mergemesh", transformation=T_EXAMPLE):
    g17, g18 = cpu.gold(), sc.gold18()
    a = sc.approach_for(g18, adaption)
    a.transformation = list(transformation)
    t = g18["target_t"]
    return g17, g18, a, (int(t[0]), int(t[1]), float(t[2]), float(t[3]))


def _source(g17, **kw):
    from lidar_transfer_amd.ingest import SequenceSource
    raw = cpu.raw_scans(g17)
    return SequenceSource(scans=[x for x, _ in raw], labels=[l for _, l in raw], poses=g17["poses"], **kw)


_SEQ_ORACLE = dict(outs=[], bnds=None)


def _oracle_sequence(n):
    """the composed chain over the first ``n`` output scans of the sequence on ONE bounds array (cached: the sequence test
    compares its files with the same scans); the merged clouds are the restated ingest's (tests/test_ingest_cpu.py)"""
    import oracle_chain as oc
    g17, g18, a, target = _seq_setup()
    st = _SEQ_ORACLE
    if st["bnds"] is None:
        st["bnds"] = a.voxel_bounds.copy()
        st["rays"] = _device_rays(target, _pose_of(T_EXAMPLE))
    raw, poses = cpu.raw_scans(g17), [np.array(p, np.float64) for p in g17["poses"]]
    from lidar_transfer_amd.ingest import relative_indices
    H, W = ev.SOURCE[0], ev.SOURCE[1]
    tfu, tfd = target[2], target[3]
    indices = [int(x) for x in a.scan_indices(len(raw))]
    while len(st["outs"]) < n:
        idx = indices[len(st["outs"])]
        slots = [idx + r for r in relative_indices(a.number_of_scans)]
        pts, rem, lab = cpu.restate(raw, poses, slots, np.linalg.inv(poses[idx]), a.ignore, a.moving, merged=True)[0]
        rng, remi, labi, kept = oc.project(pts, rem, lab.astype(np.int64), H, W, tfu, tfd)
        dim, origin, given = oc.mergemesh_bounds(st["bnds"], kept, a.voxel_size)
        vol = oc.RefVolume(dim, origin, a.voxel_size, tfu, tfd)
        vol.integrate(labi, rng, remi)
        w = _posed_finish(vol, target, _pose_of(T_EXAMPLE), T_EXAMPLE, st["rays"])
        w.update(idx=idx, vol_dim=tuple(int(x) for x in dim), bnds_after=st["bnds"].copy())
        st["outs"].append(w)
    return st["outs"][:n]


@pytest.mark.parametrize("source_images", [False, True])
def test_mergemesh_sequence_with_a_mounting_equals_the_composed_oracle_chain(source_images):
    """three output scans on one bounds array; projection, bounds and fusion are those of the run without a mounting"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    _need_reference_builds()
    g17, g18, a, target = _seq_setup()
    want = _oracle_sequence(3)
    src = _source(g17)
    ing = ScanIngest(src, a)
    b = a.voxel_bounds.copy()
    ties = {}
    with DeviceDeform(ev.SOURCE, target, b, a.voxel_size, mesh_volume=False, transformation=a.mount()) as dd:
        for w in want:
            got = dd.deform("mergemesh", ing, w["idx"], source_images=source_images)
            torch.cuda.synchronize()
            tag = f"mm{w['idx']}/{source_images}"
            assert got["vol_dim"] == w["vol_dim"], tag
            assert np.array_equal(np.array(got["vol_bnds_after"]).reshape(3, 2), w["bnds_after"].astype(np.float64)), tag
            assert np.array_equal(b, w["bnds_after"]) and b.dtype == w["bnds_after"].dtype, tag
            _check_mounted_scan(got, w, tag, ties)
    src.close()
    print(f"\nmergemesh with the example mounting vs the composed oracle chain: (exact-t tie pixels, in-plane pixels) {ties}")


# ---- 7: cp ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", ["example", "general"])
def test_cp_with_a_mounting_writes_the_oracles_bytes(pose):
    """the merged cloud goes into the target's frame on ingest, ``back = T . inv(pose of the primary scan)``; the oracle: the
    restated ingest with that matrix, oracle/projection.py, the restated reverse projection and write()"""
    import oracle_chain as oc
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest, relative_indices
    from oracle import projection as op
    T = mc.transformation_of(dict(mc.RENDER_POSES)[pose])
    g17, g18, a, target = _seq_setup("cp", T)
    raw, poses = cpu.raw_scans(g17), [np.array(p, np.float64) for p in g17["poses"]]
    src = _source(g17)
    ing = ScanIngest(src, a)
    tH, tW, tfu, tfd = target
    with DeviceDeform(ev.SOURCE, target, None, preserve_float=a.preserve_float, transformation=T) as dd, \
            DeviceDeform(ev.SOURCE, target, None, preserve_float=a.preserve_float) as plain:
        for idx in a.scan_indices(len(raw))[:3]:
            got = dd.deform("cp", ing, idx)
            base = plain.deform("cp", ing, idx)
            torch.cuda.synchronize()
            back = np.matmul(np.array(T).reshape(4, 4), np.linalg.inv(poses[idx]))
            slots = [idx + r for r in relative_indices(a.number_of_scans)]
            pts, rem, lab = cpu.restate(raw, poses, slots, back, a.ignore, a.moving, merged=True)[0]
            p = op.range_projection(pts, rem, tH, tW, tfu, tfd, remove=True, method="new")
            label = op.label_projection(p["index"], lab[p["kept"]].astype(np.int64))
            px, py = p["px"][p["index"]], p["py"][p["index"]]        # an empty cell: numpy's index -1, the last kept point
            pts_back = oc.reverse_projection(p["range"], px, py, tfu, tfd)
            wb, wl = oc.pack_write(pts_back, label, p["remission"], index=p["index"])
            assert wb.shape[0] > 100
            assert np.array_equal(got["index"].cpu().numpy(), p["index"]), idx
            assert np.array_equal(got["bin"].cpu().numpy().view(np.uint8), wb.view(np.uint8)), f"cp {pose} {idx}: velodyne bytes"
            assert np.array_equal(got["label_file"].cpu().numpy().view(np.uint32), wl), f"cp {pose} {idx}: label bytes"
            assert got["bin"].cpu().numpy().tobytes() != base["bin"].cpu().numpy().tobytes()
    src.close()


# ---- 8: a sequence ----------------------------------------------------------------------------------------------------------
def _run_sequence(a, target, out_dir, chains, **kw):
    from lidar_transfer_amd.sequence import SequenceTransfer
    g17, g18 = cpu.gold(), sc.gold18()
    src = _source(g17)
    with SequenceTransfer(src, a, ev.SOURCE, target, out_dir=str(out_dir), chains=chains, nclasses=int(g18["nclasses"]), **kw) as tr:
        recs = list(tr.run())
        mounted, evaluate, summary = tr.mounted, tr.evaluate, tr.summary
    src.close()
    return recs, mounted, evaluate, summary


def _read(out_dir, idx):
    from lidar_transfer_amd.sequence import output_paths
    b, l = output_paths(str(out_dir), "00", idx)
    return open(b, "rb").read(), open(l, "rb").read()


def test_sequence_with_a_mounting_writes_the_oracles_files(tmp_path):
    """the mergemesh sequence with the example mounting: every written file equals the composed oracle chain's bytes, one
    chain and three chains write the same files, nothing is compared with the source scans, and the files are NOT those of
    the same sequence without the mounting"""
    from lidar_transfer_amd.sequence import SequenceTransfer
    _need_reference_builds()
    g17, g18, a, target = _seq_setup()
    assert ev.SOURCE[:2] == target[:2]            # (without the mounting this run would compare)
    r1, mounted, evaluate, summary = _run_sequence(a, target, tmp_path / "c1", 1)
    assert mounted and evaluate is False and summary["mounted"] is True
    r3, _, _, s3 = _run_sequence(a, target, tmp_path / "c3", 3)
    assert s3["chains"] == 3
    ident = sc.approach_for(g18, "mergemesh")
    ident.transformation = list(IDENTITY)
    r0, mounted0, evaluate0, _ = _run_sequence(ident, target, tmp_path / "id", 1)
    assert not mounted0 and evaluate0 is True and all(r["m_iou"] is not None for r in r0)
    indices = [r["idx"] for r in r1]
    assert indices == [int(x) for x in a.scan_indices(8)] == [r["idx"] for r in r3] == [r["idx"] for r in r0]
    assert len(indices) >= 3
    want = _oracle_sequence(len(indices))
    ties = {}
    for rec, rec3, w in zip(r1, r3, want):
        idx = rec["idx"]
        assert w["idx"] == idx
        for r in (rec, rec3):
            assert r["m_iou"] is None and r["m_acc"] is None and r["MSE"] is None and r["iou"] is None and not r["skipped"]
            assert np.array_equal(r["bnds_after"], w["bnds_after"].astype(np.float64)), idx
        if "bin" not in w:                        # (scans the DeviceDeform test did not visit: the rule's bytes from the oracle alone)
            import oracle_chain as oc
            sel = _rule_images(w)
            w["bin"], w["label_file"] = oc.pack_write(mc.to_frame(sel["endpoints"], w["T"], w["brute"]["tri"]), sel["label"],
                                                      sel["endrem"])
        b1, l1 = _read(tmp_path / "c1", idx)
        assert b1 == w["bin"].tobytes(), f"scan {idx}: velodyne file"
        assert l1 == w["label_file"].astype(np.uint32).tobytes(), f"scan {idx}: label file"
        assert rec["n_points"] == w["bin"].shape[0]
        assert (b1, l1) == _read(tmp_path / "c3", idx), f"scan {idx}: one chain vs three"
        b0, l0 = _read(tmp_path / "id", idx)
        assert b0 != b1, f"scan {idx}: the mounting changed nothing"
    with pytest.raises(ValueError):
        src = _source(g17)
        try:
            SequenceTransfer(src, a, ev.SOURCE, target, evaluate=True)
        finally:
            src.close()
    bad = sc.approach_for(g18, "mergemesh")
    bad.transformation = list(T_EXAMPLE[:15])
    with pytest.raises(ValueError):
        src = _source(g17)
        try:
            SequenceTransfer(src, bad, ev.SOURCE, target)
        finally:
            src.close()


def test_cli_with_a_mounting_prints_no_metrics_and_logs_mounted(tmp_path):
    import json
    import subprocess
    g17, g18, a, target = _seq_setup()
    data = tmp_path / "data"
    seq = data / "sequences" / "00"
    (seq / "velodyne").mkdir(parents=True)
    (seq / "labels").mkdir()
    for k, (xyzr, lab) in enumerate(cpu.raw_scans(g17)):
        xyzr.tofile(seq / "velodyne" / f"{k:06d}.bin")
        lab.tofile(seq / "labels" / f"{k:06d}.label")
    g17["calib_txt"].tofile(seq / "calib.txt")
    g17["poses_txt"].tofile(seq / "poses.txt")
    H, W, fu, fd = ev.SOURCE
    (data / "config.yaml").write_text(f"name: src\nfov_up: {fu}\nfov_down: {fd}\nbeams: {H}\nangle_res_hor: {360.0 / W!r}\nfov_hor: 360.0\n")
    outs = {}
    for name, t in (("mounted", T_EXAMPLE), ("identity", IDENTITY)):
        cfg = tmp_path / f"{name}.yaml"
        cm = "\n".join(f"  {k}: {list(v)}" for k, v in ev.COLOR_DICT.items())
        cfg.write_text(f"adaption: mergemesh\npreserve_float: false\nnumber_of_scans: {a.number_of_scans}\n"
                       f"batch_interval: {a.batch_interval}\nvoxel_size: {a.voxel_size!r}\n"
                       f"voxel_bounds: {[float(x) for x in np.asarray(a.voxel_bounds).reshape(-1)]}\n"
                       f"transformation: {[float(x) for x in t]}\nignore: {a.ignore}\nmoving: {a.moving}\ncolor_map:\n{cm}\n")
        out = tmp_path / f"out_{name}"
        out.mkdir()
        log = tmp_path / f"{name}.jsonl"
        res = subprocess.run([sys.executable, "-m", "lidar_transfer_amd", "-d", str(data), "-c", str(cfg), "-s", "00", "-w", "-p",
                              str(out), "--one_scan", "--log", str(log)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-3000:]
        rows = [json.loads(x) for x in log.read_text().splitlines()]
        outs[name] = (res.stdout, rows, _read(out, rows[0]["idx"]))
    so, rows, files = outs["mounted"]
    assert "IoU:" not in so and "MSE:" not in so and rows[0]["mounted"] is True and rows[0]["m_iou"] is None
    assert rows[-1]["summary"]["mounted"] is True
    so, rows, files0 = outs["identity"]
    assert "IoU:" in so and "mounted" not in rows[0] and rows[-1]["summary"]["mounted"] is False
    assert files[0] != files0[0]


# ---- 9: the identity guard ----------------------------------------------------------------------------------------------------
def _same(a, b, tag):
    import torch
    for k in sorted(set(a) | set(b)):
        if k.startswith("_") or k in ("volume", "source"):
            continue
        x, y = a[k], b[k]
        if isinstance(x, torch.Tensor):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (tag, k)
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y)), (tag, k)


@pytest.mark.parametrize("adaption", ["cp", "mesh", "mergemesh"])
def test_identity_and_empty_transformations_change_nothing(adaption):
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    g17, g18, a, target = _seq_setup(adaption, [])
    src = _source(g17)
    ing = ScanIngest(src, a)
    res = []
    for kw in ({}, dict(transformation=[]), dict(transformation=[float(x) for x in IDENTITY]), dict(transformation=None),
               dict(transformation=np.eye(4))):
        bnds = None if adaption == "cp" else a.voxel_bounds.copy()
        with DeviceDeform(ev.SOURCE, target, bnds, a.voxel_size, mesh_volume=adaption == "mesh", **kw) as dd:
            assert dd.mount is None and dd.origin == (0.0, 0.0, 0.0)
            assert dd.rayset is None or dd.rayset.pose is None
            outs = []
            for idx in a.scan_indices(8)[:2]:
                out = dd.deform(adaption, ing, idx)
                torch.cuda.synchronize()
                outs.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
            res.append(outs)
    for other in res[1:]:
        for x, y in zip(res[0], other):
            _same(x, y, adaption)
    assert res[0][0]["bin"].shape[0] > 100
    src.close()


def test_identity_transformation_changes_nothing_in_the_fusion_pipeline():
    import torch
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.pipeline import FusionScanPipeline
    res = {}
    for name, kw in (("none", {}), ("identity", dict(transformation=IDENTITY)), ("empty", dict(transformation=[]))):
        g17, g18, a, target = _seq_setup("mergemesh", [])
        am = sc.approach_for(g18, "mesh")
        src = _source(g17)
        rays = create_rays_device(target[2], target[3], target[0], target[1], device=0)
        got = []
        with FusionScanPipeline(a.voxel_bounds.copy(), a.voxel_size, target[2], target[3], rays, target[0], chains=2, device=0,
                                label_image=True, source_hw=ev.SOURCE[:2], fixed_volume=False, **kw) as pipe:
            assert pipe.mount is None and pipe.origin == (0.0, 0.0, 0.0)
            ing = ScanIngest(src, a)
            tickets = []
            for idx in a.scan_indices(8)[:3]:
                clouds = ing.prepare(idx, merged=True)
                torch.cuda.synchronize()
                tickets.append(pipe.submit_mergemesh(clouds, inputs_ready=True))
            got += [pipe.wait(t) for t in tickets]
        with FusionScanPipeline(am.voxel_bounds.copy(), am.voxel_size, ev.SOURCE[2], ev.SOURCE[3], rays, target[0], chains=2,
                                device=0, label_image=True, source_hw=ev.SOURCE[:2], **kw) as pipe:
            ing = ScanIngest(src, am)
            clouds = ing.prepare(am.scan_indices(8)[0], merged=False)
            torch.cuda.synchronize()
            got.append(pipe.wait(pipe.submit_clouds(clouds, inputs_ready=True)))
        res[name] = got
        src.close()
    for name in ("identity", "empty"):
        for x, y in zip(res["none"], res[name]):
            assert "endpoints_scene" not in y
            _same(x, y, name)


def test_a_shared_rayset_must_have_been_built_for_the_same_pose():
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.raytracer import RaySet
    src, tgt = (16, 64, 3.0, -25.0), (16, 64, 10.0, -30.0)
    bnds = np.array([[-4.0, 4.0], [-4.0, 4.0], [-2.0, 2.0]])
    P = mc.POSE_GENERAL
    plain = RaySet(create_rays_device(tgt[2], tgt[3], tgt[0], tgt[1]), tgt[0])
    posed = RaySet(create_rays_device(tgt[2], tgt[3], tgt[0], tgt[1], rot=P[:3, :3]), tgt[0], pose=np.linalg.inv(np.array(T_GENERAL).reshape(4, 4)))
    other = RaySet(create_rays_device(tgt[2], tgt[3], tgt[0], tgt[1], rot=mc.POSE_EXAMPLE[:3, :3]), tgt[0], pose=mc.POSE_EXAMPLE)
    for rs, t, ok in ((plain, None, True), (plain, T_GENERAL, False), (posed, T_GENERAL, True), (posed, None, False),
                      (other, T_GENERAL, False), (plain, IDENTITY, True)):
        if ok:
            DeviceDeform(src, tgt, bnds.copy(), 0.25, mesh_volume=False, rayset=rs, transformation=t).close()
        else:
            with pytest.raises(ValueError):
                DeviceDeform(src, tgt, bnds.copy(), 0.25, mesh_volume=False, rayset=rs, transformation=t)
    for rs in (plain, posed, other):
        rs.close()
