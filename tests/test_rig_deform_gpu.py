"""RigDeform (lidar_transfer_amd/rig.py): several target sensors around one chain.  Every comparison is of bytes.

mesh       every head's result and packed rows equal those of a single DeviceDeform of that sensor on the same clouds;
mergemesh  head 0 equals the single DeviceDeform; every further head equals Scene.render of its ray set on the scene as
           head 0's call left it, followed by its own Sensing -- over three scans, one of which moves the geometry (a re-run);
and the refusals (field of view, cp), and the merged rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mount_common as mc  # noqa: E402

pytestmark = pytest.mark.gpu

SRC = (16, 256, 10.0, -25.0)
BNDS = np.array([[-10.0, 10.0], [-10.0, 10.0], [-3.0, 3.0]])
VOXEL = 0.2
PLAIN = dict(name="plain", fov_up=10.0, fov_down=-25.0, beams=16, angle_res_hor=360.0 / 256, fov_hor=360)
TABLE = dict(name="table", fov_up=8.0, fov_down=-24.0, beams=8, angle_res_hor=360.0 / 128, fov_hor=360, beam_model="table",
             beam_angles=[8.0, 3.0, -1.0, -4.0, -8.0, -13.0, -18.0, -24.0],
             return_model=dict(min_range=0.5, max_range=9.0, max_incidence=80.0, remission="lambert", drop_rate=0.1, seed=3),
             noise_model=dict(range_sigma=0.02, range_sigma_rel=0.0005, range_resolution=0.002, remission_sigma=0.02,
                              remission_levels=256, seed=5))
SECTOR = dict(name="sector", fov_up=5.0, fov_down=-22.0, beams=12, angle_res_hor=120.0 / 96, fov_hor=120, azimuth_model="sector",
              azimuth_center=10.0, echo_model=dict(divergence=0.6, subrays=4, ring=0.7071, separation=0.3, min_subrays=1,
                                                   mode="strongest"))
TALL = dict(PLAIN, name="tall", fov_up=12.0)
RIG = [dict(name="roof", sensor=PLAIN), dict(name="side", sensor=TABLE, transformation=mc.transformation_of(mc.POSE_EXAMPLE)),
       dict(name="front", sensor=SECTOR, transformation=mc.transformation_of(mc.POSE_GENERAL))]


def _approach(rig, **kw):
    from lidar_transfer_amd.config import load_approach
    return load_approach(dict(dict(adaption="mesh", preserve_float=False, voxel_size=VOXEL, number_of_scans=1,
                                   voxel_bounds=BNDS.reshape(-1).tolist(), ignore=[], moving=[], transformation=[],
                                   color_map={0: [0, 0, 0]}, rig=rig), **kw))


_CLOUDS = {}


def _clouds(seed, n_scans=2, scale=1.0):
    """the source scans of a seeded street scene (tests/pin_cases.py), rendered by the brute-force oracle; once per seed"""
    import pin_cases
    import test_default_chain_gpu as dc
    import torch
    if seed not in _CLOUDS:
        _CLOUDS[seed] = pin_cases.deform_mesh_clouds(seed, n_scans, SRC, dc._host_render)
    return [(torch.from_numpy(np.ascontiguousarray(p * scale)).cuda(), torch.from_numpy(np.ascontiguousarray(r)).cuda(),
             torch.from_numpy(np.ascontiguousarray(l).astype(np.int32)).cuda()) for p, r, l in _CLOUDS[seed]]


def _single(head, **kw):
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.rig import head_keywords
    target, hkw = head_keywords(head.sensor)
    return DeviceDeform(SRC, target, BNDS.copy(), VOXEL, transformation=head.mount, **hkw, **kw)


def _same(a, b, tag, skip=("volume", "source", "vol_dim", "vol_origin", "vol_bnds_after")):
    import torch
    keys = sorted(k for k in set(a) | set(b) if not k.startswith("_") and k not in skip)
    assert keys, tag
    for k in keys:
        assert k in a and k in b, (tag, k)
        x, y = a[k], b[k]
        if isinstance(x, dict):
            _same(x, y, f"{tag}/{k}", skip)
        elif isinstance(x, torch.Tensor):
            assert x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (tag, k)
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y)), (tag, k)


def _hits_and_misses(res, tag):
    tri = res["tri"].cpu().numpy()
    assert (tri >= 0).any() and (tri < 0).any(), (tag, int((tri >= 0).sum()), tri.size)


def test_mesh_every_head_equals_its_single_device_deform():
    import torch
    from lidar_transfer_amd.rig import RigDeform
    heads = _approach(RIG).rig()
    clouds = _clouds(11)
    with RigDeform(SRC, heads, BNDS.copy(), VOXEL) as rig:
        for scan_index in (0, 3):
            got = rig.mesh(clouds, scan_index=scan_index)
            torch.cuda.synchronize()
            assert len(got) == 3 and got.bin is None
            for h, g in zip(heads, got):
                _hits_and_misses(g, h.name)
                with _single(h) as dd:
                    want = dd.mesh(clouds, scan_index=scan_index)
                    torch.cuda.synchronize()
                    _same(g, want, f"mesh/{h.name}/{scan_index}")
                    assert g["bin"].shape[0] > 50 and g["bin"].shape[0] == g["label_file"].shape[0]
        # the models really ran on their heads, and on them alone
        assert "incidence" in got[1] and "range_error" in got[1] and "n_echoes" in got[2]
        assert "incidence" not in got[0] and "n_echoes" not in got[0] and "incidence" not in got[2]
        # a head with a return or a noise model needs the scan's index
        with pytest.raises(ValueError, match="scan_index"):
            rig.mesh(clouds)
        # a second RigDeform of the same rig takes every ray set from the first
        with RigDeform(SRC, heads, BNDS.copy(), VOXEL, share=rig) as second:
            assert second.primary.rayset is rig.primary.rayset
            assert all(a.rayset is b.rayset for a, b in zip(second.heads, rig.heads))
            assert second.heads[1].sensing.echoes.rayset is rig.heads[1].sensing.echoes.rayset
            again = second.mesh(clouds, scan_index=3)
            torch.cuda.synchronize()
            for h, g, w in zip(heads, again, got):
                _same(g, w, f"shared/{h.name}")
        rig.mesh(clouds, scan_index=3)   # (the first still owns them)
        torch.cuda.synchronize()


def test_mergemesh_sequence_with_a_rerun():
    import torch
    from lidar_transfer_amd.rig import Head, RigDeform
    heads = _approach(RIG).rig()
    # three scans: the second one's geometry is the first one's (the prediction holds), the third one's has moved (a re-run)
    scans = [_clouds(11), _clouds(11), _clouds(11, scale=0.8)]
    with RigDeform(SRC, heads, BNDS.copy(), VOXEL, mesh_volume=False) as rig, _single(heads[0], mesh_volume=False) as dd:
        fresh = [Head(h, rig.device.index) for h in heads[1:]]   # ray sets and Sensing of their own
        try:
            for i, clouds in enumerate(scans):
                got = rig.mergemesh(clouds, scan_index=i)
                torch.cuda.synchronize()
                want0 = dd.mergemesh(clouds, scan_index=i)
                torch.cuda.synchronize()
                _same(got[0], want0, f"mergemesh/roof/{i}", skip=("volume", "source"))
                _hits_and_misses(got[0], "roof")
                scene = rig.primary.scene
                st = torch.cuda.current_stream()
                for h, g in zip(fresh, got[1:]):
                    plan = h.plan(scene)
                    scene.render(h.render_set, h.origin, out=plan[2], label_image=True)
                    want = h.finish(plan, i, scene, rig.primary.mesh_obj, st)
                    torch.cuda.synchronize()
                    _hits_and_misses(g, h.name)
                    _same({k: g[k] for k in want}, want, f"mergemesh/{h.name}/{i}")
                    assert g["bin"].shape[0] > 20 and g["n_faces"] == got[0]["n_faces"]
            stats = rig.primary.mm_state.stats
            assert stats["scans"] == 3 and stats["rerun"] >= 1, stats
            # a shared head is held to the shared ray set's pose, as a DeviceDeform's shared ray set is
            assert heads[1].mount is not None and heads[2].mount is not None and heads[1].sensor is not heads[2].sensor
            with pytest.raises(ValueError, match="rig head 'side': the shared rayset was built for another sensor pose"):
                Head(heads[1], rig.device.index, share=fresh[1])
        finally:
            for h in fresh:
                h.close()


def test_field_of_view_refusal_and_cp_refusal():
    from lidar_transfer_amd.rig import RigDeform
    heads = _approach([dict(name="roof", sensor=PLAIN), dict(name="tall", sensor=TALL)]).rig()
    clouds = _clouds(11)
    with RigDeform(SRC, heads, BNDS.copy(), VOXEL) as rig:
        with pytest.raises(ValueError, match="'tall'.*widest first"):
            rig.mergemesh(clouds)
        with pytest.raises(ValueError, match="cp renders no ray"):
            rig.cp(clouds)
        assert len(rig.mesh(clouds)) == 2   # mesh has no such limit: its volume is the source sensor's
    # widest first is accepted
    with RigDeform(SRC, list(reversed(heads)), BNDS.copy(), VOXEL, mesh_volume=False) as rig:
        rig.check_mergemesh()


def test_merged_rows():
    import torch
    from lidar_transfer_amd.rig import RigDeform
    heads = _approach(RIG, rig_merged=True).rig()
    clouds = _clouds(11)
    with RigDeform(SRC, heads, BNDS.copy(), VOXEL, merged=True) as rig:
        got = rig.mesh(clouds, scan_index=1)
        torch.cuda.synchronize()
        assert got.bin is not None and got.bin.shape[0] == sum(g["bin"].shape[0] for g in got) == got.label_file.shape[0]
        at = 0
        for h, g in zip(heads, got):
            n = g["bin"].shape[0]
            rows, labels = got.bin[at:at + n].cpu().numpy(), got.label_file[at:at + n].cpu().numpy()
            at += n
            assert labels.tobytes() == g["label_file"].cpu().numpy().tobytes(), h.name
            assert rows[:, 3].tobytes() == g["bin"][:, 3].cpu().numpy().tobytes(), h.name
            # the rows are the head's hits as rendered, in the primary scan's frame: what T of the head takes into its own
            tri = g["tri"].cpu().numpy()
            scene_pts = g["endpoints_scene"].cpu().numpy()
            if h.mount is None:
                assert rows[:, :3].tobytes() == g["bin"][:, :3].cpu().numpy().tobytes(), h.name
            else:
                assert rows[:, :3].tobytes() != g["bin"][:, :3].cpu().numpy().tobytes(), h.name
                back = mc.to_frame(rows[:, :3], h.mount[0])
                assert back.tobytes() == g["bin"][:, :3].cpu().numpy().tobytes(), h.name
            assert set(map(bytes, rows[:, :3])) <= set(map(bytes, scene_pts)) and (tri >= 0).any()
        assert rig.mesh(clouds, scan_index=1, pack=False).bin is None
