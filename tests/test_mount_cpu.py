"""The target sensor at a pose of its own, host side: ``Approach.mount()`` and the choice of the scene and poses that
tests/test_mount_gpu.py renders (the compiled reference raytracer alone must stay within its known culling slack on them)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mount_common as mc  # noqa: E402

IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]


def _approach(transformation):
    from lidar_transfer_amd.config import Approach
    return Approach(adaption="mergemesh", preserve_float=False, voxel_size=0.1, voxel_bounds=np.zeros((3, 2)), number_of_scans=1,
                    ignore=[], moving=[], transformation=transformation, batch_interval=1, color_map={}, labels={})


def test_mount_is_none_for_the_identity_and_the_inverse_pose_otherwise():
    for t in ([], None, IDENTITY, [float(x) for x in IDENTITY], np.eye(4)):
        assert _approach(t).mount() is None
    for _, P in mc.RENDER_POSES:
        t = mc.transformation_of(P)
        T, Pm = _approach(t).mount()
        assert T.dtype == Pm.dtype == np.float64 and T.shape == Pm.shape == (4, 4)
        assert np.array_equal(T, np.array(t).reshape(4, 4))
        assert np.array_equal(Pm, np.linalg.inv(T))
        assert np.allclose(Pm, P, rtol=0, atol=1e-12)
    # a pure translation is a mounting too
    T, Pm = _approach([1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, -0.25, 0, 0, 0, 1]).mount()
    assert np.array_equal(Pm[:3, 3], [-0.5, 0.0, 0.25]) and np.array_equal(Pm[:3, :3], np.eye(3))


def test_mount_refuses_what_is_not_a_rigid_motion():
    good = mc.transformation_of(mc.POSE_GENERAL)
    sheared = list(good)
    sheared[1] += 1e-3
    scaled = [x * (1.001 if k % 4 < 3 and k < 12 else 1.0) for k, x in enumerate(good)]
    reflection = [1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    bad_row = list(good)
    bad_row[12] = 0.1
    bad_w = list(good)
    bad_w[15] = 2.0
    for name, t in (("15 numbers", good[:15]), ("17 numbers", good + [0.0]), ("sheared", sheared), ("scaled", scaled),
                    ("reflection", reflection), ("last row", bad_row), ("last element", bad_w),
                    ("nan", [float("nan")] + good[1:])):
        with pytest.raises(ValueError):
            _approach(t).mount()
            pytest.fail(f"{name} was accepted")
    # inside the tolerance: the 16 numbers of a YAML written with seven decimals
    T, _ = _approach([round(x, 7) for x in good]).mount()
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() <= 1e-6


def test_the_example_approach_file_is_the_pose_it_says():
    from lidar_transfer_amd.config import load_approach
    a = load_approach(os.path.join(os.path.dirname(HERE), "config", "approach_mount_example.yaml"))
    assert a.adaption == "mergemesh"
    T, P = a.mount()
    assert np.allclose(P, mc.POSE_EXAMPLE, rtol=0, atol=1e-9)
    assert np.allclose(P[:3, 3], [0, 0, -0.4]) and P[2, 0] < 0      # 0.4 m lower; its x axis points down
    assert abs(np.degrees(np.arcsin(-P[2, 0])) - 5.0) < 1e-6
    # the shipped default stays the identity
    assert load_approach(os.path.join(os.path.dirname(HERE), "config", "approach_mergemesh.yaml")).mount() is None


def test_restated_frame_transform_is_the_matrix_product():
    rng = np.random.default_rng(3)
    p = rng.normal(size=(1000, 3)).astype(np.float32) * 20
    T = np.array(mc.transformation_of(mc.POSE_GENERAL)).reshape(4, 4)
    want = (T[:3, :3] @ p.astype(np.float64).T).T + T[:3, 3]
    got = mc.to_frame(p, T)
    assert got.dtype == np.float32 and np.abs(got - want).max() < 1e-5
    tri = np.where(np.arange(1000) % 3 == 0, -1, 5)
    got = mc.to_frame(p, T, tri)
    assert np.array_equal(got[tri < 0], p[tri < 0]) and not np.array_equal(got[tri >= 0], p[tri >= 0])
    r = mc.posed_rays(3, -25, 8, 16, np.eye(3))
    assert np.array_equal(r, mc.rays_f64(3, -25, 8, 16).astype(np.float32))


# Observed where they were chosen (compiled reference against MODE_BRUTE, both with the host's own RSQRTSS seed, 65 536 rays;
# the cap is 6 rays = 1e-4 of them, rounded down), on an Intel host and again on the AMD host of the GPU machine, where
# tests/test_mount_gpu.py counts them once more on the product's own rays:
#   "example"  0 rays differ, 64 554 rays hit
#   "general"  0 rays differ, 65 145 rays hit
REF_DIFFERS = {"example": 0, "general": 0}


def test_the_compiled_reference_alone_stays_within_its_culling_slack_on_the_chosen_scene_and_poses(oracle, capfd):
    """The condition on the INPUTS of the render-at-a-pose test: for its scene and both poses the compiled reference
    raytracer differs from the brute-force minimum -- its unpadded slab test can cull a hit an ulp closer,
    tests/test_trace_gpu.py:82-84 -- at no more than 1e-4 of the rays.  CPU only; rays from the host restatement."""
    from lidar_transfer_amd.synth import synth_scene
    if not oracle.ref_available("strict"):
        pytest.skip("oracle/_ref not built (the reference checkout was absent at build time)")
    v, f, c, r = synth_scene(mc.RENDER_SEED, mc.RENDER_TRIS)
    assert f.shape[0] >= 200000
    H, W = mc.RENDER_H, mc.RENDER_W
    seen = {}
    for name, P in mc.RENDER_POSES:
        rays = mc.posed_rays(mc.RENDER_FOV[0], mc.RENDER_FOV[1], H, W, P[:3, :3])
        org = mc.origin_of(P)
        ref = oracle.ref_trace(rays, org, v, f, c, r, H, kind="strict")
        capfd.readouterr()  # the reference printf()s
        brute = oracle.oracle_trace(rays, org, v, f, c, r, H, mode=oracle.MODE_BRUTE, norm=oracle.NORM_SSE, nthreads=16)
        differs = np.zeros(H * W, bool)
        for k in ("range", "endrem", "endpoints", "endcolors"):
            a, b = np.ascontiguousarray(ref[k]).view(np.int32), np.ascontiguousarray(brute[k]).view(np.int32)
            differs |= (a != b).reshape(H * W, -1).any(1)
        n = int(differs.sum())
        seen[name] = (n, int((brute["tri"] >= 0).sum()))
        assert n <= mc.REF_CULL_CAP * H * W, (name, n)
        assert (brute["tri"] >= 0).sum() > 0.5 * H * W, f"{name}: the pose looks past the scene"
    print(f"\nthe compiled reference differs from MODE_BRUTE at (rays, of hits) {seen} of {H * W} rays; when chosen: {REF_DIFFERS}")
