"""What the mount tests share (TEST INFRASTRUCTURE): the poses, the scene of the render-at-a-pose test, and the host
restatements of the two arithmetic contracts -- posed rays and the frame transform -- in the operation order the issue fixes.
Nothing here imports ``lidar_transfer_amd`` for arithmetic."""
from __future__ import annotations

import numpy as np


def rot_zyx(yaw_deg, pitch_deg, roll_deg):
    """R = Rz(yaw) . Ry(pitch) . Rx(roll), float64; a positive pitch turns the x axis DOWN (towards -z)"""
    y, p, r = np.radians([yaw_deg, pitch_deg, roll_deg])
    rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    return rz @ ry @ rx


def pose(R, t):
    P = np.eye(4)
    P[:3, :3] = R
    P[:3, 3] = t
    return P


def transformation_of(P):
    """the approach file's 16 numbers for a target sensor standing at pose ``P`` in the source frame: T = inv(P)"""
    T = np.eye(4)
    T[:3, :3] = P[:3, :3].T
    T[:3, 3] = -(P[:3, :3].T @ P[:3, 3])
    return [float(x) for x in T.reshape(-1)]


#: the pose of config/approach_mount_example.yaml: 0.4 m lower, pitched 5 degrees down
POSE_EXAMPLE = pose(rot_zyx(0.0, 5.0, 0.0), [0.0, 0.0, -0.4])
#: a general one: every angle, every offset
POSE_GENERAL = pose(rot_zyx(31.0, -3.5, 2.25), [0.55, -0.35, 0.2])

# ---- the scene of the render-at-a-pose test (tests/test_mount_cpu.py chooses them, tests/test_mount_gpu.py renders them) ----
RENDER_SEED, RENDER_TRIS, RENDER_H, RENDER_W, RENDER_FOV = 0, 200000, 64, 1024, (3.0, -25.0)
RENDER_POSES = (("example", POSE_EXAMPLE), ("general", POSE_GENERAL))
#: rays at which the compiled reference may differ from the brute-force minimum: 1e-4 of the rays (tests/test_trace_gpu.py:82-84)
REF_CULL_CAP = 1e-4


def rays_f64(fov_up, fov_down, H, W):
    """the three float64 components of ``create_rays`` (laserscan.py:1092-1119) BEFORE its cast, [H*W, 3]"""
    yaw = np.linspace(0, 360, W) + 180
    yaw[yaw > 360] -= 360
    yaw = yaw / 180.0 * np.pi
    pitch = np.pi / 2 - np.linspace(fov_up, fov_down, H) / 180.0 * np.pi
    sp, cp = np.sin(pitch), np.cos(pitch)
    out = np.empty((H, W, 3), np.float64)
    out[:, :, 0] = sp[:, None] * np.cos(-yaw)[None, :]
    out[:, :, 1] = sp[:, None] * np.sin(-yaw)[None, :]
    out[:, :, 2] = cp[:, None] * np.ones(W)[None, :]
    return out.reshape(H * W, 3)


def posed_rays(fov_up, fov_down, H, W, rot):
    """``Rp . d`` as the issue fixes it: ((r0 * x + r1 * y) + r2 * z) per component in float64 -- numpy rounds every
    elementwise product and sum on its own --, cast to float32 last"""
    d = rays_f64(fov_up, fov_down, H, W)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    r = np.asarray(rot, np.float64)
    out = np.stack([(r[k, 0] * x + r[k, 1] * y) + r[k, 2] * z for k in range(3)], 1)
    return np.ascontiguousarray(out.astype(np.float32))


def to_frame(points, T, tri=None):
    """float32 points widened to float64, ((m0 * x + m1 * y) + m2 * z) + m3 per row of ``T``, rounded to float32; rows with
    ``tri < 0`` are copied as they are"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    m = np.asarray(T, np.float64).reshape(4, 4)
    with np.errstate(over="ignore", invalid="ignore"):
        out = np.stack([((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)], 1).astype(np.float32)
    if tri is not None:
        miss = np.asarray(tri).reshape(-1) < 0
        out[miss] = p[miss]
    return out


def origin_of(P):
    return np.asarray(P, np.float64)[:3, 3].astype(np.float32)
