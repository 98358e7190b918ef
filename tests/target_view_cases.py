"""What the target-view tests share (TEST INFRASTRUCTURE): the contract of ``lt_target_view_dev`` (include/lidarhip.h, rules
1-6) restated in numpy, the route it must equal -- ignore filter, optional transform, then the existing restatement of the
model's ``do_range_projection_new(remove=True)`` -- the target models of the tests and their seeded clouds.  The restatement
takes only the PER-POINT part (kept, row, column) from the existing restatements; filtering, the raw index and the winner
rule (ONE minimum of the 64-bit key) are its own, which is what the comparison with the sequential loops holds up."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_az_cases as baz  # noqa: E402
import beam_cases as bc  # noqa: E402
import projection_cases as pc  # noqa: E402
import sector_cases as sc  # noqa: E402
from test_evaluate_cpu import COLOR_DICT, color_lut  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT = color_lut(COLOR_DICT)                        # 354 rows; 0 is black, so are the rows no class fills (48 + 1 .. 49 ...)
IGNORE_SHORT = [0, 1, 70]                          # kernel arguments
IGNORE_LONG = [0, 1] + list(range(300, 316)) + [65535, 50]   # 20 entries: the bitmap
LABELS = np.array([0, 1, 10, 40, 48, 50, 70, 80, 252, 253, 2, 9999], np.uint32)   # 2: a black row of the LUT; 9999: beyond it
SEAM_SECTOR = (170.0, 100.0)                       # straddles the seam behind the sensor (azimuth +-180)
SIZES = ((4, 8), (32, 171))
COUNTS = (0, 1, 255, 257, 5000)


def model(H, W, fov, table=None, az=None, sector=None):
    """a target model of the tests: ``fov`` = (fov_up, fov_down) degrees, ``table`` / ``az`` degrees [H], ``sector`` (center,
    span) degrees"""
    return dict(H=int(H), W=int(W), fov=(float(fov[0]), float(fov[1])), table=None if table is None else np.asarray(table, np.float64),
                az=None if az is None else np.asarray(az, np.float64), sector=sector)


def table_of(H):
    """an H-row table with the VLP-32C's uneven spacing (its own for 32 rows, every eighth beam for 4, one beam for 1)"""
    return {32: bc.VLP32C, 4: bc.VLP32C[3::8].copy(), 1: np.array([-3.0])}[H]


def models(H, W):
    """name -> model, the six of the GPU test at image size H x W (the one-row table is 1 x W)"""
    t, fov = table_of(H), bc.VLP32C_FOV
    az = baz.offsets("mixed", H)
    return {"linear": model(H, W, (10.0, -30.0)),                       # another field of view than the source's 3 / -25
            "table": model(H, W, fov, t),
            "table_az": model(H, W, fov, t, az),
            "sector": model(H, W, (10.0, -30.0), sector=SEAM_SECTOR),
            "sector_table_az": model(H, W, fov, t, az, SEAM_SECTOR),
            "one_row": model(1, W, (2.0, -10.0), table_of(1))}


def target_model(m):
    """the ``lidar_transfer_amd.config.TargetModel`` of a model"""
    from lidar_transfer_amd.config import TargetModel
    return TargetModel(m["table"], m["sector"], m["az"], "tests")


def mounting():
    """T of config/approach_mount_example.yaml, float64 [4, 4] (x_target = T x_source)"""
    from lidar_transfer_amd.config import load_approach
    return np.ascontiguousarray(load_approach(os.path.join(ROOT, "config", "approach_mount_example.yaml")).mount()[0], np.float64)


def cloud(n, seed, sector=None, nan=True):
    """(xyzr [n, 4] f32, label [n] u32), seeded.  Directions over the whole sphere band from -40 to +30 degrees and the full
    circle (so: outside any sector, outside every beam's keep window, above and below every field of view), ranges 0.5 .. 60 m.
    From 64 points on, in file order scattered: exact copies of earlier points with another label and remission (depth ties),
    copies moved by one float32 ulp in x (the same float32 depth bucket, another float64 depth), depth-0 points and
    (``nan``) NaNs.  Labels carry instance ids in their upper half and include values beyond the LUT."""
    rng = np.random.default_rng(seed)
    az = rng.uniform(-np.pi, np.pi, n)
    if sector is not None and n:                    # two thirds inside the sector, to fill its cells
        c, s = np.radians(sector[0]), np.radians(sector[1])
        inside = rng.random(n) < 0.67
        az = np.where(inside, c + rng.uniform(-0.5, 0.5, n) * s, az)
    el = np.radians(rng.uniform(-40.0, 30.0, n))
    r = rng.uniform(0.5, 60.0, n)
    xyzr = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rng.random(n)], 1).astype(np.float32)
    label = (rng.choice(LABELS, n) | (rng.integers(0, 4000, n).astype(np.uint32) << 16)).astype(np.uint32)
    if n >= 64:
        k = n // 16
        who = rng.permutation(n)
        src, dup, ulp, zero, bad = who[:k], who[k:2 * k], who[2 * k:3 * k], who[3 * k:3 * k + 4], who[3 * k + 4:3 * k + 8]
        xyzr[dup, :3] = xyzr[src, :3]
        half = len(ulp) // 2
        xyzr[ulp, :3] = xyzr[src, :3]
        xyzr[ulp[:half], 0] = np.nextafter(xyzr[ulp[:half], 0], np.float32(np.inf))
        xyzr[ulp[half:], 0] = np.nextafter(xyzr[ulp[half:], 0], np.float32(-np.inf))
        xyzr[zero, :3] = 0
        xyzr[zero[0], 2] = -0.0
        if nan:
            xyzr[bad[:2], 1] = np.nan
            xyzr[bad[2:], :3] = np.nan
    return np.ascontiguousarray(xyzr), label


def widen(xyzr, T=None):
    """rule 3: float64 [n, 3]; with T every row as ((m0*x + m1*y) + m2*z) + m3, each operation rounded on its own"""
    p = np.asarray(xyzr, np.float32)[:, :3].astype(np.float64)
    if T is None:
        return p
    T = np.asarray(T, np.float64).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(3)], 1)


def _existing(pts, rem, lab, m):
    """the existing restatement of the model's projection (new=True, remove=True, no beam angles) on a float64 cloud"""
    H, W, fov = m["H"], m["W"], m["fov"]
    with np.errstate(all="ignore"):
        if m["az"] is not None:
            return baz.project(pts, rem, lab, m["table"], fov, m["az"], W, m["sector"])
        if m["sector"] is not None:
            return sc.project(pts, rem, lab, m["sector"], W, H, fov, m["table"])
        if m["table"] is not None:
            return bc.project(pts, rem, lab, m["table"], fov, W)
        return pc.restate(pts, rem, lab, H, W, fov[0], fov[1], None, True, True)


def per_point(pts, m):
    """rule 4 for every point: (bids [n] bool, cell [n] int64, depth [n] f64) by the model's existing per-point restatement"""
    H, W, fov = m["H"], m["W"], m["fov"]
    if len(pts) == 0:
        return np.zeros(0, bool), np.zeros(0, np.int64), np.zeros(0)
    with np.errstate(all="ignore"):
        depth = np.sqrt((pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2])
    if m["table"] is None and m["sector"] is None:
        p = pc.project_points(pts, H, W, fov[0], fov[1], None, True, True)
        return p["keep"], p["py"].astype(np.int64) * W + p["px"], depth
    r = _existing(pts, None, None, m)
    return r["kept"], r["row"].astype(np.int64) * W + r["col"], depth


def restate_view(xyzr, label, ignore, T, m, lut):
    """rules 1-6: dict(range, rem, label, black [H, W], bad_labels, index [H, W] (raw index of the winner, -1 empty))"""
    H, W = m["H"], m["W"]
    n = len(label)
    l = (np.asarray(label, np.uint32) & 0xFFFF).astype(np.int64)                      # rule 1
    bad = int((l >= len(lut)).sum())
    dropped = np.isin(l, ignore)                                                      # rule 2
    pts = widen(xyzr, T)                                                              # rule 3
    keep, cell, depth = per_point(pts, m)                                             # rule 4
    bids = keep & ~dropped
    i = np.arange(n, dtype=np.uint64)                                                 # rule 5: ONE minimum of the key
    with np.errstate(all="ignore"):
        df = depth.astype(np.float32)
    up = depth < df.astype(np.float64)
    lo = np.where(up, np.uint64(0x7fffffff) - i, np.uint64(0x80000000) | i)
    key = (df.view(np.uint32).astype(np.uint64) << np.uint64(32)) | lo
    best = np.full(H * W, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    np.minimum.at(best, cell[bids], key[bids])
    has = best != np.uint64(0xFFFFFFFFFFFFFFFF)
    low = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    index = np.where(has, np.where(low & 0x80000000, low & 0x7fffffff, 0x7fffffff - low), -1)
    rng = np.where(has, (best >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(-1)).astype(np.float32)   # rule 6
    win = np.where(has, index, 0)
    if n:
        rem = np.where(has, np.asarray(xyzr, np.float32)[win, 3], np.float32(-1)).astype(np.float32)
        lab = np.where(has, l[win], 0).astype(np.int32)
    else:
        rem, lab = np.full(H * W, -1, np.float32), np.zeros(H * W, np.int32)
    col = np.zeros((H * W, 3), np.float64)
    inside = has & (lab < len(lut))
    col[inside] = np.asarray(lut)[lab[inside]]
    black = (((col[:, 0] + col[:, 1]) + col[:, 2]) == 0).astype(np.uint8)
    return dict(range=rng.reshape(H, W), rem=rem.reshape(H, W), label=lab.reshape(H, W), black=black.reshape(H, W),
                bad_labels=bad, index=index.reshape(H, W))


def composed_view(xyzr, label, ignore, T, m):
    """the route the view must equal: ignore filter -> optional transform -> the existing restatement with its sequential
    loop.  dict(range, rem, label [H, W], has [H, W] bool, index [H, W] raw index of the winner)"""
    H, W = m["H"], m["W"]
    l = (np.asarray(label, np.uint32) & 0xFFFF)
    kept_raw = np.flatnonzero(~np.isin(l, ignore))
    x = np.asarray(xyzr, np.float32)[kept_raw]
    pts = widen(x, T)
    r = _existing(pts, x[:, 3].copy(), l[kept_raw].astype(np.int32), m)
    idx = np.asarray(r["idx"]).reshape(H, W)                          # numbering of the points the projection kept
    proj_kept = np.flatnonzero(r["kept"])
    has = idx >= 0
    index = np.where(has, kept_raw[proj_kept[np.where(has, idx, 0)]] if len(proj_kept) else 0, -1)
    return dict(range=np.asarray(r["range"], np.float32).reshape(H, W), rem=np.asarray(r["rem"], np.float32).reshape(H, W),
                label=np.asarray(r["label"], np.int32).reshape(H, W), has=has, index=index)
