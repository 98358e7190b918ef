"""What the beam-azimuth tests share (TEST INFRASTRUCTURE): the offset sets, and host restatements of the three arithmetic
contracts of a beam-table target whose beams carry azimuth offsets (``beam_azimuth_offsets``) -- its rays, the
column of a projected point with the reference's sequential z-min loop, and the reverse projection -- in the operation order
the contracts fix.  Nothing here imports ``lidar_transfer_amd`` for arithmetic; the row rule of a beam table is
tests/beam_cases.py's, the sector's column rule tests/sector_cases.py's."""
from __future__ import annotations

import numpy as np

import beam_cases as bc
import sector_cases as sc

#: the sector of these tests: it straddles the seam behind the sensor
SEAM_SECTOR = (170.0, 100.0)
NEAR_CAP = 1e-3
#: (n, dtype) of the GPU projection test's clouds
CLOUDS = tuple((n, dt) for n in (1, 2, 65, 20000) for dt in (np.float32, np.float64))
#: (n, dtype, seed) of the first cloud of its two-cloud batch (the second is the 20000-point float32 cloud above)
BATCH_CLOUD = (257, np.float32, 3)
#: (name, table, (fov_up, fov_down), W) of the sensors: the table's H == 1 keep rule, two rows, the VLP-32C
SENSORS = (("1x1", bc.TINY[0][1], bc.TINY[0][2], 1), ("2x3", bc.TINY[1][1], bc.TINY[1][2], 3), ("32x171", bc.VLP32C, bc.VLP32C_FOV, 171))


def offsets(kind, H):
    """The two offset sets, degrees, float64 [H] in the table's row order.  ``mixed``: the VLP-32C's four published values
    with exact zeros between them.  ``ninety``: the same with a +90 row first and a -90 row last (H == 1: the one row -90)."""
    a = np.resize(np.array([1.4, 0.0, -4.2, -1.4, 0.0, 4.2]), H).astype(np.float64)
    if kind == "ninety":
        a[0], a[-1] = 90.0, -90.0
    elif kind != "mixed":
        raise ValueError(kind)
    return a


def nominal_deg(W, sector=None):
    """the nominal yaw of every column in degrees, float64 [W]: ``create_rays``' full circle (laserscan.py:1100-1102) or the
    centre of the sector's cell"""
    if sector is not None:
        return sc.yaw_deg(sector, W)
    yaw = np.linspace(0, 360, W) + 180
    yaw[yaw > 360] -= 360
    return yaw


def rays_f64(table, az, W, sector=None):
    """the three float64 components of the rays BEFORE the cast, [H*W, 3]: yaw_deg = nominal(w) - az[h], no further wrap,
    then ``create_rays``' expressions with the table's angle of row h"""
    yaw = (nominal_deg(W, sector)[None, :] - np.asarray(az, np.float64)[:, None]) / 180. * np.pi
    pitch = np.pi / 2 - np.asarray(table, np.float64) / 180. * np.pi
    sp, cp = np.sin(pitch), np.cos(pitch)
    out = np.empty((len(pitch), W, 3), np.float64)
    out[:, :, 0] = sp[:, None] * np.cos(-yaw)
    out[:, :, 1] = sp[:, None] * np.sin(-yaw)
    out[:, :, 2] = cp[:, None] * np.ones(W)[None, :]
    return out.reshape(-1, 3)


def turned(d, rot):
    """float64 directions turned as ((r0 * x + r1 * y) + r2 * z) per component"""
    if rot is None:
        return d
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    r = np.asarray(rot, np.float64)
    return np.stack([(r[k, 0] * x + r[k, 1] * y) + r[k, 2] * z for k in range(3)], 1)


def az_rays(table, az, W, sector=None, rot=None):
    """the rays, float32 [H*W, 3]: one cast, after the rotation when there is one"""
    return np.ascontiguousarray(turned(rays_f64(table, az, W, sector), rot).astype(np.float32))


def columns(points, row, az, W, sector=None):
    """The column contract in the cloud's dtype T, constants rounded to T once: a = T(az[row] / 180 * pi); the nominal yaw
    y' = -atan2(y, x) + a (the yaw float32: through double, rounded once).  Full circle: one wrap back into [-pi, pi], only
    when strictly outside; px = 0.5 * (y' / pi + 1) * W; column = floor(px) clamped; every point is inside.  Sector: d = y' -
    yc, then tests/sector_cases.py's wrap, u, inside and column.  ``near`` and ``slack`` as in ``sector_cases.columns``: px
    within 4 ulp of an integer (u of 0 or 1), the ulp of the yaw scaled by W / span included, span = 2 pi on the full circle.
    The ulp of the yaw is taken where the yaw is largest on its way -- of -atan2 or of the unwrapped sum, whichever is the
    larger: both roundings go into y', and after the wrap y' may be much smaller than either."""
    pts = np.asarray(points)
    T = pts.dtype.type
    pi_t, twopi_t = T(np.pi), T(2) * T(np.pi)
    a = (np.asarray(az, np.float64) / 180. * np.pi)[np.asarray(row)].astype(pts.dtype)
    with np.errstate(all="ignore"):
        yaw0 = -np.arctan2(pts[:, 1].astype(np.float64), pts[:, 0].astype(np.float64)).astype(pts.dtype)
        yaw = yaw0 + a
        yulp = np.spacing(np.maximum(np.abs(yaw0), np.abs(yaw))).astype(np.float64)
        if sector is None:
            yaw = np.where(yaw > pi_t, yaw - twopi_t, np.where(yaw < -pi_t, yaw + twopi_t, yaw))
            px = T(0.5) * (yaw / pi_t + T(1.0))
            px = px * T(W)
            inside = np.ones(len(pts), bool)
            span = 2 * np.pi
            edge = np.zeros(len(pts), bool)
        else:
            c, s = float(sector[0]), float(sector[1])
            yc, span_t = T(-c / 180. * np.pi), T(s / 180. * np.pi)
            d = yaw - yc
            d = np.where(d < -pi_t, d + twopi_t, d)
            d = np.where(d >= pi_t, d - twopi_t, d)
            u = d / span_t + T(0.5)
            inside = (u >= 0) & (u < 1)
            px = u * T(W)
            span = float(span_t)
        col = np.maximum(0, np.minimum(W - 1, np.floor(px)))
        col = np.where(np.isnan(col), W - 1, col).astype(np.int32)
        slack = 4 * np.spacing(np.abs(px)).astype(np.float64) + 4 * yulp * (W / span)
        pxd = px.astype(np.float64)
        if sector is not None:
            ud = u.astype(np.float64)
            edge = (np.abs(ud) * W <= slack) | (np.abs(ud - 1) * W <= slack)
        near = ((np.abs(pxd - np.round(pxd)) <= slack) & inside) | edge
        near &= ~np.isnan(pxd)
    return dict(yaw=yaw, px=px.astype(pts.dtype), col=col, inside=inside, near=near, slack=slack)


def project(points, rem, label, table, fov, az, W, sector=None):
    """``do_range_projection_new(remove=True)`` + ``do_label_projection_new`` (laserscan.py:294-391, :672-676) for a table
    sensor with azimuth offsets: the row and the keep rule by tests/beam_cases.py, the column (and, in a sector, the extra
    keep condition) by :func:`columns` from the point's row, then the literal sequential loop of :372-382.  The result has
    ``tests/sector_cases.project``'s keys (an empty cell holds 0 in the four coordinate images, as with any table)."""
    pts = np.asarray(points)
    T = pts.dtype.type
    H = len(table)
    full = bc.project(pts, None, None, table, fov, W)              # rows and their keep rule; its columns are not used
    ok, row, near_row, yf = full["kept"], full["row"].astype(np.int32), full["near"], full["pitch"]
    cl = columns(pts, row, az, W, sector)
    with np.errstate(all="ignore"):
        depth = np.sqrt((pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2])
    kept = ok & cl["inside"]
    near = (cl["near"] | near_row) & ok
    col = cl["col"]
    kd, kc, kr, kxf, kyf, ksl = depth[kept], col[kept], row[kept], cl["px"][kept], yf[kept], cl["slack"][kept]
    krem = np.asarray(rem)[kept] if rem is not None else None
    klab = np.asarray(label)[kept] if label is not None else None
    index = np.full((H, W), -1, np.int32)
    range_image = np.full((H, W), 0, np.float32)
    rem_image = np.full((H, W), -1, np.float32)
    for i in range(len(kd)):                                   # laserscan.py:373-382
        y, x = kr[i], kc[i]
        if kd[i] < range_image[y, x] or index[y, x] == -1:
            range_image[y, x] = kd[i]
            index[y, x] = i
            if krem is not None:
                rem_image[y, x] = krem[i]
    n = len(kd)
    has = index >= 0
    win = np.where(has, index, 0)
    pick = lambda a, zero: np.where(has, a[win], zero) if n else np.full((H, W), zero, a.dtype)   # noqa: E731
    lab_image = pick(klab.astype(np.int32), np.int32(0)) if klab is not None else np.zeros((H, W), np.int32)
    return dict(idx=index, range=range_image, rem=rem_image, label=lab_image.astype(np.int32),
                proj_x=pick(kc, np.int32(0)).astype(np.int32), proj_y=pick(kr, np.int32(0)).astype(np.int32),
                proj_xf=pick(kxf, T(0)).astype(pts.dtype), proj_yf=pick(kyf, T(0)).astype(pts.dtype),
                xf_slack=pick(ksl, np.float64(0)), kept=kept, near=near, row=row, col=col, inside=cl["inside"])


def reverse_projection(range_image, proj_x, proj_y_or_pitch, table, az, preserve_float, sector=None):
    """float64 [H*W, 3]: the nominal yaw -- (px / W * 2 - 1) * pi, or the sector's yc + ((px + 0.5) / W - 0.5) * span
    (``preserve_float``: (xf / W - 0.5)) -- minus az_rad[row]; the row is proj_y clamped to the table (int32 coordinates) or
    the cell's own row (``preserve_float``, where the second image holds the pitch); the elevation the table's angle of
    proj_y or the pitch image; the three products left to right"""
    depth = np.asarray(range_image)
    H, W = depth.shape
    Brad = bc.rows_of(table)[0]
    az_rad = np.asarray(az, np.float64) / 180. * np.pi
    px = np.asarray(proj_x, np.float64)
    if sector is None:
        yaw = (px / W * 2 - 1.0) * np.pi
    else:
        yc, span = -float(sector[0]) / 180. * np.pi, float(sector[1]) / 180. * np.pi
        x = px / W if preserve_float else (px + 0.5) / W
        yaw = yc + (x - 0.5) * span
    if preserve_float:
        row = np.repeat(np.arange(H), W).reshape(H, W)
        e = np.asarray(proj_y_or_pitch, np.float64)
    else:
        row = np.clip(np.asarray(proj_y_or_pitch), 0, H - 1)
        e = Brad[row]
    yaw = yaw - az_rad[row]
    pitch = np.pi / 2 - e
    X = depth * np.sin(pitch) * np.cos(-yaw)
    Y = depth * np.sin(pitch) * np.sin(-yaw)
    Z = depth * np.cos(pitch)
    return np.stack([X, Y, Z], 2).reshape(-1, 3)


def seeded_cloud(table, fov, az, n, dtype, seed, sector=None):
    """tests/beam_cases.py's seeded cloud (full circle, from 1000 points on) or tests/sector_cases.py's, and from 65 points on a chosen
    point in its last row, ON a beam whose offset differs from its lower neighbour's.  Full circle, ``seam``: its own
    offset carries the point across the +-pi seam (|y'| > pi before the wrap).  Sector, ``edge``: inside the sector by its
    own row's offset, outside by the neighbour's.  Returns (points, rem, label, special) -- ``special``: name -> (index,
    row)."""
    if sector is None and n < 1000:                               # (the chosen rows of tests/beam_cases.py lie ON row boundaries: a
        pts, rem, lab = sc.seeded_cloud(SEAM_SECTOR, fov, n, dtype, seed)   # small cloud has no room for them under the cap)
    elif sector is None:
        pts, rem, lab = bc.seeded_cloud(table, fov, n, dtype, seed)
    else:
        pts, rem, lab = sc.seeded_cloud(sector, fov, n, dtype, seed)
    special = {}
    H = len(table)
    if n < 65 or H < 2:
        return pts, rem, lab, special
    Brad = bc.rows_of(table)[0]
    a = np.asarray(az, np.float64) / 180. * np.pi
    r = next(k for k in range(H - 1) if a[k] != a[k + 1] and a[k] != 0.0)
    if sector is None:                                            # y' = yaw0 + a[r] leaves [-pi, pi] by |a[r]| / 2
        yaw0 = np.sign(a[r]) * (np.pi - abs(a[r]) / 2)
        special["seam"] = (n - 1, r)
    else:                                                         # the edge lies midway between the two nominal yaws
        yc, span = -np.radians(sector[0]), np.radians(sector[1])
        lo, hi = min(a[r], a[r + 1]), max(a[r], a[r + 1])
        edge = yc + span / 2 if a[r] == lo else yc - span / 2     # the smaller sum stays inside at the right edge
        yaw0 = edge - (lo + hi) / 2
        special["edge"] = (n - 1, r)
    phi, el = -yaw0, Brad[r]
    pts[n - 1] = np.array([7.5 * np.cos(el) * np.cos(phi), 7.5 * np.cos(el) * np.sin(phi), 7.5 * np.sin(el)]).astype(dtype)
    return pts, rem, lab, special


def cloud_seed(si, n, sector):
    """the seeds of the GPU projection test's clouds (chosen in tests/test_beam_az_cpu.py: at most NEAR_CAP near a boundary)"""
    return 2000 * si + n % 997 + (500 if sector is not None else 0)
