"""What the beam-table tests share (TEST INFRASTRUCTURE): the two tables, and float64 host restatements of the three
arithmetic contracts of a target sensor with a beam table -- its rays, the row and keep rule of a projected point with the
reference's sequential z-min loop, and the reverse projection -- in the operation order the contracts fix.  Nothing here
imports ``lidar_transfer_amd`` for arithmetic."""
from __future__ import annotations

import numpy as np

#: Velodyne VLP-32C: 22 of the 32 beams within +-4 degrees at 0.333 degree steps, the rest out to +15 / -25 (config/vlp32c_table_1024.yaml)
VLP32C = np.array([15.0, 10.333, 7.0, 4.667, 3.333, 2.333, 1.667, 1.333, 1.0, 0.667, 0.333, 0.0,
                   -0.333, -0.667, -1.0, -1.333, -1.667, -2.0, -2.333, -2.667, -3.0, -3.333, -3.667, -4.0,
                   -4.667, -5.333, -6.148, -7.254, -8.843, -11.31, -15.639, -25.0], np.float64)
VLP32C_FOV = (15.0, -25.0)
#: two blocks of 32 beams with different spacing (the HDL-64E's construction)
TWO_BLOCK = np.array([2.0 - k / 3 for k in range(32)] + [-8.83 - 0.5 * k for k in range(32)], np.float64)
TWO_BLOCK_FOV = (2.0, -24.8)
#: (name, table, (fov_up, fov_down), W of the render cases)
TABLES = (("vlp32c", VLP32C, VLP32C_FOV, 1024), ("two_block", TWO_BLOCK, TWO_BLOCK_FOV, 512))
#: H = 1 and H = 2 sensors of the row tests
TINY = (("h1", np.array([-3.0]), (2.0, -10.0)), ("h2", np.array([1.5, -2.25]), (3.0, -5.0)))


def rays_f64(table, W):
    """the three float64 components of the table's rays BEFORE the cast, [H*W, 3]: ``create_rays``' expressions
    (laserscan.py:1092-1119) with the table's angle of row h in place of the ``linspace`` term"""
    yaw = np.linspace(0, 360, W) + 180
    yaw[yaw > 360] -= 360
    yaw = yaw / 180. * np.pi
    pitch = np.pi / 2 - np.asarray(table, np.float64) / 180. * np.pi
    sp, cp = np.sin(pitch), np.cos(pitch)
    out = np.empty((len(pitch), W, 3), np.float64)
    out[:, :, 0] = sp[:, None] * np.cos(-yaw)[None, :]
    out[:, :, 1] = sp[:, None] * np.sin(-yaw)[None, :]
    out[:, :, 2] = cp[:, None] * np.ones(W)[None, :]
    return out.reshape(-1, 3)


def table_rays(table, W, rot=None):
    """the table's rays, float32 [H*W, 3]; with ``rot`` turned in float64 as ((r0 * x + r1 * y) + r2 * z) per component
    before the one cast"""
    d = rays_f64(table, W)
    if rot is not None:
        x, y, z = d[:, 0], d[:, 1], d[:, 2]
        r = np.asarray(rot, np.float64)
        d = np.stack([(r[k, 0] * x + r[k, 1] * y) + r[k, 2] * z for k in range(3)], 1)
    return np.ascontiguousarray(d.astype(np.float32))


def rows_of(table):
    """``Brad = B / 180 * pi`` and ``halfw[k]``: half the smaller gap to the two neighbours in radians, the one existing gap
    for the first and the last row (zeros for H = 1, where it is not used)"""
    Brad = np.asarray(table, np.float64) / 180.0 * np.pi
    H = len(Brad)
    halfw = np.zeros(H)
    for k in range(H):
        gaps = []
        if k > 0:
            gaps.append(Brad[k - 1] - Brad[k])
        if k < H - 1:
            gaps.append(Brad[k] - Brad[k + 1])
        if gaps:
            halfw[k] = min(gaps) / 2
    return Brad, halfw


def argmin_rows(q, Brad):
    """the row of every pitch: the first minimum of |q - Brad[k]|"""
    q = np.asarray(q, np.float64)
    out = np.empty(len(q), np.int64)
    for a in range(0, len(q), 1 << 16):
        out[a:a + (1 << 16)] = np.argmin(np.abs(q[a:a + (1 << 16), None] - Brad[None, :]), 1)
    return out


def search_rows(q, Brad):
    """the same row by a binary search over the descending table and one comparison of the bracketing pair"""
    q = np.asarray(q, np.float64)
    H = len(Brad)
    lo = np.searchsorted(-Brad, -q, side="left")      # the first k with Brad[k] <= q (H: none)
    a, b = np.clip(lo - 1, 0, H - 1), np.clip(lo, 0, H - 1)
    return np.where(np.abs(q - Brad[b]) < np.abs(q - Brad[a]), b, a).astype(np.int64)


def asin_cr(x):
    """float64 ``arcsin``, correctly rounded: numpy's float64 loop and a C library's differ in the last place in one argument
    of ten, so neither is THE pitch of a float64 point.  Long double first (64 bits of mantissa, an ulp of its own at most off);
    where that lies too close to the middle between two doubles to tell which is nearer, 200-bit arithmetic decides."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        if np.finfo(np.longdouble).nmant < 63:
            risky = np.isfinite(x) & (np.abs(x) <= 1)
            out = np.arcsin(x)
        else:
            ld = np.arcsin(x.astype(np.longdouble))
            out = ld.astype(np.float64)
            off = np.abs(np.abs(ld - out.astype(np.longdouble)) - (np.spacing(np.abs(out)) / 2).astype(np.longdouble))
            risky = np.isfinite(out) & (off <= 8 * np.spacing(np.abs(ld)))
    idx = np.nonzero(risky)[0]
    if idx.size:
        import mpmath
        with mpmath.workprec(200):
            for i in idx:
                out[i] = float(mpmath.asin(mpmath.mpf(float(x[i]))))
    return out


def project(points, rem, label, table, fov, W):
    """``do_range_projection_new(remove=True)`` + ``do_label_projection_new`` (laserscan.py:294-391, :672-676) for a sensor
    with a beam table: the column as there, in the cloud's dtype; the pitch in the cloud's dtype, widened to float64; the row
    its nearest beam (argmin); kept iff within ``halfw`` of that beam (H = 1: iff inside the field of view); then the literal
    sequential loop of :372-382.  Returns the images (``idx``: numbering of the kept points; ``proj_x`` / ``proj_y`` /
    ``proj_xf`` / ``proj_yf`` of the winner, 0 in empty cells), ``kept`` (mask over the input) and ``near`` (mask over the
    input: kept or not, the point lies within 4 ulp of its pitch of a row or keep boundary)."""
    pts = np.asarray(points)
    T = pts.dtype.type
    Brad, halfw = rows_of(table)
    H = len(Brad)
    with np.errstate(all="ignore"):
        depth = np.sqrt((pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2])
        # the correctly rounded pitch in either dtype (numpy's own loops are not correctly rounded and differ between builds
        # and CPUs): float32 through double, rounded once; float64 by asin_cr.  The yaw decides the column only.
        yaw = -np.arctan2(pts[:, 1].astype(np.float64), pts[:, 0].astype(np.float64)).astype(pts.dtype)
        ratio = pts[:, 2] / depth
        pitch = asin_cr(ratio) if pts.dtype == np.float64 else np.arcsin(ratio.astype(np.float64)).astype(np.float32)
        q = pitch.astype(np.float64)
        proj_x = T(0.5) * (yaw / T(np.pi) + T(1.0))
        ok = (depth != 0) & ~np.isnan(depth) & ~np.isnan(q) & ~np.isnan(proj_x)
        qs = np.where(ok, q, 0.0)
        row = argmin_rows(qs, Brad)
        d = np.abs(qs - Brad[row])
        if H > 1:
            inside = d <= halfw[row]
            # near a boundary: the two nearest beams almost equally far, or the distance almost halfw
            dd = np.sort(np.abs(qs[:, None] - Brad[None, :]), 1)[:, :2] if len(qs) else np.zeros((0, 2))
            ulp = np.spacing(np.abs(pitch)).astype(np.float64)
            near = (np.abs(dd[:, 0] - dd[:, 1]) <= 4 * ulp) | (np.abs(d - halfw[row]) <= 4 * ulp)
        else:
            fu, fd = fov[0] / 180.0 * np.pi, fov[1] / 180.0 * np.pi
            inside = (qs >= fd) & (qs <= fu)
            ulp = np.spacing(np.abs(pitch)).astype(np.float64)
            near = (np.abs(qs - fd) <= 4 * ulp) | (np.abs(qs - fu) <= 4 * ulp)
        kept = ok & inside
        near = near & ok
        proj_x = proj_x * T(W)
        col = np.maximum(0, np.minimum(W - 1, np.floor(proj_x)))
    col = np.where(kept, col, 0).astype(np.int32)
    kd, kc, kr = depth[kept], col[kept], row[kept].astype(np.int32)
    kxf, kq = proj_x[kept], pitch[kept]
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
    has = index >= 0
    win = np.where(has, index, 0)
    n = len(kd)
    pick = lambda a, zero: np.where(has, a[win], zero) if n else np.full((H, W), zero, a.dtype)   # noqa: E731
    lab_image = pick(klab.astype(np.int32), np.int32(0)) if klab is not None else np.zeros((H, W), np.int32)
    return dict(idx=index, range=range_image, rem=rem_image, label=lab_image.astype(np.int32),
                proj_x=pick(kc, np.int32(0)).astype(np.int32), proj_y=pick(kr, np.int32(0)).astype(np.int32),
                proj_xf=pick(kxf, T(0)).astype(pts.dtype), proj_yf=pick(kq, T(0)).astype(pts.dtype),
                kept=kept, near=near, row=row, col=col, pitch=pitch)


def near_cells(p, W):
    """[H, W] mask of the cells touched by a point flagged ``near`` (its own row and the rows beside it)"""
    H = p["idx"].shape[0]
    m = np.zeros((H, W), bool)
    r, c = p["row"][p["near"]], p["col"][p["near"]]
    for dr in (-1, 0, 1):
        m[np.clip(r + dr, 0, H - 1), c] = True
    return m


def reverse_projection(range_image, proj_x, proj_y_or_pitch, table, preserve_float):
    """float64 [H*W, 3]: yaw = (proj_x / W * 2 - 1) * pi; the elevation the table's angle of the row (or the pitch image
    with ``preserve_float``); pitch = pi / 2 - e; the point as in ``do_reverse_projection_new`` (laserscan.py:492-497)"""
    depth = np.asarray(range_image)
    H, W = depth.shape
    Brad = rows_of(table)[0]
    yaw = (np.asarray(proj_x) / W * 2 - 1.0) * np.pi
    e = np.asarray(proj_y_or_pitch, np.float64) if preserve_float else Brad[np.asarray(proj_y_or_pitch)]
    pitch = np.pi / 2 - e
    x = depth * np.sin(pitch) * np.cos(-yaw)
    y = depth * np.sin(pitch) * np.sin(-yaw)
    z = depth * np.cos(pitch)
    return np.stack([x, y, z], 2).reshape(-1, 3)


def seeded_cloud(table, fov, n, dtype, seed):
    """``n`` random points (depth 2 .. 60 m, elevations over the field of view and a little beyond) whose first rows are the
    chosen ones: on a beam, exactly midway between two beams, just inside and just outside ``halfw``, inside the widest gap,
    at depth 0 and NaN -- cycled when ``n`` is small.  Returns (points [n, 3] dtype, rem [n] f32, label [n] i32)."""
    rng = np.random.default_rng(seed)
    Brad, halfw = rows_of(table)
    H = len(Brad)
    fu, fd = np.radians(fov[0]), np.radians(fov[1])
    el = rng.uniform(fd - 0.03, fu + 0.03, n)
    az = rng.uniform(-np.pi, np.pi, n)
    dist = rng.uniform(2.0, 60.0, n)
    special = []
    if H > 1:
        g = int(np.argmax(Brad[:-1] - Brad[1:]))                 # the widest gap: rows g, g + 1
        k = H // 2
        special = [Brad[0], Brad[k], Brad[H - 1], (Brad[k] + Brad[min(k + 1, H - 1)]) / 2, (Brad[g] + Brad[g + 1]) / 2,
                   Brad[g] - halfw[g] * 0.999, Brad[g] - halfw[g] * 1.001, Brad[g + 1] + halfw[g + 1] * 1.001,
                   Brad[0] + halfw[0] * 0.999, Brad[0] + halfw[0] * 1.001, Brad[H - 1] - halfw[H - 1] * 1.001]
    else:
        special = [Brad[0], fu, fd, fu + 1e-3, fd - 1e-3, (fu + fd) / 2]
    for j, e in enumerate(special):
        if j < n:
            el[j] = e
    pts = np.stack([dist * np.cos(el) * np.cos(az), dist * np.cos(el) * np.sin(az), dist * np.sin(el)], 1).astype(dtype)
    for j, v in enumerate(([0, 0, 0], [np.nan, 1, 1], [1, 1, np.nan])):
        if len(special) + j < n:
            pts[len(special) + j] = v
    if n > 64:                                                    # several points per cell: the z-min and its tie rule
        m = n // 8
        pts[n // 2:n // 2 + m] = pts[:m]
        pts[n // 2 + m:n // 2 + 2 * m] = pts[:m] * dtype(0.5)
    rem = rng.random(n).astype(np.float32)
    lab = rng.integers(1, 250, n).astype(np.int32)
    return np.ascontiguousarray(pts), rem, lab
