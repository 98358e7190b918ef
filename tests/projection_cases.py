"""What the range-projection tests share (TEST INFRASTRUCTURE; numpy only, no GPU, no torch): a restatement of
csrc/lt_project.hip's default and legacy-`beams` models in the cloud's dtype, and seeded generators of the clouds that drive
it -- bulk clouds, constructed edge points, and float64 clouds with several depths of ONE float32 bucket in one cell.

The float32 path of `project_point` (csrc/lt_projpoint.h) is exactly restatable: `atan2` and `asin` are computed in float64
and rounded once, everything else is plain IEEE float32 (the build has -ffp-contract=off).  Two float64 math libraries may
differ in the last place of such a value; after the one rounding to float32 that shows only next to a float32 rounding
MIDPOINT, so the generators replace the (about one in 1e7) float32 points that lie there -- see `near_midpoint`."""
from __future__ import annotations

import numpy as np

#: what the generators may replace at most, per generated cloud (the expected share is about 1e-7)
GUARD_ULPS = 64
GUARD_CAP = 1e-4
SENT32, SENT64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _trig(pts, depth):
    """yaw and pitch in the cloud's dtype: float32 through float64, rounded once; float64 by numpy's own loops"""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    if pts.dtype == np.float32:
        yaw = -(np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32))
        pitch = np.arcsin((z / depth).astype(np.float64)).astype(np.float32)
    else:
        yaw = -np.arctan2(y, x)
        pitch = np.arcsin(z / depth)
    return yaw, pitch


def project_points(points, H, W, fov_up, fov_down, beams=None, remove=True, new=True):
    """`project_point` for every point of [n, 3] `points`, in their dtype T.  Constants are rounded to T once;
    depth = sqrt((x*x + y*y) + z*z); with `beams` the pitch is the first nearest of those angles (compared in float64);
    px = 0.5 * (yaw / pi + 1), py = 1 - (pitch + |fov_down|) / fov; dropped: depth 0 (`remove` or `new`), py outside [0, 1]
    (`remove`), NaN; then * W resp. * H, floor, clamp.  Returns a dict of [n] arrays over ALL points."""
    pts = np.ascontiguousarray(points)
    T = pts.dtype.type
    fu, fd = fov_up / 180.0 * np.pi, fov_down / 180.0 * np.pi
    fov = abs(fd) + abs(fu)
    pi_t, afd, fov_t = T(np.pi), T(abs(fd)), T(fov)
    with np.errstate(all="ignore"):
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        depth = np.sqrt((x * x + y * y) + z * z)
        yaw, pitch = _trig(pts, depth)
        if beams is not None and len(beams):
            b = np.asarray(beams, np.float64)
            p64 = pitch.astype(np.float64)
            best, bi = np.abs(p64 - b[0]), np.zeros(len(pts), np.int64)
            for k in range(1, len(b)):
                d = np.abs(p64 - b[k])
                better = d < best
                best, bi = np.where(better, d, best), np.where(better, k, bi)
            pitch = b[bi].astype(pts.dtype)
        px = T(0.5) * (yaw / pi_t + T(1.0))
        py = T(1.0) - (pitch + afd) / fov_t
        keep = np.ones(len(pts), bool)
        if remove or new:
            keep &= ~(depth == 0)
        if remove:
            keep &= (py >= 0) & (py <= 1)
        keep &= ~(np.isnan(depth) | np.isnan(px) | np.isnan(py))
        xf, yf = px * T(W), py * T(H)

        def pixel(v, n):
            f = np.floor(v)
            f = np.where(f < T(n - 1), f, T(n - 1))
            f = np.where(f > T(0), f, T(0))
            return f.astype(np.int32)

        col, row = pixel(xf, W), pixel(yf, H)
    assert depth.dtype == xf.dtype == yf.dtype == pts.dtype
    return dict(keep=keep, depth=depth, xf=xf, yf=yf, px=col, py=row, unit_x=px, unit_y=py)


def default_inits(new):
    """(range, remission, xyz) of an empty cell as the reference initialises them: -1 for the old variant, 0 / -1 / 0 for
    the new one (include/lidarhip.h)"""
    return (0.0, -1.0, 0.0) if new else (-1.0, -1.0, -1.0)


def restate(points, rem, label, H, W, fov_up, fov_down, beams=None, remove=True, new=True, lut=None, inits=None):
    """Everything the single-cloud call and the batched call produce for one cloud.

    Per point, COMPACTED to the kept ones in input order: ``kept`` (mask over the input), ``n_kept``, ``points_kept``,
    ``rem_kept``, ``label_kept``, ``depth``, ``proj_x``, ``proj_y``, ``proj_xf``, ``proj_yf``.
    Images [H*W] by the literal loops -- old: closest point, lowest index among equal depths; new: a float32 running minimum
    replaced when ``depth[i] < image`` -- ``idx`` (numbering of the kept points, -1 empty), ``range``, ``xyz``, ``rem``,
    ``label``, ``color``, ``mask`` (= idx > 0, sic), ``label_folded`` (float32 floor(label * 65536)); empty cells hold
    ``inits`` = (range, rem, xyz), label 0, colour 0.  A colour needs ``lut`` and ``label < len(lut)``, else 0.
    The batched call's pixel images ``img_px``, ``img_py``, ``img_xf``, ``img_yf``: the winner's; an empty cell holds the
    LAST kept point's (numpy's index -1), 0 when nothing is kept.  ``bnds``: (min, max) per axis of the kept points,
    (+inf, -inf) when there is none."""
    pts = np.ascontiguousarray(points)
    n = len(pts)
    p = project_points(pts, H, W, fov_up, fov_down, beams, remove, new)
    r_init, m_init, x_init = default_inits(new) if inits is None else inits
    kept = p["keep"]
    ki = np.nonzero(kept)[0]
    depth, col, row = p["depth"][ki], p["px"][ki], p["py"][ki]
    cell = row.astype(np.int64) * W + col
    cells = H * W
    idx = np.full(cells, -1, np.int32)
    if new:
        image = np.zeros(cells, np.float32)
        with np.errstate(over="ignore"):
            for i in range(len(ki)):
                c = cell[i]
                if idx[c] == -1 or depth[i] < image[c]:
                    image[c] = depth[i]
                    idx[c] = i
    else:
        best = np.full(cells, np.inf)
        for i in range(len(ki)):
            c = cell[i]
            if idx[c] == -1 or depth[i] < best[c]:
                best[c] = depth[i]
                idx[c] = i
    has = idx >= 0
    win = ki[idx[has]]                                      # original index of every winner
    out = dict(kept=kept, n_kept=len(ki), points_kept=pts[ki], depth=depth, proj_x=col, proj_y=row, proj_xf=p["xf"][ki],
               proj_yf=p["yf"][ki], rem_kept=None if rem is None else np.asarray(rem, np.float32)[ki],
               label_kept=None if label is None else np.asarray(label).astype(np.uint32)[ki], idx=idx, cell=cell)
    with np.errstate(over="ignore"):
        rng = np.full(cells, r_init, np.float32)
        rng[has] = p["depth"][win].astype(np.float32)
        xyz = np.full((cells, 3), x_init, np.float32)
        xyz[has] = pts[win].astype(np.float32)
    remi = np.full(cells, m_init, np.float32)
    if rem is not None:
        remi[has] = np.asarray(rem, np.float32)[win]
    lab = np.zeros(cells, np.uint32)
    if label is not None:
        lab[has] = np.asarray(label).astype(np.uint32)[win]
    color = np.zeros((cells, 3), np.float32)
    if lut is not None and len(lut):
        ok = has & (lab < len(lut))
        color[ok] = np.asarray(lut, np.float32)[lab[ok]]
    out.update(range=rng, xyz=xyz, rem=remi, label=lab.view(np.int32), color=color, mask=(idx > 0).astype(np.float32),
               label_folded=np.floor(lab.astype(np.float32) * np.float32(256.0) * np.float32(256.0)))
    src = np.full(cells, ki[-1] if len(ki) else -1, np.int64)
    src[has] = win
    some = src >= 0
    for name, a in (("img_px", p["px"]), ("img_py", p["py"]), ("img_xf", p["xf"]), ("img_yf", p["yf"])):
        img = np.zeros(cells, a.dtype)
        img[some] = a[src[some]]
        out[name] = img
    b = np.empty(6)
    for a in range(3):
        v = pts[ki, a].astype(np.float64)
        b[2 * a], b[2 * a + 1] = (v.min(), v.max()) if len(ki) else (np.inf, -np.inf)
    out["bnds"] = b
    return out


# ---- float64 proj_xf / proj_yf between two float64 math libraries ---------------------------------------------------------------
def tol_xf(W):
    """|device - host| of a float64 ``proj_xf = 0.5 * (yaw / pi + 1) * W`` when the two ``atan2`` differ by one ulp of the yaw
    (|yaw| <= pi: at most spacing(pi)), which reaches the result scaled by W / (2 pi); the quotient (|.| <= 1), the sum (<= 2,
    halved exactly) and the product then round on their own, each to within one ulp of a value of at most W once scaled: three
    times spacing(W)"""
    return float(np.spacing(np.pi) * W / (2 * np.pi) + 3 * np.spacing(np.float64(W)))


def tol_yf(H, fov):
    """the same for ``proj_yf = (1 - (pitch + |fov_down|) / fov) * H``: one ulp of the pitch (|pitch| <= pi / 2) scaled by
    H / fov; the sum rounds to within one ulp of a value below 4 (pitch + |fov_down| < pi / 2 + pi), scaled by H / fov as well;
    the quotient q, 1 - q and the product each to within one ulp of a value of at most Q * H, Q = 1 + (pi / 2 + |fov_down|) / fov"""
    fu, fd = fov[0] / 180.0 * np.pi, fov[1] / 180.0 * np.pi
    f = abs(fd) + abs(fu)
    Q = 1.0 + (np.pi / 2 + abs(fd)) / f
    return float((np.spacing(np.pi / 2) + np.spacing(2.0)) * H / f + 3 * np.spacing(np.float64(Q * H)))


# ---- the float32 guard --------------------------------------------------------------------------------------------------------
def _near_mid(v):
    """float64 values within GUARD_ULPS of their ulps of the middle between two neighbouring float32 values"""
    with np.errstate(all="ignore"):
        f = v.astype(np.float32)
        other = np.nextafter(f, np.where(v >= f.astype(np.float64), np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        mid = (f.astype(np.float64) + other.astype(np.float64)) / 2
        return np.abs(v - mid) <= GUARD_ULPS * np.spacing(np.abs(v))


def near_midpoint(points):
    """[n] mask of the float32 points whose float64 `asin(z / depth)` or `atan2(y, x)` lies within GUARD_ULPS float64 ulps
    of the middle between two neighbouring float32 values: only there can a last-place difference between two float64 math
    libraries change the float32 result"""
    pts = np.asarray(points, np.float32)
    with np.errstate(all="ignore"):
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        depth = np.sqrt((x * x + y * y) + z * z)
        return _near_mid(np.arcsin((z / depth).astype(np.float64))) | _near_mid(np.arctan2(y.astype(np.float64), x.astype(np.float64)))


def guard(points, redraw):
    """replace the float32 points next to a rounding midpoint by `redraw(k)` (the next k points of the cloud's own stream)
    until none is left; returns (points, number replaced) and raises beyond GUARD_CAP.  float64 clouds pass unchanged."""
    pts = np.ascontiguousarray(points)
    if pts.dtype != np.float32 or not len(pts):
        return pts, 0
    replaced = 0
    for _ in range(64):
        bad = np.nonzero(near_midpoint(pts))[0]
        if not len(bad):
            break
        pts[bad] = redraw(len(bad)).astype(np.float32)
        replaced += len(bad)
    else:
        raise AssertionError("the guard does not converge")
    if replaced > GUARD_CAP * len(pts):
        raise AssertionError(f"the guard replaced {replaced} of {len(pts)} points: more than 1 in 10 000")
    return pts, replaced


#: replacement counts of every cloud generated in this process: (what, n, replaced)
GUARD_LOG = []


# ---- generators ---------------------------------------------------------------------------------------------------------------
def _sphere(rng, n, fov, margin=3.0, r=(0.5, 80.0)):
    fu, fd = fov
    d = rng.uniform(r[0], r[1], n)
    yaw = rng.uniform(-np.pi, np.pi, n)
    pitch = np.deg2rad(rng.uniform(fd - margin, fu + margin, n))
    return np.stack([d * np.cos(pitch) * np.cos(yaw), d * np.cos(pitch) * np.sin(yaw), d * np.sin(pitch)], 1)


def bulk(n, dtype, fov, seed, margin=3.0, zero=True):
    """a random cloud with exact duplicates, same-pixel / different-depth runs and (``zero``) one point at depth 0.
    Returns (points [n, 3] dtype, rem [n] f32, label [n] u32)."""
    rng = np.random.default_rng(seed)
    pts = _sphere(rng, n, fov, margin).astype(dtype)
    if n >= 40:
        m = max(1, n // 10)
        pts[n // 2:n // 2 + m] = pts[:m]                     # exact duplicates: depth ties in one cell
        pts[n // 4:n // 4 + m // 2] = pts[:m // 2] * dtype(2.0)   # the same pixel, another depth
        if zero:
            pts[5] = 0
    pts, replaced = guard(pts, lambda k: _sphere(rng, k, fov, margin))
    GUARD_LOG.append((f"bulk({n}, {np.dtype(dtype).name}, seed {seed})", n, replaced))
    rem = rng.uniform(0, 1, n).astype(np.float32)
    lab = rng.integers(0, 260, n).astype(np.uint32)
    return pts, rem, lab


def with_keep_pattern(pts, keep, fov, how="fov"):
    """pull the points where ``keep`` is True well inside the field of view and force the others out: ``how`` = "fov" puts
    them almost straight up (dropped under `remove` only), "nan" gives them a NaN coordinate (dropped by every variant)"""
    pts = pts.copy()
    T = pts.dtype.type
    fu, fd = fov
    rng = np.random.default_rng(len(pts))
    inside = _sphere(rng, len(pts), (fu - 1.0, fd + 1.0), 0.0).astype(pts.dtype)
    pts[keep] = inside[keep]
    out = np.nonzero(~keep)[0]
    if how == "fov":
        pts[out] = np.array([0.25, 0.5, 30.0], pts.dtype)
    else:
        pts[out, out % 3] = T(np.nan)
    pts, replaced = guard(pts, lambda k: _sphere(rng, k, (fu - 1.0, fd + 1.0), 0.0))
    GUARD_LOG.append((f"keep pattern({len(pts)}, {pts.dtype.name})", len(pts), replaced))
    return pts


def seam_keep(n, phase):
    """a keep mask over n points: a random 70 %, with the first and the last point and both sides of every wave (64) and
    block (256) seam forced in or out in turn -- ``phase`` 0 .. 3 moves the turn"""
    k = np.random.default_rng(1000 + n).random(n) < 0.7
    if n == 0:
        return k
    seam = np.arange(64, n, 64)
    k[seam] = ((seam // 64) + phase) % 2 == 0
    k[seam - 1] = ((seam // 64) + phase // 2) % 2 == 0
    k[0] = phase % 2 == 0
    k[-1] = phase // 2 == 0
    return k


def _bisect(lo, hi, pred):
    """two NEIGHBOURING float32 values between lo and hi (same sign, pred(lo) != pred(hi)) with different `pred`"""
    f = lambda i: np.array(i, np.int32).view(np.float32)[()]   # noqa: E731
    a, b = int(np.array(lo, np.float32).view(np.int32)), int(np.array(hi, np.float32).view(np.int32))
    assert (a < 0) == (b < 0) and a != 0 and b != 0, "the stepped coordinate changes its sign"
    pa = pred(f(a))
    assert pa != pred(f(b))
    while abs(b - a) > 1:
        m = (a + b) // 2
        if pred(f(m)) == pa:
            a = m
        else:
            b = m
    return f(a), f(b)


def edge_points(dtype, H, W, fov, cols=None, rows=None):
    """Constructed points (see the list in the code) for one image shape and field of view.  Returns a dict:
    ``points`` [n, 3] dtype; ``pairs``: (i, j, what) index pairs of points on the two sides of a column edge, a row edge,
    py = 0 or py = 1 of the restatement that differ by ONE float32 step of one coordinate -- in float64 clouds too (what a
    posed .bin scan holds): two float64 NEIGHBOURS always lie within `tol_xf` / `tol_yf` of the edge they straddle, where the
    column is not one value between two math libraries; ``exact``: how many kept points have py exactly 0 / exactly 1;
    ``left_out``: float64 pairs dropped because they lie within those bounds all the same."""
    T = np.dtype(dtype).type
    fu, fd = fov[0] / 180.0 * np.pi, fov[1] / 180.0 * np.pi
    fovr = abs(fd) + abs(fu)
    P, pairs = [], []
    Z, NZ = T(0.0), T(-0.0)
    # the seam behind the sensor (both signs of zero), the z axis (both signs, and both signs of its zeros), the origin, the axes
    P += [[-7.5, Z, 0.1], [-7.5, NZ, 0.1], [-3.0, Z, -0.3], [-3.0, NZ, -0.3],
          [Z, Z, 4.0], [Z, Z, -4.0], [NZ, Z, 4.0], [Z, NZ, -4.0], [NZ, NZ, 4.0], [Z, Z, Z], [NZ, NZ, NZ],
          [5.0, Z, Z], [-5.0, Z, Z], [Z, 5.0, Z], [Z, -5.0, Z], [6.0, NZ, NZ], [Z, 6.0, NZ]]
    mid_pitch = (fu + fd) / 2

    def one(p):
        return project_points(np.array([p], dtype), H, W, fov[0], fov[1], None, True, True)

    def add_pair(base, axis, lo, hi, pred, what):
        def at(v):
            q = list(base)
            q[axis] = v
            return q
        a, b = _bisect(lo, hi, lambda v: pred(one(at(float(v)))))
        pairs.append((len(P), len(P) + 1, what))
        P.extend([at(float(a)), at(float(b))])

    cols = [c for c in (cols if cols is not None else (1, W // 5, W // 3, W // 2 + 1, (7 * W) // 8, W - 1)) if 0 < c < W and (4 * c) % W != 0]
    for c in dict.fromkeys(cols):                               # column edges: px * W crosses the integer c
        yaw = (2.0 * c / W - 1.0) * np.pi                       # yaw = -atan2(y, x): x = rc cos(yaw), y = -rc sin(yaw)
        rc, d = (11.0 + c % 7) * np.cos(mid_pitch), 0.2 * 2.0 * np.pi / W
        base = [float(T(rc * np.cos(yaw))), float(T(-rc * np.sin(yaw))), float(T(rc * np.tan(mid_pitch)))]
        axis = 1 if abs(base[1]) <= abs(base[0]) else 0         # step the smaller coordinate: the finer one
        ends = [rc * np.cos(yaw + s * d) if axis == 0 else -rc * np.sin(yaw + s * d) for s in (-1, 1)]
        add_pair(base, axis, ends[0], ends[1], lambda o, c=c: int(o["px"][0]) >= c, f"column {c}")
    rows = [r for r in (rows if rows is not None else (1, H // 3, H // 2, H - 1)) if 0 < r < H]
    targets = [(f"row {r}", (1.0 - r / H) * fovr - abs(fd), (lambda o, r=r: int(o["py"][0]) >= r)) for r in dict.fromkeys(rows)]
    targets.append(("py 0", fovr - abs(fd), lambda o: bool(o["unit_y"][0] >= 0)))
    targets.append(("py 1", -abs(fd), lambda o: bool(o["unit_y"][0] <= 1)))
    for what, pitch, pred in targets:
        if abs(pitch) < 2e-3:
            continue                                            # (z would change its sign between the two ends)
        r, yaw0, d = 9.0, 0.3, min(fovr / H * 0.25, abs(pitch) * 0.5)
        base = [float(T(r * np.cos(pitch) * np.cos(yaw0))), float(T(r * np.cos(pitch) * np.sin(yaw0))), float(T(r * np.sin(pitch)))]
        hxy = np.hypot(base[0], base[1])
        add_pair(base, 2, hxy * np.tan(pitch - d), hxy * np.tan(pitch + d), pred, what)
    if dtype == np.float32:
        P += [[1e20, 1.0, 2.0], [3.0, -1e20, 1e19], [1e20, 1e20, -1e20],             # squares overflow: depth inf, pitch 0
              [1e-30, 2e-30, -1e-31], [1e-30, 1e-30, 1e-30],                           # squares underflow to 0
              [1e-20, 2e-20, -3e-21], [-2e-21, 1e-22, 1e-22],                          # squares are denormal
              [1e-40, 2e-41, 1e-42], [1e-45, Z, Z], [3e-39, -1e-39, 1e-40]]          # denormals
    else:
        P += [[1e200, 1.0, 2.0], [1e-200, 2e-200, 1e-201], [1e-310, 2e-311, 1e-312], [5e-324, Z, Z]]
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            q = [2.0, -3.0, 0.25]
            q[a] = bad
            P.append(q)
    P.append([np.inf, np.inf, np.inf])
    pts = np.array(P, dtype)
    o = project_points(pts, H, W, fov[0], fov[1], None, True, True)
    for i, j, what in pairs:                                    # neighbours, on the two sides
        df = pts[i] != pts[j]
        sa, sb = pts[i][df].astype(np.float32), pts[j][df].astype(np.float32)
        assert df.sum() == 1 and (sa == pts[i][df]).all() and abs(int(sa.view(np.int32)[0]) - int(sb.view(np.int32)[0])) == 1, what
        if what.startswith("column"):
            assert o["px"][i] != o["px"][j] and o["keep"][i] and o["keep"][j], what
        elif what.startswith("row"):
            assert o["py"][i] != o["py"][j] and o["keep"][i] and o["keep"][j], what
        else:
            assert o["keep"][i] != o["keep"][j], what
    if dtype == np.float32:
        near = near_midpoint(pts)
        # a constructed point is not redrawn: a pair with a member next to a midpoint is dropped whole, single points too
        drop = near.copy()
        for i, j, _ in pairs:
            if near[i] or near[j]:
                drop[[i, j]] = True
        if drop.any():
            keep_i = np.nonzero(~drop)[0]
            remap = -np.ones(len(pts), np.int64)
            remap[keep_i] = np.arange(len(keep_i))
            pairs = [(int(remap[i]), int(remap[j]), w) for i, j, w in pairs if not drop[i]]
            pts = pts[keep_i]
            o = {k: v[keep_i] for k, v in o.items()}
        GUARD_LOG.append((f"edge_points(float32, {H}x{W})", len(P), int(drop.sum())))
    left_out = 0
    if dtype == np.float64:
        # a pair whose float64 proj_xf / proj_yf lies within the two libraries' difference of the integer it straddles is
        # left out whole (its column or row is not ONE value); at most 1 pair in 20
        tx, ty = tol_xf(W), tol_yf(H, fov)
        drop = np.zeros(len(pts), bool)
        for i, j, what in pairs:
            kind, _, num = what.partition(" ")
            for k in (i, j):
                dist = abs(o["xf"][k] - int(num)) if kind == "column" else abs(o["yf"][k] - (int(num) if kind == "row" else int(num) * H))
                if dist <= (tx if kind == "column" else ty):
                    drop[[i, j]] = True
        left_out = sum(1 for i, _, _ in pairs if drop[i])
        if 20 * left_out > len(pairs):
            raise AssertionError(f"{left_out} of {len(pairs)} float64 pairs lie within the bound of their edge")
        if left_out:
            keep_i = np.nonzero(~drop)[0]
            remap = -np.ones(len(pts), np.int64)
            remap[keep_i] = np.arange(len(keep_i))
            pairs = [(int(remap[i]), int(remap[j]), w) for i, j, w in pairs if not drop[i]]
            pts = pts[keep_i]
            o = {k: v[keep_i] for k, v in o.items()}
    exact = (int(((o["unit_y"] == 0) & o["keep"]).sum()), int(((o["unit_y"] == 1) & o["keep"]).sum()))
    return dict(points=np.ascontiguousarray(pts), pairs=pairs, exact=exact, n_built=len(P), left_out=left_out)


def edge_cloud(dtype, H, W, fov, seed=0, **kw):
    """the edge points among 150 bulk points (so they land in several waves), shuffled by a seeded permutation.
    Returns (points, rem, label, pairs)."""
    e = edge_points(dtype, H, W, fov, **kw)
    b, _, _ = bulk(150, dtype, fov, 900 + seed)
    pts = np.concatenate([e["points"], b])
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(pts))
    inv = np.argsort(perm)
    pairs = [(int(inv[i]), int(inv[j]), w) for i, j, w in e["pairs"]]
    pts = np.ascontiguousarray(pts[perm])
    rem = rng.uniform(0, 1, len(pts)).astype(np.float32)
    lab = rng.integers(0, 260, len(pts)).astype(np.uint32)
    return pts, rem, lab, pairs


def valid_for_reference(points, H, W, fov, beams, remove, new):
    """mask of the points the REFERENCE defines under this variant: it divides by depth 0 in the old variant without `remove`
    and casts NaN pixel coordinates to integers wherever it does not drop them"""
    p = project_points(points, H, W, fov[0], fov[1], beams, remove, new)
    bad = np.isnan(p["depth"]) | np.isnan(p["unit_x"]) | np.isnan(p["unit_y"])
    if not (remove or new):
        bad |= p["depth"] == 0
    return ~bad


# ---- several float64 depths of ONE float32 bucket in one cell ----------------------------------------------------------------
#: name -> depths as (float32 value index, side): side -1 / 0 / +1 = the float64 below / equal to / above the float32 value v[k]
BUCKET_ORDERS = {
    "eq_lt_lt": [(0, 0), (0, -1), (0, -2)],
    "lt_eq": [(0, -1), (0, 0)],
    "gt_lt_gt": [(0, +1), (0, -1), (0, +1)],
    "lt_alone": [(0, -1)],
    "dup_eq": [(0, 0), (0, 0), (0, 0)],
    "dup_lt": [(0, -1), (0, -1)],
    "nearer_last": [(1, +1), (1, -1), (1, 0), (1, -1), (0, +1), (0, 0)],
}
BUCKET_PLACES = ("first", "wave_seam", "block_seam", "last", "spread")
BUCKET_N = 2000


def rule_winner(depths):
    """the rule of csrc/lt_project.hip's header comment for the `_new` loop: of the bucket of the smallest float32 value, the
    LAST point lying below that value wins, else the FIRST point of the bucket"""
    d = np.asarray(depths, np.float64)
    f = d.astype(np.float32)
    m = f.min()
    bucket = np.nonzero(f == m)[0]
    below = bucket[d[bucket] < np.float64(m)]
    return int(below[-1]) if len(below) else int(bucket[0])


def bucket_cases(H, W, fov):
    """float64 clouds of BUCKET_N points.  The points of a case lie on one coordinate axis -- sqrt(x * x) is |x| exactly, so
    their depths are exactly the chosen float64 neighbours of a float32 value, and they share one cell whatever H and W -- in
    front of a background that is further away.  Yields dicts: name, place, points, rem, label, at (indices of the case's
    points, in order), depths, axis."""
    v = [np.float32(2.7182817), np.nextafter(np.float32(2.7182817), np.float32(10))]     # two neighbouring float32 values
    axes = [(0, 1.0), (1, 1.0), (1, -1.0)]                     # +x (column W / 2), +y and -y (W / 4, 3 W / 4)
    out = []
    for ci, (name, order) in enumerate(BUCKET_ORDERS.items()):
        depths = []
        for k, side in order:
            d = np.float64(v[k])
            for _ in range(abs(side)):
                d = np.nextafter(d, np.inf if side > 0 else 0.0)
            depths.append(d)
        for pi, place in enumerate(BUCKET_PLACES):
            axis, sign = axes[(ci + pi) % 3]
            pts, rem, lab = bulk(BUCKET_N, np.float64, fov, 5000 + 10 * ci + pi, zero=False)
            near = np.linalg.norm(pts, axis=1) < 4.0
            pts[near] *= 8.0                                     # the background stays behind the case
            k = len(depths)
            start = {"first": 0, "wave_seam": 64 - (k + 1) // 2, "block_seam": 256 - (k + 1) // 2, "last": BUCKET_N - k}.get(place)
            at = np.sort(np.array([5, 300, 70, 600, 1000, 1500][:k])) if place == "spread" else start + np.arange(k)
            for j, d in zip(at, depths):
                pts[j] = 0.0
                pts[j, axis] = sign * d
            out.append(dict(name=name, place=place, points=pts, rem=rem, label=lab, at=at, depths=np.array(depths), axis=axis))
    return out


# ---- the clouds the GPU file runs (tests/test_projection_shapes_gpu.py); the CPU file generates every one of them too ---------
import functools  # noqa: E402

FOV = (3.0, -25.0)
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537)
SIZES_SHAPE = (16, 301)
SHAPES = ((1, 1), (1, 257), (255, 1), (3, 85), (4, 64), (16, 301), (64, 2048))
VARIANTS = ((True, True), (True, False), (False, True), (False, False))      # (new, remove)
LEGACY_BEAMS = tuple(np.deg2rad(np.linspace(FOV[0], FOV[1], 16)))             # the `beams` model: nearest of these angles
WORKSPACE_STEPS = ((4, 64, 700), (64, 2048, 5000), (3, 85, 650), (64, 2048, 4000), (16, 301, 200000), (4, 64, 700))
BATCH_COUNTS = (1, 7, 8, 9, 16, 17)
BATCH_BIG = (16383, 16384, 16385, 16448, 65537)
LUT_LEN = 256


def lut():
    return np.random.default_rng(77).uniform(0, 1, (LUT_LEN, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def size_case(n, dtype, remove, phase=None):
    """n points with `seam_keep`'s pattern: out-of-view points where the variant removes them, NaN points where it does not"""
    pts, rem, lab = bulk(n, dtype, FOV, 100 + n, zero=False)
    keep = seam_keep(n, n % 4 if phase is None else phase)
    return with_keep_pattern(pts, keep, FOV, "fov" if remove else "nan"), rem, lab, keep


@functools.lru_cache(maxsize=None)
def shape_case(H, W, dtype, zero=True, seed=0, n=None):
    n = n if n is not None else (5000 if (H, W) == (64, 2048) else 700)
    return bulk(n, dtype, FOV, 7000 + 131 * H + W + seed, zero=zero)


@functools.lru_cache(maxsize=None)
def edge_case(H, W, dtype):
    return edge_cloud(dtype, H, W, FOV, seed=H + W)


@functools.lru_cache(maxsize=None)
def bucket_case_list(H, W):
    return tuple(bucket_cases(H, W, FOV))


def dropped_cloud(n, dtype, remove, seed):
    """a cloud all of whose points are dropped"""
    pts, rem, lab = bulk(n, dtype, FOV, seed, zero=False)
    return with_keep_pattern(pts, np.zeros(n, bool), FOV, "fov" if remove else "nan"), rem, lab


@functools.lru_cache(maxsize=None)
def batch_case(count, dtype, remove, zero):
    """`count` clouds: an empty one first, in the middle and last, one all of whose points are dropped, a one-point cloud,
    ragged sizes for the rest (count 1: the regular cloud alone; the special ones go through calls of their own)"""
    sizes = [300, 257, 64, 1000, 65, 511, 129, 700, 256, 63, 2049, 1, 400, 513, 90, 255, 333]
    out = []
    for k in range(count):
        if count > 1 and k in (0, count // 2, count - 1):
            out.append((np.zeros((0, 3), dtype), np.zeros(0, np.float32), np.zeros(0, np.uint32)))
        elif count > 1 and k == 1:
            out.append(dropped_cloud(130, dtype, remove, 40 + count))
        elif count > 1 and k == 2:
            p, r, l = bulk(1, dtype, (FOV[0] - 1, FOV[1] + 1), 50 + count, margin=0.0)
            out.append((p, r, l))
        else:
            out.append(bulk(sizes[k], dtype, FOV, 60 + 20 * count + k, zero=zero))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def big_batch_case(dtype, remove):
    return tuple(size_case(n, dtype, remove, phase=(n // 3) % 4)[:3] for n in BATCH_BIG)


def every_gpu_cloud():
    """generate every cloud the GPU file uses (so GUARD_LOG holds the replacement count of each)"""
    for dtype in (np.float32, np.float64):
        for remove in (True, False):
            for n in SIZES:
                size_case(n, dtype, remove)
            big_batch_case(dtype, remove)
            for count in BATCH_COUNTS:
                for zero in (True, False):
                    batch_case(count, dtype, remove, zero)
        for H, W in SHAPES:
            edge_case(H, W, dtype)
            for zero in (True, False):
                shape_case(H, W, dtype, zero)
        for s, (H, W, n) in enumerate(WORKSPACE_STEPS):
            for zero in (True, False):
                shape_case(H, W, dtype, zero, seed=s + 1, n=n)
    bucket_case_list(*SIZES_SHAPE)
    return list(GUARD_LOG)
