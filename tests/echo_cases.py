"""The target sensor's echo model (include/lidarhip.h) restated in numpy: the offsets table, the sub-rays and the
resolve in float64 from the widened float32 values with every product, sum, quotient and square root an operation of its own
(IEEE, rounded one by one) in the stated order; and the builders of the cases the CPU and GPU tests share."""
import numpy as np

MODES = ("first", "strongest", "last")
MAX_SUBRAYS = 8


def offsets(divergence, subrays, ring=0.7071):
    """row 0 (0, 0); row k >= 1 tan(rho) (cos phi_k, sin phi_k), rho = radians(divergence / 2 * ring), phi_k = 2 pi (k - 1) /
    (S - 1) + pi / (S - 1); float64 [S, 2]"""
    S = int(subrays)
    off = np.zeros((S, 2), np.float64)
    rho = np.radians(float(divergence) / 2.0 * float(ring))
    for k in range(1, S):
        phi = 2.0 * np.pi * (k - 1) / (S - 1) + np.pi / (S - 1)
        off[k] = np.tan(rho) * np.cos(phi), np.tan(rho) * np.sin(phi)
    return off


def params(off, separation=0.5, min_subrays=1, mode="strongest"):
    """the kernels' view of a model: ``lt_echo_model``'s fields"""
    off = np.asarray(off, np.float64).reshape(-1, 2)
    return dict(off=off, S=off.shape[0], separation=float(separation), min_subrays=int(min_subrays), mode=MODES.index(mode))


def params_of(model):
    """the kernels' view of a ``config.EchoModel``"""
    return params(model.offsets(), model.separation, model.min_subrays, model.mode)


def frame(rays):
    """``(h, u, v, dd, h2)`` of the rays [n, 3] f32: the unit direction, the horizontal to the left, h x u; float64, nan where
    dd is not positive"""
    d = np.asarray(rays, np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        h2 = x * x + y * y
        dd = h2 + z * z
        nn = np.sqrt(dd)
        hx, hy, hz = x / nn, y / nn, z / nn
        hh = np.sqrt(h2)
        flat = h2 > 0
        ux = np.where(flat, -y / hh, 1.0)
        uy = np.where(flat, x / hh, 0.0)
        vx = -(hz * uy)
        vy = hz * ux
        vz = hx * uy - hy * ux
    return np.stack([hx, hy, hz], 1), np.stack([ux, uy, np.zeros_like(ux)], 1), np.stack([vx, vy, vz], 1), dd, h2


def restate_subrays(rays, off):
    """``k_subrays``: [S * n, 3] f32, plane by plane"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 3)
    off = np.asarray(off, np.float64).reshape(-1, 2)
    n = rays.shape[0]
    h, u, v, dd, _ = frame(rays)
    plain = ~(dd > 0) | ~np.isfinite(dd)
    out = np.empty((off.shape[0], n, 3), np.float32)
    for k, (a, b) in enumerate(off):
        if a == 0.0 and b == 0.0:
            out[k] = rays
            continue
        with np.errstate(all="ignore"):
            s = np.stack([(h[:, 0] + a * u[:, 0]) + b * v[:, 0], (h[:, 1] + a * u[:, 1]) + b * v[:, 1], h[:, 2] + b * v[:, 2]],
                         1).astype(np.float32)
        out[k] = np.where(plain[:, None], rays, s)
    return out.reshape(-1, 3)


def walk(p, t, tri, rem):
    """one cell: the detected echoes as dicts ``c, st, sr, rep`` in walk order and the index of the chosen one (``None``: no
    echo).  ``t`` f32, ``tri`` i32, ``rem`` f32, each [S]."""
    hits = sorted((float(t[k]), k) for k in range(p["S"]) if tri[k] >= 0 and t[k] > 0)
    echoes = []
    for tk, k in hits:
        with np.errstate(all="ignore"):
            far = bool(echoes) and (np.float64(tk) - echoes[-1]["t_first"] > p["separation"])
        if not echoes or far:
            echoes.append(dict(t_first=np.float64(tk), c=1, st=np.float64(tk), sr=np.float64(rem[k]), rep=k))
        else:
            e = echoes[-1]
            with np.errstate(all="ignore"):
                e["st"] = e["st"] + np.float64(tk)
                e["sr"] = e["sr"] + np.float64(rem[k])
            e["c"] += 1
            e["rep"] = min(e["rep"], k)
    det = [e for e in echoes if e["c"] >= p["min_subrays"]]
    if not det:
        return det, None
    if p["mode"] == 0:
        return det, 0
    if p["mode"] == 2:
        return det, len(det) - 1
    best = 0
    for j in range(1, len(det)):
        if det[j]["sr"] > det[best]["sr"] or (det[j]["sr"] == det[best]["sr"] and det[j]["c"] > det[best]["c"]):
            best = j
    return det, best


def restate_resolve(p, rays, origin, sub_range, sub_tri, sub_label=None, sub_rem=None):
    """``k_echo_resolve``: the sub-images [S * n] plane by plane -> a dict of NEW arrays endpoints [n, 3] f32, endcolors [n] i32,
    range, endrem, fraction [n] f32, tri [n] i32, n_echoes [n] u8"""
    S = p["S"]
    rays = np.asarray(rays, np.float32).reshape(-1, 3)
    n = rays.shape[0]
    t = np.asarray(sub_range, np.float32).reshape(S, n)
    tri = np.asarray(sub_tri, np.int32).reshape(S, n)
    rem = np.zeros((S, n), np.float32) if sub_rem is None else np.asarray(sub_rem, np.float32).reshape(S, n)
    lab = np.zeros((S, n), np.int32) if sub_label is None else np.asarray(sub_label, np.int32).reshape(S, n)
    o = np.asarray(origin, np.float32).astype(np.float64)
    h, _, _, dd, _ = frame(rays)
    out = dict(endpoints=np.zeros((n, 3), np.float32), endcolors=np.zeros(n, np.int32), range=np.zeros(n, np.float32),
               endrem=np.zeros(n, np.float32), tri=np.full(n, -1, np.int32), n_echoes=np.zeros(n, np.uint8),
               fraction=np.zeros(n, np.float32))
    for i in range(n):
        det, j = walk(p, t[:, i], tri[:, i], rem[:, i])
        out["n_echoes"][i] = len(det)
        if j is None or not dd[i] > 0:
            continue
        e = det[j]
        with np.errstate(all="ignore"):
            r = np.float32(e["st"] / np.float64(e["c"]))
            out["range"][i] = r
            out["endrem"][i] = np.float32(e["sr"] / np.float64(S))
            out["fraction"][i] = np.float32(np.float64(e["c"]) / np.float64(S))
            out["endpoints"][i] = (o + h[i] * np.float64(r)).astype(np.float32)
        out["endcolors"][i] = lab[e["rep"], i]
        out["tri"][i] = tri[e["rep"], i]
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------
#: rays a sensor never makes but the kernel must take: straight up and down (no horizontal part: u = (1, 0)), the zero ray and
#: a NaN row (copied), rays that are no unit vectors, and a horizontal part that is a float32 denormal beside z = 1
SPECIAL_RAYS = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 0], [np.nan, 0.5, 0.5], [3, -4, 12], [1e-3, 2e-3, -5e-4], [1e-40, 0, 1],
                         [0, -1e-42, -1], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [1e20, 1e20, 1e20]], np.float32)


def ray_case(n, seed=0):
    """``n`` rays [n, 3] f32: random directions of random lengths with SPECIAL_RAYS spread over them (all of them from 21 rays
    on; a single ray is straight up)"""
    rs = np.random.default_rng(500 + seed + 3 * n)
    d = rs.normal(size=(n, 3))
    d *= rs.uniform(0.2, 3.0, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    rays = d.astype(np.float32)
    if n == 1:
        rays[0] = SPECIAL_RAYS[0]
    elif n >= 21:
        at = (np.arange(len(SPECIAL_RAYS)) * (n // len(SPECIAL_RAYS)) + n // 40) % n
        rays[at] = SPECIAL_RAYS
    return rays


def resolve_case(n, S, seed=0, origin=(0.0, 0.0, 0.0)):
    """made-up sub-images of ``n`` cells and ``S`` sub-rays: every cell sees one to three surfaces between 2 and 60 m, 0.2 to 3 m
    apart, each sub-ray one of them with a jitter of a few centimetres or none (equal ranges in two sub-rays), remissions from
    a few levels per surface (so that sums tie); a quarter of the sub-rays miss, a few hold ``tri >= 0`` with range 0 or ``tri
    = -1`` with a range, and (from 21 cells on) one cell in nineteen sees nothing at all.  Host arrays: rays [n, 3], origin, range, tri, label, rem [S * n]."""
    rs = np.random.default_rng(900 + seed + 11 * n + S)
    rays = ray_case(n, seed + 1) if n >= 21 else ray_case(21, seed + 1)[4:4 + n].copy()
    base = rs.uniform(2.0, 60.0, n)
    step = rs.uniform(0.2, 3.0, (3, n))
    step[0] = 0
    depth = base[None, :] + np.cumsum(step, 0)                      # [3, n]
    n_surf = rs.integers(1, 4, n)
    which = rs.integers(0, 3, (S, n)) % n_surf[None, :]
    t = np.take_along_axis(depth, which, 0)
    jitter = rs.choice([0.0, 0.0, 0.01, 0.02, 0.05], (S, n))
    t = (t + jitter).astype(np.float32)
    levels = np.array([0.125, 0.25, 0.5, 0.75], np.float32)
    surf_rem = levels[rs.integers(0, 4, (3, n))]
    rem = np.take_along_axis(surf_rem, which, 0).astype(np.float32)
    lab = (which + 10 * rs.integers(1, 20, (1, n))).astype(np.int32)
    tri = rs.integers(0, 100000, (S, n)).astype(np.int32)
    kind = rs.integers(0, 16, (S, n))
    tri[kind < 4] = -1
    t[kind < 3] = 0
    t[kind == 5] = 0                                               # a triangle with range 0: no hit
    rem[kind < 3] = 0
    if n >= 21:                                                    # a cell in nineteen sees nothing at all
        tri[:, 3::19], t[:, 3::19], rem[:, 3::19] = -1, 0, 0
    return dict(rays=rays, origin=np.asarray(origin, np.float32), range=t.reshape(-1), tri=tri.reshape(-1),
                label=lab.reshape(-1), rem=rem.reshape(-1))


def crafted_cells(S=5, origin=(0.0, 0.0, 0.0)):
    """hand-written cells for ``S = 5`` sub-rays and ``separation = 0.5``, one column each; ``names`` says what each is for.
    A sub-ray is ``(t, rem)`` or ``None`` for a miss; its label is ``100 + 10 * cell + k``, its triangle ``1000 * cell + k``."""
    f = np.float32
    cells = [
        ("all misses", [None] * 5),
        ("one hit", [None, None, (7.0, 0.5), None, None]),
        ("equal t in two sub-rays", [None, (9.0, 0.25), None, (9.0, 0.75), None]),
        ("a gap exactly equal to separation", [(4.0, 0.5), (4.5, 0.5), None, None, None]),
        ("a chain of close hits spanning more", [(4.0, 0.5), (4.3, 0.5), (4.6, 0.5), (4.9, 0.5), (5.2, 0.5)]),
        ("min_subrays removes the nearest", [None, (3.0, 0.75), (8.0, 0.25), (8.1, 0.25), None]),
        ("min_subrays removes every echo", [(3.0, 0.5), None, (6.0, 0.5), None, (9.0, 0.5)]),
        ("strongest ties on the sum", [(3.0, 0.5), (3.1, 0.25), (7.0, 0.75), None, None]),
        ("strongest ties on the sum and the count", [(3.0, 0.5), (7.0, 0.5), None, None, None]),
        ("the sum decides against the count", [(3.0, 0.125), (3.1, 0.125), (3.2, 0.125), (7.0, 0.75), None]),
        ("first == last", [(5.0, 0.5), (5.1, 0.5), (5.2, 0.5), (5.3, 0.5), (5.4, 0.5)]),
        ("a zero central ray", [(5.0, 0.5), (5.1, 0.5), None, None, None]),
        ("the centre is not the nearest", [(10.0, 0.5), (5.0, 0.25), (5.02, 0.25), (10.02, 0.5), (10.04, 0.5)]),
    ]
    n = len(cells)
    t = np.zeros((S, n), f)
    rem = np.zeros((S, n), f)
    tri = np.full((S, n), -1, np.int32)
    lab = np.zeros((S, n), np.int32)
    for i, (_, subs) in enumerate(cells):
        for k, s in enumerate(subs):
            if s is not None:
                t[k, i], rem[k, i], tri[k, i], lab[k, i] = s[0], s[1], 1000 * i + k, 100 + 10 * i + k
    rays = np.tile(np.array([[0.6, 0.0, 0.8]], f), (n, 1))
    rays[[c[0] for c in cells].index("a zero central ray")] = 0
    return dict(names=[c[0] for c in cells], rays=rays, origin=np.asarray(origin, f), range=t.reshape(-1), tri=tri.reshape(-1),
                label=lab.reshape(-1), rem=rem.reshape(-1))


# ---- the end-to-end scene ----------------------------------------------------------------------------------------------------
def edge_scene(rays, H, W):
    """A wall at x = 10 m and a plate at x = 5 m in front of it whose right edge lies in the vertical plane through the central
    ray of the column ``w0`` that looks most nearly along +x: ``(verts [8, 3] f32, faces [4, 3] i32, colors [8, 3] i32, rem [8]
    f32, w0)``.  The plate (label 7, remission 0.75) reaches from that edge 4 m to the LEFT (larger y); the wall (label 3,
    remission 0.25) spans 40 m.  Both reach 20 m up and down."""
    r = np.asarray(rays, np.float32).reshape(H, W, 3).astype(np.float64)
    mid = r[H // 2]
    w0 = int(np.argmax(mid[:, 0] / np.hypot(mid[:, 0], mid[:, 1])))
    dx, dy = mid[w0, 0], mid[w0, 1]
    ye = 5.0 * dy / dx
    verts = np.array([[10, -20, -20], [10, 20, -20], [10, 20, 20], [10, -20, 20],
                      [5, ye, -20], [5, ye + 4, -20], [5, ye + 4, 20], [5, ye, 20]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    colors = np.zeros((8, 3), np.int32)
    colors[:4, 2], colors[4:, 2] = 3, 7
    rem = np.array([0.25] * 4 + [0.75] * 4, np.float32)
    return verts, faces, colors, rem, w0


def two_plane_cast(sub, ye):
    """the analytic caster of :func:`edge_scene` from the origin: ``(range f64, surface)`` per sub-ray (``sub`` [m, 3] f32, not
    normalised), surface 1 = the plate (x = 5, y in [ye, ye + 4]), 0 = the wall (x = 10), -1 = neither"""
    d = np.asarray(sub, np.float32).astype(np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        tp = 5.0 / d[:, 0]
        tw = 10.0 / d[:, 0]
    yp, zp = tp * d[:, 1], tp * d[:, 2]
    on_plate = (d[:, 0] > 0) & (yp >= ye) & (yp <= ye + 4) & (np.abs(zp) <= 20)
    on_wall = (d[:, 0] > 0) & (np.abs(tw * d[:, 1]) <= 20) & (np.abs(tw * d[:, 2]) <= 20)
    return np.where(on_plate, tp, np.where(on_wall, tw, 0.0)), np.where(on_plate, 1, np.where(on_wall, 0, -1))
