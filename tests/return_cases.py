"""The target sensor's return model (include/lidarhip.h) restated in numpy: float64 from the widened float32
values, every product and sum a numpy operation of its own (IEEE, rounded one by one) in the stated order; the hash in
uint64 arithmetic masked to 32 bits; and the generators of the cases the CPU and GPU tests share."""
import numpy as np

CODES = ("kept", "no hit", "below min_range", "beyond max_range", "beyond max_incidence", "dropped at random")
M32 = np.uint64(0xFFFFFFFF)


def mix(x):
    """mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16  (uint32)"""
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def hash32(seed, scan, i):
    """hash(seed, scan, i) = mix(mix(mix(seed) + scan) + i), uint32 sums wrap; ``i`` may be an array.  Returns uint64 < 2^32."""
    a = (mix(seed) + np.uint64(int(scan) & 0xFFFFFFFF)) & M32
    return mix((mix(a) + (np.asarray(i, dtype=np.uint64) & M32)) & M32)


def cosine(v0, v1, v2, d):
    """the cosine of the incidence angle of rays ``d`` [n, 3] on triangles ``v0, v1, v2`` [n, 3] (float32 inputs), float64 [n]"""
    return cosine64(*(np.asarray(a, np.float32).astype(np.float64) for a in (v0, v1, v2, d)))


def cosine64(v0, v1, v2, d):
    """the float64 chain itself, on float64 values (the contract feeds it widened float32 values: :func:`cosine`)"""
    v0, v1, v2, d = (np.asarray(a, np.float64) for a in (v0, v1, v2, d))
    e1x, e1y, e1z = (v1[:, k] - v0[:, k] for k in range(3))
    e2x, e2y, e2z = (v2[:, k] - v0[:, k] for k in range(3))
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    nx = e1y * e2z - e1z * e2y
    ny = e1z * e2x - e1x * e2z
    nz = e1x * e2y - e1y * e2x
    dot = (nx * dx + ny * dy) + nz * dz
    nn = (nx * nx + ny * ny) + nz * nz
    dd = (dx * dx + dy * dy) + dz * dz
    zero = (nn == 0) | (dd == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.abs(dot) / np.sqrt(nn * dd)
    c = np.where(q < 1.0, q, 1.0)
    return np.where(zero, 0.0, c)


def params_of(model):
    """the kernel's view of a ``config.ReturnModel``"""
    return dict(min_range=model.min_range, max_range=model.max_range, min_cos=model.min_cos, drop_threshold=model.drop_threshold,
                seed=model.seed, lambert=model.lambert)


def params(min_range=0.0, max_range=np.inf, min_cos=0.0, drop_threshold=0, seed=0, lambert=False):
    return dict(min_range=float(min_range), max_range=float(max_range), min_cos=float(min_cos), drop_threshold=int(drop_threshold),
                seed=int(seed), lambert=bool(lambert))


def restate(p, scan, rays, verts, faces, tri, rng, endrem=None, endpoints=None, endcolors=None):
    """The model ``p`` (:func:`params`) on one rendered scan.  ``rays`` [n, 3] f32, ``verts`` [V, 3] f32, ``faces`` [F, 3]
    i32; images as the render left them (``endcolors`` [n] or [n, 3]; any of the optional ones ``None``).  Returns a dict of
    NEW arrays: the images given, ``incidence`` f32 [n], ``drop`` u8 [n] and ``cos`` f64 [n] (0 where there is no hit).  A
    ``tri`` outside [-1, F), or a face with a vertex outside [0, V), is "no hit": code 1, the cell untouched."""
    tri = np.asarray(tri, np.int32)
    n = tri.shape[0]
    rays = np.asarray(rays, np.float32).reshape(-1, 3)[:n]
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    rng = np.asarray(rng, np.float32)
    hit = (tri >= 0) & (tri < faces.shape[0])
    idx = faces[np.where(hit, tri, 0)] if faces.shape[0] else np.zeros((n, 3), np.int32)
    hit &= ((idx >= 0) & (idx < verts.shape[0])).all(1)
    idx = np.where(hit[:, None], idx, 0)
    c = np.zeros(n, np.float64)
    if hit.any():
        c[hit] = cosine(verts[idx[hit, 0]], verts[idx[hit, 1]], verts[idx[hit, 2]], rays[hit])
    r64 = rng.astype(np.float64)
    h = hash32(p["seed"], scan, np.arange(n))
    code = np.zeros(n, np.uint8)
    undecided = np.ones(n, bool)
    for k, rule in ((1, ~hit), (2, r64 < p["min_range"]), (3, r64 > p["max_range"]), (4, c < p["min_cos"]),
                    (5, h < np.uint64(p["drop_threshold"]))):
        code[undecided & rule] = k
        undecided &= ~rule
    gone = code >= 2
    out = dict(drop=code, cos=np.where(code == 1, 0.0, c), incidence=np.where(code == 0, c, -1.0).astype(np.float32),
               tri=np.where(gone, -1, tri).astype(np.int32), range=np.where(gone, np.float32(0), rng).astype(np.float32))
    if endrem is not None:
        er = np.asarray(endrem, np.float32)
        kept = (er.astype(np.float64) * c).astype(np.float32) if p["lambert"] else er
        out["endrem"] = np.where(gone, np.float32(0), np.where(code == 0, kept, er)).astype(np.float32)
    if endpoints is not None:
        out["endpoints"] = np.where(gone[:, None], np.float32(0), np.asarray(endpoints, np.float32).reshape(n, 3)).astype(np.float32)
    if endcolors is not None:
        ec = np.asarray(endcolors, np.int32)
        out["endcolors"] = np.where(gone if ec.ndim == 1 else gone[:, None], 0, ec).astype(np.int32)
    return out


def totals(drop):
    return np.bincount(np.asarray(drop, np.uint8).reshape(-1), minlength=len(CODES)).tolist()


# ---- cases -------------------------------------------------------------------------------------------------------------------
#: (H, W) of the ray counts 1, 63, 64, 65, 185 and 2 080 (nine workgroups, the last one ragged)
SHAPES = ((1, 1), (7, 9), (8, 8), (5, 13), (5, 37), (16, 130))
HASH_KNOWN = (((1, 0, 0), 0x24009c6d), ((1, 0, 1), 0x6a25388a), ((1, 0, 2), 0xcc844ea7), ((7, 5, 0), 0xda12d531),
              ((7, 5, 1), 0x33e82788))


def tilted_plane(theta_deg, n=64, seed=0):
    """Triangles in the plane through (5, 0, 0) whose normal makes ``theta_deg`` with the ray direction (1, 0, 0), rays along
    +x: ``(v0, v1, v2, d, cos(theta))`` with ``n`` triangles of varied size and orientation in that plane (float64: rounding
    the vertices to float32 moves the plane by 1e-7, see :func:`exact_cosine`)."""
    rs = np.random.default_rng(seed)
    t = np.deg2rad(theta_deg)
    normal = np.array([np.cos(t), 0.0, np.sin(t)])
    u = np.array([0.0, 1.0, 0.0])
    w = np.cross(normal, u)
    o = np.array([5.0, 0.0, 0.0])
    pts = [o + rs.uniform(-2, 2, (n, 1)) * u + rs.uniform(-2, 2, (n, 1)) * w for _ in range(3)]
    d = np.tile(np.array([1.0, 0.0, 0.0]), (n, 1))
    return tuple(pts) + (d, float(np.cos(t)))


def exact_cosine(v0, v1, v2, d):
    """|n . d| / sqrt((n . n) (d . d)) of ONE triangle and ray given as float32 values, in exact rational arithmetic up to the
    final square root (50 digits): the analytic cosine of the geometry the float32 numbers describe"""
    from decimal import Decimal, getcontext
    from fractions import Fraction
    getcontext().prec = 50
    F = lambda a: [Fraction(float(np.float32(x))) for x in a]   # noqa: E731
    v0, v1, v2, d = F(v0), F(v1), F(v2), F(d)
    e1, e2 = [b - a for a, b in zip(v0, v1)], [b - a for a, b in zip(v0, v2)]
    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    dot = sum(a * b for a, b in zip(n, d))
    sq = sum(a * a for a in n) * sum(a * a for a in d)
    if sq == 0:
        return 0.0
    return float(abs(Decimal(dot.numerator) / Decimal(dot.denominator)) / (Decimal(sq.numerator) / Decimal(sq.denominator)).sqrt())
