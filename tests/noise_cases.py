"""The target sensor's noise model (include/lidarhip.h) restated in numpy: the hash in uint64 arithmetic masked to
32 bits, the draws as integer sums, the float64 chain from the widened float32 values with every product, sum and quotient a
numpy operation of its own (IEEE, rounded one by one; ``np.rint`` rounds ties to even) in the stated order; and the builders
of the cases the CPU and GPU tests share."""
import numpy as np

STATES = ("untouched", "noised", "lost")
M32 = np.uint64(0xFFFFFFFF)
STREAM = 0x6e6f6973                       # "nois": what the seed is folded with, so the stream is not the dropout hash's

#: the issue's vectors: g(1, 0, 0..2), S and z of the range draw, S of the remission draw
G_KNOWN = (0xd2d8b243, 0xa1082cb9, 0x517d33d0)
S_RANGE_KNOWN = (329225, 420091, 305650)
Z_RANGE_KNOWN = (-0.9763336181640625, 0.4101715087890625, -1.3360595703125)
S_REM_KNOWN = (333939, 453070, 352530)
#: the cell counts of the kernel cases: a lane, around a wave, around a workgroup, three workgroups with a ragged end
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)


def mix(x):
    """mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16  (uint32)"""
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def g32(seed, scan, i):
    """g = mix(mix(mix(seed ^ 0x6e6f6973) + scan) + i), uint32 sums wrap; ``i`` may be an array.  uint64 below 2^32."""
    a = (mix((int(seed) & 0xFFFFFFFF) ^ STREAM) + np.uint64(int(scan) & 0xFFFFFFFF)) & M32
    return mix((mix(a) + (np.asarray(i, dtype=np.uint64) & M32)) & M32)


def draw_sums(seed, scan, i):
    """``(S_range, S_rem)``: the sums of the twelve 16-bit halves of w_1 .. w_6 and of w_7 .. w_12, int64"""
    g = g32(seed, scan, i)
    S = []
    for first in (1, 7):
        s = np.zeros(np.shape(g), np.int64)
        for k in range(first, first + 6):
            w = mix((g + np.uint64(k)) & M32)
            s = s + (w & np.uint64(0xFFFF)).astype(np.int64) + (w >> np.uint64(16)).astype(np.int64)
        S.append(s)
    return S[0], S[1]


def z_of(S):
    """z = (double)(S - 393210) / 65536.0: exact in float64"""
    return (np.asarray(S, np.int64) - 393210).astype(np.float64) / 65536.0


def draws(seed, scan, i):
    """``(z_range, z_rem)`` of the cells ``i``, float64"""
    a, b = draw_sums(seed, scan, i)
    return z_of(a), z_of(b)


def params(range_sigma=0.0, range_sigma_rel=0.0, range_resolution=0.0, remission_sigma=0.0, remission_levels=0, seed=0,
           min_range=0.0, max_range=np.inf):
    """the kernel's view of a model: ``lt_noise_model``'s fields"""
    return dict(range_sigma=float(range_sigma), range_sigma_rel=float(range_sigma_rel), range_resolution=float(range_resolution),
                remission_sigma=float(remission_sigma), remission_levels=int(remission_levels), seed=int(seed),
                min_range=float(min_range), max_range=float(max_range))


def params_of(model, returns=None):
    """the kernel's view of a ``config.NoiseModel`` beside the sensor's ``config.ReturnModel`` (its gate; ``None``: none)"""
    gate = (0.0, np.inf) if returns is None else (returns.min_range, returns.max_range)
    return params(model.range_sigma, model.range_sigma_rel, model.range_resolution, model.remission_sigma, model.remission_levels,
                  model.seed, *gate)


def restate(p, scan, origin, tri, rng, endrem=None, endpoints=None, endcolors=None):
    """The model ``p`` (:func:`params`) on one rendered scan: ``tri`` [n] i32 and ``rng`` [n] f32 as the render (and the
    return model) left them, ``origin`` [3] f32, the optional images ``None`` or given (``endcolors`` [n] or [n, 3]).
    Returns a dict of NEW arrays: the images given, ``range_error`` f32 [n] and ``state`` u8 [n]."""
    tri = np.asarray(tri, np.int32)
    n = tri.shape[0]
    rng = np.asarray(rng, np.float32)
    o = np.asarray(origin, np.float32).astype(np.float64)
    ret = (tri >= 0) & (rng > 0)
    z_r, z_e = draws(p["seed"], scan, np.arange(n))
    r = rng.astype(np.float64)
    with np.errstate(all="ignore"):
        sig = p["range_sigma"] + p["range_sigma_rel"] * r
        r1 = r + sig * z_r
        res = p["range_resolution"]
        r2 = np.rint(r1 / res) * res if res > 0 else r1
        lost = ret & (~(r2 > 0) | (r2 < p["min_range"]) | (r2 > p["max_range"]))
        ok = ret & ~lost
        s = r2 / r
    state = np.where(lost, 2, np.where(ok, 1, 0)).astype(np.uint8)
    with np.errstate(all="ignore"):
        out = dict(state=state, range_error=np.where(ok, (r2 - r).astype(np.float32), np.float32(0)).astype(np.float32),
                   tri=np.where(lost, -1, tri).astype(np.int32),
                   range=np.where(lost, np.float32(0), np.where(ok, r2.astype(np.float32), rng)).astype(np.float32))
    if endpoints is not None:
        pts = np.asarray(endpoints, np.float32).reshape(n, 3)
        with np.errstate(all="ignore"):
            moved = (o[None, :] + (pts.astype(np.float64) - o[None, :]) * s[:, None]).astype(np.float32)
        out["endpoints"] = np.where(lost[:, None], np.float32(0), np.where(ok[:, None], moved, pts)).astype(np.float32)
    if endrem is not None:
        er = np.asarray(endrem, np.float32)
        with np.errstate(all="ignore"):
            e = er.astype(np.float64) + p["remission_sigma"] * z_e
            e = np.where(e < 0, 0.0, np.where(e > 1, 1.0, e))
            L = p["remission_levels"]
            if L:
                e = np.rint(e * float(L - 1)) / float(L - 1)
            e = e.astype(np.float32)
        out["endrem"] = np.where(lost, np.float32(0), np.where(ok, e, er)).astype(np.float32)
    if endcolors is not None:
        ec = np.asarray(endcolors, np.int32)
        out["endcolors"] = np.where(lost if ec.ndim == 1 else lost[:, None], 0, ec).astype(np.int32)
    return out


def totals(state):
    return np.bincount(np.asarray(state, np.uint8).reshape(-1), minlength=len(STATES)).tolist()


# ---- cases -------------------------------------------------------------------------------------------------------------------
def scan_case(n, seed=0, label=True, origin=(0.0, 0.0, 0.0)):
    """A made-up rendered scan of ``n`` cells about ``origin``: three quarters returns between 0.5 and 60 m whose end point is
    ``float32(origin + range * direction)``, the rest a mixture of the cells the kernel must leave alone -- the written miss
    (tri -1, range 0, zeros), ``tri = -1`` with a positive range and ``tri >= 0`` with range 0, the last two holding values a
    render never leaves, so that any write shows.  Host arrays: endpoints, endcolors, range, endrem, tri, origin."""
    rs = np.random.default_rng(1000 + seed + 7 * n)
    o = np.asarray(origin, np.float32)
    d = rs.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rng = rs.uniform(0.5, 60.0, n).astype(np.float32)
    tri = rs.integers(0, 5000, n).astype(np.int32)
    pts = (o.astype(np.float64) + rng.astype(np.float64)[:, None] * d).astype(np.float32)
    rem = rs.uniform(0.0, 1.0, n).astype(np.float32)
    col = rs.integers(1, 260, n if label else (n, 3)).astype(np.int32)
    kind = rs.integers(0, 12, n)                       # 0: written miss, 1: tri -1 alone, 2: range 0 alone, else a return
    if n == 1:
        kind[:] = 5
    miss, no_tri, no_rng = kind == 0, kind == 1, kind == 2
    tri[miss | no_tri] = -1
    rng[miss | no_rng] = 0
    pts[miss] = 0
    rem[miss] = 0
    col[miss] = 0
    return dict(endpoints=pts, endcolors=col, range=rng, endrem=rem, tri=tri, origin=o)
