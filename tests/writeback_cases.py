"""Inputs and expected buffers for the write-back of a render (k_sc_resolve of lt_scatter.hip, trace_writeback of
lt_trace.hip), numpy only: tests/test_writeback_cases_cpu.py proves them without a GPU, tests/test_render_writeback_gpu.py
runs them.

A render writes up to five images through five pointers, any of which may be NULL (include/lidarhip.h).  What it owes
the caller, per cell: a hit gets the reference's values (RayTracer.cpp:73-90), a miss gets 0 / -1 with
LT_TRACE_WRITE_MISSES and keeps the caller's bytes without it, and nothing else is touched -- not the rays beyond W * H,
not a byte in front of a pointer or behind the last ray, whatever the pointer's alignment.  So every output here is a
view into its own larger buffer filled with a sentinel, and `expected` states the WHOLE buffer."""
import collections
import functools

import numpy as np

from lidar_transfer_amd.laserscan import create_rays

KEYS = ("endpoints", "endcolors", "range", "endrem", "tri")
ORIGIN = (0.37, -0.21, 0.13)
SENTINEL = 0x5A5A5A5A   # as int32; as a float ~1.5e16: finite, no value of any image
MISS = dict(endpoints=0, endcolors=0, range=0, endrem=0, tri=-1)   # int32 bits of what LT_TRACE_WRITE_MISSES writes

# (H, W, extra): the smallest shapes at which the resolve can go wrong -- one ray, the edges of a wave (63 / 64 / 65) and
# of a workgroup of 256 (255 / 256 / 257; 511 / 512; 1008), several rows, and `extra` trailing rays beyond H * W, which
# no strategy may touch (RayTracer.cpp:56: width = n_rays / height)
SHAPES = ((1, 1, 0), (1, 2, 0), (1, 63, 0), (1, 64, 0), (1, 65, 0), (3, 85, 0), (4, 64, 0), (1, 257, 0), (7, 73, 0),
          (8, 64, 0), (16, 63, 0), (5, 8, 3), (4, 64, 2))
SUBSET_SHAPES = ((1, 65, 0), (7, 73, 0))
EDGE_SHAPE = (4, 64, 0)

# element offsets of the five views inside their buffers: 0, 4, 8, 12 and 4 bytes past an allocation's alignment -- the
# header promises no alignment for these pointers beyond that of their element type
LEAD = dict(endpoints=0, endcolors=1, range=2, endrem=3, tri=1)

# pointer subsets: all five, each one alone, each one missing, none at all
SUBSETS = (KEYS,) + tuple((k,) for k in KEYS) + tuple(tuple(x for x in KEYS if x != k) for k in KEYS) + ((),)

# write_misses, label_image, the images wanted (the other pointers are NULL), trailing rays beyond H * W
Variant = collections.namedtuple("Variant", "write_misses label_image ptrs extra")
FLAGS = ((False, False), (False, True), (True, False), (True, True))   # (write_misses, label_image)

# Colours span the whole int32 range: the reference keeps them as float on the way (RayTracer.cpp:36, :80-84), so what it
# writes is (int)(float)c, which differs from c for most |c| > 2^24.  (float)c rounds to 2^31 for c > 2^31 - 65, and the
# conversion of 2^31 back to int is undefined behaviour in C (x86's cvttss2si gives INT_MIN, the GPU's conversion
# saturates to INT_MAX): the draws stay at |c| <= 2^31 - 128, the largest int32 a float holds exactly.
C_MAX = 2 ** 31 - 128
PLANTED_COLORS = (2 ** 24 + 1, -(2 ** 24 + 1), C_MAX, -2 ** 31)

# value_edges: remissions (r0, r1, r2) of the first faces -> ((r0 + r1) + r2) / 3 (Triangle.h:69)
F_DENORM = float(np.float32(1.401298464324817e-45))
F_MAX = float(np.finfo(np.float32).max)
PLANTED_REM = collections.OrderedDict([
    ("denormal_kept", (F_DENORM, F_DENORM, F_DENORM)),        # 3 * 2^-149 / 3: the smallest denormal again
    ("denormal_lost", (F_DENORM, 0.0, 0.0)),                  # 2^-149 / 3 rounds to +0
    ("minus_zero", (-0.0, -0.0, -0.0)),                       # -0 / 3 = -0: the sign bit alone
    ("minus_zero_first", (-0.0, 0.0, 0.75)),
    ("overflow", (F_MAX, F_MAX, F_MAX)),                      # the sum overflows: +inf
    ("cancelled_overflow", (F_MAX, F_MAX, -F_MAX)),           # (r0 + r1) + r2 = +inf; r0 + (r1 + r2) would be FLT_MAX
    ("inf", (float("inf"), 0.5, 0.25)),
    ("nan", (float("nan"), 0.5, 0.25)),
])


# ---- scenes ---------------------------------------------------------------------------------------------------------
def seed_of(shape):
    H, W, extra = shape
    return 7000 + 1000 * H + 10 * W + extra


def _facing(centre, u, w, radius, rng):
    """triangles [n, 3, 3] around `centre` in the plane spanned by the unit vectors u, w; circumradius `radius`"""
    ang = rng.uniform(0, 2 * np.pi, centre.shape[0])[:, None] + np.arange(3)[None] * (2 * np.pi / 3)
    return centre[:, None] + radius[:, None, None] * (np.cos(ang)[..., None] * u[:, None] + np.sin(ang)[..., None] * w[:, None])


def attrs(n_verts, seed):
    """colours [V, 3] over the whole int32 range, remissions [V] in [0, 1).  PLANTED_COLORS sit in vertex 0 of the first
    (up to four) faces of a soup, rotated through the channels: face k has PLANTED_COLORS[k % 4] in channel 2."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-C_MAX, C_MAX, (n_verts, 3), endpoint=True, dtype=np.int64).astype(np.int32)
    for k in range(min(n_verts // 3, 4)):
        for ch in range(3):
            c[3 * k, ch] = PLANTED_COLORS[(k + 2 - ch) % 4]
    return c, rng.uniform(0, 1, n_verts).astype(np.float32)


def value_edges(n_verts, seed):
    """attrs with PLANTED_REM in the three vertices of faces 0 .. 7 of a soup"""
    c, r = attrs(n_verts, seed)
    assert n_verts >= 3 * len(PLANTED_REM)
    for k, vals in enumerate(PLANTED_REM.values()):
        r[3 * k:3 * k + 3] = np.array(vals, np.float32)
    return c, r


def soup_of(tri, attr):
    """triangles [n, 3, 3] -> (verts, faces, colours, remissions) with three private vertices per face"""
    v = np.ascontiguousarray(tri.reshape(-1, 3).astype(np.float32))
    f = np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)
    return (v, f) + tuple(attr)


@functools.lru_cache(maxsize=None)
def tiles(H, W, seed, edges=False):
    """Small triangles, each centred on its own ray of create_rays(10, -10, H, W) as seen from ORIGIN, 0.2 pixel pitches
    in radius and 3-8 m away, on half of the usable rays (rounded up), dealt by a seeded permutation.  The last column of
    create_rays repeats the first and stays unused; W = 2 therefore has ONE direction, and both of its rays hit.
    edges: the value_edges attributes.  -> mesh, rays [H * W, 3], ray_of [n]"""
    rays = create_rays(10.0, -10.0, H, W)
    rng = np.random.default_rng(seed)
    ncol = max(W - 1, 1)
    usable = (np.arange(H)[:, None] * W + np.arange(ncol)[None]).reshape(-1)
    n = (usable.size + 1) // 2
    ray_of = rng.permutation(usable)[:n]
    d = rays[ray_of].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = rng.uniform(3.0, 8.0, n)
    pitch = min(2 * np.pi / (W - 1) if W >= 3 else 0.1, np.deg2rad(20.0) / (H - 1) if H >= 2 else 0.1, 0.1)
    u = np.cross(d, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    tri = _facing(np.asarray(ORIGIN, np.float32).astype(np.float64) + d * dist[:, None], u, np.cross(d, u), 0.2 * pitch * dist, rng)
    mesh = soup_of(tri, (value_edges if edges else attrs)(3 * n, seed + 1))
    for a in mesh + (rays, ray_of):
        a.setflags(write=False)
    return mesh, rays, ray_of


WALL_SECTOR = (0.0, 90.0)   # (centre, span) in degrees: the wall's rays look along +x


@functools.lru_cache(maxsize=None)
def wall(H, W):
    """One triangle in the plane x = ORIGIN.x + 4 that every ray hits.  No plane is hit by every direction of a full turn,
    so the rays are those of a 90 degree sector (create_rays(10, -10, H, W, sector=WALL_SECTOR)); the triangle spans 168
    degrees of azimuth.  -> mesh, rays"""
    rays = create_rays(10.0, -10.0, H, W, sector=WALL_SECTOR)
    o = np.asarray(ORIGIN, np.float32).astype(np.float64)
    tri = (o + np.array([[4.0, -40.0, -30.0], [4.0, 40.0, -30.0], [4.0, 0.0, 50.0]]))[None]
    mesh = soup_of(tri, attrs(3, 4242))
    for a in mesh + (rays,):
        a.setflags(write=False)
    return mesh, rays


def empty_mesh():
    return (np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((3, 3), np.int32), np.zeros(3, np.float32))


def with_extra(rays, extra, seed=99):
    """`extra` trailing rays beyond H * W: random directions that would hit nothing in particular -- they are never cast"""
    if extra == 0:
        return rays
    tail = np.random.default_rng(seed).normal(size=(extra, 3)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([rays, tail]))


def reference(oracle, mesh, rays, H, n):
    """the brute-force oracle's images of the first n = H * W rays, read-only"""
    ref = oracle.oracle_trace(np.ascontiguousarray(rays[:n]), np.asarray(ORIGIN, np.float32), *mesh, H,
                              mode=oracle.MODE_BRUTE, norm=oracle.NORM_SSE_TABLE)
    for k in KEYS:
        ref[k].setflags(write=False)
    return ref


# ---- buffers --------------------------------------------------------------------------------------------------------
def width_of(key, label_image):
    return 3 if key == "endpoints" or (key == "endcolors" and not label_image) else 1


def tail_of(R):
    """Elements of sentinel behind the last ray.  The likely wrong writes land inside it and show up as a changed guard
    instead of leaving the allocation: three channels written into a label image (2 R elements too many), a whole
    workgroup of 256 rays written past a ragged end (up to 255 x 3 elements)."""
    return max(2 * R, 768) + 64


def layout(R, label_image):
    """key -> (lead, elements of the view, shape of the view, elements of the whole buffer) for R rays (H * W + extra)"""
    out = {}
    for k in KEYS:
        w = width_of(k, label_image)
        out[k] = (LEAD[k], R * w, (R, 3) if w == 3 else (R,), LEAD[k] + R * w + tail_of(R))
    return out


def buffers(R, label_image, sentinel=SENTINEL):
    return {k: np.full(total, sentinel, np.int32) for k, (_, _, _, total) in layout(R, label_image).items()}


def expected(ref, hit, variant, sentinel=SENTINEL):
    """The full contents (int32) of the five padded buffers after one render of `variant`.  ref: the oracle's images of
    the n = H * W rays that are cast, hit [n]: ref["tri"] >= 0.  Hits hold the oracle's bits; misses 0 / -1 with
    write_misses, else the sentinel; the variant's trailing rays, both guards, and every buffer whose pointer was not
    passed hold the sentinel.  endcolors is [R] and holds channel 2 with label_image."""
    n = hit.size
    out = buffers(n + variant.extra, variant.label_image, sentinel)
    for k, (lead, _, _, _) in layout(n + variant.extra, variant.label_image).items():
        if k not in variant.ptrs:
            continue
        w = width_of(k, variant.label_image)
        img = ref[k][:, 2] if (k == "endcolors" and variant.label_image) else ref[k]
        img = np.ascontiguousarray(img).view(np.int32).reshape(n, w)
        body = out[k][lead:lead + n * w].reshape(n, w)
        body[hit] = img[hit]
        if variant.write_misses:
            body[~hit] = MISS[k]
    return out


def differences(got, want, what):
    """[] when the buffers `got` equal `want` as int32 bits -- except where the expected remission is NaN, which is held
    to isnan (a NaN's payload is not what the reference promises) -- else one line per buffer that differs"""
    out = []
    for k in KEYS:
        g, w = np.asarray(got[k]).view(np.int32).reshape(-1), want[k]
        if g.shape != w.shape:
            out.append(f"{what} {k}: {g.shape[0]} elements, expected {w.shape[0]}")
            continue
        bad = g != w
        if k == "endrem":
            nan = np.isnan(w.view(np.float32))
            bad = np.where(nan, ~np.isnan(g.view(np.float32)), bad)
        if bad.any():
            i = np.flatnonzero(bad)
            lead = LEAD[k]
            out.append(f"{what} {k}: {i.size} elements differ, first at buffer element {i[0]} (view starts at {lead}): "
                       f"got {g[i[0]]:#x} expected {w[i[0]]:#x}; elements {i[:8].tolist()}")
    return out


# ---- batch ----------------------------------------------------------------------------------------------------------
# Groups of lt_scene_render_batch_dev: their ray counts put 1, 255, 256, 257 and 512 next to each other, so a scan's first
# workgroup of k_sc_resolve (resolve_block0) follows a full and a ragged last workgroup of its neighbour.  "no_rays" is a
# ray set without rays (the scan is skipped), "empty" an empty mesh under the rays of (7, 73): all misses, no triangle block.
BATCH_GROUPS = (
    ((1, 257, 0),),
    ((3, 85, 0), (4, 64, 0)),
    ((4, 64, 0), (1, 1, 0), (1, 257, 0)),
    ((1, 1, 0), (3, 85, 0), "no_rays", (4, 64, 0), (1, 257, 0), "empty", (8, 64, 0), (4, 64, 2)),
    ((8, 64, 0), (1, 257, 0), "empty", (4, 64, 0), (3, 85, 0), "no_rays", (1, 1, 0), (1, 65, 0)),
)
EMPTY_SHAPE = (7, 73, 0)
NO_RAYS_H = 4


def batch_subset(g, i):
    """the pointer subset of scan i of group g: every scan of a group a different one"""
    return SUBSETS[(5 * g + i) % len(SUBSETS)]
