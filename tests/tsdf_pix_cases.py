"""Constructed inputs that drive every path of the TSDF pixel pass (pix_body, k_wd_keys, k_wd_finish, tsdf_rowtab and the
quirk kernels of lidar_transfer_amd/csrc/lt_tsdf.hip) on purpose, and the numpy restatement of the geometry-only dispatch
facts.  numpy only, imports without a GPU: tests/test_tsdf_pix_cases_cpu.py proves what each case reaches,
tests/test_tsdf_pix_paths_gpu.py holds the product to its oracles on these inputs and reads the kernel's path counters.

A case = a volume (bounds, voxel size, field of view), an image shape and a list of observations.  The sensor is the world
origin (the kernel's pt_x, pt_y, pt_z are world coordinates).  An ITEM is one group of 64 pixels of the transposed image
(pixel p = px * H + row): what a workgroup of the pixel pass takes at a time.

Shapes that differ from the first sketch of these cases, and why:
  unstaged_direct  130 x 130 x 16 columns, origin shifted by half a voxel (not 128 x 128): with the sensor on a column, the
                   64 columns on each half axis lie exactly on an image-column boundary and count for neither bound, and the
                   y = dim_y - 1 columns are quirk columns: the smallest wedge came to 3900 < 3840 + 64.  Now: >= 4095.
  staged_agg       field of view (60, -60) degrees (not (10, -25)): 64 rows over 35 degrees are 0.05 m thick at 5 m, a fifth
                   of a voxel -- four pairs in five had an empty z interval and no chunk of 512 pairs came to 256 voxels.
                   Rows of 1.9 degrees hold a voxel in most pairs: chunks of several voxel rounds.
                   Field of view (60, -60) degrees for the same reason as staged_agg: with rows a fifth of a voxel thick no
                   pair held two voxels, and marking `z .. z` for `z .. zend` in the direct path went unnoticed in this case.
  beyond_2p24      265 x 255 x 257 (17.4 M voxels, not 257 x 256 x 256): there dim_y * dim_z = 2^16 and every column starts on
                   an even index, so the only non-plain column was (dim_x - 1, dim_y - 1) -- a quirk column twice over.  With
                   odd dim_y * dim_z the columns (259, 0) and (263, 0) start on odd indices above 2^24 and are non-plain.
  outside          64 x 15 pixels (not 64 x 16): for a width that is a power of two k_wd_finish puts the quirk columns at
                   the tail of the LAST wedge (quirk_tail_in_last_wedge), which then is not empty.
  holes            field of view (10, -60) degrees, rows of 17.5 degrees (not 8.75): a column's written range lies strictly
                   inside its row's pitch span [a, b] only if (D + trunc) cos b <= D cos a for a surface at depth D; at
                   8.75-degree rows down to -25 degrees that needs D >= 4.2 m, outside an 8 m volume; at (-42.5, -60) it
                   holds from 0.6 m on.  The colour-0 surface at 3 m comes LAST (everything in front of it is written by it:
                   nothing after it could be cut or disjoint); the order is: surface at 2 m, the same one voxel further,
                   one voxel nearer, the first again, colour 0 at 3 m.
"""
import functools
import os
import re

import numpy as np

from tsdf_update_cases import fma32, fold  # noqa: F401  (fold: what the device makes of a label image)

f32, f64 = np.float32, np.float64

# the constants of lt_tsdf.hip the reach of the cases depends on (checked against its text: source_constants)
LT_PIX_STAGE = 3840     # rho quanta of an item staged in LDS for the binary searches
LT_PIX_AGG = 1024       # table entries whose written ranges an item merges in LDS
LT_PIX_CHUNK = 512      # pairs per chunk
LT_AXIS_RHO = 1e-3      # columns with rho <= LT_AXIS_RHO * max|pt_z| are quirk columns

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lidar_transfer_amd", "csrc", "lt_tsdf.hip")


def source_constants():
    """{name: value} of the four #defines, read from the text of lt_tsdf.hip."""
    text = open(HIP).read()
    out = {}
    for name in ("LT_PIX_STAGE", "LT_PIX_AGG", "LT_PIX_CHUNK", "LT_AXIS_RHO"):
        m = re.findall(r"^\s*#define\s+" + name + r"\s+([0-9.eE+-]+)f?\b", text, re.M)
        assert len(m) == 1, f"{name}: {len(m)} definitions in lt_tsdf.hip"
        out[name] = float(m[0])
    return out


# words of lt_debug_tsdf_pix_paths (LT_PIXC_* of lt_tsdf.hip)
CNT = dict(pairs=0, cand=1, written=2, chunks=7, items=8, staged=9, unstaged=10, agg=11, direct=12, t0=13, chunks_n=14,
           chunks_1=15, empty=16, clip_all=17, clip_lo=18, clip_hi=19, clip_hole=20, clip_disj=21, clip_clean=22,
           hole_skip=23, sign_pos=24, sign_neg=25, sign_both=26, two_cols=27, v0=28, rounds=29, max_items=30, rounds_n=31)
N_CNT = 32

CLASSES = (0.0, 7.0, 300.0)        # folded colours: 0 (the fresh volume's own), (0, 0, 7), (0, 1, 44)


def _label3(cls):
    c = np.asarray(cls, f32)
    g = np.floor(c / f32(256))
    return np.stack([np.zeros_like(c), g, c - g * f32(256)], -1).astype(f32)


def _case(bnds, voxel, fov, shape, obs, expect=None):
    bnds = np.array(bnds, f64)
    dims = tuple(int(x) for x in np.ceil((bnds[:, 1] - bnds[:, 0]) / voxel).astype(int))
    return dict(bnds=bnds, voxel=voxel, fov=fov, H=shape[0], W=shape[1], dims=dims, origin=bnds[:, 0].astype(f32),
                obs=obs, expect=expect)


def _image(H, W, seed, depth, p0=0.25, specials=True, neg=-0.5):
    """One observation (label3, depth, rem): `depth` (scalar or [H, W]) with +-1 % noise, classes 0 / 7 / 300 (colour 0 with
    probability p0), remissions in [0, 255] with zeros and -1, and -- specials -- at least one pixel each of depth 0, -1, `neg`
    (a negative depth above -trunc_margin: it writes voxels next to the sensor), NaN and +inf, alternately with colour 0 and
    with a class."""
    rng = np.random.default_rng(seed)
    d = (np.broadcast_to(np.asarray(depth, f64), (H, W)) * (1.0 + 0.02 * (rng.random((H, W)) - 0.5))).astype(f32)
    cls = rng.choice(np.array(CLASSES, f32), (H, W), p=[p0, (1 - p0) / 2, (1 - p0) / 2])
    rem = rng.uniform(0.0, 255.0, (H, W)).astype(f32)
    u = rng.random((H, W))
    rem[u < 0.1] = 0.0
    rem[(u >= 0.1) & (u < 0.15)] = -1.0
    if specials:
        n_sp = max(1, (H * W) // 100)
        pos = rng.permutation(H * W)[:5 * n_sp]
        vals = (0.0, -1.0, neg, np.nan, np.inf)
        for j, p in enumerate(pos):
            d.flat[p] = vals[j % 5]
            cls.flat[p] = CLASSES[0] if (j // 5 + j) % 2 == 0 else CLASSES[1 + j % 2]
    return _label3(cls), d, rem


def _freeze(obs):
    for o in obs:
        for a in o:
            a.setflags(write=False)
    return tuple(obs)


def _obs_staged_agg():
    H, W = 64, 16
    yaw = np.linspace(0, 2 * np.pi, W)[None, :]
    out = []
    for k, seed in enumerate((101, 102, 101)):      # the third repeats the first: every interval done already
        l3, d, r = _image(H, W, seed, 5.0 + 1.0 * np.sin(yaw + k) + 0.0 * np.zeros((H, 1)), p0=0.3)
        d[:, 5] = 0.0                                 # an item of 64 empty pixels: T == 0
        d[:, 3] = 0.0
        d[10:14, 3] = 4.0                             # an item of four pixels ...
        l3[10:14, 3] = _label3(np.full(4, 7.0))       # ... of a class: a few dozen pairs, one chunk
        out.append((l3, d, r))
    return _freeze(out)


def _obs_unstaged_direct():
    H, W = 64, 4
    out = []
    for seed in (111, 112):
        l3, d, r = _image(H, W, seed, 9.0, p0=0.0)
        rng = np.random.default_rng(seed + 1000)
        for p in rng.permutation(H * W)[:12]:         # colour-0 pixels at ~14 m, three per image column on average
            d.flat[p] = 14.0
            l3.reshape(-1, 3)[p] = 0.0
        for px in range(W):                           # ... and one in every image column for certain
            d[7 + px, px] = 14.0
            l3[7 + px, px] = 0.0
        out.append((l3, d, r))
    return _freeze(out)


def _obs_plain(H, W, seeds, depth, **kw):
    return _freeze([_image(H, W, s, depth, **kw) for s in seeds])


def _obs_outside():
    """... and a third observation of pairs without a voxel: only the lowest eight rows see something, at 12 m -- 4.5 m below
    the sensor, under the volume's floor at -3 m: every pair's z interval is empty (T > 0, V == 0)."""
    H, W = 64, 15
    obs = [tuple(np.array(a) for a in _image(H, W, s, 9.0)) for s in (141, 142)]
    l3, d, r = (np.array(a) for a in _image(H, W, 143, 12.0, p0=0.0, specials=False))
    d[:H - 8] = 0.0
    return _freeze(obs + [(l3, d, r)])


def _obs_holes():
    H, W = 4, 32
    base = _image(H, W, 131, 2.0, p0=0.0, neg=-0.1)

    def moved(delta):
        d = np.array(base[1])
        ok = np.isfinite(d) & (d > 0)
        d[ok] += f32(delta)
        return (np.array(base[0]), d, np.array(base[2]))
    l3z, dz, rz = _image(H, W, 132, 3.0, p0=1.0, specials=False)
    return _freeze([tuple(np.array(a) for a in base), moved(0.05), moved(-0.05), tuple(np.array(a) for a in base),
                    (l3z, dz, rz)])


def _obs_tiny(H, W, seed):
    """Images too small for a sprinkling: the special depths in turn, over five observations."""
    rng = np.random.default_rng(seed)
    out = []
    specials = (0.0, -1.0, -0.5, np.nan, np.inf)
    for k in range(5):
        d = (2.0 + rng.random((H, W))).astype(f32)
        cls = rng.choice(np.array(CLASSES, f32), (H, W))
        d.flat[k % (H * W)] = specials[k]
        cls.flat[k % (H * W)] = CLASSES[k % 3]
        out.append((_label3(cls), d, rng.uniform(0, 255, (H, W)).astype(f32)))
    return _freeze(out)


B2P24 = [[-33.125, 33.125], [-31.875, 31.875], [-32.125, 32.125]]    # 265 x 255 x 257
MISPLACED = ((259, 0, 0), (263, 0, 0))


def _obs_beyond():
    """MISPLACED: the first voxels of the two non-plain columns with y = 0.  Their index x * dim_y * dim_z is odd and above
    2^24: (float)voxel_idx is the even neighbour below, and the reference's decomposition makes (x - 1, dim_y, 0) of it -- a
    point outside the column table, 36 degrees below the horizon (hence the field of view of +-40 degrees).  The pixels that
    point projects into carry colour 0 and an infinite depth in the first observation, so that these voxels ARE written and
    a kernel that took the column's own coordinates for them would differ."""
    H, W = 16, 16
    obs = [tuple(np.array(a) for a in _image(H, W, s, 20.0)) for s in (161, 162)]
    for x, _, _ in MISPLACED:
        pt = np.array([B2P24[0][0] + (x - 1) * 0.25, B2P24[1][0] + 255 * 0.25, B2P24[2][0]])
        pitch = np.arcsin(pt[2] / np.linalg.norm(pt))
        row = int(np.floor((1.0 - (pitch + np.radians(40.0)) / np.radians(80.0)) * H))
        px = int(np.floor(0.5 * (-np.arctan2(pt[1], pt[0]) / np.pi + 1.0) * W))
        obs[0][1][row, px] = np.inf
        obs[0][0][row, px] = 0.0
    return _freeze(obs)


B64 = [[-8.0, 8.0], [-8.0, 8.0], [-3.0, 3.0]]
CASES = {
    # wedges of ~250 entries: staged searches, ranges merged in LDS; items of no, one and many chunks
    "staged_agg": lambda: _case(B64, 0.25, (60.0, -60.0), (64, 16), _obs_staged_agg(), "staged"),
    # every wedge beyond LT_PIX_STAGE: searches in global memory; colour-0 pixels at 14 m: runs beyond LT_PIX_AGG
    "unstaged_direct": lambda: _case([[-16.125, 16.375], [-16.125, 16.375], [-2.0, 2.0]], 0.25, (60.0, -60.0), (64, 4),
                                     _obs_unstaged_direct(), "unstaged"),
    # an item = two image columns
    "two_wedges": lambda: _case(B64, 0.25, (10.0, -25.0), (32, 16), _obs_plain(32, 16, (121, 122), 5.0), "staged"),
    # items straddle image columns at every offset; 325 = 5 * 64 + 5; W not a power of two
    "straddle_partial": lambda: _case(B64, 0.25, (10.0, -25.0), (25, 13), _obs_plain(25, 13, (123, 124), 5.0), "staged"),
    # the five outcomes of the zw_snap clipping (module docstring)
    "holes": lambda: _case([[-4.0, 4.0], [-4.0, 4.0], [-2.0, 2.0]], 0.05, (10.0, -60.0), (4, 32), _obs_holes()),
    # the sensor outside the volume: empty wedges at both ends of the image and in runs, items without a pair
    "outside": lambda: _case([[5.0, 13.0], [-8.0, 8.0], [-3.0, 3.0]], 0.25, (10.0, -25.0), (64, 15),
                             _obs_outside(), "staged"),
    # one column at exactly rho == 0 / none within the axis limit
    "axis_on": lambda: _case([[-6.0, 6.0], [-6.0, 6.0], [-5.0, 5.0]], 0.25, (10.0, -25.0), (16, 16),
                             _obs_plain(16, 16, (151, 152), 4.0), "staged"),
    "axis_off": lambda: _case([[-6.125, 5.875], [-6.125, 5.875], [-5.0, 5.0]], 0.25, (10.0, -25.0), (16, 16),
                              _obs_plain(16, 16, (151, 152), 4.0), "staged"),
    # 17.4 M voxels: columns at x boundaries whose voxel indices the reference's float division misplaces
    "beyond_2p24": lambda: _case(B2P24, 0.25, (40.0, -40.0), (16, 16), _obs_beyond()),
    # row boundary on pitch 0; every row below the horizon; row 0's clamp
    "rows_level": lambda: _case([[-8.0, 8.0], [-8.0, 8.0], [-4.0, 4.0]], 0.25, (15.0, -15.0), (8, 16),
                                _obs_plain(8, 16, (171, 172), 5.0), "staged"),
    "rows_below": lambda: _case([[-8.0, 8.0], [-8.0, 8.0], [-4.0, 4.0]], 0.25, (-2.0, -25.0), (8, 16),
                                _obs_plain(8, 16, (173, 174), 5.0), "staged"),
    "rows_clamp": lambda: _case([[-8.0, 8.0], [-8.0, 8.0], [-4.0, 4.0]], 0.25, (3.0, -25.0), (8, 16),
                                _obs_plain(8, 16, (175, 176), 5.0), "staged"),
}
# degenerate images: px_bits of W = 1, 2, 3; one-row and one-wedge tables
for _h, _w in ((1, 1), (1, 7), (3, 1), (5, 2), (2, 3)):
    CASES[f"degenerate_{_h}x{_w}"] = (lambda h=_h, w=_w: _case([[-4.0, 4.0], [-4.0, 4.0], [-2.0, 2.0]], 0.25, (10.0, -25.0),
                                                               (h, w), _obs_tiny(h, w, 180 + 10 * h + w), "staged"))
NAMES = list(CASES)
BIG = ("beyond_2p24",)      # compared on the device only


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ---- the restatement of the geometry-only dispatch facts ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def columns(name):
    """Per table column c = x * dim_y + y, in float32 exactly as k_wd_keys: `plain` (both ends of the column decompose to x by
    the reference's float division), `last_y`, `axis`, their union `quirk`; and in float64: `px_lo`, `px_hi` -- the image
    columns the voxel column can fall into (equal unless its azimuth lies within 1e-4 rad of an image-column boundary)."""
    c = case(name)
    dx, dy, dz = c["dims"]
    vs, org, W = f32(c["voxel"]), c["origin"], c["W"]
    col = np.arange(dx * dy, dtype=np.int64)
    x, y = col // dy, col % dy
    dyz = f32(dy * dz)
    i0, i1 = col * dz, col * dz + dz - 1
    plain = (np.floor(i0.astype(f32) / dyz) == x.astype(f32)) & (np.floor(i1.astype(f32) / dyz) == x.astype(f32))
    pt_x, pt_y = fma32(x.astype(f32), vs, org[0]), fma32(y.astype(f32), vs, org[1])
    rho = np.sqrt(fma32(pt_y, pt_y, pt_x * pt_x))
    limit = f32(LT_AXIS_RHO) * np.maximum(np.abs(org[2]), np.abs(fma32(f32(dz - 1), vs, org[2])))
    last_y, axis = y == dy - 1, rho <= limit
    yaw = -np.arctan2(pt_y.astype(f64), pt_x.astype(f64))
    proj = 0.5 * (yaw / np.pi + 1.0) * W
    eps = 1e-4 / (2 * np.pi) * W
    px_lo = np.clip(np.floor(proj - eps), 0, W - 1).astype(np.int64)
    px_hi = np.clip(np.floor(proj + eps), 0, W - 1).astype(np.int64)
    return dict(plain=plain, last_y=last_y, axis=axis, quirk=~plain | last_y | axis, px_lo=px_lo, px_hi=px_hi, rho=rho)


def quirk_tail_in_last_wedge(W):
    """k_wd_finish bins a key by min(key >> rho_bits, W) and the quirk key is all ones: bin 2^px_bits - 1.  Where that is
    W - 1 (W a power of two >= 2) the quirk columns are the tail of the LAST wedge (entries of column -1) and wd_start[W] is the
    number of columns; otherwise it is the bin W and wd_start[W] = n_cols - n_quirk."""
    px_bits = 1
    while (1 << px_bits) < W:
        px_bits += 1
    return (1 << px_bits) - 1 < W


@functools.lru_cache(maxsize=None)
def wedge_bounds(name):
    """(lo [W], hi [W]): bounds on the number of table entries of every image column's wedge, wd_start[px + 1] - wd_start[px]."""
    c, t = case(name), columns(name)
    W = c["W"]
    ok = ~t["quirk"]
    sure = ok & (t["px_lo"] == t["px_hi"])
    lo = np.bincount(t["px_lo"][sure], minlength=W)
    unsure = ok & ~sure
    hi = lo + np.bincount(t["px_lo"][unsure], minlength=W) + np.bincount(t["px_hi"][unsure], minlength=W)
    if quirk_tail_in_last_wedge(W):
        nq = int(t["quirk"].sum())
        lo[W - 1] += nq
        hi[W - 1] += nq
    return lo, hi


def items(name):
    """[(first image column, last image column)] of every item."""
    c = case(name)
    H, n_pix = c["H"], c["H"] * c["W"]
    return [(p0 // H, min(p0 + 63, n_pix - 1) // H) for p0 in range(0, n_pix, 64)]


def stage_bounds(name):
    """Per item: (lower, upper) bound of n_stage, the table entries of the wedges its 64 pixels search."""
    lo, hi = wedge_bounds(name)
    return [(int(lo[a:b + 1].sum()), int(hi[a:b + 1].sum())) for a, b in items(name)]
