"""Restatements of the three post-render contracts of csrc/lt_post.hip in plain numpy -- reverse projection
(auxiliary/laserscan.py:475-501), the filter chain and packing of write() (laserscan.py:1138-1178), the array part of compare()
(laserscan.py:1200-1281, np_ioueval.py:40-47) -- and the seeded inputs that drive the kernels at their seams.  No GPU import:
tests/test_post_cpu.py pins the restatements to golden F7 and holds the generators to what they claim;
tests/test_post_shapes_gpu.py compares `lt_reverse_projection_dev`, `lt_pack_scan_dev` and `lt_compare_dev` with them."""
import math

import numpy as np

INT_MAX, INT_MIN = 2147483647, -2147483648
BLOCK, WAVE, CHUNK = 256, 64, 1024 * 256          # cells per workgroup, per wave, per turn of k_pack_scan's chunk loop

# what tests/test_post_shapes_gpu.py fills its output buffers with before a call
SENT_F32 = 0x7FA5A5A5                              # a NaN no conversion produces (numpy and the hardware give 0x7FC00000)
SENT_U32 = 0xA5A5A5A5
SENT_F64 = 0x7FF4DEADBEEF0001
SENT_U64 = 0x5A5A5A5A5A5A5A5A


# ---- reverse projection -----------------------------------------------------------------------------------------------------
def restate_reverse(range_img, px, py, fov_up, fov_down):
    """[H*W, 3] float64.  Every step in float64, in the reference's order: angles to radians, the total field of view from the
    two absolute values, pixel coordinates over the image size, yaw from x and pitch from y, then (depth * sin(pitch)) times
    the cosine / sine of -yaw, and depth * cos(pitch)."""
    rng = np.asarray(range_img)
    H, W = rng.shape
    up = fov_up / 180.0 * np.pi
    down = fov_down / 180.0 * np.pi
    fov = abs(down) + abs(up)
    depth = rng.astype(np.float64)
    x = np.asarray(px).astype(np.float64) / float(W)
    y = np.asarray(py).astype(np.float64) / float(H)
    yaw = (x * 2 - 1.0) * np.pi
    inner = 1.0 * fov - y * fov
    pitch = np.pi / 2 - (inner - abs(down))
    with np.errstate(all="ignore"):
        flat = depth * np.sin(pitch)
        out = np.stack([flat * np.cos(-yaw), flat * np.sin(-yaw), depth * np.cos(pitch)], axis=-1)
    return out.reshape(-1, 3)


def near_f32_tie(v, rel=1e-13):
    """Elements of the float64 array `v` within rel * |v| of the midpoint between two adjacent float32 values: where two float64
    math libraries that agree to rel may round to different float32.

    The window is relative only.  With an absolute 1e-13 added, every element below about 1e-13 lies "near a tie" (float32
    values are spaced far closer than that down there): the whole y column at yaw 0 and at -pi, the z row on the horizon of a
    symmetric field of view, every cell of range 0 or 1e-40 -- a third of the 1 x 1 case -- which no seed can bring under
    1e-4 on a full integer grid.  The relative window marks fewer elements, so more of them have to be bit-equal."""
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        f = v.astype(np.float32)
        up = f.astype(np.float64) < v
        other = np.where(up, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf)))
        other = np.where(f.astype(np.float64) == v, f, other)           # exactly a float32: as far from a tie as it gets
        mid = (f.astype(np.float64) + other.astype(np.float64)) / 2
        near = np.abs(v - mid) <= rel * np.abs(v)
    return near & np.isfinite(v) & (f.astype(np.float64) != v)


REVERSE_SHAPES = [(1, 1), (3, 85), (16, 301), (64, 2048), (128, 2048)]
REVERSE_FOVS = [(3.0, -25.0), (15.0, -15.0), (0.0, -10.0), (-5.0, -25.0)]       # the last one exercises both abs()


def reverse_case(H, W, fov, float_coords, seed=0):
    """(range_img [H, W] f32, px, py, description).  Ranges uniform in 0.5 .. 120 with a fifth of the cells at -1 (empty cells
    of the closest-point adaption) and, from 8 cells on, one cell each at 0, 1e-40 and 3e38.  Integer coordinates: the full
    grid (column 0 and W - 1, row H - 1).  Float coordinates: uniform, with the exact values 0.0 and (size - 2^-40)."""
    rng = np.random.default_rng([seed, H, W, int(float_coords), int(fov[0] * 10) + 1000, int(fov[1] * 10) + 1000])
    n = H * W
    r = rng.uniform(0.5, 120.0, n).astype(np.float32)
    r[rng.random(n) < 0.2] = -1
    if n >= 8:
        r[n // 3], r[n // 2], r[2 * n // 3] = 0.0, 1e-40, 3e38
    if float_coords:
        px, py = rng.uniform(0, W, n), rng.uniform(0, H, n)
        px[-1], py[-1] = W - 2.0 ** -40, H - 2.0 ** -40
        px[0], py[0] = 0.0, (0.0 if n > 1 else H - 2.0 ** -40)          # (one cell: x at one end, y at the other)
        if n >= 8:
            px[1], py[1] = W - 2.0 ** -40, 0.0
            px[2], py[2] = 0.0, H - 2.0 ** -40
    else:
        py, px = (a.reshape(-1).astype(np.int32) for a in np.mgrid[0:H, 0:W])
    what = f"{H}x{W} fov {fov[0]:g}/{fov[1]:g} {'float' if float_coords else 'int'}"
    return r.reshape(H, W), px.reshape(H, W), py.reshape(H, W), what


# ---- scan packer ------------------------------------------------------------------------------------------------------------
def restate_pack(points, label, rem, index=None):
    """(bin [N, 4] float32, label [N] uint32): `index > 0` where there is an index image, then `label >= 0`, then the
    coordinate sum != 0 taken left to right IN THE DTYPE OF THE POINTS; the survivors in order, coordinates rounded to
    float32 the way struct.pack("f") rounds a double, labels as the unsigned 32 bits of the int32."""
    pts = np.asarray(points)
    assert pts.dtype in (np.float32, np.float64), pts.dtype
    pts = pts.reshape(-1, 3)
    lab, rm = np.asarray(label).reshape(-1), np.asarray(rem, np.float32).reshape(-1)
    if index is not None:
        m = np.asarray(index).reshape(-1) > 0
        pts, rm, lab = pts[m], rm[m], lab[m].astype(np.int32)
    m = lab >= 0
    pts, rm, lab = pts[m], rm[m], lab[m].astype(np.int32)
    with np.errstate(all="ignore"):
        s = (pts[:, 0] + pts[:, 1]) + pts[:, 2]
        assert s.dtype == pts.dtype
        m = s != 0
        pts, rm, lab = pts[m], rm[m], lab[m]
        b = np.concatenate([pts.astype(np.float32), rm[:, None]], axis=1)
    return np.ascontiguousarray(b), lab.view(np.uint32).copy()


PACK_NB = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049]          # 1025 / 2049: second / third turn of the chunk loop
PACK_SIZES = [BLOCK * (nb - 1) + 1 for nb in PACK_NB] + [63, 64, 65, 255, 256, 257]
KEEP_PATTERNS = ["all", "none", "first", "last", "one_per_block", "odd_waves", "seam64", "seam256", "seam_chunk", "random50"]


def one_per_block_lane(b, n):
    """the lane kept in block b of n cells: varies with b, inside a ragged last block"""
    return (b * 37 + 11) % min(BLOCK, n - BLOCK * b)


def keep_pattern(name, n, seed=0):
    i = np.arange(n)
    if name == "all":
        return np.ones(n, bool)
    if name == "none":
        return np.zeros(n, bool)
    if name == "first":
        return i == 0
    if name == "last":
        return i == n - 1
    if name == "one_per_block":
        k = np.zeros(n, bool)
        for b in range((n + BLOCK - 1) // BLOCK):
            k[BLOCK * b + one_per_block_lane(b, n)] = True
        return k
    if name == "odd_waves":
        return (i // WAVE) % 2 == 1
    if name == "seam64":
        return np.isin(i % WAVE, (0, WAVE - 1))
    if name == "seam256":
        return np.isin(i % BLOCK, (0, BLOCK - 1))
    if name == "seam_chunk":
        return ((i % CHUNK == 0) | (i % CHUNK == CHUNK - 1)) & (i > 0)
    if name == "random50":
        return np.random.default_rng([seed, n]).random(n) < 0.5
    raise KeyError(name)


def pack_case(n, dtype, keep=None, with_index=False, seed=0):
    """dict(points, label, rem, index, keep).  Row identity: rem[i] = float32(i) (exact below 2^24), label[i] = i | 7 << 16,
    coordinates positive (their sum is not 0 in either dtype).  Cells outside `keep` are dropped by one of the rules in turn:
    (0, 0, 0); label -1 - i; x + y + z == 0 off the origin (1.5, 2.5, -4: exact in both dtypes); index 0; index -1 - i."""
    rng = np.random.default_rng([seed, n, int(with_index), np.dtype(dtype).itemsize])
    keep = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    assert keep.shape == (n,) and n < 1 << 24
    pts = rng.uniform(0.5, 60.0, (n, 3)).astype(dtype)
    i = np.arange(n, dtype=np.int64)
    label = (i | (7 << 16)).astype(np.int32)
    rem = i.astype(np.float32)
    index = (i + 1).astype(np.int32) if with_index else None
    drop = np.flatnonzero(~keep)
    how = (drop * 2654435761 >> 7) % (5 if with_index else 3)
    pts[drop[how == 0]] = 0
    label[drop[how == 1]] = (-1 - drop[how == 1]).astype(np.int32)
    pts[drop[how == 2]] = np.array([1.5, 2.5, -4.0], dtype)
    if with_index:
        index[drop[how == 3]] = 0
        index[drop[how == 4]] = (-1 - drop[how == 4]).astype(np.int32)
    return dict(points=pts, label=label, rem=rem, index=index, keep=keep)


# (point, label, index, kept in float32, kept in float64)
PACK_VALUE_EDGES = [
    ([1e8, -1e8, 1.0], 1, 1, True, True),                      # dropped only by x + (y + z) in float32
    ([1e8, 1.0, -1e8], 2, 2, False, True),                     # (1e8 + 1) rounds back to 1e8 in float32
    ([1e-45, 0.0, 0.0], 3, 3, True, True),                     # float32: the smallest denormal; lost where those are flushed
    ([-0.0, 0.0, 0.0], 4, 4, False, False),
    ([np.nan, 0.0, 0.0], 5, 5, True, True),                    # nan != 0
    ([1.0 + 2.0 ** -24, 2.0, 3.0], 6, 6, True, True),          # float64 -> float32 on a tie: to even, 1.0
    ([1.0 + 2.0 ** -23 + 2.0 ** -24, 2.0, 3.0], 7, 7, True, True),   # the tie above it: to even, upwards
    ([1e-40, 2.0, 3.0], 8, 8, True, True),                     # float64 -> float32 into the denormal range
    ([3e38, -3e38, 3e38], 9, 9, True, True),                   # below float32's maximum
    ([4.0, 5.0, 6.0], (0xFFFF << 16) | 40, 10, True, True),    # bit 31 set: negative as int32, dropped
    ([4.0, 5.0, 6.0], 0x7FFFFFFF, INT_MAX, True, True),
    ([4.0, 5.0, 6.0], (0x7FFF << 16) | 40, 11, True, True),                  # every instance bit below bit 31
    ([4.0, 5.0, 6.0], 12, 0, True, True),                      # index 0 / -1: dropped where there is an index image
    ([4.0, 5.0, 6.0], 13, -1, True, True),
    ([7.0, 8.0, 9.0], 14, 1, True, True),
]


def pack_value_edges(dtype, with_index):
    """the rows of PACK_VALUE_EDGES in `dtype`, and which of them stay.  A label with bit 31 set is negative as int32 and is
    dropped by `label >= 0`; index <= 0 drops the row where there is an index image."""
    pts = np.array([e[0] for e in PACK_VALUE_EDGES], np.float64).astype(dtype)
    label = np.array([e[1] for e in PACK_VALUE_EDGES], np.int64).astype(np.uint32).view(np.int32)
    index = np.array([e[2] for e in PACK_VALUE_EDGES], np.int32)
    keep = np.array([e[3] if np.dtype(dtype) == np.float32 else e[4] for e in PACK_VALUE_EDGES], bool)
    keep &= label >= 0
    if with_index:
        keep &= index > 0
    rem = (np.arange(len(pts)) + 0.25).astype(np.float32)
    return dict(points=pts, label=label, rem=rem, index=index if with_index else None, keep=keep)


# ---- compare ----------------------------------------------------------------------------------------------------------------
def restate_compare_arrays(src_label, src_color, tgt_label, src_range, tgt_range, src_rem, tgt_rem, n_labels):
    """dict(source_label, target_label, range_diff, rem_diff, conf, sq_exact), flat.  A cell whose float32 colour sum
    (r + g) + b is 0 has label 0 in both images; a cell whose source label is 0 has target label 0, and range and remission 0
    in both.  Differences: float32 (a - b) * (a - b).  conf[target, source]: int64 counts of the cells with both masked
    labels in 0 .. n_labels - 1.  sq_exact: the exactly rounded sum of range_diff."""
    f32 = np.float32
    sl = np.array(src_label, np.int32).reshape(-1)
    tl = np.array(tgt_label, np.int32).reshape(-1)
    c = np.asarray(src_color, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        black = ((c[:, 0] + c[:, 1]) + c[:, 2]) == 0
    sl[black] = 0
    tl[black] = 0
    bg = sl == 0
    tl[bg] = 0

    def diff(a, b):
        a = np.where(bg, f32(0), np.asarray(a, f32).reshape(-1))
        b = np.where(bg, f32(0), np.asarray(b, f32).reshape(-1))
        d = a - b
        assert d.dtype == f32
        return d * d

    range_diff = diff(src_range, tgt_range)
    rem_diff = diff(src_rem, tgt_rem) if src_rem is not None else None
    ok = (sl >= 0) & (sl < n_labels) & (tl >= 0) & (tl < n_labels)
    conf = np.bincount(tl[ok].astype(np.int64) * n_labels + sl[ok], minlength=n_labels * n_labels).reshape(n_labels, n_labels)
    return dict(source_label=sl, target_label=tl, range_diff=range_diff, rem_diff=rem_diff, conf=conf.astype(np.int64),
                sq_exact=math.fsum(range_diff.astype(np.float64).tolist()))


def block_tree_sum(d2):
    """the sum of up to 256 float32 values as ONE workgroup of k_compare adds them in float64: a xor butterfly over the 64 lanes
    of each wave (lane 0 ends with the halving tree), the four waves as (w0 + w1) + (w2 + w3), added onto 0.0"""
    v = np.asarray(d2, np.float32).reshape(-1).astype(np.float64)
    assert len(v) <= BLOCK
    v = np.concatenate([v, np.zeros(BLOCK - len(v))]).reshape(4, WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v[:, :o] + v[:, o:2 * o]
    return 0.0 + ((v[0, 0] + v[1, 0]) + (v[2, 0] + v[3, 0]))


COMPARE_SIZES = [1, 63, 65, 255, 257, 4096, 131072]
COMPARE_NLABELS = [1, 20, 64, 300, 512]
OUTSIDE = lambda n_labels: [-1, n_labels, INT_MAX, INT_MIN]    # noqa: E731  labels no cell is counted under


def compare_random(n, n_labels, seed=0):
    """dict of flat inputs: labels over 0 .. n_labels - 1 (four in five target labels agree), 3 % of either image outside
    that range, a tenth of the colours black, ranges 0 .. 80, remissions 0 .. 1"""
    rng = np.random.default_rng([seed, n, n_labels])
    sl = rng.integers(0, n_labels, n).astype(np.int32)
    tl = np.where(rng.random(n) < 0.8, sl, rng.integers(0, n_labels, n)).astype(np.int32)
    out = np.array(OUTSIDE(n_labels), np.int64)
    m = rng.random(n) < 0.03
    sl[m] = rng.choice(out, int(m.sum())).astype(np.int32)
    m = rng.random(n) < 0.03
    tl[m] = rng.choice(out, int(m.sum())).astype(np.int32)
    color = rng.uniform(0.05, 1.0, (n, 3)).astype(np.float32)
    color[rng.random(n) < 0.1] = 0
    return dict(src_label=sl, src_color=color, tgt_label=tl, src_range=rng.uniform(0, 80, n).astype(np.float32),
                tgt_range=rng.uniform(0, 80, n).astype(np.float32), src_rem=rng.random(n).astype(np.float32),
                tgt_rem=rng.random(n).astype(np.float32), n_labels=n_labels, what=f"random n={n} n_labels={n_labels}")


BLACK_COLORS = [(0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (0.5, -0.5, 0.0)]
NOT_BLACK = (1e-30, 0.0, 0.0)
WAVE_KINDS = ["distinct64", "one_pair", "target_only", "source_only", "zeros_and_uncounted", "wave_per_pair", "black"]


def compare_waves(n_labels, seed=0):
    """Constructed waves, each kind in a block of its own (`kinds[b]` names block b; needs n_labels >= 9):
    distinct64           wave 0: 64 lanes, 64 distinct pairs (source 1 .. 8, target 0 .. 7); the other waves: another 64 each
    one_pair             256 lanes, one pair
    target_only          one source label, five target labels in turn;  source_only: the other way round
    zeros_and_uncounted  even lanes genuine (0, 0) cells, odd lanes a label outside 0 .. n_labels - 1 in either image
    wave_per_pair        four waves, each with one pair of its own
    black                the three black colours and the one that is not, over non-zero labels"""
    assert n_labels >= 9
    rng = np.random.default_rng([seed, n_labels])
    lane = np.arange(BLOCK)
    top = n_labels - 1
    out = np.array(OUTSIDE(n_labels), np.int64)
    sl, tl, col, kinds = [], [], [], []

    def add(kind, s, t, c=None):
        kinds.append(kind)
        sl.append(np.broadcast_to(np.asarray(s, np.int64), (BLOCK,)).astype(np.int32))
        tl.append(np.broadcast_to(np.asarray(t, np.int64), (BLOCK,)).astype(np.int32))
        col.append(np.full((BLOCK, 3), 0.5, np.float32) if c is None else np.asarray(c, np.float32))

    w = lane // WAVE
    add("distinct64", 1 + (lane % 8), ((lane % WAVE) // 8 + w) % n_labels)
    add("one_pair", top, 3)
    add("target_only", 3, lane % 5)
    add("source_only", 1 + lane % 5, 3)
    odd = lane % 2 == 1
    pick = out[(lane // 2) % 4]
    in_source = (lane // 8) % 2 == 0
    add("zeros_and_uncounted", np.where(odd, np.where(in_source, pick, 2), 0), np.where(odd, np.where(in_source, 2, pick), 5))
    add("wave_per_pair", np.array([1, top, 2, 1])[w], np.array([top, 1, 2, 0])[w])
    c = np.array((BLACK_COLORS + [NOT_BLACK])[:4], np.float32)[lane % 4]
    add("black", 1 + lane % 3, 4)
    col[-1] = c
    n = BLOCK * len(kinds)
    return dict(src_label=np.concatenate(sl), src_color=np.concatenate(col), tgt_label=np.concatenate(tl),
                src_range=rng.uniform(0, 80, n).astype(np.float32), tgt_range=rng.uniform(0, 80, n).astype(np.float32),
                src_rem=rng.random(n).astype(np.float32), tgt_rem=rng.random(n).astype(np.float32), n_labels=n_labels,
                kinds=kinds, what=f"waves n_labels={n_labels}")
