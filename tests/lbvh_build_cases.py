"""The LBVH build (lidar_transfer_amd/csrc/lt_build.hip) restated in numpy from its definition, the meshes that take each
of its seams on purpose, and the comparers.  Imports without a GPU: tests/test_lbvh_build_cpu.py pins the restatement
itself, tests/test_lbvh_build_gpu.py holds the device's sorted keys, triangle records, params, node arrays and queue
counter to it bit for bit.

restate_build(verts, faces) is float32 throughout and follows the definition, not the kernels:
  * bounds over ALL vertices with fmin / fmax (a NaN is dropped as fminf drops it), scale = 1024 / ext or 0,
    pad = 1e-4f + 2e-6f * maxabs;
  * key of a face: centroid ((v0 + v1) + v2) / 3, each axis clamped to [0, 1023] and truncated, 10 bits per axis, x bit
    highest; a face with an index outside [0, n_verts) gets 0x3FFFFFFF, a zero record with its face id, the empty box;
  * order = stable argsort of the keys; record (v0, v1 - v0, v2 - v0, face); leaf box = min / max of the three vertices
    -+ pad;
  * the tree TOP DOWN: the node that owns [first, last] splits it where the unique keys (key << 32 | slot) first differ
    from first's in the highest bit in which first and last differ -- a count of the slots below that bit boundary, no
    search; left child = node g, right child = node g + 1, root = node 0;
  * the box of a range is the plain reduction over its leaf boxes.
"""
import collections
import functools
import os
import re

import numpy as np

import lbvh_cases as lc

LT_LEAF_MAX = lc._define("LT_LEAF_MAX")
LT_SORT_TILE = lc._define("LT_SORT_TILE")
LT_SEG_SUB = lc._define("LT_SEG_SUB")


def _define_build(name):
    """A constant of lt_build.hip, from the source."""
    with open(os.path.join(lc.ROOT, "lidar_transfer_amd", "csrc", "lt_build.hip")) as f:
        m = re.search(r"^#define %s\s+(\d+)\b" % name, f.read(), re.M)
    return int(m.group(1))


LT_HBIG = _define_build("LT_HBIG")
LT_HNODES = _define_build("LT_HNODES")
LT_HWIN = _define_build("LT_HWIN")
LT_RB = 10                        # digit width of the radix sort (lt_build.hip, the default of LT_RB)
SCAN_ROUND = 256                  # tiles k_scan takes per round (its workgroup size)
UNUSED = lc.UNUSED
BAD_KEY = 0x3FFFFFFF
FILL = 0xAB                       # byte the tests fill the node array with before the build under test
F32 = np.float32
INF_BITS = int(np.array([np.inf], F32).view(np.uint32)[0])

# lt_debug_build_get's `what`
GET_KEYS, GET_TRIS, GET_PARAMS, GET_NODES2, GET_QUEUED = range(5)

Build = collections.namedtuple(
    "Build", "n params keys order tris nodes2 nodes4 live first last split leaf_lo leaf_hi pad valid")


def leaf_ref(start, count):
    return ~(start | ((count - 1) << 28)) & 0xFFFFFFFF


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def morton30(q):
    """[n, 3] cell coordinates (0 .. 1023) -> 30-bit key, bit b of axis a at position 3 b + (2 - a)"""
    q = np.asarray(q, np.uint32)
    key = np.zeros(len(q), np.uint32)
    for b in range(10):
        for a in range(3):
            key |= ((q[:, a] >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + (2 - a))
    return key


def karras_ranges(keys):
    """Sorted 32-bit keys -> (first, last, split) of every node 0 .. n - 2, by the top-down definition: node 0 owns
    [0, n - 1]; the owner of [first, last] splits after the last slot whose unique key lies below the boundary 'common
    prefix of first and last, then a one'; its left part belongs to node split, its right part to node split + 1."""
    n = len(keys)
    ukey = (np.asarray(keys, np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    first = np.full(max(n - 1, 0), -1, np.int64)
    last = np.full(max(n - 1, 0), -1, np.int64)
    split = np.full(max(n - 1, 0), -1, np.int64)
    todo = [(0, 0, n - 1)] if n > 1 else []
    while todo:
        i, a, b = todo.pop()
        assert first[i] < 0, "a node is owned twice"
        diff = int(ukey[a]) ^ int(ukey[b])
        top = diff.bit_length() - 1                      # the highest bit in which a and b differ
        boundary = (int(ukey[a]) >> top | 1) << top
        g = a + int(np.count_nonzero(ukey[a:b + 1] < np.uint64(boundary))) - 1
        first[i], last[i], split[i] = a, b, g
        if g > a:
            todo.append((g, a, g))
        if b > g + 1:
            todo.append((g + 1, g + 1, b))
    return first, last, split


def restate_build(verts, faces, fill=FILL):
    """-> Build: params [5] f32, keys [n] u32 (sorted), order [n] (face id of every sorted slot), tris [n, 12] u32,
    nodes2 [n, 16] u32 (binary; a dead node: both references UNUSED, boxes zero here and unspecified on the device),
    nodes4 [n, 32] u32 (a dead node: the fill pattern), live [n] bool, first / last / split of every Karras node, the
    padded leaf boxes of the sorted slots.  Node arrays have n rows: row n - 1 is never a node and stays dead."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    n, nv = len(f), len(v)
    with np.errstate(all="ignore"):
        lo = np.fmin.reduce(v, axis=0, initial=F32(np.inf))
        hi = np.fmax.reduce(v, axis=0, initial=F32(-np.inf))
        d = hi - lo
        ext = np.fmax(np.fmax(d[0], d[1]), d[2])
        scale = F32(1024.0) / ext if ext > 0 else F32(0.0)
        al, ah = np.abs(lo), np.abs(hi)
        maxabs = np.fmax(np.fmax(np.fmax(al[0], ah[0]), np.fmax(al[1], ah[1])), np.fmax(al[2], ah[2]))
        pad = F32(1e-4) + F32(2e-6) * maxabs
        params = np.array([lo[0], lo[1], lo[2], scale, pad], F32)
        valid = np.all((f >= 0) & (f < nv), axis=1)
        t = np.zeros((n, 3, 3), F32)
        t[valid] = v[f[valid]]
        cen = ((t[:, 0] + t[:, 1]) + t[:, 2]) / F32(3.0)
        q = np.fmin(np.fmax((cen - lo) * scale, F32(0.0)), F32(1023.0))
        keys = np.where(valid, morton30(q.astype(np.uint32)), np.uint32(BAD_KEY)).astype(np.uint32)
        order = np.argsort(keys, kind="stable")
        skeys = keys[order]
        ts, ok = t[order], valid[order]
        rec = np.zeros((n, 12), np.uint32)
        rec[:, 0:3] = _bits(ts[:, 0])
        rec[:, 3:6] = _bits(ts[:, 1] - ts[:, 0])
        rec[:, 6:9] = _bits(ts[:, 2] - ts[:, 0])
        rec[~ok, 0:9] = 0
        rec[:, 9] = order.astype(np.uint32)
        leaf_lo = np.fmin(np.fmin(ts[:, 0], ts[:, 1]), ts[:, 2]) - pad
        leaf_hi = np.fmax(np.fmax(ts[:, 0], ts[:, 1]), ts[:, 2]) + pad
        leaf_lo[~ok], leaf_hi[~ok] = np.inf, -np.inf

    def box(a, b):
        return np.concatenate([np.fmin.reduce(leaf_lo[a:b + 1], axis=0), np.fmax.reduce(leaf_hi[a:b + 1], axis=0)])

    fill_word = np.uint32(fill * 0x01010101)
    nodes4 = np.full((n, 32), fill_word, np.uint32)
    nodes2 = np.zeros((n, 16), np.uint32)
    nodes2[:, 12:14] = UNUSED
    live = np.zeros(n, bool)
    empty = np.array([INF_BITS] * 6 + [UNUSED, 0], np.uint32)
    first, last, split = karras_ranges(skeys)

    def ref(a, b, node):
        """reference of the child that owns [a, b]: a leaf of at most LT_LEAF_MAX slots, or `node`"""
        return leaf_ref(a, b - a + 1) if b - a + 1 <= LT_LEAF_MAX else node

    def entries(a, b, node):
        """the entries the range [a, b] (owned by `node` unless it is a leaf) contributes to its parent's 4-wide node"""
        if b - a + 1 <= LT_LEAF_MAX:
            return [(a, b, ref(a, b, node))]
        g = int(split[node])
        return [(a, g, ref(a, g, g)), (g + 1, b, ref(g + 1, b, g + 1))]

    if n == 1:
        live[0] = True
        nodes4[0] = np.tile(empty, 4)
        nodes4[0, 0:6] = _bits(box(0, 0))
        nodes4[0, 6] = leaf_ref(0, 1)
        nodes2[0, 0:6] = _bits(box(0, 0))
        nodes2[0, 6:12] = INF_BITS
        nodes2[0, 12:14] = leaf_ref(0, 1)
    for i in range(n - 1):
        a, b, g = int(first[i]), int(last[i]), int(split[i])
        if i != 0 and b - a + 1 <= LT_LEAF_MAX:
            continue
        live[i] = True
        nodes2[i, 0:6] = _bits(box(a, g))
        nodes2[i, 6:12] = _bits(box(g + 1, b))
        nodes2[i, 12] = ref(a, g, g)
        nodes2[i, 13] = ref(g + 1, b, g + 1)
        ent = entries(a, g, g) + entries(g + 1, b, g + 1)
        row = np.tile(empty, 4)
        for k, (ea, eb, child) in enumerate(ent):
            row[8 * k:8 * k + 6] = _bits(box(ea, eb))
            row[8 * k + 6] = child
        nodes4[i] = row
    return Build(n, params, skeys, order, rec, nodes2, nodes4, live, first, last, split, leaf_lo, leaf_hi, pad, valid)


def queued_expected(b):
    """nodes k_hierarchy4 hands to k_hierarchy4_big: those whose range has at least LT_HBIG + 1 slots"""
    return int(np.count_nonzero(b.last - b.first + 1 >= LT_HBIG + 1)) if b.n > 1 else 0


# ---- comparers ----------------------------------------------------------------------------------------------------------
FIELDS4 = ("mn.x", "mn.y", "mn.z", "mx.x", "mx.y", "mx.z", "ref", "zero")
Finding = collections.namedtuple("Finding", "node entry field got want")


def _float_words_differ(got, want):
    """uint32 words of floats: equal bits, or both NaN whatever the payload"""
    g, w = got.view(F32), want.view(F32)
    return (got != want) & ~(np.isnan(g) & np.isnan(w))


def compare_nodes(got, want, fill=FILL):
    """[n, 32] uint32 4-wide node arrays -> list of Finding(node, entry, field, got word, want word).  A node that is dead
    in `want` (all 128 bytes the fill pattern) must hold the fill pattern in `got`; of a live node the box words compare
    as float bits with NaN == NaN, the reference and the trailing zero as bits."""
    got = np.ascontiguousarray(got, np.uint32).reshape(-1, 32)
    want = np.ascontiguousarray(want, np.uint32).reshape(-1, 32)
    if got.shape != want.shape:
        return [Finding(-1, -1, "shape", got.shape, want.shape)]
    dead = np.all(want == np.uint32(fill * 0x01010101), axis=1)
    is_float = np.tile(np.array([1, 1, 1, 1, 1, 1, 0, 0], bool), 4)
    bad = np.where(dead[:, None] | ~is_float[None, :], got != want, _float_words_differ(got, want))
    out = []
    for node, word in zip(*np.nonzero(bad)):
        field = "fill" if dead[node] else FIELDS4[word % 8]
        out.append(Finding(int(node), int(word // 8), field, int(got[node, word]), int(want[node, word])))
    return out


FIELDS2 = ("b0.mn.x", "b0.mn.y", "b0.mn.z", "b0.mx.x", "b0.mx.y", "b0.mx.z", "b1.mn.x", "b1.mn.y", "b1.mn.z", "b1.mx.x",
           "b1.mx.y", "b1.mx.z", "c0", "c1", "zero", "zero")


def compare_nodes2(got, want):
    """[n, 16] uint32 binary node arrays (lt_internal.h: b0, b1, c0, c1, -, -) -> findings; entry = child 0 or 1.  A node
    that is dead in `want` (both references UNUSED) must be dead in `got`: its boxes are unspecified."""
    got = np.ascontiguousarray(got, np.uint32).reshape(-1, 16)
    want = np.ascontiguousarray(want, np.uint32).reshape(-1, 16)
    if got.shape != want.shape:
        return [Finding(-1, -1, "shape", got.shape, want.shape)]
    dead = np.all(want[:, 12:14] == UNUSED, axis=1)
    bad = got != want
    bad[:, :12] = _float_words_differ(got[:, :12], want[:, :12]) & ~dead[:, None]
    out = []
    for node, word in zip(*np.nonzero(bad)):
        entry = int(word // 6) if word < 12 else int(word - 12) % 2
        out.append(Finding(int(node), entry, FIELDS2[word], int(got[node, word]), int(want[node, word])))
    return out


def compare_words(got, want, float_cols, what):
    """two [n, k] uint32 arrays whose columns `float_cols` hold floats (NaN == NaN), the others integers -> findings with
    node = row, entry = column"""
    got = np.ascontiguousarray(got, np.uint32).reshape(np.shape(want))
    want = np.ascontiguousarray(want, np.uint32)
    isf = np.zeros(want.shape[-1], bool)
    isf[list(float_cols)] = True
    bad = np.where(isf, _float_words_differ(got, want), got != want)
    return [Finding(int(r), int(c), what, int(got[r, c]), int(want[r, c])) for r, c in zip(*np.nonzero(bad))]


def compare_build(b, keys, tris, params, queued):
    """the products of lt_debug_build_get against a Build -> findings"""
    out = compare_words(np.reshape(keys, (-1, 1)), b.keys.reshape(-1, 1), (), "key")
    out += compare_words(np.reshape(tris, (-1, 12)), b.tris, range(9), "tris")
    out += compare_words(np.reshape(_bits(params), (1, 5)), _bits(b.params).reshape(1, 5), range(5), "params")
    if int(queued) != queued_expected(b):
        out.append(Finding(-1, -1, "queued", int(queued), queued_expected(b)))
    return out


def sort_reference(keys, vals, key_bits):
    keys, vals = np.asarray(keys, np.uint32), np.asarray(vals, np.uint32)
    mask = np.uint32((1 << key_bits) - 1)
    order = np.argsort(keys & mask, kind="stable")
    return keys[order], vals[order]


def compare_sort(keys, vals, key_bits, keys_out, vals_out):
    """-> findings of a (keys_out, vals_out) against the stable sort of (keys, vals) on the low key_bits bits.  Field
    "key": a key is out of place; "stability": the keys are right and every run of equal sort keys holds its own values,
    but not in input order; "value": a value left its key."""
    want_k, want_v = sort_reference(keys, vals, key_bits)
    keys_out, vals_out = np.asarray(keys_out, np.uint32), np.asarray(vals_out, np.uint32)
    if keys_out.shape != want_k.shape or vals_out.shape != want_v.shape:
        return [Finding(-1, -1, "shape", keys_out.shape, want_k.shape)]
    bad = np.nonzero(keys_out != want_k)[0]
    if bad.size:
        return [Finding(int(p), 0, "key", int(keys_out[p]), int(want_k[p])) for p in bad[:16]]
    bad = np.nonzero(vals_out != want_v)[0]
    if not bad.size:
        return []
    # the same values inside every run of equal sort keys?
    masked = want_k & np.uint32((1 << key_bits) - 1)
    run = np.concatenate([[0], np.cumsum(masked[1:] != masked[:-1])])
    same_runs = np.array_equal(vals_out[np.lexsort((vals_out, run))], want_v[np.lexsort((want_v, run))])
    field = "stability" if same_runs else "value"
    return [Finding(int(p), 1, field, int(vals_out[p]), int(want_v[p])) for p in bad[:16]]


# ---- the sort cases -----------------------------------------------------------------------------------------------------
SORT_SIZES = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289)
SCAN_TILES = SCAN_ROUND * LT_SORT_TILE               # 1 048 576 keys: the most one round of k_scan covers
SORT_BIG_SIZES = (SCAN_TILES - 1, SCAN_TILES, SCAN_TILES + 1, 2 * SCAN_TILES + LT_SORT_TILE + 1)
SORT_PATTERN_SIZES = (1025, 4097, 12289, SCAN_TILES + 1)
SORT_PATTERNS = ("random30", "equal", "digit0", "digit1", "digit2", "two", "ascending", "descending", "ties17",
                 "random32")
SORT_BIG_PATTERNS = ("random30", "ties17")


def sort_tiles_rounds(n):
    """(tiles of a sort of n keys, rounds k_scan makes over a digit's row)"""
    tiles = -(-n // LT_SORT_TILE)
    return tiles, -(-tiles // SCAN_ROUND)


def sort_input(pattern, n, seed=0):
    """-> (keys u32 [n], vals u32 [n], key_bits).  vals: a seeded permutation of distinct words with high bits set -- not
    arange, so a kernel that recomputes a value instead of carrying it fails."""
    rng = np.random.default_rng([seed, n, SORT_PATTERNS.index(pattern)])
    vals = (rng.permutation(n).astype(np.uint32) * np.uint32(2654435761) + np.uint32(0x80000001)).astype(np.uint32)
    bits = 30
    if pattern == "random30":
        keys = rng.integers(0, 1 << 30, n, dtype=np.uint32)
    elif pattern == "equal":
        keys = np.full(n, 0x2AAAAAAA, np.uint32)
    elif pattern in ("digit0", "digit1", "digit2"):
        d = int(pattern[-1])
        keys = (np.uint32(0x15555555 & ~(0x3FF << (LT_RB * d)))
                | (rng.integers(0, 1 << LT_RB, n, dtype=np.uint32) << np.uint32(LT_RB * d))).astype(np.uint32)
    elif pattern == "two":
        keys = np.where(np.arange(n) % 2 == 0, 0x3FFFFFFF, 0x00000400).astype(np.uint32)
    elif pattern == "ascending":
        keys = np.sort(rng.integers(0, 1 << 30, n, dtype=np.uint32))
    elif pattern == "descending":
        keys = np.sort(rng.integers(0, 1 << 30, n, dtype=np.uint32))[::-1].copy()
    elif pattern == "ties17":
        keys = rng.integers(0, 1 << 30, 17, dtype=np.uint32)[rng.integers(0, 17, n)]
    elif pattern == "random32":
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    else:
        raise KeyError(pattern)
    return np.ascontiguousarray(keys, np.uint32), vals, bits


# ---- the build cases ----------------------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 4, 5, 6, 8, 9, 255, 256, 257, 258, 511, 512, 513, 1024, 1025, 1026, 2049, 4095, 4096, 4097, 8193)


class Case:
    """A named, seeded mesh.  `bad_index`: lt_scene_status must report LT_ERR_BAD_INDEX; `finite`: every vertex is."""

    def __init__(self, name, seed, make, bad_index=False, finite=True):
        self.name, self.seed, self._make, self.bad_index, self.finite = name, seed, make, bad_index, finite

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def mesh(self):
        v, f, c, r = self._make(np.random.default_rng(self.seed))
        return (np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int32), np.ascontiguousarray(c, np.int32),
                np.ascontiguousarray(r, F32))

    @functools.lru_cache(maxsize=None)
    def build(self):
        v, f, _, _ = self.mesh()
        return restate_build(v, f)

    @property
    def n(self):
        return len(self.mesh()[1])


@functools.lru_cache(maxsize=None)
def _synth_pool():
    from lidar_transfer_amd.synth import synth_scene
    return synth_scene(3, 9000)


def synth_faces(rng, n):
    """n faces of one indexed mesh with shared vertices, drawn without replacement; all its vertices stay (the
    unreferenced ones count for the bounds)"""
    v, f, c, r = _synth_pool()
    return v, f[rng.choice(len(f), n, replace=False)], c, r


def _with_far_vertices(rng):
    v, f, c, r = synth_faces(rng, 700)
    far = np.array([[900.0, -40.0, 3.0], [-20.0, 30.0, -700.0]], F32)
    return (np.concatenate([v, far]), f, np.concatenate([c, np.zeros((2, 3), np.int32)]),
            np.concatenate([r, np.zeros(2, F32)]))


def _with_bad_indices(rng):
    v, f, c, r = synth_faces(rng, 600)
    f = f.copy()
    f[17, 0] = -1
    f[301, 1] = len(v)
    f[599, 2] = len(v) + 12345
    return v, f, c, r


def _with_values(vals):
    def make(rng):
        v, f, c, r = synth_faces(rng, 900)
        v = v.copy()
        used = np.unique(f)
        for k, val in enumerate(vals):
            v[used[rng.integers(0, len(used))], k % 3] = val
        return v, f, c, r
    return make


def _cases():
    out = []
    for n in SIZES:
        out.append(Case(f"synth_{n}", 1000 + n, lambda rng, n=n: synth_faces(rng, n)))
        out.append(Case(f"soup_{n}", 2000 + n, lambda rng, n=n: lc.adversarial_soup(rng, n)))
    for n in (5, 257, 600, 1300, 3000):
        out.append(Case(f"identical_{n}", 3000 + n, lambda rng, n=n: lc.mesh_of(lc.identical(n), rng)))
    for copies in (40, 600):
        out.append(Case(f"stairs_14x{copies}", 4000 + copies,
                        lambda rng, c=copies: lc.mesh_of(np.concatenate(lc.cluster_stairs(rng, 14, c)), rng)))
    out.append(Case("same_box_pinned_300", 5300, lambda rng: lc.mesh_of(lc.same_box_pinned(300, rng), rng)))
    out.append(Case("deep_staircase_64", 4242, lambda rng: lc.deep_staircase(64)))
    out.append(Case("far_vertices", 6001, _with_far_vertices))
    out.append(Case("bad_index", 6002, _with_bad_indices, bad_index=True))
    out.append(Case("nan_vertex", 6003, _with_values([np.nan, np.nan, np.nan, np.nan]), finite=False))
    out.append(Case("inf_vertex", 6004, _with_values([np.inf, -np.inf, np.inf]), finite=False))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
BINARY_CASES = ("synth_1", "synth_5", "synth_257", "synth_1026", "identical_600", "bad_index")


# ---- which path a case takes, from the restatement ------------------------------------------------------------------------
def figures(b):
    """What decides the build's paths for a Build:
    tiles, quarter: sort tiles, and the 1024-key wave quarters the last tile fills; np, seg_blocks: leaves of the segment
    tree, workgroups of k_seg_sub (more than one: k_seg_top runs); workgroups: of k_hierarchy4; live: nodes written;
    queued: nodes of at least LT_HBIG + 1 slots (k_hierarchy4_big); second_wg: live nodes beyond the first LT_HNODES;
    crossing: small live nodes whose range leaves the LT_HNODES slots of their own workgroup (they need the key window);
    max_range: slots of the largest range."""
    n = b.n
    np_ = 1
    while np_ < n:
        np_ <<= 1
    fig = dict(n=n, tiles=-(-n // LT_SORT_TILE), quarter=-(-(n % LT_SORT_TILE or LT_SORT_TILE) // 1024), np=np_,
               seg_blocks=np_ // min(np_, LT_SEG_SUB), workgroups=-(-max(n - 1, 1) // LT_HNODES),
               live=int(b.live.sum()), queued=queued_expected(b), second_wg=int(b.live[LT_HNODES:].sum()), crossing=0,
               max_range=int((b.last - b.first + 1).max()) if n > 1 else 1)
    if n > 1:
        i = np.nonzero(b.live[:n - 1])[0]
        size = b.last[i] - b.first[i] + 1
        small = size <= LT_HBIG
        i, f, l, size = i[small], b.first[i][small], b.last[i][small], size[small]
        w0 = i // LT_HNODES * LT_HNODES
        fig["crossing"] = int(np.count_nonzero((f < w0) | (l >= w0 + LT_HNODES)))
    return fig
