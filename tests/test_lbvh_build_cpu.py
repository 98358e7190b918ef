"""The numpy restatement of the LBVH build (tests/lbvh_build_cases.py), pinned without a GPU: what a correct tree must
hold whatever built it, the Karras rule checked node by node against the textbook per-node formula with linear scans,
the comparers' sensitivity, and -- a case whose condition does not hold is a wrong input, not a pass -- the figures that
say which seam of lt_build.hip every case of tests/test_lbvh_build_gpu.py crosses."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import lbvh_build_cases as bc  # noqa: E402
import lbvh_cases as lc  # noqa: E402

NAMES = [c.name for c in bc.CASES]


def _signed(ref):
    ref = int(ref)
    return ref - (1 << 32) if ref >> 31 else ref


def _leaf(ref):
    r = ~_signed(ref)
    return r & 0x0FFFFFFF, (r >> 28) + 1


def _walk4(b):
    """-> (leaves [(start, count, box words)], node entries [(node, child node, box words)]) reachable from node 0 of the
    4-wide array"""
    leaves, inner, todo, seen = [], [], [0], set()
    while todo:
        i = todo.pop()
        assert i not in seen and b.live[i], f"node {i} is referenced twice or dead"
        seen.add(i)
        for k in range(4):
            e = b.nodes4[i, 8 * k:8 * k + 8]
            if e[6] == bc.UNUSED:
                assert np.all(e[:6] == bc.INF_BITS) and e[7] == 0
                assert np.all(b.nodes4[i, 8 * k + 6::8] == bc.UNUSED), "entries are not compacted"
                continue
            assert e[7] == 0
            if _signed(e[6]) < 0:
                leaves.append(_leaf(e[6]) + (e[:6].view(np.float32),))
            else:
                inner.append((i, int(e[6]), e[:6].view(np.float32)))
                todo.append(int(e[6]))
    return leaves, inner


def _walk2(b):
    leaves, todo = [], [0]
    while todo:
        i = todo.pop()
        refs = b.nodes2[i, 12:14]
        assert np.all(b.nodes2[i, 14:16] == 0)
        if b.n == 1:   # one leaf, the second child is the never-hit box with the same reference
            assert refs[0] == refs[1] and np.all(b.nodes2[i, 6:12] == bc.INF_BITS)
            refs = refs[:1]
        for r in refs:
            assert r != bc.UNUSED, f"dead node {i} is referenced"
            if _signed(r) < 0:
                leaves.append(_leaf(r))
            else:
                todo.append(int(r))
    return leaves


@pytest.mark.parametrize("name", NAMES)
def test_tree_invariants(name):
    case = bc.BY_NAME[name]
    b = case.build()
    v, f, _, _ = case.mesh()
    n = b.n
    assert n == len(f) and sorted(b.order.tolist()) == list(range(n))
    assert np.all(b.keys[1:] >= b.keys[:-1])
    leaves, inner = _walk4(b)
    cover = np.zeros(n, int)
    for start, count, _ in leaves:
        assert 1 <= count <= bc.LT_LEAF_MAX
        cover[start:start + count] += 1
    assert np.all(cover == 1), "a sorted slot is in no leaf, or in two"
    assert sorted(l[:2] for l in leaves) == sorted(_walk2(b)), "binary and 4-wide arrays name different leaves"
    # live = the root and every node of more than LT_LEAF_MAX slots; every live node is reachable in the binary tree
    if n > 1:
        size = b.last - b.first + 1
        want_live = size > bc.LT_LEAF_MAX
        want_live[0] = True
        assert np.array_equal(b.live[:n - 1], want_live) and not b.live[n - 1]
    # boxes: every entry holds the vertices of its triangles with `pad` to spare (valid faces of finite meshes)
    assert case.finite == bool(np.all(np.isfinite(v)))
    assert case.bad_index == (not np.all(b.valid))
    assert int((~b.valid).sum()) == (3 if case.bad_index else 0)
    if case.finite:
        pad = b.pad
        t = np.zeros((n, 3, 3), np.float32)
        t[b.valid] = v[f[b.valid]]
        t = t[b.order]
        ok = b.valid[b.order]
        ranges = [(s, s + c - 1, box) for s, c, box in leaves]
        ranges += [(int(b.first[c]), int(b.last[c]), box) for _, c, box in inner]
        for a, z, box in ranges:
            tv = t[a:z + 1][ok[a:z + 1]].reshape(-1, 3)
            if len(tv):
                assert np.all(box[:3] <= tv - pad) and np.all(box[3:] >= tv + pad), (a, z)
            else:
                assert np.all(box[:3] == np.inf) and np.all(box[3:] == -np.inf)
    # no case may depend on the sign of a zero: fminf(-0, +0) is pinned on neither side
    # (no padded leaf box holds a zero; the bounds may -- deep_staircase pins a corner at the origin -- but then no vertex
    # is a NEGATIVE zero, so the minimum is +0 in any order)
    assert not np.any(b.leaf_lo == 0) and not np.any(b.leaf_hi == 0)
    assert not np.any((v == 0) & np.signbit(v))
    if case.finite and not case.bad_index:
        assert np.array_equal(b.keys, lc.morton_keys(v, f)[b.order])
    if case.bad_index:
        bad = np.nonzero(~b.valid)[0]
        assert np.array_equal(b.order[-3:], bad) and np.all(b.keys[-3:] == bc.BAD_KEY)
        assert np.all(b.tris[-3:, :9] == 0) and np.array_equal(b.tris[-3:, 9], bad)
    assert np.all(b.tris[:, 10:] == 0) and np.array_equal(b.tris[:, 9], b.order)


# ---- the Karras rule, exhaustively on small n ---------------------------------------------------------------------------
def _textbook(keys):
    """Karras 2012, per node, with linear scans: direction from the neighbours' deltas, the range end as the farthest slot
    whose delta stays above dmin, the split as the farthest slot whose delta stays above the range's own"""
    n = len(keys)
    uk = [(int(k) << 32) | p for p, k in enumerate(keys)]

    def delta(i, j):
        return -1 if j < 0 or j >= n else 64 - (uk[i] ^ uk[j]).bit_length()

    out = []
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        j = i
        while delta(i, j + d) > dmin:
            j += d
        dn = delta(i, j)
        s = i
        while delta(i, s + d) > dn:
            s += d
        g = s + min(d, 0)
        out.append((min(i, j), max(i, j), g))
    return out


def _small_key_sets():
    rng = np.random.default_rng(31)
    yield np.zeros(1, np.uint32)
    for n in list(range(2, 34)) + [47, 64, 65, 100]:
        yield np.zeros(n, np.uint32)                                            # the index alone decides
        yield np.sort(rng.choice(1 << 30, n, replace=False).astype(np.uint32))  # the keys alone decide
        yield np.sort(rng.integers(0, 1 << 30, 3, dtype=np.uint32)[rng.integers(0, 3, n)])   # long runs of ties
        yield np.sort(rng.integers(0, 8, n, dtype=np.uint32) << np.uint32(rng.integers(0, 27)))
        yield np.sort(np.uint32(0x3FFFFFFF) >> rng.integers(0, 30, n).astype(np.uint32))     # a staircase of prefixes


def test_recursion_equals_the_textbook_delta_rule_on_every_node():
    count = 0
    for keys in _small_key_sets():
        first, last, split = bc.karras_ranges(keys)
        got = list(zip(first.tolist(), last.tolist(), split.tolist()))
        assert got == _textbook(keys), keys
        count += len(got)
    for name in ("synth_9", "soup_9", "synth_257", "soup_258", "deep_staircase_64", "same_box_pinned_300", "identical_257"):
        b = bc.BY_NAME[name].build()
        assert list(zip(b.first.tolist(), b.last.tolist(), b.split.tolist())) == _textbook(b.keys), name
        count += b.n - 1
    assert count > 5000


def test_four_wide_layout_by_hand():
    """five triangles in a row along x: keys ascending, the root splits 4 | 1 at the top x bit -- left child a leaf of 4,
    right child a leaf of 1: two entries, two empty ones"""
    x = np.array([0.0, 1.0, 2.0, 3.0, 100.0])
    tri = lc.ONE[None] * 0.01 + np.stack([x, np.full(5, 7.0), np.full(5, -3.0)], 1)[:, None, :]
    v, f, _, _ = lc.mesh_of(tri, np.random.default_rng(0))
    b = bc.restate_build(v, f)
    assert b.order.tolist() == [0, 1, 2, 3, 4] and (b.first[0], b.last[0], b.split[0]) == (0, 4, 3)
    row = b.nodes4[0]
    assert row[6] == bc.leaf_ref(0, 4) == 0xCFFFFFFF and row[14] == bc.leaf_ref(4, 1) == 0xFFFFFFFB
    assert row[22] == row[30] == bc.UNUSED and np.all(row[16:22] == bc.INF_BITS) and np.all(row[7::8] == 0)
    vf = v.reshape(5, 3, 3)
    assert np.array_equal(row[0:3].view(np.float32), vf[:4].min((0, 1)) - b.pad)
    assert np.array_equal(row[11:14].view(np.float32), vf[4].max(0) + b.pad)
    assert np.all(b.nodes4[1:] == 0xABABABAB)
    assert b.nodes2[0, 12] == 0xCFFFFFFF and b.nodes2[0, 13] == 0xFFFFFFFB
    # one triangle: entry 0 the leaf (0, 1), three empty entries
    b1 = bc.restate_build(v[:3], f[:1])
    assert b1.nodes4[0, 6] == 0xFFFFFFFF and np.all(b1.nodes4[0, 14::8] == bc.UNUSED)
    assert np.all(b1.nodes4[0, 8:14] == bc.INF_BITS)


# ---- the comparers must see one changed word ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synth_9", "synth_1026", "identical_600", "nan_vertex"])
def test_comparer_reports_single_changes_at_the_right_place(name):
    b = bc.BY_NAME[name].build()
    want = b.nodes4
    assert bc.compare_nodes(want.copy(), want) == []
    live = np.nonzero(b.live)[0]
    node = int(live[len(live) // 2])
    # one box word moved by one ulp
    for word, field in ((1, "mn.y"), (11, "mx.x")):
        got = want.copy()
        got[node, word] += 1
        assert np.isfinite(got[node, word:word + 1].view(np.float32)[0])
        fnd = bc.compare_nodes(got, want)
        assert len(fnd) == 1 and fnd[0][:3] == (node, word // 8, field), fnd
    # one reference changed
    got = want.copy()
    got[node, 14] ^= 1
    fnd = bc.compare_nodes(got, want)
    assert len(fnd) == 1 and fnd[0][:3] == (node, 1, "ref")
    # the trailing word
    got = want.copy()
    got[node, 7] = 1
    assert [x[:3] for x in bc.compare_nodes(got, want)] == [(node, 0, "zero")]
    # one dead node overwritten
    dead = np.nonzero(~b.live)[0]
    got = want.copy()
    got[dead[0], 17] = 0
    assert [x[:3] for x in bc.compare_nodes(got, want)] == [(int(dead[0]), 2, "fill")]
    got = want.copy()
    got[dead[-1]] = want[node]
    assert {x[:3] for x in bc.compare_nodes(got, want)} == {(int(dead[-1]), k, "fill") for k in range(4)}
    # a live node left unwritten
    got = want.copy()
    got[node] = 0xABABABAB
    assert {x[0] for x in bc.compare_nodes(got, want)} == {node}
    # two entries of a node swapped
    two = [int(i) for i in live if want[i, 14] != bc.UNUSED and not np.array_equal(want[i, 0:8], want[i, 8:16])]
    i = two[len(two) // 2]
    got = want.copy()
    got[i, 0:8], got[i, 8:16] = want[i, 8:16], want[i, 0:8]
    fnd = bc.compare_nodes(got, want)
    assert {x[0] for x in fnd} == {i} and {x[1] for x in fnd} == {0, 1} and "ref" in {x[2] for x in fnd}


def test_comparer_nan_rule_and_binary_comparer():
    b = bc.BY_NAME["synth_1026"].build()
    live = np.nonzero(b.live)[0]
    node = int(live[3])
    want = b.nodes4.copy()
    want[node, 2] = 0x7FC00000
    got = want.copy()
    got[node, 2] = 0xFFC00001          # another NaN: equal
    assert bc.compare_nodes(got, want) == []
    got[node, 2] = bc.INF_BITS          # not a NaN
    assert [x[:3] for x in bc.compare_nodes(got, want)] == [(node, 0, "mn.z")]
    got = want.copy()
    got[node, 6] = 0x7FC00001           # a reference compares as bits even where it reads as a NaN
    want[node, 6] = 0x7FC00000
    assert [x[:3] for x in bc.compare_nodes(got, want)] == [(node, 0, "ref")]
    # binary: boxes of a dead node are free, its references are not
    w2 = b.nodes2
    assert bc.compare_nodes2(w2.copy(), w2) == []
    dead = int(np.nonzero(~b.live)[0][0])
    got = w2.copy()
    got[dead, :12] = 12345
    assert bc.compare_nodes2(got, w2) == []
    got[dead, 13] = 5
    assert [x[:3] for x in bc.compare_nodes2(got, w2)] == [(dead, 1, "c1")]
    got = w2.copy()
    got[node, 7] += 1
    assert [x[:3] for x in bc.compare_nodes2(got, w2)] == [(node, 1, "b1.mn.y")]
    got = w2.copy()
    got[node, 12:14] = bc.UNUSED
    assert {x[:3] for x in bc.compare_nodes2(got, w2)} == {(node, 0, "c0"), (node, 1, "c1")}


def test_build_comparer_sees_keys_records_params_and_the_counter():
    b = bc.BY_NAME["synth_513"].build()
    q = bc.queued_expected(b)
    assert bc.compare_build(b, b.keys.copy(), b.tris.copy(), b.params.copy(), q) == []
    k = b.keys.copy(); k[100] ^= 1
    assert [x[:3] for x in bc.compare_build(b, k, b.tris, b.params, q)] == [(100, 0, "key")]
    t = b.tris.copy(); t[7, 4] += 1
    assert [x[:3] for x in bc.compare_build(b, b.keys, t, b.params, q)] == [(7, 4, "tris")]
    t = b.tris.copy(); t[7, 9] = 0xFFFFFFFF
    assert [x[:3] for x in bc.compare_build(b, b.keys, t, b.params, q)] == [(7, 9, "tris")]
    p = b.params.copy(); p.view(np.uint32)[4] += 1
    assert [x[:3] for x in bc.compare_build(b, b.keys, b.tris, p, q)] == [(0, 4, "params")]
    assert [x[2:] for x in bc.compare_build(b, b.keys, b.tris, b.params, q + 1)] == [("queued", q + 1, q)]


def test_sort_reference_reports_a_swap_under_equal_keys_as_a_stability_failure():
    for pattern in ("ties17", "equal", "two", "digit1"):
        keys, vals, bits = bc.sort_input(pattern, 4097)
        assert len(np.unique(vals)) == len(vals) and int((vals >> 31).sum()) > 1000
        assert not np.array_equal(vals, np.arange(len(vals)))
        ko, vo = bc.sort_reference(keys, vals, bits)
        assert bc.compare_sort(keys, vals, bits, ko, vo) == []
        masked = ko & np.uint32((1 << bits) - 1)
        p = int(np.nonzero(masked[1:] == masked[:-1])[0][5])
        bad = vo.copy()
        bad[p], bad[p + 1] = vo[p + 1], vo[p]
        fnd = bc.compare_sort(keys, vals, bits, ko, bad)
        assert [x[:3] for x in fnd] == [(p, 1, "stability"), (p + 1, 1, "stability")]
    keys, vals, bits = bc.sort_input("random30", 1025)
    ko, vo = bc.sort_reference(keys, vals, bits)
    bad = vo.copy()
    bad[3], bad[900] = vo[900], vo[3]
    assert {x[2] for x in bc.compare_sort(keys, vals, bits, ko, bad)} == {"value"}
    bad = ko.copy()
    bad[10] ^= 0x80000000     # above the sorted bits: still carried
    assert [x[:3] for x in bc.compare_sort(keys, vals, bits, bad, vo)] == [(10, 0, "key")]
    # the two top bits of random32 keys must not order anything
    keys, vals, bits = bc.sort_input("random32", 4097)
    ko, _ = bc.sort_reference(keys, vals, bits)
    assert int((ko >> 30).max()) == 3 and not np.all(ko[1:] >= ko[:-1])
    assert np.all((ko & 0x3FFFFFFF)[1:] >= (ko & 0x3FFFFFFF)[:-1])


def test_sort_inputs_are_what_their_names_say():
    for n in bc.SORT_PATTERN_SIZES[:3]:
        for d in range(3):
            keys, _, _ = bc.sort_input(f"digit{d}", n)
            varying = np.bitwise_or.reduce(keys ^ keys[0])
            assert varying != 0 and varying & ~np.uint32(0x3FF << (10 * d)) == 0
        assert len(np.unique(bc.sort_input("equal", n)[0])) == 1
        assert len(np.unique(bc.sort_input("two", n)[0])) == 2
        assert len(np.unique(bc.sort_input("ties17", n)[0])) == 17
        a = bc.sort_input("ascending", n)[0]
        assert np.all(a[1:] >= a[:-1]) and np.all(bc.sort_input("descending", n)[0][1:] <= bc.sort_input("descending", n)[0][:-1])
    # k_scan: one round up to 256 tiles, the carry from the 257th
    assert [bc.sort_tiles_rounds(n) for n in bc.SORT_BIG_SIZES] == [(256, 1), (256, 1), (257, 2), (514, 3)]
    assert max(bc.sort_tiles_rounds(n)[1] for n in bc.SORT_SIZES) == 1
    assert bc.SCAN_TILES == 1048576


# ---- which seam a case crosses ------------------------------------------------------------------------------------------
def _fig(name):
    return bc.figures(bc.BY_NAME[name].build())


def test_case_list_is_the_one_the_issue_names():
    assert len(NAMES) == len(set(NAMES)) == 2 * len(bc.SIZES) + 13
    assert max(c.n for c in bc.CASES) <= 9000
    for n in bc.SIZES:
        assert bc.BY_NAME[f"synth_{n}"].n == bc.BY_NAME[f"soup_{n}"].n == n
    v, f, _, _ = bc.BY_NAME["synth_8193"].mesh()
    assert len(v) < 3 * len(f) and len(np.unique(f)) < f.size, "the synth mesh shares vertices"
    v, f, _, _ = bc.BY_NAME["far_vertices"].mesh()
    unref = np.setdiff1d(np.arange(len(v)), f)
    assert {len(v) - 1, len(v) - 2} <= set(unref.tolist())
    lo, hi = v[np.unique(f)].min(0), v[np.unique(f)].max(0)
    assert v[:, 0].max() > hi[0] + 500 and v[:, 2].min() < lo[2] - 500, "the unreferenced vertices widen the bounds"
    v, f, _, _ = bc.BY_NAME["bad_index"].mesh()
    assert -1 in f and len(v) in f and f.max() > len(v)
    assert np.isnan(bc.BY_NAME["nan_vertex"].mesh()[0]).sum() >= 2
    assert np.isinf(bc.BY_NAME["inf_vertex"].mesh()[0]).sum() >= 2
    assert set(bc.BINARY_CASES) <= set(NAMES)


@pytest.mark.parametrize("kind", ["synth", "soup"])
def test_path_conditions_of_the_sized_cases(kind):
    fig = {n: _fig(f"{kind}_{n}") for n in bc.SIZES}
    for n, g in fig.items():
        assert g["n"] == n and g["max_range"] == n
    # n == 1 and the first sizes around LT_LEAF_MAX: the root alone up to 2 LT_LEAF_MAX would need both halves small
    assert bc.LT_LEAF_MAX == 4
    assert all(fig[n]["live"] == 1 for n in (1, 2, 3, 4)) and fig[9]["live"] >= 2
    # LT_HBIG: k_hierarchy4_big gets a node from 257 slots on, and nothing below
    assert bc.LT_HBIG == 256
    assert all(fig[n]["queued"] == 0 for n in bc.SIZES if n <= 256)
    assert all(fig[n]["queued"] >= 1 for n in bc.SIZES if n >= 257)
    assert fig[257]["queued"] == fig[258]["queued"] == 1
    # LT_SEG_SUB: k_seg_sub alone up to 512 leaves, k_seg_top from 513 on
    assert bc.LT_SEG_SUB == 512
    assert fig[511]["seg_blocks"] == fig[512]["seg_blocks"] == 1 and fig[513]["seg_blocks"] == 2
    assert fig[8193]["seg_blocks"] == 32
    # LT_HNODES: a second workgroup of k_hierarchy4 from 1026 faces (1025 nodes) on
    assert bc.LT_HNODES == 1024 and bc.LT_HWIN == 512
    assert fig[1024]["workgroups"] == fig[1025]["workgroups"] == 1 and fig[1026]["workgroups"] == 2
    assert all(fig[n]["second_wg"] > 0 for n in (2049, 4095, 4096, 4097, 8193)) and fig[8193]["workgroups"] == 8
    # the sort: tile and quarter-tile seams
    assert bc.LT_SORT_TILE == 4096
    assert [fig[n]["tiles"] for n in (4095, 4096, 4097, 8193)] == [1, 1, 2, 3]
    assert [fig[n]["quarter"] for n in (1024, 1025, 2049, 4095, 4096, 4097)] == [1, 2, 3, 4, 4, 1]
    if kind == "synth":
        # ranges of small nodes that leave their workgroup's own LT_HNODES slots: served by the LDS key window alone
        assert fig[1026]["second_wg"] >= 1
        assert all(fig[n]["crossing"] > 0 for n in (1026, 2049, 4095, 4096, 4097, 8193))


def test_path_conditions_of_the_shaped_cases():
    # identical(n): one key; every node of at least 257 slots is queued, and they are the whole top of the tree
    for n, queued in ((5, 0), (257, 1), (600, 2), (1300, 5), (3000, 11)):
        b = bc.BY_NAME[f"identical_{n}"].build()
        assert len(np.unique(b.keys)) == 1 and np.array_equal(b.order, np.arange(n))
        g = bc.figures(b)
        assert g["queued"] == queued and g["max_range"] == n
    assert _fig("identical_600")["max_range"] > bc.LT_HNODES // 2 + 0 and _fig("identical_1300")["workgroups"] == 2
    assert _fig("identical_1300")["second_wg"] > 0 and _fig("identical_3000")["workgroups"] == 3
    # ranges longer than the LDS window on each side of the workgroup
    assert _fig("identical_3000")["max_range"] > bc.LT_HNODES + 2 * bc.LT_HWIN
    g = _fig("stairs_14x40")
    assert g["n"] == 560 and g["queued"] >= 2 and g["workgroups"] == 1
    g = _fig("stairs_14x600")
    assert g["n"] == 8400 and g["queued"] >= 14 and g["workgroups"] == 9 and g["tiles"] == 3
    b = bc.BY_NAME["stairs_14x600"].build()
    assert 10 <= len(np.unique(b.keys)) <= 28, "a few keys, hundreds of triangles each"
    g = _fig("same_box_pinned_300")
    b = bc.BY_NAME["same_box_pinned_300"].build()
    assert g["n"] == 302 and g["queued"] >= 1 and np.unique(b.keys, return_counts=True)[1].max() == 300
    g = _fig("deep_staircase_64")
    b = bc.BY_NAME["deep_staircase_64"].build()
    assert g["n"] == 96 and g["queued"] == 0
    # the chain: node m splits one leaf off everything behind it, 30 times
    chain = [int(b.last[i] - b.first[i] + 1) for i in range(2, 32)]
    assert chain == list(range(94, 64, -1)), chain
    for name in ("far_vertices", "bad_index", "nan_vertex", "inf_vertex"):
        g = _fig(name)
        assert g["queued"] >= 1 and g["seg_blocks"] == 2 and g["live"] > 100, name
    # an infinite vertex: scale 0, every key 0; pad infinite
    b = bc.BY_NAME["inf_vertex"].build()
    assert b.params[3] == 0 and np.isinf(b.pad) and np.all(b.keys == 0)
    b = bc.BY_NAME["nan_vertex"].build()
    assert np.all(np.isfinite(b.params)) and len(np.unique(b.keys)) > 100
    assert np.isnan(b.tris[:, :9].view(np.float32)).any()
