"""What keeps tests/post_cases.py honest without a GPU: the three restatements against golden F7 (vectors written by the
reference's own Python) and the pinned oracle/compare.py, and every generator against what tests/test_post_shapes_gpu.py
assumes of it -- the cells a keep pattern claims to hit, the points that separate the float32 from the float64 keep rule,
the constructed waves, and how few reverse-projection elements sit near a float32 tie."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_cases as pc  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "f7_post.npz"))


# ---- the restatements against the reference's vectors -----------------------------------------------------------------------
def test_restate_pack_reproduces_the_reference_files_byte_for_byte(g):
    b, l = pc.restate_pack(g["back_points_float"], g["label_image"], g["proj_remissions"], g["index"])
    assert b.dtype == np.float32 and l.dtype == np.uint32 and len(l) == 1731
    assert np.array_equal(b.view(np.uint8).reshape(-1), g["cp_bin_bytes"])
    assert np.array_equal(l.view(np.uint8).reshape(-1), g["cp_label_bytes"])
    g4 = np.load(os.path.join(GOLD, "f4_50k_64x256.npz"))
    b, l = pc.restate_pack(g4["endpoints"], g4["label"], g4["endrem"])
    assert len(l) == 16225 == int(g4["n_hits"])
    assert np.array_equal(b.view(np.uint8).reshape(-1), g["mesh_bin_bytes"])
    assert np.array_equal(l.view(np.uint8).reshape(-1), g["mesh_label_bytes"])


@pytest.mark.parametrize("pf", [False, True])
def test_restate_reverse_equals_the_reference_back_points(g, pf):
    """the same numpy on the same host: exact.  (Should a numpy build ever differ in the last bit of sin / cos, the bound to
    fall back to is the rtol = atol = 1e-13 of tests/test_post_gpu.py; this one does not, so equality is asserted.)"""
    px, py = (g["proj_x_float"], g["proj_y_float"]) if pf else (g["proj_x"], g["proj_y"])
    got = pc.restate_reverse(g["range_image"], px, py, float(g["fov_up"]), float(g["fov_down"]))
    ref = g[f"back_points_{'float' if pf else 'int'}"]
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.array_equal(got.view(np.int64), ref.view(np.int64))


def _ranks(oracle_out, masked_s, masked_t):
    """oracle.compare renumbers the masked labels by rank among the values present (non-negative labels: no merging)"""
    present = np.union1d(masked_s, masked_t)
    return np.searchsorted(present, masked_s), np.searchsorted(present, masked_t)


def test_restate_compare_agrees_with_the_pinned_compare(g):
    from oracle.compare import compare as ocompare
    a = [g[k] for k in ("cmp_source_label", "cmp_source_color", "cmp_target_label", "cmp_source_range", "cmp_target_range",
                        "cmp_source_rem", "cmp_target_rem")]
    want = ocompare(*a, nclasses=20)
    got = pc.restate_compare_arrays(*a, n_labels=512)
    shape = a[0].shape
    assert min(got["source_label"].min(), got["target_label"].min()) >= 0
    rs, rt = _ranks(want, got["source_label"], got["target_label"])
    assert np.array_equal(rs.reshape(shape), want["source_label"]) and np.array_equal(rt.reshape(shape), want["target_label"])
    for k in ("range_diff", "rem_diff"):
        assert got[k].dtype == np.float32
        assert np.array_equal(got[k].view(np.int32).reshape(shape), want[k].view(np.int32))
        assert np.array_equal(got[k].view(np.int32).reshape(shape), g[f"cmp_{k}"].view(np.int32))
    assert got["conf"].sum() == a[0].size and got["conf"].dtype == np.int64
    # the histogram over raw labels, folded to ranks, is the matrix iouEval fills
    present = np.union1d(got["source_label"], got["target_label"])
    cm = np.zeros((20, 20), np.int64)
    np.add.at(cm, (rt, rs), 1)
    assert np.array_equal(got["conf"][np.ix_(present, present)], cm[:len(present), :len(present)])
    assert abs(got["sq_exact"] / a[0].size - float(g["cmp_mse"])) < 1e-6 * float(g["cmp_mse"])
    # a random case as well, with labels outside the table (those the oracle would count; the restatement must not)
    c = pc.compare_random(4096, 20, seed=1)
    r = pc.restate_compare_arrays(*[c[k] for k in ("src_label", "src_color", "tgt_label", "src_range", "tgt_range", "src_rem",
                                                     "tgt_rem")], n_labels=20)
    inside = (r["source_label"] >= 0) & (r["source_label"] < 20) & (r["target_label"] >= 0) & (r["target_label"] < 20)
    assert 0 < (~inside).sum() < 400 and r["conf"].sum() == inside.sum()
    o = ocompare(c["src_label"].reshape(64, 64), c["src_color"].reshape(64, 64, 3), c["tgt_label"].reshape(64, 64),
                 c["src_range"].reshape(64, 64), c["tgt_range"].reshape(64, 64), c["src_rem"].reshape(64, 64),
                 c["tgt_rem"].reshape(64, 64), nclasses=64)
    assert np.array_equal(r["range_diff"].view(np.int32), o["range_diff"].reshape(-1).view(np.int32))
    assert np.array_equal(r["rem_diff"].view(np.int32), o["rem_diff"].reshape(-1).view(np.int32))


def test_block_tree_sum_is_the_first_level_of_the_evaluators_fixed_order():
    import test_evaluate_cpu as ev
    d2 = (np.random.default_rng(5).uniform(0, 80, 255).astype(np.float32)) ** 2
    assert pc.block_tree_sum(d2) == ev.fixed_order_sum(d2)            # one workgroup: the same tree
    assert abs(pc.block_tree_sum(d2) - float(np.sum(d2.astype(np.float64)))) <= 255 * 2.0 ** -52 * float(d2.sum())


# ---- the pack generators -----------------------------------------------------------------------------------------------------
def test_pack_sizes_cover_the_chunk_loop_and_the_ragged_blocks():
    nb = [(n + 255) // 256 for n in pc.PACK_SIZES]
    assert nb[:9] == [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049] and max(pc.PACK_SIZES) == 524289
    assert sum(b > 1024 for b in nb) == 2 and sum(b > 2048 for b in nb) == 1          # a second and a third turn
    assert {n % 256 for n in pc.PACK_SIZES} == {1, 63, 64, 65, 255, 0}


@pytest.mark.parametrize("nb", [65, 2049])
def test_keep_patterns_hit_what_they_claim(nb):
    n = 256 * (nb - 1) + 1
    k = {name: pc.keep_pattern(name, n) for name in pc.KEEP_PATTERNS}
    assert k["all"].all() and not k["none"].any()
    assert list(np.flatnonzero(k["first"])) == [0] and list(np.flatnonzero(k["last"])) == [n - 1]
    one = k["one_per_block"]
    padded = np.concatenate([one, np.zeros(nb * 256 - n, bool)]).reshape(nb, 256)
    assert (padded.sum(1) == 1).all()                                                  # exactly one cell in EVERY block
    lanes = padded.argmax(1)
    assert len(set(lanes[:-1].tolist())) == min(nb - 1, 256) and lanes[-1] == 0        # at a lane that varies
    assert len(set((lanes[:-1] // 64).tolist())) == 4                                  # and in every wave
    w = np.arange(n) // 64
    assert (k["odd_waves"] == (w % 2 == 1)).all() and k["odd_waves"][64:128].all() and not k["odd_waves"][:64].any()
    for name, step in (("seam64", 64), ("seam256", 256), ("seam_chunk", 262144)):
        edges = np.arange(step, n, step)
        if name != "seam_chunk":
            assert len(edges) > 0
        assert k[name][edges - 1].all() and k[name][edges].all(), name                # last before, first after
        assert k[name].sum() <= 2 * len(edges) + 2, name                               # and nothing else (cell 0 / n - 1)
    assert k["seam64"][edges - 1].all() and k["seam256"][np.arange(256, n, 256)].all()
    if nb == 2049:
        assert list(np.flatnonzero(k["seam_chunk"])) == [262143, 262144, 524287, 524288]
    else:
        assert not k["seam_chunk"].any()
    assert 0.49 < k["random50"].mean() < 0.51


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("with_index", [False, True])
def test_pack_case_keeps_exactly_its_pattern_and_names_every_row(dtype, with_index):
    n = 256 * 64 + 1
    for name in pc.KEEP_PATTERNS:
        keep = pc.keep_pattern(name, n)
        c = pc.pack_case(n, dtype, keep, with_index)
        assert c["points"].dtype == dtype and c["label"].dtype == np.int32 and c["rem"].dtype == np.float32
        b, l = pc.restate_pack(c["points"], c["label"], c["rem"], c["index"])
        rows = np.flatnonzero(keep)
        assert np.array_equal(b[:, 3], rows.astype(np.float32)), name                  # the rows kept, in order, by name
        assert np.array_equal(l, (rows | (7 << 16)).astype(np.uint32)), name
        assert np.array_equal(b[:, :3], c["points"][keep].astype(np.float32))
        # no input carries a sentinel's bit pattern
        assert not (b.view(np.uint32) == pc.SENT_F32).any() and not (l == pc.SENT_U32).any()
    c = pc.pack_case(n, dtype, pc.keep_pattern("none", n), with_index)
    used = [(c["points"] == 0).all(1).any(), (c["label"] < 0).any(), ((c["points"] != 0).any(1) & (c["points"].sum(1) == 0)).any()]
    if with_index:
        used += [(c["index"] == 0).any(), (c["index"] < 0).any()]
    assert all(used)                                                                   # every drop rule is in use


def test_the_points_that_separate_the_float32_from_the_float64_rule():
    f32, f64 = np.float32, np.float64

    def kept(point, dtype):
        p = np.array([point], f64).astype(dtype)
        return len(pc.restate_pack(p, np.array([1], np.int32), np.array([0], f32))[1]) == 1

    assert kept([1e8, -1e8, 1], f32) and kept([1e8, -1e8, 1], f64)
    assert f32(1e8) + (f32(-1e8) + f32(1)) == 0                 # ... and x + (y + z) in float32 would have dropped it
    assert not kept([1e8, 1, -1e8], f32) and kept([1e8, 1, -1e8], f64)
    assert kept([1e-45, 0, 0], f32) and kept([1e-45, 0, 0], f64) and f32(1e-45) != 0
    assert not kept([-0.0, 0, 0], f32) and not kept([-0.0, 0, 0], f64)
    assert kept([np.nan, 0, 0], f32) and kept([np.nan, 0, 0], f64)
    # the restatement's left-to-right sum is numpy's own for three contiguous elements (laserscan.py:1151 uses np.sum)
    for dtype in (f32, f64):
        p = np.array([[1e8, -1e8, 1], [1e8, 1, -1e8], [1e-45, 0, 0], [-0.0, 0, 0]], f64).astype(dtype)
        assert np.array_equal(np.sum(p, axis=1) != 0, ((p[:, 0] + p[:, 1]) + p[:, 2]) != 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("with_index", [False, True])
def test_pack_value_edges_keep_what_the_table_says(dtype, with_index):
    c = pc.pack_value_edges(dtype, with_index)
    b, l = pc.restate_pack(c["points"], c["label"], c["rem"], c["index"])
    assert np.array_equal(b[:, 3], c["rem"][c["keep"]])
    assert np.abs(c["points"][np.isfinite(c["points"])]).max() < np.finfo(np.float32).max
    bits = b.view(np.uint32)
    row = {int(r): k for k, r in enumerate(b[:, 3] - 0.25)}
    assert bits[row[2], 0] == 1 and bits[row[4], 0] == 0x7FC00000        # the smallest denormal; the quiet NaN
    assert b[row[5], 0] == 1.0 and b[row[6], 0] == np.float32(1.0 + 2.0 ** -22)       # ties to even, down and up
    if dtype == np.float64:
        assert 0 < b[row[7], 0] < np.finfo(np.float32).tiny and c["points"][7, 0] != b[row[7], 0]
    assert (l == 0x7FFFFFFF).sum() == 1 and (l == (0x7FFF << 16) | 40).sum() == 1 and not (l >> 31).any()
    assert (c["label"] < 0).sum() == 1                                   # bit 31: dropped
    if with_index:
        assert c["index"].max() == pc.INT_MAX and {0, -1} <= set(c["index"].tolist())
        assert not np.isin(c["rem"][[12, 13]], b[:, 3]).any()
    else:
        assert np.isin(c["rem"][[12, 13]], b[:, 3]).all()


# ---- the reverse-projection cases: how few elements sit near a float32 tie ----------------------------------------------------
@pytest.mark.parametrize("float_coords", [False, True])
@pytest.mark.parametrize("shape", pc.REVERSE_SHAPES)
def test_reverse_cases_leave_out_at_most_one_element_in_ten_thousand(shape, float_coords, capsys):
    """a condition on the inputs, asserted from the restatement alone: the elements the GPU test leaves out of its float32
    comparison (post_cases.near_f32_tie) are at most 1e-4 of any case.  The count under the wider window with an absolute
    1e-13 is printed next to it (see near_f32_tie for why that one cannot be the condition on a full integer grid)."""
    H, W = shape
    for fov in pc.REVERSE_FOVS:
        r, px, py, what = pc.reverse_case(H, W, fov, float_coords)
        assert r.dtype == np.float32 and px.dtype == (np.float64 if float_coords else np.int32)
        if H * W >= 8:
            assert 0.15 < (r == -1).mean() < 0.25 or H * W < 1000
            assert (r == 0).any() and (r == np.float32(1e-40)).any() and (r == np.float32(3e38)).any()
        if float_coords:
            assert px.min() == 0.0 and py.max() == H - 2.0 ** -40 < H
            assert H * W == 1 or (px.max() == W - 2.0 ** -40 < W and py.min() == 0.0)
        else:
            assert np.array_equal(px, np.tile(np.arange(W), (H, 1))) and np.array_equal(py, np.repeat(np.arange(H), W).reshape(H, W))
        v = pc.restate_reverse(r, px, py, *fov)
        assert v.shape == (H * W, 3) and np.isfinite(v).all() and np.abs(v).max() < np.finfo(np.float32).max
        near = pc.near_f32_tie(v)
        tiny = np.abs(v) < 1e-13
        f = v.astype(np.float32).astype(np.float64)
        wide = near | (tiny & (f != v))
        with capsys.disabled():
            print(f"\n{what}: {int(near.sum())} of {v.size} elements near a float32 tie "
                  f"({int(wide.sum())} with the absolute 1e-13; {int(tiny.sum())} elements below 1e-13)", end="")
        assert near.sum() <= 1e-4 * v.size, what


def test_near_f32_tie_marks_ties_and_nothing_else():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2))
    mid = (float(one) + float(up)) / 2
    v = np.array([mid, mid * (1 + 5e-14), mid * (1 - 5e-14), mid * (1 + 1e-12), 1.0, float(up), 0.0, -mid, 1e-300, 3e38])
    assert list(pc.near_f32_tie(v)) == [True, True, True, False, False, False, False, True, False, False]
    d = float(np.float32(1e-45))                                 # between 0 and the smallest denormal
    assert list(pc.near_f32_tie(np.array([d / 2, d / 2 * (1 + 1e-12), 1.5 * d]))) == [True, False, True]


# ---- the compare generators ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_labels", [20, 64, 300])
def test_constructed_waves_are_what_they_say(n_labels):
    c = pc.compare_waves(n_labels)
    assert c["kinds"] == pc.WAVE_KINDS
    r = pc.restate_compare_arrays(*[c[k] for k in ("src_label", "src_color", "tgt_label", "src_range", "tgt_range", "src_rem",
                                                     "tgt_rem")], n_labels=n_labels)
    sl, tl = r["source_label"].astype(np.int64), r["target_label"].astype(np.int64)
    counted = (sl >= 0) & (sl < n_labels) & (tl >= 0) & (tl < n_labels)
    pair = np.where(counted, tl * n_labels + sl, -1).reshape(len(c["kinds"]), 4, 64)
    blk = {k: pair[i] for i, k in enumerate(c["kinds"])}
    assert all(len(set(wv.tolist())) == 64 for wv in blk["distinct64"]) and (blk["distinct64"] >= 0).all()
    assert len(set(blk["one_pair"].reshape(-1).tolist())) == 1 and blk["one_pair"][0, 0] == 3 * n_labels + n_labels - 1
    for kind, same, other in (("target_only", sl, tl), ("source_only", tl, sl)):
        i = c["kinds"].index(kind)
        assert len(set(same[256 * i:256 * i + 256].tolist())) == 1 and len(set(other[256 * i:256 * i + 64].tolist())) == 5
    z = blk["zeros_and_uncounted"]
    assert (z[:, 0::2] == 0).all() and (z[:, 1::2] == -1).all()              # (0, 0) next to uncounted lanes, in every wave
    i = c["kinds"].index("zeros_and_uncounted")
    raw_s, raw_t = c["src_label"][256 * i:256 * i + 256], c["tgt_label"][256 * i:256 * i + 256]
    for bad in pc.OUTSIDE(n_labels):
        assert (raw_s == bad).any() and (raw_t == bad).any()
    w = blk["wave_per_pair"]
    assert all(len(set(wv.tolist())) == 1 for wv in w) and len({int(wv[0]) for wv in w}) == 4
    i = c["kinds"].index("black")
    col = c["src_color"][256 * i:256 * i + 256]
    assert (c["src_label"][256 * i:256 * i + 256] != 0).all()
    is_black = sl[256 * i:256 * i + 256] == 0
    assert is_black[[0, 1, 2]].all() and not is_black[3] and is_black.sum() == 192
    assert np.signbit(col[1, 0]) and col[2, 0] == 0.5 and col[2, 1] == -0.5 and col[3, 0] == np.float32(1e-30) != 0
    # no counter may overflow unnoticed, and garbage left in conf would show
    assert r["conf"].sum() == counted.sum() and r["conf"].max() < 2 ** 31


def test_compare_random_has_labels_on_both_sides_of_the_table():
    for n_labels in pc.COMPARE_NLABELS:
        c = pc.compare_random(4096, n_labels)
        for bad in pc.OUTSIDE(n_labels):
            assert (c["src_label"] == bad).any() and (c["tgt_label"] == bad).any()
        assert 0.05 < (c["src_color"].sum(1) == 0).mean() < 0.15
        if n_labels > 1:
            assert (c["src_label"] == n_labels - 1).any() and (c["src_label"] != c["tgt_label"]).mean() > 0.1
    assert sorted(set(pc.COMPARE_NLABELS) - {1, 64, 512}) == [20, 300]      # two that are no power of two
