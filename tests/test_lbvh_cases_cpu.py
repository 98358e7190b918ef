"""tests/lbvh_cases.py without a GPU: the generators do to the tree what they claim (held against the oracle's LBVH model,
oracle/lt_lbvh_model.h, binary nodes), and replay_identical gives the answers worked out by hand below."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbvh_cases as lc  # noqa: E402

KEYS = ("tri", "range", "endpoints", "endcolors", "endrem")
H, W = 8, 33


@pytest.mark.parametrize("name", lc.SCENES)
def test_lbvh_model_equals_brute_force_on_every_scene(oracle, name):
    (v, f, c, r), origin = lc.scene(name)
    rays = lc.scene_rays(name, H * W)
    o = np.asarray(origin, np.float32)
    a = oracle.oracle_trace(rays, o, v, f, c, r, H, mode=oracle.MODE_LBVH, norm=oracle.NORM_SSE_TABLE)
    b = oracle.oracle_trace(rays, o, v, f, c, r, H, mode=oracle.MODE_BRUTE, norm=oracle.NORM_SSE_TABLE)
    for k in KEYS:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    hits = int((b["tri"] >= 0).sum())
    print(f"{name}: {f.shape[0]} faces, {hits} of {H * W} rays hit, model max_stack {a['stats']['max_stack']}")
    assert hits >= 20
    assert a["stats"]["max_stack"] < lc.LT_STACK_MAX   # the binary kernel's stack (and the model's own) holds the walk
    if name == "identical":   # the lowest face index among 20 000 ties
        assert np.all(b["tri"][b["tri"] >= 0] == 0)
    # no ties: the nearest triangle of a ray is any of them (the staircase's 66 rays through c* share theirs)
    if name == "same_box":
        assert np.unique(b["tri"]).size > 50
    if name == "deep_staircase_tilted":
        assert np.unique(b["tri"]).size > 20


def test_same_box_has_the_box_of_identical():
    n = 1000
    v, f, c, r = lc.mesh_of(lc.same_box(n, np.random.default_rng(6)), np.random.default_rng(6))
    t, one = v[f], lc.ONE.astype(np.float32)
    assert np.all(t.min(1) == one.min(0)) and np.all(t.max(1)[:, 1:] == one.max(0)[1:])
    assert np.all(t.max(1)[:, 0] == np.float32(4.0 + lc.SAME_BOX_DX))


def test_same_box_pinned_has_one_key_and_many_nearest_faces(oracle):
    rng = np.random.default_rng(5)
    n = 20000
    v, f, c, r = lc.mesh_of(lc.same_box_pinned(n, rng), rng)
    keys = lc.morton_keys(v, f)
    assert keys[0] == 0 and keys[-1] == (1 << 30) - 1 and np.all(keys[1:-1] == keys[1]) and 0 < keys[1] < keys[-1]
    t = v[f[1:-1]]
    assert np.all(t.min(1) == t.min(1)[0]) and np.all(t.max(1) == t.max(1)[0])
    rays = lc.rays_along_x(np.random.default_rng(9), 8 * 16)
    a = oracle.oracle_trace(rays, np.zeros(3, np.float32), v, f, c, r, 8, mode=oracle.MODE_LBVH, norm=oracle.NORM_SSE_TABLE)
    b = oracle.oracle_trace(rays, np.zeros(3, np.float32), v, f, c, r, 8, mode=oracle.MODE_BRUTE, norm=oracle.NORM_SSE_TABLE)
    for k in KEYS:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    assert np.unique(b["tri"]).size > 50 and b["tri"].max() > n // 2 and b["tri"][0] >= 1


@pytest.mark.parametrize("tilted", [False, True])
@pytest.mark.parametrize("n_cluster", [1024, 4096, lc.N_STAIR_CLUSTER])
def test_deep_staircase_passes_the_binary_lds_stack(oracle, n_cluster, tilted):
    """max_stack of the binary model: 38, 40, 42 for 1024, 4096, 16384 -- 30 chain levels plus one per two-fold of the
    cluster's leaves -- above LT_STACK_LDS = 32; the rays through c* all return the first cluster face."""
    v, f, c, r = lc.deep_staircase(n_cluster, tilted)
    rays = lc.staircase_rays(8 * 32)
    o = np.asarray(lc.STAIR_ORIGIN, np.float32)
    a = oracle.oracle_trace(rays, o, v, f, c, r, 8, mode=oracle.MODE_LBVH, norm=oracle.NORM_SSE_TABLE)
    b = oracle.oracle_trace(rays, o, v, f, c, r, 8, mode=oracle.MODE_BRUTE, norm=oracle.NORM_SSE_TABLE)
    for k in KEYS:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    print(f"n_cluster {n_cluster}: max_stack {a['stats']['max_stack']}, {int((b['tri'] >= 0).sum())} hits")
    assert a["stats"]["max_stack"] == 30 + int(np.log2(n_cluster // 4)) > lc.LT_STACK_LDS
    assert int((b["tri"] >= 0).sum()) >= 100
    assert np.all(b["tri"][::4] == b["tri"][0]) and b["tri"][0] >= lc.STAIR_FIRST_SPLIT + lc.N_CHAIN
    if not tilted:
        assert b["tri"][0] == lc.STAIR_FIRST_SPLIT + lc.N_CHAIN


def test_deep_staircase_keys_form_a_chain():
    """split-off m shares exactly m leading key bits with the cluster; nothing leaves the cube, whose corners are met"""
    v, f, c, r = lc.deep_staircase(64, tilted=True)
    assert v.min() == 0.0 and v.max() == lc.CUBE and np.all(v.min(0) == 0.0) and np.all(v.max(0) == lc.CUBE)
    keys = lc.morton_keys(v, f)
    first = lc.STAIR_FIRST_SPLIT
    cluster = keys[first + lc.N_CHAIN:]
    assert np.all(cluster == (1 << 30) - 1)
    for m in range(lc.N_CHAIN):
        shared = 30 - int(keys[first + m] ^ cluster[0]).bit_length()
        assert shared == m, (m, shared)
    assert list(np.argsort(keys[first:first + lc.N_CHAIN], kind="stable")) == list(range(lc.N_CHAIN))
    # every split-off's box holds c* with a margin, so a ray through c* meets every box of the chain
    t = v[f[first:first + lc.N_CHAIN]]
    assert np.all(t.min(1) < lc.C_STAR - 0.05 * lc.CELL) and np.all(t.max(1) > lc.C_STAR + 0.05 * lc.CELL)


def _leaf(k):
    return ~(4 * k)   # a leaf reference: ~(start | (count - 1) << 28), one triangle at slot 4k


def _nodes(children):
    a = np.full((len(children), 32), 0xABABABAB, np.uint32)   # boxes: never read by the replay
    for i, ch in enumerate(children):
        refs = list(ch) + [lc.UNUSED] * (4 - len(ch))
        a[i, 6::8] = np.array(refs, np.int64).astype(np.uint32)
    return a


def test_replay_on_a_hand_built_tree():
    """root 0 = [node 1, leaf A, node 2, leaf B], node 1 = [L1, L2, L3], node 2 = [M1, M2].

    No cap: root, node 1, L1, L2, L3, A, node 2, M1, M2, B = 10 steps; the quad's stack is [B, 2, A] after the root and
    [B, 2, A, L3, L2] after node 1: 5 entries.
    cap 1: parked after the root with [B, 2, A | 1] = 4 entries.  Round 1 takes all four (quad 0: node 1, quad 1: A, quad 2:
    node 2, quad 3: B); node 2's children land at 0 + (1 - rank), node 1's above them at 2 + (2 - rank): [M2, M1, L3, L2, L1],
    5 entries.  Round 2 takes the five leaves.
    cap 3: root, node 1, L1, then parked with [B, 2, A, L3 | L2] = 5 entries.  Round 1: four leaves and node 2 -> [M2, M1];
    round 2 takes both."""
    A, B, L1, L2, L3, M1, M2 = (_leaf(k) for k in range(7))
    nodes = _nodes([[1, A, 2, B], [L1, L2, L3], [M1, M2]])
    assert lc.node_children(nodes, 0) == [1, A, 2, B] and lc.node_children(nodes, 2) == [M1, M2]
    assert lc.tree_depth(nodes) == 2
    assert lc.replay_identical(nodes, 0) == lc.Replay(high_water=0, rounds=0, saved_sp=0, quad_sp=5, steps=10)
    assert lc.replay_identical(nodes, 40) == lc.Replay(0, 0, 0, 5, 10)
    assert lc.replay_identical(nodes, 1) == lc.Replay(high_water=5, rounds=2, saved_sp=4, quad_sp=3, steps=1)
    assert lc.replay_identical(nodes, 3) == lc.Replay(high_water=5, rounds=2, saved_sp=5, quad_sp=5, steps=3)
    assert lc.replay_identical(nodes, 10) == lc.Replay(0, 0, 0, 5, 10)
    assert lc.replay_identical(nodes, 9) == lc.Replay(high_water=1, rounds=1, saved_sp=1, quad_sp=5, steps=9)


def test_replay_enters_the_one_at_a_time_mode_on_a_complete_tree():
    """A complete 4-ary tree, node levels 0 .. 8, leaves below, cap 1: parked with the root's 4 children.  The rounds
    take everything (4 -> 16 -> 64 entries), then 16 of the top level each and push their 64 children: 112, 160, 208,
    256 (the level 7 nodes on top), 304 (level 8 on top).  304 > LT_TAIL_DFS: one node of level 8 is taken, its 4 leaves
    land: 307, the high-water mark -- leaves only come off from there until the stack is back at 256.  Without the
    one-at-a-time mode the next round would take 16 nodes and reach 352."""
    levels = 9
    n_int = (4 ** levels - 1) // 3
    first_last = (4 ** (levels - 1) - 1) // 3
    kids = 4 * np.arange(n_int, dtype=np.int64)[:, None] + np.arange(1, 5)
    kids[first_last:] = ~(4 * (kids[first_last:] - n_int))
    nodes = np.zeros((n_int, 32), np.uint32)
    nodes[:, 6::8] = kids.astype(np.uint32)
    assert lc.tree_depth(nodes) == levels
    r = lc.replay_identical(nodes, 1)
    assert (r.high_water, r.saved_sp, r.steps) == (307, 4, 1)
    assert lc.LT_TAIL_DFS < r.high_water <= 304 + 3 * levels < lc.LT_TAIL_STACK
    assert lc.replay_identical(nodes, 1, tail_dfs=1 << 30).high_water == 352
