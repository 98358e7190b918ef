"""tests/writeback_cases.py without a GPU: the scenes have the hits, misses and values they claim (held against the
brute-force oracle), and `expected` lays the oracle's images into the padded buffers as stated."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import writeback_cases as wc  # noqa: E402


def _ref(oracle, shape, edges=False, offset=0):
    H, W, extra = shape
    mesh, rays, ray_of = wc.tiles(H, W, wc.seed_of(shape) + offset, edges)
    ref = wc.reference(oracle, mesh, wc.with_extra(rays, extra), H, H * W)
    return mesh, rays, ray_of, ref


@pytest.mark.parametrize("shape", wc.SHAPES)
def test_tiles_have_hits_and_misses_in_every_group_of_64(oracle, shape):
    H, W, extra = shape
    for offset in (0, 100):   # the mesh of a case, and the different one rendered after the all-NULL render
        mesh, rays, ray_of, ref = _ref(oracle, shape, offset=offset)
        n = H * W
        hit = ref["tri"] >= 0
        assert rays.shape == (n, 3) and hit.shape == (n,)
        # every face wins the ray it was built on, and no other cell is hit -- but for the last column, which repeats the first
        assert np.array_equal(ref["tri"][ray_of], np.arange(ray_of.size))
        twin = hit.reshape(H, W)[:, -1] if W >= 2 else np.zeros(H, bool)
        assert int(hit.sum()) == ray_of.size + int(twin.sum())
        if W >= 2:
            assert np.array_equal(rays.reshape(H, W, 3)[:, -1], rays.reshape(H, W, 3)[:, 0])
            assert np.array_equal(ref["tri"].reshape(H, W)[:, -1], ref["tri"].reshape(H, W)[:, 0])
        if W >= 3:   # (W <= 2 is one direction: one outcome)
            assert hit.any() and not hit.all(), "a tiles shape with two directions needs hits and misses"
            for g in range(n // 64):
                grp = hit[64 * g:64 * g + 64]
                assert grp.any() and not grp.all(), f"rays {64 * g} .. {64 * g + 63} are all {'hits' if grp.all() else 'misses'}"
        else:
            assert hit.all()


def test_the_two_meshes_of_a_shape_differ_where_it_matters(oracle):
    """after the all-NULL render of one mesh the other is rendered on the same scene: a cell that was not re-armed shows
    only if the first mesh hits a ray that the second misses; the face counts are equal, so a stale face index stays
    inside the second mesh"""
    for shape in wc.SUBSET_SHAPES:
        a, b = _ref(oracle, shape), _ref(oracle, shape, offset=100)
        assert a[0][1].shape == b[0][1].shape
        assert int(((a[3]["tri"] >= 0) & (b[3]["tri"] < 0)).sum()) >= 8


@pytest.mark.parametrize("shape", wc.SHAPES)
def test_the_float_round_trip_changes_a_hit_colour(oracle, shape):
    mesh, rays, ray_of, ref = _ref(oracle, shape)
    v, f, c, r = mesh
    hit = ref["tri"] >= 0
    raw = c[f[ref["tri"][hit], 0]]   # the colour of vertex 0, as stored
    got = ref["endcolors"][hit]
    assert np.array_equal(got, raw.astype(np.float32).astype(np.int64).astype(np.int32))   # (int)(float)c, in range
    assert (got[:, 2] != raw[:, 2]).any(), "channel 2 of no hit is changed by (int)(float)"
    assert (got != raw).any(axis=0).all() or ray_of.size < 2
    assert np.abs(c.astype(np.int64)).max() <= 2 ** 31 and c.max() <= wc.C_MAX
    planted = set(int(x) for x in c[f[ref["tri"][hit], 0]].reshape(-1))
    assert set(wc.PLANTED_COLORS[:min(ray_of.size, 4)]) <= planted
    if ray_of.size >= 4:   # each planted value is seen in channel 2 = the label image
        assert set(wc.PLANTED_COLORS) <= set(int(x) for x in raw[:, 2])
    # the other two vertices have other colours: a write-back that reads vertex 1 or 2 writes something else
    assert (c[f[:, 0]] != c[f[:, 1]]).all() and (c[f[:, 0]] != c[f[:, 2]]).all()


def test_value_edges_reach_a_hit_with_each_planted_value(oracle):
    mesh, rays, ray_of, ref = _ref(oracle, wc.EDGE_SHAPE, edges=True)
    v, f, c, r = mesh
    rem = ref["endrem"][ray_of[:len(wc.PLANTED_REM)]]   # face k is hit by ray_of[k]
    bits = rem.view(np.int32)
    want = dict(denormal_kept=0x00000001, denormal_lost=0x00000000, minus_zero=-0x80000000, overflow=0x7F800000,
                cancelled_overflow=0x7F800000, inf=0x7F800000)
    for k, name in enumerate(wc.PLANTED_REM):
        assert np.array_equal(r[f[k]].view(np.int32), np.array(wc.PLANTED_REM[name], np.float32).view(np.int32)), name
        if name in want:
            assert int(bits[k]) == want[name], (name, hex(int(bits[k]) & 0xFFFFFFFF))
    assert np.isnan(rem[list(wc.PLANTED_REM).index("nan")]) and int(np.isnan(ref["endrem"]).sum()) >= 1
    assert rem[list(wc.PLANTED_REM).index("minus_zero_first")] == np.float32(0.25)
    # r0 + (r1 + r2) gives another result somewhere: the order of the sum is observable
    t = ref["tri"][ref["tri"] >= 0]
    r0, r1, r2 = (r[f[t, j]] for j in range(3))
    with np.errstate(all="ignore"):
        other = (r0 + (r1 + r2)) / np.float32(3)
        same = ((r0 + r1) + r2) / np.float32(3)
    assert np.array_equal(same.view(np.int32)[~np.isnan(same)], ref["endrem"][ref["tri"] >= 0].view(np.int32)[~np.isnan(same)])
    assert int((other.view(np.int32) != same.view(np.int32)).sum()) >= 4


@pytest.mark.parametrize("H,W", [s[:2] for s in wc.SUBSET_SHAPES])
def test_wall_is_hit_by_every_ray_and_the_empty_mesh_by_none(oracle, H, W):
    mesh, rays = wc.wall(H, W)
    ref = wc.reference(oracle, mesh, rays, H, H * W)
    assert (ref["tri"] == 0).all()
    ref = wc.reference(oracle, wc.empty_mesh(), rays, H, H * W)
    assert (ref["tri"] == -1).all() and not ref["range"].view(np.int32).any()


@pytest.mark.parametrize("shape", wc.SHAPES)
def test_expected_reproduces_the_oracle_and_the_guards(oracle, shape):
    H, W, extra = shape
    mesh, rays, ray_of, ref = _ref(oracle, shape)
    n, R = H * W, H * W + extra
    hit = ref["tri"] >= 0
    assert wc.tail_of(R) >= max(2 * R, 768) + 64
    assert [wc.LEAD[k] for k in wc.KEYS] == [0, 1, 2, 3, 1]
    for label in (False, True):
        lay = wc.layout(R, label)
        full = wc.expected(ref, hit, wc.Variant(True, label, wc.KEYS, extra))
        for k in wc.KEYS:
            lead, count, shp, total = lay[k]
            assert full[k].shape == (total,) and total - lead - count == wc.tail_of(R) and count == int(np.prod(shp))
            body = full[k][lead:lead + count].reshape(shp)
            img = ref[k][:, 2] if (k == "endcolors" and label) else ref[k]
            assert np.array_equal(body[:n], np.ascontiguousarray(img).view(np.int32)), k   # the oracle's own arrays, misses included
            assert (body[n:] == wc.SENTINEL).all() and (full[k][:lead] == wc.SENTINEL).all()
            assert (full[k][lead + count:] == wc.SENTINEL).all()
        # hits only: misses keep the sentinel; a NULL pointer: the whole buffer does
        part = wc.expected(ref, hit, wc.Variant(False, label, ("range", "tri"), extra))
        for k in wc.KEYS:
            lead, count, shp, total = lay[k]
            body = part[k][lead:lead + count].reshape(shp)
            if k in ("range", "tri"):
                assert np.array_equal(body[:n][hit], full[k][lead:lead + count].reshape(shp)[:n][hit])
                assert (body[:n][~hit] == wc.SENTINEL).all() and (body[n:] == wc.SENTINEL).all()
            else:
                assert (part[k] == wc.SENTINEL).all()
        assert wc.differences(full, full, "same") == []
        assert len(wc.differences(part, full, "other")) == (3 if hit.all() else 5)


def test_differences_holds_a_nan_to_isnan_and_everything_else_to_its_bits(oracle):
    mesh, rays, ray_of, ref = _ref(oracle, wc.EDGE_SHAPE, edges=True)
    hit = ref["tri"] >= 0
    want = wc.expected(ref, hit, wc.Variant(True, False, wc.KEYS, 0))
    got = {k: x.copy() for k, x in want.items()}
    i = int(np.flatnonzero(np.isnan(want["endrem"].view(np.float32)))[0])
    got["endrem"][i] ^= 1   # another NaN
    assert wc.differences(got, want, "x") == []
    got["endrem"][i] = 0x7F800000   # +inf is no NaN
    assert len(wc.differences(got, want, "x")) == 1
    got["endrem"][i] = want["endrem"][i]
    got["endrem"][-1] = 0   # the last guard element
    assert len(wc.differences(got, want, "x")) == 1


def test_subsets_and_batch_groups():
    assert len(wc.SUBSETS) == 12 == len(set(wc.SUBSETS))
    assert wc.SUBSETS[0] == wc.KEYS and wc.SUBSETS[-1] == () and sorted(len(s) for s in wc.SUBSETS) == [0] + [1] * 5 + [4] * 5 + [5]
    assert sorted(len(g) for g in wc.BATCH_GROUPS) == [1, 2, 3, 8, 8]
    pairs = set()
    for g, group in enumerate(wc.BATCH_GROUPS):
        cast = [0 if s == "no_rays" else (wc.EMPTY_SHAPE if s == "empty" else s) for s in group]
        live = [s[0] * s[1] for s in cast if s]   # a scan without rays gets no resolve block: its neighbours are adjacent
        pairs |= set(zip(live, live[1:]))
        assert len(set(wc.batch_subset(g, i) for i in range(len(group)))) == len(group)
        if len(group) == 8:
            assert "no_rays" in group[1:-1] and "empty" in group[1:-1]
        assert all(s in ("no_rays", "empty") or s in wc.SHAPES for s in group)
    # a first resolve block after a full last block (256, 512) and after ragged ones (1, 255, 257)
    assert {(255, 256), (256, 1), (1, 257), (1, 255), (256, 257), (512, 256), (512, 257), (256, 255)} <= pairs
