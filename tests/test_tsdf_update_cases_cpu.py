"""tests/tsdf_update_cases.py without a GPU: a census of what the cases reach, the update restatement pinned bit for bit to
the C oracle (oracle/lt_tsdf_oracle.c), and the host-mode restatement pinned to the golden volumes F8.

The census carries the state from observation to observation with the C oracle.  Each voxel's pixel and truncated distance
come from a PROBE volume rather than from a second statement of the projection: the C oracle run on a fresh volume with the
plain average, weight 1, the observation's depth image and a colour image that holds `pixel index + 1` (below 2^24, every
channel <= 255: it comes back unchanged) leaves `colour - 1` = the pixel and `tsdf` = the distance, for exactly the voxels
that pass the depth tests (weight 1).

The thresholds are conditions ("at least 100 voxels"), not measurements.  "A voxel with a weight" below is weight > 0: a
voxel that some same-class update has integrated.  A voxel another class has won while fresh keeps weight 0 and goes on
rejecting every dist >= 0 at ANY obs_weight; the blind spot of weight 1 is the voxel WITH a weight, which then accepts every
dist < 1 (dist < 1 <= w)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_update_cases as tc  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("tsdf", "weight", "color", "rem")
AT_LEAST = 100


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _probe(oracle, depth):
    """(hit, dist, pixel) of every voxel for one depth image -- see the module docstring."""
    vols = tc.fresh_volumes()
    index = (np.arange(tc.H * tc.W, dtype=np.float32) + 1).reshape(tc.H, tc.W)
    oracle.tsdf_integrate(vols, tc.DIMS, tc.ORIGIN, tc.VOXEL, tc.FOV_UP, tc.FOV_DOWN, index, depth, np.zeros_like(depth), 1.0,
                          merge=False)
    hit = vols[1] == 1
    pixel = np.where(hit, vols[2] - 1, 0).astype(np.int64)
    assert pixel.max() < tc.H * tc.W and (vols[2][~hit] == 0).all()
    return hit, vols[0], pixel


@functools.lru_cache(maxsize=None)
def _census(case):
    """Runs the case on the C oracle and on the update restatement side by side; returns the counts and the final volume."""
    from oracle import binding as oracle
    c = tc.CASES[case]
    ref = tc.fresh_volumes()
    cnt = dict(same=0, wins=0, rejected_weighted_lt1=0, rejected=0, tie=0, clamp=0, fused_differs=0, hit=0)
    for k, (label3, depth, rem) in enumerate(tc.observations(case)):
        folded = tc.fold(label3)
        hit, dist, pixel = _probe(oracle, depth)
        new_color, new_rem = folded.reshape(-1)[pixel], rem.reshape(-1)[pixel]
        got, info = tc.update(ref, hit, dist, new_color, new_rem, c["weight"], c["merge"])
        t0, w0 = ref[0].copy(), ref[1].copy()
        oracle.tsdf_integrate(ref, tc.DIMS, tc.ORIGIN, tc.VOXEL, tc.FOV_UP, tc.FOV_DOWN, folded, depth, rem, c["weight"],
                              merge=c["merge"])
        for name, a, b in zip(NAMES, got, ref):      # (bit patterns: NaN positions count)
            bad = int((_bits(a) != _bits(b)).sum())
            assert bad == 0, f"{case}, observation {k}: the update restatement differs from the C oracle in {bad} voxels of {name}"
        arm = info["arm"]
        cnt["hit"] += int(hit.sum())
        averaged = (arm == tc.ARM_SAME) | (arm == tc.ARM_PLAIN)
        if c["merge"]:
            cnt["same"] += int((arm == tc.ARM_SAME).sum())
            cnt["wins"] += int((arm == tc.ARM_WINS).sum())
            cnt["rejected"] += int((arm == tc.ARM_REJECTED).sum())
            cnt["rejected_weighted_lt1"] += int(((arm == tc.ARM_REJECTED) & (w0 > 0) & (dist < 1)).sum())
        else:
            avg = info["avg"][:, hit].astype(np.float64)
            cnt["tie"] += int((avg - np.floor(avg) == 0.5).sum())
            cnt["clamp"] += int((avg > 255.5).sum())
        # the running average's numerator, fused (one rounding) against unfused (two), each divided as the kernel divides
        with np.errstate(all="ignore"):
            w_new = w0 + np.float32(c["weight"])
            fused = tc.fma32(t0, w0, dist) / w_new
            unfused = (t0 * w0 + dist) / w_new
        cnt["fused_differs"] += int((averaged & (_bits(fused) != _bits(unfused))).sum())
    return cnt, ref


DEVICE_CASES = tc.DEVICE_CASES


def test_the_geometry_is_the_one_the_cases_are_named_for():
    dims = np.ceil((tc.BNDS[:, 1] - tc.BNDS[:, 0]) / tc.VOXEL).astype(int)
    assert tuple(dims) == tc.DIMS == (65, 63, 24) and (65 * 63) % 64 != 0
    f = tc.fold(tc.CLASSES[None, :, :])[0]
    assert f[-1] == 16974792.0 and f[-1] > 2 ** 24, "the fold above 2^24 is the rounded float every implementation is handed"
    assert sorted(tc.CASES) == sorted(tc.DEVICE_CASES + tc.HOST_CASES) and len(tc.DEVICE_CASES) == 13
    for case in tc.CASES:
        for label3, depth, rem in tc.observations(case):
            assert (depth == 0).mean() > 0.02 and (depth == -1).sum() == 4 * tc.H
            assert rem.min() == -1.0 and rem.max() == 255.0 and (rem == 0).sum() > 0
            assert np.isnan(depth).any() == tc.CASES[case]["broken"] == np.isinf(depth).any()
    a, b = tc.observations("A-1.0"), tc.observations("D-nine")
    keep = np.mean([(a[k][0] == a[k + 1][0]).all(axis=2).mean() for k in range(3)])
    assert 0.4 < keep < 0.7, "about half of the pixels keep their class from one observation to the next"
    assert all(np.array_equal(x, y) for o, p in zip(a, b) for x, y in zip(o, p))   # D's first four are A's


def test_fma32_rounds_once():
    """The restatement's fmaf against exact rational arithmetic, on operands made to land on float32 midpoints."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.uniform(0.5, 2.0, 4000).astype(np.float32)
    b = rng.uniform(0.5, 2.0, 4000).astype(np.float32)
    c = (rng.uniform(-1, 1, 4000) * 2.0 ** rng.integers(-60, 3, 4000)).astype(np.float32)
    # a * b + c exactly half-way between two float32 but for a residue far below float64's last bit
    a[:1000] = 1.5
    b[:1000] = (1.0 + (2 * rng.integers(0, 2 ** 21, 1000) + 1) * 2.0 ** -23).astype(np.float32)   # odd last bit: 1.5 b has 25 bits
    c[:1000] = (rng.choice([-1.0, 1.0], 1000) * 2.0 ** -70).astype(np.float32)
    got = tc.fma32(a, b, c)

    def exact(x, y, z):
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(v))            # float(Fraction) is correctly rounded; then to float32: may be the wrong side
        cands = {lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))}
        best = min(cands, key=lambda q: (abs(Fraction(float(q)) - v), int(np.float32(q).view(np.int32)) & 1))
        return np.float32(best)
    want = np.array([exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (_bits(naive) != _bits(want)).sum() > 100, "the operands do not meet the double rounding"


@pytest.mark.parametrize("case", DEVICE_CASES)
def test_census(oracle, case):
    c = tc.CASES[case]
    cnt, (tsdf, weight, color, rem) = _census(case)
    w = c["weight"]
    print(f"\n{case}: {cnt}; tsdf > 1: {int((tsdf > 1).sum())}; weight not an integer: {int((weight != np.floor(weight)).sum())}")
    assert cnt["hit"] > 0.3 * tsdf.size
    if c["merge"]:
        assert cnt["same"] >= AT_LEAST and cnt["wins"] >= AT_LEAST and cnt["rejected"] >= AT_LEAST
        if w < 1:
            assert cnt["rejected_weighted_lt1"] >= AT_LEAST, "other class, dist < 1, the voxel has a weight, still rejected"
            # a fresh same-class voxel: tsdf = dist / obs_weight
            assert int((tsdf > 1).sum()) >= AT_LEAST
        if w == 1:
            assert cnt["rejected_weighted_lt1"] == 0, "the blind spot of obs_weight = 1"
    else:
        b, g, r = tc.unfold(color)
        if w in (1.0, 0.25):
            assert cnt["tie"] >= AT_LEAST, "channel averages exactly on x.5"
        # the clamp decides only where a channel can exceed 255: a fresh voxel holds new / obs_weight, so weights <= 1
        # (259 / 1, 255 / 0.7); at 2.5 the largest average is (255 * w_old + 259) / w_new < 255.5
        if w <= 1:
            assert cnt["clamp"] >= AT_LEAST, "channel averages above 255.5"
        # at 2^24 every average is new / 2^24 or old + new / 2^25: all colours stay 0
        if w < tc.W24:
            assert int(((g != 0) & (r != 0)).sum()) >= AT_LEAST
        else:
            assert float(color.max()) == 0.0
    if w != np.floor(w):
        assert int((weight != np.floor(weight)).sum()) >= AT_LEAST
    if w == tc.W24:
        assert cnt["fused_differs"] >= AT_LEAST, "fmaf(t, w, d) / w_new and (t * w + d) / w_new agree: the weight proves nothing"
    # (not a blind spot of weight 1, as it turns out: from the fourth observation on w_old = 3 and tsdf * 3 is inexact, so
    # the fused form matters at every weight -- tests before these fed at most three observations to one volume)
    if c["broken"]:
        assert np.isfinite(tsdf).all() and np.isfinite(rem).all()      # a NaN / infinite depth is dist = 1, not a NaN


def _host_mode_run(g, n_obs, weight=1.0):
    dims = tuple(np.ceil((g["bnds"][:, 1] - g["bnds"][:, 0]) / float(g["voxel"])).astype(int))
    vols = tc.fresh_volumes(dims)
    folded = tc.fold(g["label3"])
    for _ in range(n_obs):
        tc.host_mode_integrate(vols, g["bnds"][:, 0], float(g["voxel"]), float(g["fov_up"]), float(g["fov_down"]), folded,
                               g["depth_im"], weight)
    return vols


def test_host_mode_restatement_equals_the_golden_cpu_mode_volumes():
    """Two integrations at weight 1, as tests/test_tsdf_gpu.py::test_numpy_mode_equals_the_reference_numpy_cpu_mode asks of
    the device: tsdf bits, weight and colour, with that test's allowance for voxels within an ulp of a pixel boundary."""
    g = np.load(os.path.join(GOLD, "f8_tsdf_cpu_mode.npz"))
    tsdf, weight, color, rem = _host_mode_run(g, 2)
    assert tsdf.shape == g["tsdf"].shape
    n = tsdf.size
    diff = (_bits(tsdf) != _bits(g["tsdf"])) | (weight != g["weight"]) | (color != g["color"])
    assert diff.sum() <= max(2, 1e-5 * n), f"{diff.sum()} of {n} voxels differ"
    assert (g["weight"] > 0).sum() > 0.02 * n and float(np.abs(rem).max()) == 0.0


@pytest.mark.parametrize("case", tc.HOST_CASES)
def test_host_mode_cases_meet_the_ties(case):
    """At 1 and 2.5 the two roundings part on at least 100 channel averages.  At 0.25 with two observations they cannot: the
    first observation leaves min(255, 4 * new) -- a multiple of 4, or 255 -- and the second averages old / 2 + 2 * new, which is
    x.5 only for old = 255: 127.5 + 2 * new, between an odd number below and an even one above, where half to even and half
    away from zero both go up.  There the case holds the clamp and the ties as such; the count of parting ties is 0 by that
    arithmetic and asserted as such."""
    c = tc.CASES[case]
    vols, ties, on_half = tc.host_case(case)
    print(f"\n{case}: {on_half} channel averages on x.5, {ties} of them where half-to-even and half-away differ")
    assert on_half >= AT_LEAST
    if c["weight"] == 0.25:
        assert ties == 0
    else:
        assert ties >= AT_LEAST
    assert (vols[1] > 0).sum() > 0.3 * vols[1].size and float(np.abs(vols[3]).max()) == 0.0
