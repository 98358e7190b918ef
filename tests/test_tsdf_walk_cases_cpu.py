"""What the cases of tests/tsdf_walk_cases.py reach, proven without a GPU: the dead, dead-but-walked and live columns of every
observation, the live and dead chunks, the trip counts, band on or off, what the z range leaves out, the voxels the reference's
float index misplaces and the columns they sit in, and -- with the C restatement of the reference kernel,
oracle/lt_tsdf_oracle.c -- which columns an observation finds written.  A case whose condition does not hold is a wrong input.
Which branch the kernel then takes is read from its counters and tables in tests/test_tsdf_walk_paths_gpu.py, which compares
the tables k_tsdf_columns makes with the restatement used here, column by column."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tsdf_walk_cases as wc  # noqa: E402

SMALL = [n for n in wc.NAMES if n not in wc.BIG]
OWN_SMALL = [n for n in wc.OWN if n not in wc.BIG]


def test_constants_are_those_of_the_source():
    src = wc.source_constants()
    assert src["LT_AXIS_RHO"] == float(wc.LT_AXIS_RHO) and src["RHO_LO"] == wc.RHO_LO
    assert (src["PAD_VOXELS"], src["PAD_RHO"]) == (wc.PAD_VOXELS, wc.PAD_RHO)
    assert src["TAN_LIMIT"] == (wc.TAN_LIMIT, wc.TAN_LIMIT) and src["BAND"] == (wc.BAND_SIN, wc.BAND_SIN, wc.BAND_ROW)
    words = src["words"]
    assert words.pop("N") == wc.N_CNT
    assert {k.lower(): v for k, v in words.items()} == wc.CNT


def test_the_pixel_pass_cases_are_walk_cases_as_they_stand():
    import tsdf_pix_cases as pc
    for name in pc.NAMES:
        a, b = pc.case(name), wc.case(name)
        assert name in wc.NAMES and b["merge"] and not b["touch"]
        assert all(a[k] is b[k] for k in ("bnds", "obs", "origin")) and a["dims"] == b["dims"] and a["fov"] == b["fov"]


@pytest.mark.parametrize("name", SMALL)
def test_the_proofs_leave_out_at_most_two_per_cent_of_the_columns(name):
    """A column whose image column, dead-or-live decision or z range lies within the margin of the restatement counts for
    neither side.  The share is a condition on the case."""
    g = wc.geometry(name)
    for k in range(len(wc.case(name)["obs"])):
        sure = wc.walk_tables(name, k)["sure_walked"] & g["z_sure"]
        assert 1.0 - sure.mean() <= 0.02, f"{name}, observation {k}: {1.0 - sure.mean():.4f} of the columns within the margin"


def _chunks(name, flag):
    g = wc.geometry(name)
    pad = np.zeros(g["n_chunks"] * 64, np.asarray(flag).dtype)
    pad[:g["n_cols"]] = flag
    return pad.reshape(g["n_chunks"], 64)


@pytest.mark.parametrize("name", SMALL)
def test_which_kernel_the_default_environment_runs(name):
    c = wc.case(name)
    walk = not c["merge"] or c["touch"] or name in ("fov80", "wide") or name.startswith("trips_dz")
    assert wc.pix_applies(c) == (not walk)


@pytest.mark.parametrize("name", [n for n in wc.NAMES if n.startswith("colmax_")])
def test_colmax_cases(name):
    c, g = wc.case(name), wc.geometry(name)
    H, W = c["H"], c["W"]
    assert (H, W) in ((3, 70), (1, 64), (5, 65), (4, 129))
    sp = wc.colmax_special_columns(W)
    assert sp["inf"] // 64 == (W - 1) // 64 and (W % 64 == 0 or sp["inf"] % 64 < W % 64)
    for k in range(2):
        T = wc.walk_tables(name, k)
        cm = T["colmax"]
        assert cm[sp["zero"]] == -np.inf and cm[sp["m1"]] == -1.0 and cm[sp["neg"]] == -0.5
        assert cm[sp["nan"]] == np.inf and cm[sp["inf"]] == np.inf and np.isnan(c["obs"][k][1][:, sp["nan"]]).sum() == 1
        under = lambda px: (g["px_lo"] == px) & (g["px_hi"] == px) & T["sure"]     # noqa: E731
        assert under(sp["zero"]).sum() >= 8 and T["dead"][under(sp["zero"])].all()
        for nm, n_live in (("m1", 1), ("neg", 2)):      # the voxel columns next to the sensor, and they alone
            u = under(sp[nm])
            assert (~T["dead"][u]).sum() == n_live and T["dead"][u].sum() >= 4, nm
            assert float(g["rho"][u & ~T["dead"]].max()) < 0.8
        assert not T["dead"][under(sp["nan"])].any() and not T["dead"][under(sp["inf"])].any()


def test_dead_partial_has_dead_chunks_partly_dead_chunks_and_a_partial_last_chunk():
    name = "dead_partial"
    g = wc.geometry(name)
    assert g["n_cols"] % 64 == 3 and g["n_chunks"] == 134
    for k in range(2):
        T = wc.walk_tables(name, k)
        assert T["sure"].all()
        per = _chunks(name, T["walked"]).sum(1)
        assert (per == 0).sum() >= 35, "dead chunks"
        assert (per == 1).sum() >= 50, "chunks that hold the dead, walked column with y = dim_y - 1 and nothing else"
        assert ((per >= 2) & (per < 64)).sum() >= 20 and (per == 64).sum() == 0, "partly dead chunks"
        assert per[-1] >= 1, "the partial last chunk is walked: it holds (dim_x - 1, dim_y - 1)"
        assert T["info_m2"].sum() >= 60 and (T["dead"] & ~g["whole"]).sum() > 7000


def test_dead_ulp_decides_one_column_by_the_last_bit():
    name = "dead_ulp"
    c, g = wc.case(name), wc.geometry(name)
    col = wc.DEAD_ULP_COL[0] * c["dims"][1] + wc.DEAD_ULP_COL[1]
    px, rho_lo = wc._dead_ulp_target()
    assert g["px_lo"][col] == g["px_hi"][col] == px and g["rho_lo"][col] == rho_lo and not g["whole"][col]
    trunc = np.float32(c["voxel"] * 5)
    for k, steps in enumerate(wc.DEAD_ULP_STEPS):
        T = wc.walk_tables(name, k)
        cm = T["colmax"][px]
        assert bool(T["dead"][col]) == (steps < 0), f"observation {k}"
        # within a few float32 steps of the threshold, on the promised side
        assert abs(float(cm) - (float(rho_lo) - float(trunc))) <= 4 * float(np.spacing(np.float32(rho_lo)))
        assert not T["sure"][col], "the margin of the restatement leaves this column out: its own float32 decision is the proof"


def _trips(g, walked):
    t = (g["z1"] - (g["z0"] & ~15) + 15) >> 4
    return t[walked]


def test_tall_zrange_cuts_most_columns_off_a_multiple_of_16():
    name = "tall_zrange"
    c, g = wc.case(name), wc.geometry(name)
    dz, n = c["dims"][2], g["n_cols"]
    assert (g["z0"] > 0).sum() > 0.9 * n and (g["z0"] % 16 != 0).sum() > 0.75 * n and (g["z1"] < dz).sum() > 0.9 * n
    left_out = int((g["z0"] + dz - g["z1"]).sum())
    assert left_out > 0.4 * n * dz, "the z range leaves out most of the volume"
    T = wc.walk_tables(name, 0)
    assert set(np.unique(_trips(g, T["walked"] & T["sure"]))) >= {1, 2, 3}
    assert g["whole"].sum() == c["dims"][0] and (g["z1"] - g["z0"])[g["whole"]].min() == dz


@pytest.mark.parametrize("dz", list(wc.TRIPS))
def test_trip_counts_around_the_unroll_of_three(dz):
    name = f"trips_dz{dz}"
    c, g = wc.case(name), wc.geometry(name)
    assert c["dims"][2] == dz and not wc.fov_of(c)["tan_ok"]
    assert (g["z0"] == 0).all() and (g["z1"] == dz).all()
    T = wc.walk_tables(name, 0)
    assert set(_trips(g, T["walked"])) == {wc.TRIPS[dz]} and T["walked"].sum() == g["n_cols"]


def test_fov80_walks_whole_columns_without_the_band_test():
    c, g = wc.case("fov80"), wc.geometry("fov80")
    assert not wc.fov_of(c)["tan_ok"] and not wc.band_ok(c) and (g["z1"] - g["z0"] == c["dims"][2]).all()
    assert abs(np.radians(80.0)) > wc.TAN_LIMIT > abs(np.radians(60.0))


def test_band_on_and_off():
    on = {n: wc.band_ok(wc.case(n)) for n in ("band_29_9", "band_30", "rows_3000", "rows_3100")}
    assert on == dict(band_29_9=True, band_30=False, rows_3000=True, rows_3100=False), on
    F = wc.fov_of(wc.case("band_30"))
    assert F["su"] > 0.5 and wc.fov_of(wc.case("band_29_9"))["su"] < 0.5
    fov = np.radians(35.0)
    assert fov / 3000 > wc.BAND_ROW > fov / 3100
    for n in wc.NAMES:      # elsewhere: on under the street-scene field of view, off from 30 degrees on
        c = wc.case(n)
        assert wc.band_ok(c) == (max(abs(c["fov"][0]), abs(c["fov"][1])) < 30.0 and c["H"] <= 3000), n


def test_axis_columns():
    on, off = wc.geometry("axis_on"), wc.geometry("axis_off")
    assert on["axis"].sum() == 1 and float(on["rho"][on["axis"]][0]) == 0.0 and off["axis"].sum() == 0
    dz = wc.case("axis_on")["dims"][2]
    assert (on["z1"] - on["z0"])[on["axis"]][0] == dz, "the column on the axis is walked whole"
    inner = ~on["axis"] & ~on["whole"]
    assert (on["z1"] - on["z0"])[inner].max() < dz


def test_sparse_live_has_chunks_of_one_two_three_and_five_live_columns():
    name = "sparse_live"
    assert wc.case(name)["dims"][1] == 64, "a chunk is one x row"
    seen = set()
    for k in range(len(wc.case(name)["obs"])):
        T = wc.walk_tables(name, k)
        assert T["sure"].all()
        seen |= set(_chunks(name, T["walked"]).sum(1).tolist())
    assert seen >= {1, 2, 3, 5}, seen


# ---- with the C restatement of the reference kernel: what an observation writes ------------------------------------------

@functools.lru_cache(maxsize=None)
def _census(name):
    """Per observation prefix: the mask of written voxels and the tsdf field."""
    from oracle import binding as ob
    ob.build()
    c = wc.case(name)
    vols = [np.ones(c["dims"], np.float32)] + [np.zeros(c["dims"], np.float32) for _ in range(3)]
    out = []
    for (l3, d, r), w in zip(c["obs"], c["weights"]):
        ob.tsdf_integrate(vols, c["dims"], c["origin"], c["voxel"], c["fov"][0], c["fov"][1], wc.fold(l3), d, r, w, c["merge"])
        out.append(((vols[1] > 0) | (vols[0] != 1) | (vols[2] != 0), vols[0].copy()))
    return out


@pytest.mark.parametrize("name", OWN_SMALL)
def test_no_case_is_idle_and_nothing_written_lies_outside_the_restated_tables(name):
    """The shortcuts as restated here are sound on the case: every voxel the C restatement writes lies in a walked column and
    inside its z range (columns within the margin left out).  On the GPU the same is asked of the kernel's own tables."""
    c, g = wc.case(name), wc.geometry(name)
    dx, dy, dz = c["dims"]
    prev = np.zeros(c["dims"], bool)
    z = np.arange(dz)[None, :]
    for k, (written, _) in enumerate(_census(name)):
        T = wc.walk_tables(name, k)
        new = (written & ~prev).reshape(dx * dy, dz)
        prev = written
        ok = T["sure_walked"] & g["z_sure"]
        assert not (new.any(1) & ~T["walked"] & ok).any(), f"{name}, observation {k}: written voxels in a dead column"
        outside = new & ((z < g["z0"][:, None]) | (z >= g["z1"][:, None]))
        assert not (outside.any(1) & ok).any(), f"{name}, observation {k}: written voxels outside the z range"
    floor = 40 if name in ("trips_dz1", "dead_ulp") else 300
    assert prev.sum() > floor, f"{name}: {prev.sum()} voxels written"


def test_mixed_waves_second_observation_meets_written_and_fresh_columns_in_one_chunk():
    name = "mixed_waves"
    dx, dy, dz = wc.case(name)["dims"]
    after0 = _census(name)[0][0].reshape(dx * dy, dz).any(1)
    T = wc.walk_tables(name, 1)
    live = T["walked"] & T["sure_walked"]
    w, f = _chunks(name, live & after0).sum(1), _chunks(name, live & ~after0).sum(1)
    assert ((w >= 4) & (f >= 4)).sum() >= 12, "chunks with written and fresh live columns"
    # ... and within one quad of four consecutive live columns: a wave with band and direct quarter waves
    mixed_quads = 0
    for ch in range(len(w)):
        cols = np.nonzero(_chunks(name, live)[ch])[0] + 64 * ch
        for q in range(0, len(cols) - 3, 4):
            s = after0[cols[q:q + 4]].sum()
            mixed_quads += 0 < s < 4
    assert mixed_quads >= 20


def test_flush_cases():
    thin = wc.case("class_thin")
    assert thin["dims"][2] * 16 < 64, "a wave walks at most 16 columns of a chunk: fewer than 64 candidates"
    assert all((wc.fold(o[0]) != 0).all() for o in thin["obs"])
    wall = wc.case("wall0")
    assert all((wc.fold(o[0]) == 0).all() for o in wall["obs"])
    written = _census("wall0")[0][0]
    dx, dy, dz = wall["dims"]
    per_col = written.reshape(dx * dy, dz).sum(1)
    # (a written voxel was a candidate: 4 * 64 of them in a chunk fill the queue of one of its four waves at least)
    assert (_chunks("wall0", per_col).sum(1) >= 4 * 64).sum() >= 8, "chunks with a full queue"


def test_sign_word_cases():
    for dz, merge in ((37, True), (64, True), (65, False), (130, False)):
        c = wc.case(f"signs_dz{dz}")
        assert c["dims"][2] == dz and c["merge"] == merge and not wc.band_ok(c), "every voxel through the direct path"
    for name in ("signs_dz65", "signs_dz130"):
        dx, dy, dz = wc.case(name)["dims"]
        written, tsdf = _census(name)[0]
        w = written.reshape(dx * dy, dz)
        assert (w[:, 63] & w[:, 64]).sum() >= 100, "written runs across z = 64"
    written, tsdf = _census("signs_dz130")[0]
    w, t = written.reshape(-1, 130), tsdf.reshape(-1, 130)
    for lo in (48, 64):     # a 16-aligned chunk of z that holds values <= 0, values > 0 and untouched voxels
        neg, pos = (w & (t <= 0))[:, lo:lo + 16], (w & (t > 0))[:, lo:lo + 16]
        assert (neg.any(1) & pos.any(1)).sum() >= 30, lo
    assert ((w & (t <= 0))[:, 64:].any(1)).sum() >= 100, "sign bits in the words of index >= 1"


def test_signs_nan_writes_nan_next_to_both_signs_in_one_chunk_of_a_sign_word():
    """The second observation turns the voxels the first one wrote at infinite weight into NaN (code 2 by `!(tv > 0)`), and
    writes values <= 0 and > 0 between them: all three in one 16-aligned chunk of z of one column, in the second sign word."""
    c = wc.case("signs_nan")
    assert c["dims"][2] == 130 and not c["merge"] and not c["touch"] and c["weights"] == (np.inf, 1.0, 1.0)
    (w0, t0), (w1, t1), _ = _census("signs_nan")
    t0, t1, w1 = t0.reshape(-1, 130), t1.reshape(-1, 130), w1.reshape(-1, 130)
    assert (t0[w0.reshape(-1, 130)] == 0).all() and not np.isnan(t0).any()
    for lo in (48, 64):
        sl = slice(lo, lo + 16)
        nan, neg, pos = np.isnan(t1[:, sl]), (w1 & (t1 <= 0))[:, sl], (w1 & (t1 > 0))[:, sl]
        assert (nan.any(1) & neg.any(1) & pos.any(1)).sum() >= (20 if lo == 64 else 5), lo
    assert np.isnan(t1[:, 64:]).sum() >= 200 and np.isnan(t1[:, :64]).sum() >= 200


def test_reset_cases():
    dx, dy, dz = wc.case("plain_avg_b")["dims"]
    w = _census("plain_avg_b")[-1][0].reshape(dx * dy, dz)
    lo, hi = w.argmax(1), dz - 1 - w[:, ::-1].argmax(1)
    assert ((hi - lo + 1)[w.any(1)] > 16).sum() >= 100, "written ranges longer than 16 voxels"
    dx, dy, dz = wc.case("dead_partial")["dims"]
    per = _chunks("dead_partial", _census("dead_partial")[-1][0].reshape(dx * dy, dz).any(1)).sum(1)
    assert (per % 4 != 0).sum() >= 10, "chunks whose number of dirty columns is no multiple of four"


# ---- beyond 2^24 voxels --------------------------------------------------------------------------------------------------

def _phantom_is_written(name, x, y, phantom_x):
    """Does the reference kernel, given voxel (x, y, 0), write it through the pixel of the position its float index makes of
    it -- (x - 1, dim_y, 0) or (x + 1, -2, 0) -- in the first observation?  float64; the margins are metres wide."""
    c = wc.case(name)
    dx, dy, dz = c["dims"]
    py = y + dy if phantom_x < x else y - dy        # the same index, read with another x
    pt = c["origin"].astype(np.float64) + np.array([phantom_x, py, 0]) * c["voxel"]
    depth = np.linalg.norm(pt)
    pitch = np.arcsin(pt[2] / depth)
    fu, fd = np.radians(c["fov"][0]), np.radians(c["fov"][1])
    px = int(np.floor(0.5 * (-np.arctan2(pt[1], pt[0]) / np.pi + 1.0) * c["W"]))
    row = int(np.floor((1.0 - (pitch + abs(fd)) / (abs(fu) + abs(fd))) * c["H"]))
    d = float(c["obs"][0][1][row, px])
    return fd + 1e-3 < pitch < fu - 1e-3 and d == 60.0 and depth < 50.0


def test_big_y0_misplaces_fourteen_first_voxels_of_dead_columns_with_y_zero():
    name = "big_y0"
    c, g = wc.case(name), wc.geometry(name)
    dx, dy, dz = c["dims"]
    assert c["dims"] == (1031, 1021, 17) and (dy * dz) % 2 == 1 and dx * dy * dz > 2 ** 24
    m = wc.misplaced(name)
    assert m.shape[0] == 14 and (m[:, 1] == 0).all() and (m[:, 2] == 0).all() and (m[:, 3] == m[:, 0] - 1).all()
    assert m[0, 0] == 969 and m[1, 0] == 973
    cols = m[:, 0] * dy
    assert g["whole"][cols].all(), "k_tsdf_columns' rule (both ends of the column) finds them"
    assert np.array_equal(np.nonzero(g["whole"] & (g["y"] != dy - 1))[0], cols), "... and nothing else besides y = dim_y - 1"
    inside = np.all((c["bnds"][:, 0] < 0) & (c["bnds"][:, 1] > 0))
    assert inside, "the sensor is inside the volume"
    for k in range(2):      # dead by their own geometry in both observations: a walk that asks y == dim_y - 1 alone skips them
        T = wc.walk_tables(name, k)
        assert T["sure"][cols].all() and T["dead"][cols].all() and T["info_m2"][cols].all()
    assert all(_phantom_is_written(name, int(x), 0, int(x) - 1) for x in m[:, 0]), "the reference writes all fourteen"
    # were such a column live, the tangent range would cut z = 0 off: it lies 25 degrees below the horizon only at rho < 1.2 m
    F = wc.fov_of(c)
    assert float(g["rho"][cols].min()) * float(F["tan_down"]) + 3 * c["voxel"] < float(c["origin"][2])


def test_big_ym2_misplaces_six_voxels_of_the_row_before_the_last():
    name = "big_ym2"
    c, g = wc.case(name), wc.geometry(name)
    dx, dy, dz = c["dims"]
    assert c["dims"] == (5800, 5796, 1) and dx * dy * dz > 2 ** 25
    m = wc.misplaced(name)
    assert m.shape[0] == 6 and (m[:, 1] == dy - 2).all() and (m[:, 3] == m[:, 0] + 1).all()
    cols = m[:, 0] * dy + m[:, 1]
    assert g["whole"][cols].all()
    T = wc.walk_tables(name, 0)
    assert T["sure"][cols].all() and T["dead"][cols].all() and T["info_m2"][cols].all()
    assert all(_phantom_is_written(name, int(x), dy - 2, int(x) + 1) for x in m[:, 0])


def test_beyond_2p24_of_the_pixel_pass_cases():
    import tsdf_pix_cases as pc
    m = wc.misplaced("beyond_2p24")
    assert sorted((int(a), int(b), int(z)) for a, b, z, _ in m) == sorted(pc.MISPLACED)
    g = wc.geometry("beyond_2p24")
    dy = wc.case("beyond_2p24")["dims"][1]
    assert g["whole"][m[:, 0] * dy + m[:, 1]].all()


def test_the_default_volume_has_no_such_column():
    """2000 x 2000 x 200: every column start is a multiple of 200 = 2^3 * 25 below 2^30 -- representable in float32 only where
    ... the restatement counts: every column that is not plain has y = dim_y - 1."""
    dx = dy = 2000
    dz = 200
    col = np.arange(dx * dy, dtype=np.int64)
    dyz = np.float32(dy * dz)
    xf = (col // dy).astype(np.float32)
    bad = (np.floor((col * dz).astype(np.float32) / dyz) != xf) | (np.floor((col * dz + dz - 1).astype(np.float32) / dyz) != xf)
    assert bad.sum() > 0 and (col[bad] % dy == dy - 1).all()
