"""What the cases of tests/tsdf_pix_cases.py reach, proven without a GPU: on which side of LT_PIX_STAGE every item's search
range falls (float64 bounds with every column near an image-column boundary left out), the quirk set of k_wd_keys (float32,
exact), empty wedges, and -- with the C restatement of the reference kernel, oracle/lt_tsdf_oracle.c -- that no case is idle.
Which branch the kernel then takes is read from its counters in tests/test_tsdf_pix_paths_gpu.py."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tsdf_pix_cases as pc  # noqa: E402


def test_constants_are_those_of_the_source():
    """A changed #define fails here, not in a GPU run."""
    src = pc.source_constants()
    assert src == dict(LT_PIX_STAGE=float(pc.LT_PIX_STAGE), LT_PIX_AGG=float(pc.LT_PIX_AGG), LT_PIX_CHUNK=float(pc.LT_PIX_CHUNK),
                       LT_AXIS_RHO=float(pc.LT_AXIS_RHO)), src
    text = open(pc.HIP).read()
    import re
    d = {k: int(v) for k, v in re.findall(r"^#define LT_PIX[CT]_(\w+) (\d+)\b", text, re.M)}
    assert d["N"] == pc.N_CNT and d["NPT"] == 11
    for name, word in pc.CNT.items():   # the words of lt_debug_tsdf_pix_paths as the cases module numbers them
        if 16 <= word < 27:
            assert d["THREAD0"] + d[name.upper()] == word, name
        elif word >= 8:
            assert d[name.upper()] == word, name


@pytest.mark.parametrize("name", pc.NAMES)
def test_every_item_is_on_the_intended_side_of_the_staging_limit(name):
    c = pc.case(name)
    sb = pc.stage_bounds(name)
    n_items = -(-c["H"] * c["W"] // 64)
    assert len(sb) == n_items
    lo, hi = pc.wedge_bounds(name)
    t = pc.columns(name)
    n_cols = c["dims"][0] * c["dims"][1]
    tail = int(t["quirk"].sum()) if pc.quirk_tail_in_last_wedge(c["W"]) else 0
    assert lo.sum() <= n_cols - int(t["quirk"].sum()) + tail <= hi.sum()
    if c["expect"] == "unstaged":
        assert lo.min() >= pc.LT_PIX_STAGE + 64, f"{name}: a wedge of {lo.min()} entries"
        assert all(a >= pc.LT_PIX_STAGE + 64 for a, _ in sb)
    elif c["expect"] == "staged":
        assert all(b <= pc.LT_PIX_STAGE - 64 for _, b in sb), f"{name}: an item of up to {max(b for _, b in sb)} entries"
    else:   # holes (two items of 16 wedges each) and beyond_2p24: whatever side, but the same for every item and known
        assert all(a >= pc.LT_PIX_STAGE + 64 for a, _ in sb), f"{name}: {sb}"


def test_items_of_the_cases():
    assert len(pc.items("straddle_partial")) == 6 and 25 * 13 == 5 * 64 + 5
    spans = pc.items("straddle_partial")
    assert all(b > a for a, b in spans[:-1]) and len({(p0 % 25) for p0 in range(0, 325, 64)}) == 6   # every offset differs
    assert all(b == a + 1 for a, b in pc.items("two_wedges"))
    assert all(b == a for a, b in pc.items("staged_agg")) and all(b == a for a, b in pc.items("unstaged_direct"))


def test_outside_has_empty_wedges_at_both_ends_and_in_runs():
    lo, hi = pc.wedge_bounds("outside")
    assert hi[0] == 0 and hi[-1] == 0
    empty = hi == 0
    assert empty[:5].all() and empty[-5:].all(), "runs of empty wedges at both ends (k_wd_finish fills wd_start in a loop)"
    assert (lo > 0).sum() >= 4
    assert sum(1 for a, b in pc.items("outside") if hi[a:b + 1].sum() == 0) >= 8, "whole items without a table entry"


def test_the_quirk_sets():
    on, off, big = pc.columns("axis_on"), pc.columns("axis_off"), pc.columns("beyond_2p24")
    assert int(on["axis"].sum()) == 1 and float(on["rho"][on["axis"]][0]) == 0.0
    assert int(off["axis"].sum()) == 0 and float(off["rho"].min()) > 0.1
    assert int((~on["plain"]).sum()) == 0 and int(on["quirk"].sum()) == 48 + 1
    assert int(off["quirk"].sum()) == 48
    dx, dy, dz = pc.case("beyond_2p24")["dims"]
    assert dx * dy * dz > 2 ** 24
    col = np.arange(dx * dy)
    inner = ~big["plain"] & ~big["last_y"] & (col // dy != dx - 1)
    assert int(inner.sum()) == 2, "non-plain columns besides the edge columns"
    assert sorted((int(k) // dy, int(k) % dy) for k in col[inner]) == [m[:2] for m in pc.MISPLACED]
    assert int(big["quirk"].sum()) == dx + 2
    for name in pc.NAMES:   # the three sources, counted
        t = pc.columns(name)
        assert int(t["quirk"].sum()) == int((~t["plain"] | t["last_y"] | t["axis"]).sum()) >= pc.case(name)["dims"][0]


@pytest.mark.parametrize("name", pc.NAMES)
def test_images_hold_the_special_values(name):
    obs = pc.case(name)["obs"]
    d = np.concatenate([o[1].ravel() for o in obs])
    col = np.concatenate([pc.fold(o[0]).ravel() for o in obs])
    trunc = pc.case(name)["voxel"] * 5
    assert (d == 0).any() and (d == -1).any() and np.isnan(d).any() and np.isposinf(d).any()
    assert ((d < 0) & (d > -trunc)).any(), "a negative depth above -trunc_margin"
    assert set(np.unique(col)) == {0.0, 7.0, 300.0}


@functools.lru_cache(maxsize=None)
def _census(name):
    """The C restatement over the case's observations: the volumes after each."""
    from oracle import binding as ob
    ob.build()
    c = pc.case(name)
    vols = [np.ones(c["dims"], np.float32)] + [np.zeros(c["dims"], np.float32) for _ in range(3)]
    out = []
    for l3, d, r in c["obs"]:
        ob.tsdf_integrate(vols, c["dims"], c["origin"], c["voxel"], c["fov"][0], c["fov"][1], pc.fold(l3), d, r, 1.0, True)
        out.append([v.copy() for v in vols] if name not in pc.BIG else None)
    return out, vols


@pytest.mark.parametrize("name", pc.NAMES)
def test_no_case_is_idle(name):
    """(beyond_2p24 included: two observations of 17.4 M voxels take about a second here.)"""
    _, (tsdf, weight, color, rem) = _census(name)
    written = (weight > 0) | (tsdf != 1)
    floor = 3000 if name != "degenerate_1x1" else 1000
    assert written.sum() > floor, f"{name}: {written.sum()} voxels written"
    assert (tsdf < 0).sum() > 40
    if name != "degenerate_1x1":    # (one pixel: every observation another class or no depth)
        assert (weight >= 2).sum() > 100, "no voxel written twice"
    assert (color == 7).sum() > 0 and (color == 300).sum() > 0 or name.startswith("degenerate")
    if name == "beyond_2p24":
        for x, y, z in pc.MISPLACED:
            assert weight[x, y, z] > 0, f"the misplaced voxel of column ({x}, {y}) is not written"


def test_holes_has_written_ranges_strictly_inside_their_rows():
    """After the first four observations (the surface at 2 m, moved out, moved in, repeated) there are columns whose written z
    range lies strictly inside the pitch span of ONE image row: the voxel below and the voxel above the range project into
    the same row and inside the field of view.  The last observation's interval (colour 0 at 3 m: from the sensor to 3.25 m)
    contains such a range strictly: a hole."""
    c = pc.case("holes")
    states, _ = _census("holes")
    dx, dy, dz = c["dims"]
    fu, fd = np.radians(c["fov"][0]), np.radians(c["fov"][1])
    x = (c["origin"][0] + np.arange(dx) * c["voxel"])[:, None, None]
    y = (c["origin"][1] + np.arange(dy) * c["voxel"])[None, :, None]
    z = (c["origin"][2] + np.arange(dz) * c["voxel"])[None, None, :]
    with np.errstate(invalid="ignore"):     # (the voxel at the sensor)
        pitch = np.nan_to_num(np.arcsin(z / np.sqrt(x * x + y * y + z * z)))
    row = np.clip(np.floor((1.0 - (pitch + abs(fd)) / (abs(fu) + abs(fd))) * c["H"]), 0, c["H"] - 1).astype(int)
    inside = (pitch < fu - 1e-3) & (pitch > fd + 1e-3)
    for k in (0, 3):
        tsdf, weight = states[k][0], states[k][1]
        w = (weight > 0) | (tsdf != 1)
        any_w = w.any(2)
        zlo, zhi = w.argmax(2), dz - 1 - w[:, :, ::-1].argmax(2)
        ok = any_w & (zlo >= 1) & (zhi <= dz - 2)
        ix, iy = np.nonzero(ok)
        lo, hi = zlo[ix, iy], zhi[ix, iy]
        same = (row[ix, iy, lo - 1] == row[ix, iy, lo]) & (row[ix, iy, hi + 1] == row[ix, iy, lo]) & \
               (row[ix, iy, hi] == row[ix, iy, lo]) & inside[ix, iy, lo - 1] & inside[ix, iy, hi + 1]
        depth_out = np.sqrt(x * x + y * y + z * z)[ix, iy, np.where(z[0, 0, hi + 1] < 0, lo - 1, hi + 1)]
        assert (same & (depth_out < 3.0)).sum() >= 64, f"after observation {k}: {same.sum()} columns"
    # the moved surfaces cut: voxels written by observation 2 / 3 that observation 1 had not written, next to ones it had
    wr = [(s[1] > 0) | (s[0] != 1) for s in states]   # (a voxel another class took over keeps the weight 0)
    for k in (1, 2):
        new = wr[k] & ~wr[k - 1]
        assert (new.any(2) & wr[0].any(2)).sum() >= 64 and (new.any(2) & ~wr[k - 1].any(2)).sum() >= 16
    assert np.array_equal(wr[3], wr[2]), "the repeated observation writes no new voxel"
    assert (wr[4] & ~wr[3]).sum() > 100000
