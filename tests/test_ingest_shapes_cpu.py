"""Seeded inputs for the ingest stage at the size it ships at and at its edge shapes, and what keeps them honest without
a GPU.  tests/test_ingest_shapes_gpu.py imports the generators below and compares `lt_ingest_scans_dev` with THE numpy
restatement of its five rules (tests/test_ingest_cpu.py::restate, pinned to the reference program's output on golden F17).
Here the restatement itself is checked on the new inputs against an independent evaluation -- a per-point Python `set`
lookup for the kept set and its order, `np.longdouble` arithmetic for the points -- and the generators against what the
GPU tests assume of them: no sentinel bit pattern in any input, the planted rows, lengths off the multiples of 256, the
number of workgroups, the documented size of `work`."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_ingest_cpu as cpu  # noqa: E402

# what tests/test_ingest_shapes_gpu.py::call_ingest fills its buffers with before the call
SENT_F64 = 0x7FF4DEADBEEF0001   # a NaN whose low mantissa bits no float32 -> float64 conversion can set
SENT_F32 = 0x7FA5A5A5
SENT_U32 = 0xA5A5A5A5           # (an output label is at most 0xFFFF)

# 30 classes: the ignore / moving classes of config/lidar_transfer.yaml, both ends of the 16-bit range, static ones
CLASSES = np.array([0, 1, 10, 11, 13, 15, 16, 18, 20, 30, 31, 32, 40, 44, 48, 49, 50, 51, 52, 60, 70, 71, 72, 80, 81, 99,
                    252, 253, 259, 65535], dtype=np.uint32)
# shares: 0 and 1 4 % each, 252 and 253 5 % each, the rest evenly -- slot 0 keeps ~92 %, the others ~82 %
WEIGHTS = np.where(np.isin(CLASSES, [0, 1]), 0.04, np.where(np.isin(CLASSES, [252, 253]), 0.05, 0.82 / 26))
IGNORE, MOVING = [0, 1], [252, 253]
# more than LT_INGEST_LIST_ARGS (16) entries: these travel as a bitmap
IGNORE_LONG = [0, 1, 65535] + list(range(1000, 1020))
MOVING_LONG = [252, 253, 259] + list(range(300, 337))
UPPER_ONLY = [(253 << 16) | 7, (1 << 16) | 9]   # a listed class in the UPPER 16 bits, an unlisted one (7, 9) in the lower
N = 2500                                        # the `n` of the slot-shape table

SLOT_SHAPES = [(0, N, N), (N, 0, N), (N, N, 0), (0, 0, N), (N, 0, 0), (1,), (1, 1, 1), (255, 256, 257), (256,) * 16,
               (65536, 65537, 65535), (0,), (0, 0, 0)]
CPU_TRIED = (0, 1, 255, 256, 257, 0, 120001, 65536, 65537, 131071, 3, 0)
SIXTEEN_MERGED = tuple(129000 + 137 * k for k in range(16))
SIXTEEN_PER_SLOT = tuple(20000 + 3 * k for k in range(16))
LIST_FORMS_LENGTHS = (23011, 24500, 22789)
EDGE_LENGTHS = (3000, 3000, 3000)


def nblocks(lengths):
    return sum((int(n) + 255) // 256 for n in lengths)


def deployment_lengths(seed):
    """five lengths drawn once from 110 000 .. 130 000"""
    return tuple(int(x) for x in np.random.default_rng(seed).integers(110000, 130001, 5))


# ---- generators -----------------------------------------------------------------------------------------------------------
def drive_poses(n, yaw0=0.3):
    """A smooth drive: rotation about z, 1.1 m per scan on a curve that starts some hundred metres from the origin (pose 0
    at height 0, a gentle slope after it) -- true float64 entries, structural zeros where a rotation about z has them."""
    out, p = [], np.array([-215.3, 120.7, 0.0])
    for k in range(n):
        yaw = yaw0 + 0.01 * k + 0.00005 * k * k
        c, s = np.cos(yaw), np.sin(yaw)
        M = np.eye(4)
        M[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
        M[:3, 3] = p
        out.append(M)
        p = p + np.array([1.1 * c, 1.1 * s, 0.02])
    return np.stack(out)


def make_scan(rng, n, classes=None):
    """(xyzr [n,4] f32, label [n] u32): a 3 / -25 degree sensor over a ground plane at z = -1.73 with things standing on
    it; labels (instance << 16) | class with instance >= 1, classes from CLASSES (or from ``classes`` alone)"""
    yaw = rng.uniform(-np.pi, np.pi, n)
    pitch = np.radians(rng.uniform(-25.0, 3.0, n))
    r = np.minimum(1.73 / np.maximum(np.sin(-pitch), 1e-3), rng.uniform(8.0, 60.0, n)) * (1.0 + rng.normal(0, 0.001, n))
    xyzr = np.empty((n, 4), np.float32)
    xyzr[:, 0] = r * np.cos(pitch) * np.cos(yaw)
    xyzr[:, 1] = r * np.cos(pitch) * np.sin(yaw)
    xyzr[:, 2] = r * np.sin(pitch)
    xyzr[:, 3] = rng.integers(0, 100, n) / 100
    if classes is None:
        cl = rng.choice(CLASSES, n, p=WEIGHTS)
    else:
        cl = rng.choice(np.asarray(classes, dtype=np.uint32), n)
    label = (rng.integers(1, 500, n).astype(np.uint32) << 16) | cl.astype(np.uint32)
    return xyzr, label


def make_input(lengths, seed, ignore=IGNORE, moving=MOVING, only=None, upper=0):
    """One call's worth: ``raw`` [(xyzr, label)] per slot, ``poses`` [n,4,4], ``back`` = inv(poses[0]), the lists.
    ``only``: {slot: classes} -- that slot's labels come from these classes alone; ``upper``: this many points of every
    slot get each label of UPPER_ONLY."""
    rng = np.random.default_rng(seed)
    raw = []
    for s, n in enumerate(lengths):
        xyzr, label = make_scan(rng, int(n), (only or {}).get(s))
        if upper:
            at = rng.choice(int(n), 2 * upper, replace=False)
            label[at[:upper]], label[at[upper:]] = UPPER_ONLY[0], UPPER_ONLY[1]
        raw.append((xyzr, label))
    poses = drive_poses(len(lengths))
    return dict(raw=raw, poses=poses, back=np.linalg.inv(poses[0]), ignore=list(ignore), moving=list(moving), n_nan_rows=0)


def deployment_input(seed, **kw):
    return make_input(deployment_lengths(seed), seed, **kw)


# float32 bit patterns planted by edge_input: coordinates ...
EDGE_COORDS = dict(sub_min=0x00000001, sub_min_neg=0x80000001, sub_max=0x007FFFFF, neg_zero=0x80000000,
                   big=int(np.array(3.4e38, np.float32).view(np.uint32)),
                   big_neg=int(np.array(-3.4e38, np.float32).view(np.uint32)), inf=0x7F800000, inf_neg=0xFF800000,
                   nan=0x7FC00000)
# ... and remissions: quiet and signalling NaNs with payloads, both signs; subnormals
EDGE_REMS = [0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFFFFFFF, 0x00000001, 0x807FFFFF]
EDGE_KEPT, EDGE_DROPPED = 40, (0, 252)   # class 252 is dropped in the secondary slots only


def edge_input(seed, scaled=False):
    """3 slots of 3 000 points.  Row 100 + 11 j of every slot carries the j-th planted coordinate: every value of
    EDGE_COORDS in column x, y or z, three times under a kept class and three times under a dropped one; row 2000 + 5 j the
    j-th planted remission.  ``planted``: {name: [(slot, row, column)]}.  ``scaled``: the 3 x 4 parts of the poses and of
    ``back`` times 1e-160 -- the products of the second transform are subnormal in float64."""
    inp = make_input(EDGE_LENGTHS, seed)
    planted = {k: [] for k in EDGE_COORDS}
    planted["rem"] = []
    for s, (xyzr, label) in enumerate(inp["raw"]):
        bits = xyzr.view(np.uint32)
        j = 0
        for name, pattern in EDGE_COORDS.items():
            for col in range(3):
                for rep in range(6):
                    row = 100 + 11 * j
                    bits[row, col] = pattern
                    cl = EDGE_KEPT if rep % 2 == 0 else EDGE_DROPPED[(rep // 2 + col) % 2]
                    label[row] = ((1 + j) << 16) | cl
                    planted[name].append((s, row, col))
                    j += 1
        for j in range(4 * len(EDGE_REMS)):
            row = 2000 + 5 * j
            bits[row, 3] = EDGE_REMS[j % len(EDGE_REMS)]
            label[row] = ((1 + j) << 16) | (EDGE_KEPT if (j // len(EDGE_REMS)) % 2 == 0 else EDGE_DROPPED[j % 2])
            planted["rem"].append((s, row, 3))
    if scaled:
        inp["poses"] = inp["poses"].copy()
        inp["poses"][:, :3, :] *= 1e-160
        inp["back"] = inp["back"].copy()
        inp["back"][:3, :] *= 1e-160
    inp["planted"] = planted
    inp["n_nan_rows"] = len(kept_nonfinite_rows(inp))
    return inp


def kept_nonfinite_rows(inp):
    """(slot, row) of the planted rows with an infinite or NaN coordinate that rule 2 keeps.  Every pose here is a rotation
    about z: each column of its 3 x 3 part holds a zero, 0 * inf is NaN, so such a row is NaN in ALL THREE coordinates after
    the two transforms -- the restated cloud holds exactly 3 NaN cells per row of this list."""
    out = set()
    for name in ("inf", "inf_neg", "nan"):
        for s, row, _ in inp["planted"][name]:
            cl = int(inp["raw"][s][1][row]) & 0xFFFF
            if cl not in set(inp["ignore"]) and (s == 0 or cl not in set(inp["moving"])):
                out.add((s, row))
    return sorted(out)


def input_sha(inp):
    h = hashlib.sha256()
    for xyzr, label in inp["raw"]:
        h.update(xyzr.tobytes())
        h.update(label.tobytes())
    h.update(inp["poses"].tobytes())
    h.update(inp["back"].tobytes())
    return h.hexdigest()


def restate_clouds(inp, merged):
    """(the restated clouds, kept count per slot) of an input whose slots are its scans in order"""
    slots = list(range(len(inp["raw"])))
    with np.errstate(all="ignore"):
        per = cpu.restate(inp["raw"], inp["poses"], slots, inp["back"], inp["ignore"], inp["moving"], False)
    kept = [len(c[0]) for c in per]
    if merged:
        per = [tuple(np.concatenate([c[j] for c in per]) for j in range(3))]
    return per, kept


# ---- tests ----------------------------------------------------------------------------------------------------------------
def _has(a, pattern):
    return bool((np.ascontiguousarray(a).view(np.uint32) == np.uint32(pattern)).any())


def _all_inputs():
    yield "deployment", deployment_input(17)
    yield "deployment_b", deployment_input(18)
    yield "edges", edge_input(5)
    yield "edges_scaled", edge_input(5, scaled=True)
    yield "lists", make_input(LIST_FORMS_LENGTHS, 23, upper=120)
    yield "sixteen", make_input(SIXTEEN_PER_SLOT, 29, IGNORE_LONG, MOVING_LONG)
    for k, lengths in enumerate(SLOT_SHAPES):
        yield f"shape{k}", make_input(lengths, 100 + k)


def test_generators_are_deterministic_and_free_of_the_sentinels():
    assert len(CLASSES) == 30 == len(set(CLASSES.tolist())) and all(c in CLASSES for c in (0, 1, 252, 253, 65535))
    assert abs(WEIGHTS.sum() - 1.0) < 1e-12
    assert len(IGNORE_LONG) > 16 and len(MOVING_LONG) > 16
    for name, inp in _all_inputs():
        for xyzr, label in inp["raw"]:
            assert xyzr.dtype == np.float32 and label.dtype == np.uint32 and xyzr.shape == (len(label), 4), name
            assert not _has(xyzr, SENT_F32) and not _has(label, SENT_U32), name
            if len(label):
                assert int((label >> 16).min()) >= 1, name
        assert not (inp["poses"].view(np.int64) == SENT_F64).any() and np.isfinite(inp["poses"]).all(), name
        for merged in (True, False):                      # nor does the expected output hold one
            for p, r, l in restate_clouds(inp, merged)[0]:
                assert not (np.ascontiguousarray(p).view(np.int64) == SENT_F64).any(), name
                assert not _has(r, SENT_F32) and (l <= 0xFFFF).all(), name
    for make in (lambda: deployment_input(17), lambda: edge_input(5), lambda: edge_input(5, scaled=True),
                 lambda: make_input(LIST_FORMS_LENGTHS, 23, upper=120)):
        assert input_sha(make()) == input_sha(make())
    assert input_sha(deployment_input(17)) != input_sha(deployment_input(18))


def test_deployment_input_is_what_the_gpu_tests_assume():
    for seed in (17, 18):
        inp = deployment_input(seed)
        lengths = [len(l) for _, l in inp["raw"]]
        assert len(lengths) == 5 and all(110000 <= n <= 130000 and n % 256 != 0 for n in lengths), lengths
        assert nblocks(lengths) > 2048                                     # the prefix loop makes at least 8 trips
        assert (inp["poses"] != inp["poses"].astype(np.float32)).any()     # true float64 poses
        assert all((M[:3, :3] != M[:3, :3].astype(np.float32)).any() for M in inp["poses"])
        assert 100.0 < np.abs(inp["poses"][:, :3, 3]).max() < 1000.0       # some hundred metres
        assert np.allclose(inp["back"] @ inp["poses"][0], np.eye(4), rtol=0, atol=1e-9)
        clouds, kept = restate_clouds(inp, False)
        for s, (n, k) in enumerate(zip(lengths, kept)):
            assert 0.5 < k / n < 0.95, (s, k, n)
        assert np.isin(clouds[0][2], MOVING).sum() > 1000 and not any(np.isin(c[2], MOVING).any() for c in clouds[1:])
        present = set(np.concatenate([l & 0xFFFF for _, l in inp["raw"]]).tolist())
        assert present == set(CLASSES.tolist())
    assert nblocks(SIXTEEN_MERGED) > 8000 and all(n % 256 for n in SIXTEEN_MERGED + SIXTEEN_PER_SLOT)
    assert len(SIXTEEN_MERGED) == len(SIXTEEN_PER_SLOT) == 16
    assert sum(LIST_FORMS_LENGTHS) > 70000
    inp = make_input(LIST_FORMS_LENGTHS, 23, upper=120)
    for lab in UPPER_ONLY:
        assert sum(int((l == lab).sum()) for _, l in inp["raw"]) >= 100
        assert (lab & 0xFFFF) not in CLASSES and (lab >> 16) in CLASSES
    assert nblocks((65536,)) == 256 and N % 256 != 0


def test_edge_input_holds_the_planted_rows():
    for scaled in (False, True):
        inp = edge_input(5, scaled)
        pl = inp["planted"]
        f = lambda name: np.array([inp["raw"][s][0][row, col] for s, row, col in pl[name]])   # noqa: E731
        tiny = float(np.float32(1e-45))
        assert (f("sub_min") == tiny).all() and (f("sub_min_neg") == -tiny).all() and tiny == 2.0 ** -149
        assert (f("sub_max") == np.float32(1.1754942e-38)).all() and float(f("sub_max")[0]) < 2.0 ** -126
        assert (f("neg_zero") == 0).all() and np.signbit(f("neg_zero")).all()
        assert (f("big") == np.float32(3.4e38)).all() and (f("big_neg") == np.float32(-3.4e38)).all()
        assert np.isposinf(f("inf")).all() and np.isneginf(f("inf_neg")).all() and np.isnan(f("nan")).all()
        drop0, drop_sec = set(inp["ignore"]), set(inp["ignore"]) | set(inp["moving"])
        for name in ("inf", "inf_neg", "nan", "rem"):                      # at least 20 kept and 20 dropped of each
            dropped = [(int(inp["raw"][s][1][row]) & 0xFFFF) in (drop0 if s == 0 else drop_sec) for s, row, _ in pl[name]]
            assert sum(dropped) >= 20 and len(dropped) - sum(dropped) >= 20, (name, sum(dropped), len(dropped))
        assert len({(s, row) for v in pl.values() for s, row, _ in v}) == sum(len(v) for v in pl.values())   # one each
        rems = np.array([inp["raw"][s][0].view(np.uint32)[row, 3] for s, row, _ in pl["rem"]])
        assert set(rems.tolist()) == set(EDGE_REMS) and np.isnan(rems.view(np.float32)).sum() == 4 * len(rems) // 6
        # every non-finite row that is kept is NaN in all three coordinates, and nothing else is
        clouds, kept = restate_clouds(inp, True)
        p, r, l = clouds[0]
        assert inp["n_nan_rows"] == len(kept_nonfinite_rows(inp)) >= 60
        assert int(np.isnan(p).sum()) == 3 * inp["n_nan_rows"] and int(np.isnan(p).any(1).sum()) == inp["n_nan_rows"]
        assert not np.isinf(p[~np.isnan(p).any(1)]).any()
        first = np.cumsum([0] + kept)
        raw_nan = np.concatenate([first[s] + np.flatnonzero(np.isnan(c[0]).any(1)) for s, c in enumerate(restate_clouds(inp, False)[0])])
        assert np.array_equal(raw_nan, np.flatnonzero(np.isnan(p).any(1)))
        # the planted remissions arrive bit for bit
        kept_rems = [int(inp["raw"][s][0].view(np.uint32)[row, 3]) for s, row, _ in pl["rem"]
                     if (int(inp["raw"][s][1][row]) & 0xFFFF) not in (drop0 if s == 0 else drop_sec)]
        got = r.view(np.uint32)
        assert all(int((got == v).sum()) == kept_rems.count(v) for v in EDGE_REMS)
        if scaled:
            sub = (p != 0) & (np.abs(p) < 2.0 ** -1022)
            assert int(sub.sum()) >= 100, int(sub.sum())


def _python_keep(label, drop):
    return np.array([(v & 0xFFFF) not in drop for v in label.tolist()], dtype=bool).reshape(-1)


@pytest.mark.parametrize("which", ["deployment", "edges", "edges_scaled"])
def test_restatement_equals_an_independent_evaluation(which):
    """kept set and order from a per-point Python `set` lookup; remissions and labels exactly; on a 5 000-point subsample
    the points against `plain_transform` in np.longdouble (64-bit mantissa, wider exponent) within transform_bound -- finite
    rows only.  With the poses scaled by 1e-160 the second transform's four products underflow in float64: each may be off
    by half a unit of the subnormal grid (2^-1075), the sums of such numbers are exact; 4 * 2^-1074 covers them twice."""
    inp = dict(deployment=lambda: deployment_input(17), edges=lambda: edge_input(5),
               edges_scaled=lambda: edge_input(5, scaled=True))[which]()
    slots = list(range(len(inp["raw"])))
    with np.errstate(all="ignore"):
        clouds, qs, hs = cpu.restate(inp["raw"], inp["poses"], slots, inp["back"], inp["ignore"], inp["moving"], True, world=True)
    p, r, l = clouds[0]
    ign, mov = set(inp["ignore"]), set(inp["moving"])
    keeps = [_python_keep(label, ign if s == 0 else ign | mov) for s, (_, label) in enumerate(inp["raw"])]
    assert len(p) == sum(int(k.sum()) for k in keeps)
    src_slot = np.concatenate([np.full(int(k.sum()), s) for s, k in enumerate(keeps)])
    src_row = np.concatenate([np.flatnonzero(k) for k in keeps])
    xyzr = np.concatenate([x[k] for (x, _), k in zip(inp["raw"], keeps)])
    lab = np.concatenate([lb[k] for (_, lb), k in zip(inp["raw"], keeps)])
    assert np.array_equal(r.view(np.int32), xyzr[:, 3].view(np.int32)) and np.array_equal(l, lab & 0xFFFF)
    pick = np.sort(np.random.default_rng(1).choice(len(p), min(5000, len(p)), replace=False))
    if which != "deployment":     # every planted row that survived is in the sample
        planted = {(s, row) for v in inp["planted"].values() for s, row, _ in v}
        pick = np.union1d(pick, [k for k in range(len(p)) if (int(src_slot[k]), int(src_row[k])) in planted])
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63
    worst = 0.0
    h = xyzr[pick, :3]
    fin = np.isfinite(h).all(1)
    assert fin.sum() >= 4900 or which != "deployment"
    with np.errstate(all="ignore"):
        for s in slots:
            m = fin & (src_slot[pick] == s)
            if not m.any():
                continue
            rows = pick[m]
            q_ld = cpu.plain_transform(inp["poses"][s].astype(ld), h[m].astype(ld))
            want = cpu.plain_transform(inp["back"].astype(ld), q_ld)
            absA = np.broadcast_to(np.abs(inp["poses"][s]), (len(rows), 4, 4))
            bound = cpu.transform_bound(h[m].astype(np.float64), absA, qs[0][rows], inp["back"])
            if which == "edges_scaled":
                bound = bound + 4 * 2.0 ** -1074
            err = np.abs(p[rows].astype(ld) - want).astype(np.float64)
            assert np.isfinite(err).all() and (err <= bound).all(), (s, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
    print(f"{which}: worst |restate - longdouble| / bound = {worst:.3g} over {int(fin.sum())} rows")
    assert worst > 0.0        # (the comparison is not idle: float64 and the 64-bit mantissa do differ)


def test_documented_work_size_covers_every_table():
    """bitmap (2 * 2048 words) + one count per workgroup: LT_INGEST_WORK_INTS is what call_ingest allocates, no more"""
    from lidar_transfer_amd import _lib
    tables = list(SLOT_SHAPES) + [CPU_TRIED, SIXTEEN_MERGED, SIXTEEN_PER_SLOT, LIST_FORMS_LENGTHS, EDGE_LENGTHS,
                                  deployment_lengths(17), deployment_lengths(18), (N, N, N)]
    for lengths in tables:
        assert _lib.ingest_work_ints(sum(lengths), len(lengths)) >= 4096 + nblocks(lengths), lengths
    for n_scans in range(1, 17):       # the worst case: every slot one point past a multiple of 256
        lengths = (257,) * n_scans
        assert _lib.ingest_work_ints(sum(lengths), n_scans) >= 4096 + nblocks(lengths)


def test_restatement_handles_the_slot_lengths_tried_on_the_cpu():
    inp = make_input(CPU_TRIED, 3)
    for merged in (True, False):
        clouds, kept = restate_clouds(inp, merged)
        assert [kept[s] for s, n in enumerate(CPU_TRIED) if n == 0] == [0, 0, 0]
        assert sum(len(c[0]) for c in clouds) == sum(kept) and len(clouds) == (1 if merged else len(CPU_TRIED))
