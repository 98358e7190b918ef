"""`lt_ingest_scans_dev` (csrc/lt_ingest.hip) at the size it ships at and at its edge shapes, against THE numpy restatement
of its five rules (tests/test_ingest_cpu.py::restate) -- bit for bit, on inputs generated from fixed seeds by
tests/test_ingest_shapes_cpu.py (which checks the generators and the restatement on them without a GPU).

Every call goes through `call_ingest`, which owns the buffers: outputs with sentinel-filled guards on both sides and a
sentinel in every cell, so that "every cell of [0, capacity) written exactly as stated, nothing outside it" is asserted and
not assumed; `work` of exactly the documented size with a guard behind it; `n_kept` with spare sentinel ints."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_ingest_shapes_cpu as gen  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 1024
SENT_I32 = gen.SENT_U32 - (1 << 32)   # the label / n_kept / work sentinel as torch.int32 holds it


def call_ingest(raw, poses, back, ignore, moving, merged, stream=None, defer=False):
    """One `lt_ingest_scans_dev` call the way ScanIngest.prepare makes it, on buffers of its own.  Returns host copies:
    ``rc``; ``clouds`` [{points int64 [cap,3], rem int32 [cap], label uint32 [cap], guards [(below, above)] * 3}] -- one with
    ``merged``, one per slot otherwise; ``n_kept`` int32 [n_scans + 9]; ``work_guard``.  ``defer``: queue everything on
    ``stream`` and return the function that synchronises once and makes the copies."""
    import torch
    from lidar_transfer_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    n_scans = len(raw)
    ns = [int(len(l)) for _, l in raw]
    total = sum(ns)
    caps = [total] if merged else ns
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    assert poses.shape == (n_scans, 4, 4)
    binv = None if back is None else np.ascontiguousarray(back, dtype=np.float64)
    ign = (C.c_int * max(len(ignore), 1))(*ignore)
    mov = (C.c_int * max(len(moving), 1))(*moving)
    dp = C.POINTER(C.c_double)
    with torch.cuda.stream(st), torch.cuda.device(dev):
        ins = []
        rs = (_lib.RawScan * n_scans)()
        for k, (xyzr, label) in enumerate(raw):
            x = torch.zeros((max(ns[k], 1), 4), dtype=torch.float32, device=dev)
            l = torch.zeros((max(ns[k], 1),), dtype=torch.int32, device=dev)
            if ns[k]:
                x.copy_(torch.from_numpy(np.array(xyzr, dtype=np.float32)))
                l.copy_(torch.from_numpy(np.array(label, dtype=np.uint32).view(np.int32)))
            ins.append((x, l))
            rs[k].xyzr, rs[k].label, rs[k].n = x.data_ptr(), l.data_ptr(), ns[k]
        outs = [(torch.full(((c + 2 * GUARD) * 3,), gen.SENT_F64, dtype=torch.int64, device=dev),
                 torch.full((c + 2 * GUARD,), gen.SENT_F32, dtype=torch.int32, device=dev),
                 torch.full((c + 2 * GUARD,), SENT_I32, dtype=torch.int32, device=dev)) for c in caps]
        io = (_lib.IngestOut * len(outs))()
        for k, (p, r, l) in enumerate(outs):
            io[k].points, io[k].rem, io[k].label = p.data_ptr() + 24 * GUARD, r.data_ptr() + 4 * GUARD, l.data_ptr() + 4 * GUARD
        n_kept = torch.full((n_scans + 1 + 8,), SENT_I32, dtype=torch.int32, device=dev)
        n_work = _lib.ingest_work_ints(total, n_scans)          # exactly the documented size ...
        work = torch.full((n_work + GUARD,), SENT_I32, dtype=torch.int32, device=dev)   # ... and a guard behind it
        rc = lib.lt_ingest_scans_dev(n_scans, rs, poses.ctypes.data_as(dp), binv.ctypes.data_as(dp) if binv is not None else None,
                                     ign, len(ignore), mov, len(moving), _lib.LT_INGEST_MERGED if merged else 0, io,
                                     C.c_void_p(n_kept.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(st.cuda_stream))

    def collect():
        st.synchronize()
        with torch.cuda.stream(st):
            clouds = []
            for (p, r, l), c in zip(outs, caps):
                hp, hr, hl = p.cpu().numpy().reshape(-1, 3), r.cpu().numpy(), l.cpu().numpy().view(np.uint32)
                clouds.append(dict(points=hp[GUARD:GUARD + c], rem=hr[GUARD:GUARD + c], label=hl[GUARD:GUARD + c],
                                   guards=[(hp[:GUARD], hp[GUARD + c:]), (hr[:GUARD], hr[GUARD + c:]), (hl[:GUARD], hl[GUARD + c:])]))
            res = dict(rc=rc, clouds=clouds, n_kept=n_kept.cpu().numpy(), work_guard=work[n_work:].cpu().numpy())
        del ins[:]
        return res
    return collect if defer else collect()


def run(inp, merged, **kw):
    return call_ingest(inp["raw"], inp["poses"], inp["back"], inp["ignore"], inp["moving"], merged, **kw)


def check(inp, merged, res, tag=""):
    """the four assertions every test makes of every cloud; returns the figures it compared"""
    tag = (tag, "merged" if merged else "per slot")
    want, kept = gen.restate_clouds(inp, merged)
    n = len(inp["raw"])
    assert res["rc"] == 0, tag
    # 1. the counts, in both modes; the ints behind them untouched
    nk = res["n_kept"]
    assert len(nk) == n + 9 and nk[:n].tolist() == kept and int(nk[n]) == sum(kept), (tag, nk[:n + 1].tolist(), kept)
    assert (nk[n + 1:].view(np.uint32) == gen.SENT_U32).all(), tag
    assert len(res["clouds"]) == len(want) == (1 if merged else n), tag
    n_nan = 0
    sentinels = (gen.SENT_F64, gen.SENT_F32, gen.SENT_U32)
    for j, (c, (p, r, l), k) in enumerate(zip(res["clouds"], want, [sum(kept)] if merged else kept)):
        at = tag + (j,)
        gp, gr, gl = c["points"], c["rem"], c["label"]
        assert len(p) == k <= len(gr) == len(gl) == len(gp), at
        # 2. the kept cells, bit for bit -- but where the restatement says NaN: NaN there too, bits not compared
        wp = np.ascontiguousarray(p).view(np.int64).reshape(-1, 3)
        nan = np.isnan(p).reshape(-1, 3)
        assert np.isnan(gp[:k].view(np.float64)[nan]).all(), at
        assert np.array_equal(gp[:k][~nan], wp[~nan]), (at, "points")
        n_nan += int(nan.sum())
        assert np.array_equal(gr[:k], np.ascontiguousarray(r).view(np.int32)), (at, "remissions")
        assert np.array_equal(gl[:k], l), (at, "labels")
        # 3. the tail: +0.0 / +0.0 / 0 as integers, and no cell of [0, cap) still holds the sentinel
        assert not gp[k:].any() and not gr[k:].any() and not gl[k:].any(), (at, "tail")
        assert not (gp == gen.SENT_F64).any() and not (gr == gen.SENT_F32).any() and not (gl == gen.SENT_U32).any(), at
        # 4. nothing outside [0, cap)
        for (below, above), sent in zip(c["guards"], sentinels):
            assert len(below) == len(above) == GUARD, at
            assert (below.view(np.uint64 if sent == gen.SENT_F64 else np.uint32) == sent).all(), (at, "guard below")
            assert (above.view(np.uint64 if sent == gen.SENT_F64 else np.uint32) == sent).all(), (at, "guard above")
    assert n_nan == 3 * inp["n_nan_rows"], (tag, n_nan, inp["n_nan_rows"])       # the NaN exception cannot grow
    assert len(res["work_guard"]) == GUARD and (res["work_guard"].view(np.uint32) == gen.SENT_U32).all(), (tag, "work guard")
    return dict(kept=kept, n_nan=n_nan, want=want)


def _bytes(res, n):
    return b"".join(c[k].tobytes() for c in res["clouds"] for k in ("points", "rem", "label")) + res["n_kept"][:n + 1].tobytes()


@pytest.mark.parametrize("merged", [True, False])
def test_deployment_size_merged_and_per_slot(merged):
    """5 slots of 110 000 .. 130 000 points, short lists: more than 2 048 workgroups, so every thread of the last ones
    makes 8 or more trips through the cross-workgroup prefix loop"""
    inp = gen.deployment_input(17)
    lengths = [len(l) for _, l in inp["raw"]]
    assert len(lengths) == 5 and all(110000 <= n <= 130000 and n % 256 != 0 for n in lengths), lengths
    assert gen.nblocks(lengths) > 2048
    assert inp["ignore"] == [0, 1] and inp["moving"] == [252, 253]
    assert (inp["poses"] != inp["poses"].astype(np.float32)).any()
    assert np.array_equal(inp["back"], np.linalg.inv(inp["poses"][0]))
    got = check(inp, merged, run(inp, merged), "deployment")
    for n, k in zip(lengths, got["kept"]):
        assert 0.5 < k / n < 0.95, (k, n)
    slot0 = got["want"][0][2][:got["kept"][0]]
    assert np.isin(slot0, inp["moving"]).sum() > 0
    print(f"deployment size, merged={merged}: lengths {lengths}, nblocks {gen.nblocks(lengths)}, kept {got['kept']} "
          f"(sum {sum(got['kept'])}), NaN cells compared {got['n_nan']}")


def test_sixteen_slots_long_lists():
    """LT_INGEST_MAX_SCANS slots, both lists as bitmaps: ~8 100 workgroups merged, then 16 x 20 000 per slot"""
    inp = gen.make_input(gen.SIXTEEN_MERGED, 31, gen.IGNORE_LONG, gen.MOVING_LONG)
    assert len(inp["raw"]) == 16 and len(inp["ignore"]) > 16 and len(inp["moving"]) > 16
    assert gen.nblocks(gen.SIXTEEN_MERGED) > 8000
    got = check(inp, True, run(inp, True), "16 merged")
    assert 0 < sum(got["kept"]) < sum(gen.SIXTEEN_MERGED)
    assert not np.isin(got["want"][0][2], [0, 1, 65535]).any() and np.isin(got["want"][0][2], [252, 253, 259]).any()
    inp = gen.make_input(gen.SIXTEEN_PER_SLOT, 29, gen.IGNORE_LONG, gen.MOVING_LONG)
    got = check(inp, False, run(inp, False), "16 per slot")
    assert all(0 < k < n for k, n in zip(got["kept"], gen.SIXTEEN_PER_SLOT))


N = gen.N
SHAPE_CASES = [(lengths, None, None) for lengths in gen.SLOT_SHAPES] + [
    ((1,), {0: [40]}, None), ((1,), {0: [0]}, None), ((1, 1, 1), {0: [0], 1: [252], 2: [40]}, None),
    ((1, 1, 1), {0: [252], 1: [40], 2: [1]}, None),
    ((N, N, N), {1: [0, 1]}, None),               # every label of the middle slot is ignored
    ((N, N, N), {2: [252, 253]}, None),           # every label of a secondary slot is a moving class
    ((N, N + 1, N + 2), None, ([], [])),          # empty lists: nothing is dropped, the tail is empty
]


@pytest.mark.parametrize("case", range(len(SHAPE_CASES)), ids=lambda k: "-".join(str(n) for n in SHAPE_CASES[k][0][:4]) + f"-c{k}")
def test_slot_shapes(case):
    lengths, only, lists = SHAPE_CASES[case]
    ignore, moving = lists if lists is not None else (gen.IGNORE, gen.MOVING)
    inp = gen.make_input(lengths, 100 + case, ignore, moving, only=only)
    for merged in (True, False):
        got = check(inp, merged, run(inp, merged), str(lengths))
        kept = got["kept"]
        assert [k for k, n in zip(kept, lengths) if n == 0] == [0] * lengths.count(0)
        if sum(lengths) == 0:       # an empty call: LT_OK, counts zero, nothing but sentinels (check: guards, rc)
            assert kept == [0] * len(lengths)
        if only == {1: [0, 1]}:
            assert kept[1] == 0 and kept[0] > 0 and kept[2] > 0
        if only == {2: [252, 253]}:
            assert kept[2] == 0 and kept[0] > 0 and kept[1] > 0
        if lists == ([], []):
            assert kept == list(lengths)
        if only == {0: [40]}:
            assert kept == [1]
        if only == {0: [0]}:
            assert kept == [0]
        if only == {0: [0], 1: [252], 2: [40]}:
            assert kept == [0, 0, 1]
        if only == {0: [252], 1: [40], 2: [1]}:
            assert kept == [1, 1, 0]     # a moving class stays in the primary slot
    if lengths == (65536, 65537, 65535):
        assert gen.nblocks(lengths[:1]) == 256   # slot 1 starts at the first workgroup whose threads take a second trip


IGN16 = [0, 1, 65535, 10, 11, 13, 15, 16, 18, 20, 30, 31, 32, 44, 48, 49]
MOV16 = [252, 253, 259, 50, 51, 52, 60, 70, 71, 72, 80, 81, 99, 40, 7000, 7001]
LIST_FORMS = {
    "0/0": ([], []),
    "16/16": (IGN16, MOV16),
    "17/0": (IGN16 + [2000], []),
    "0/17": ([], MOV16 + [7002]),
    "17/3": (IGN16 + [2000], [252, 253, 259]),
    "3/17": ([1, 10, 11], [0, 65535] + MOV16[:15]),          # class 0 and 65535 as MOVING classes
    "16/17": (IGN16, MOV16 + [7002]),
    # pairs and triples that denote the same sets, as lists and as bitmaps
    "16/0": (IGN16, []),
    "17dup/0": (IGN16 + [IGN16[3]], []),
    "0/16": ([], MOV16),
    "0/17dup": ([], MOV16 + [252]),
    "3/3": ([0, 1, 65535], [252, 253, 259]),
    "6dup/4dup": ([0, 1, 1, 0, 65535, 1], [253, 252, 259, 252]),
    "17dup/3": ([0, 1, 65535] + [1] * 14, [252, 253, 259]),
    "3/17dup": ([65535, 1, 0], [259] * 15 + [252, 253]),
}


def test_class_list_forms():
    """one 3-slot input of ~70 000 points under every way a class list can travel"""
    base = gen.make_input(gen.LIST_FORMS_LENGTHS, 23, upper=120)
    n_upper = [sum(int((l == lab).sum()) for _, l in base["raw"]) for lab in gen.UPPER_ONLY]
    assert min(n_upper) >= 100
    assert [len(v[0]) > 16 or len(v[1]) > 16 for v in LIST_FORMS.values()].count(True) >= 8
    results = {}
    for name, (ignore, moving) in LIST_FORMS.items():
        assert len(ignore) <= 17 and len(moving) <= 17
        inp = dict(base, ignore=list(ignore), moving=list(moving))
        for merged in (True, False):
            got = check(inp, merged, res := run(inp, merged), name)
            results[name, merged] = _bytes(res, 3)
            # rule 1: a listed class in the UPPER 16 bits drops nothing -- the planted labels all arrive, as 7 and 9
            labels = np.concatenate([c[2] for c in got["want"]])
            assert [int((labels == 7).sum()), int((labels == 9).sum())] == n_upper, name
            out = np.concatenate([c["label"][:k] for c, k in zip(res["clouds"], [sum(got["kept"])] if merged else got["kept"])])
            assert [int((out == 7).sum()), int((out == 9).sum())] == n_upper, name
        if name == "0/0":
            assert got["kept"] == list(gen.LIST_FORMS_LENGTHS)
        if name == "3/17":
            assert np.isin(got["want"][0][2], [0, 65535]).any() and not any(np.isin(c[2], [0, 65535]).any() for c in got["want"][1:])
    # forms that denote the same sets: byte-identical outputs, whichever way the lists travelled
    groups = {}
    for name, (ignore, moving) in LIST_FORMS.items():
        groups.setdefault((frozenset(ignore), frozenset(moving)), []).append(name)
    same = [g for g in groups.values() if len(g) > 1]
    assert len(same) >= 3 and sum(len(g) for g in same) == 8, same
    for g in same:
        kinds = {len(LIST_FORMS[name][0]) > 16 or len(LIST_FORMS[name][1]) > 16 for name in g}
        assert kinds == {True, False}, g          # at least one bitmap form and one argument form in every group
        for name in g[1:]:
            for merged in (True, False):
                assert results[name, merged] == results[g[0], merged], (g[0], name, merged)
    # a single scan is the primary one: `moving` is ignored, short or long.  (The kernels consult `moving` for slots other
    # than 0 only, so the entry point's `n_moving = 0` for one scan decides how the lists travel, never what comes out:
    # what is pinned here is the outcome, under either way.)
    one =dict(base, raw=base["raw"][:1], poses=base["poses"][:1])
    present = sorted(set((base["raw"][0][1] & 0xFFFF).tolist()))
    assert len(present) > 16 and 7 in present and 9 in present
    ref = None
    for moving in ([], [40, 252, 7], present):
        inp = dict(one, ignore=[0, 1], moving=list(moving))
        for merged in (True, False):
            got = check(inp, merged, res := run(inp, merged), f"one scan, {len(moving)} moving")
            assert got["kept"] == [int((~np.isin(base["raw"][0][1] & 0xFFFF, [0, 1])).sum())]
            ref = ref or _bytes(res, 1)
            assert _bytes(res, 1) == ref


@pytest.mark.parametrize("scaled", [False, True], ids=["drive", "scaled_1e-160"])
def test_float_edges(scaled):
    """float32 subnormals, -0.0, +-3.4e38, +-inf and NaN coordinates in kept and in dropped points; NaN (quiet and
    signalling, with payloads) and subnormal remissions; with ``scaled`` poses whose products are subnormal in float64"""
    inp = gen.edge_input(5, scaled)
    assert [len(l) for _, l in inp["raw"]] == [3000] * 3
    assert all(len(inp["planted"][k]) >= 40 for k in ("inf", "inf_neg", "nan")) and inp["n_nan_rows"] >= 60
    for merged in (True, False):
        res = run(inp, merged)
        got = check(inp, merged, res, "edges")
        assert got["n_nan"] == 3 * inp["n_nan_rows"] > 0
        want_p = np.concatenate([c[0] for c in got["want"]])
        out_r = np.concatenate([c["rem"][:k] for c, k in zip(res["clouds"], [sum(got["kept"])] if merged else got["kept"])])
        for pattern in gen.EDGE_REMS:            # every planted remission that is kept arrives with its bits
            n_in = sum(int(inp["raw"][s][0].view(np.uint32)[row, 3] == pattern) for s, row, _ in inp["planted"]["rem"]
                       if (int(inp["raw"][s][1][row]) & 0xFFFF) not in ([0, 1] if s == 0 else [0, 1, 252, 253]))
            assert n_in > 0 and int((out_r.view(np.uint32) == pattern).sum()) == n_in, hex(pattern)
        fin = want_p[np.isfinite(want_p)]
        if scaled:
            n_sub = int(((fin != 0) & (np.abs(fin) < 2.0 ** -1022)).sum())
            assert n_sub >= 100, n_sub
        else:
            assert np.abs(fin).max() > 1e38      # the +-3.4e38 rows stay finite in float64
        print(f"float edges, scaled={scaled}, merged={merged}: kept {got['kept']}, NaN cells compared {got['n_nan']}")


def test_two_calls_in_flight():
    """two deployment-size calls on two streams, each with its own outputs and `work`, both queued before either is
    waited for (include/lidarhip.h: `work` is the caller's, one per call in flight)"""
    import torch
    a, b = gen.deployment_input(17), gen.deployment_input(18)
    assert gen.input_sha(a) != gen.input_sha(b)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    assert s1.cuda_stream != s2.cuda_stream and 0 not in (s1.cuda_stream, s2.cuda_stream)
    wait_a = run(a, True, stream=s1, defer=True)
    wait_b = run(b, False, stream=s2, defer=True)
    res_a, res_b = wait_a(), wait_b()
    check(a, True, res_a, "in flight, stream 1")
    check(b, False, res_b, "in flight, stream 2")


def test_padded_equals_exact_at_deployment_size():
    """the public path at 5 x ~120 000 points: `cp` fed the capacity-length cloud (a tail of ~100 000 origin points) and
    the exact-length one gives byte-identical images and files"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest, SequenceSource
    inp = gen.deployment_input(17)
    sensor = (64, 2048, 3.0, -25.0)
    src = SequenceSource(scans=[x for x, _ in inp["raw"]], labels=[l for _, l in inp["raw"]], poses=inp["poses"])
    ing = ScanIngest(src, (5, inp["ignore"], inp["moving"]))
    idx = 2
    assert ing.scan_indices(idx) == [2, 0, 1, 3, 4]
    total = sum(len(l) for _, l in inp["raw"])
    res = []
    with DeviceDeform(sensor, sensor, None) as dd:
        for exact in (True, False):
            clouds = ing.prepare(idx, merged=True, exact=exact)
            n = clouds[0][0].shape[0]
            assert (n == total) != exact and total - n < 0.5 * total
            res.append((n, {k: v.cpu().numpy() for k, v in dd.cp(clouds).items() if k in ("index", "range", "rem", "label", "bin", "label_file")}))
            torch.cuda.synchronize()
    assert res[1][0] - res[0][0] > 50000          # the tail
    assert sorted(res[0][1]) == ["bin", "index", "label", "label_file", "range", "rem"]
    for k in res[0][1]:
        assert res[0][1][k].tobytes() == res[1][1][k].tobytes(), k
    assert int((res[0][1]["range"] > 0).sum()) > 50000
    assert res[0][1]["index"].max() < res[0][0]   # no pixel points into the tail
    src.close()
