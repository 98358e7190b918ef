"""Every path of the TSDF pixel pass (pix_body, k_wd_keys, k_wd_finish, tsdf_rowtab, the quirk kernels and tsdf_pix_grid of
lidar_transfer_amd/csrc/lt_tsdf.hip) driven on purpose, on the small inputs of tests/tsdf_pix_cases.py -- what they reach
by geometry alone is proven without a GPU in tests/test_tsdf_pix_cases_cpu.py; which branch the kernel took is read here from
the path counters of its debug instantiation (LIDARHIP_DEBUG_TSDF=1, lt_debug_tsdf_pix_paths) and from its wedge table
(lt_debug_tsdf_wedge).

The counters do not steer control flow (they are `if constexpr (VCOUNT)` additions to registers and to a debug buffer the
kernel never reads): what the counted instantiation reports for an input is what the shipped VCOUNT = false kernel does on
that input.  The `counters` child's volumes are held to the same oracles as the `default` child's.

LIDARHIP_DEBUG_TSDF, LIDARHIP_PIX_WGS and LIDARHIP_TSDF_PIX are read once per process: one child process per setting, one
after the other, each runs every case through TSDFVolume.integrate (every observation prefix kept), resets, runs it again, and
-- where the case has two or more observations -- through TSDFVolume.integrate_multi (the fused pass), twice as well.
  default          the shipped kernels, one workgroup per item
  counters         LIDARHIP_DEBUG_TSDF=1: the counted instantiations
  one_wg           LIDARHIP_PIX_WGS=1: one workgroup takes every item in turn (the reuse of c_buf, a_lo / a_hi, p_*)
  three_wgs        LIDARHIP_PIX_WGS=3
  counters_one_wg  both: "the largest number of items one workgroup took" must be the number of items
The oracles live in the parent: oracle/lt_tsdf_dense.hip and, where it was built, the reference's own kernel text compiled for
gfx950.  All four fields, bit for bit, no tolerance anywhere.  A volume is carried as its voxels that differ from the initial
ones (index, four words) -- beyond_2p24 alone is compared on the device, in the child, by torch.equal on int32 views."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tsdf_pix_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
CHILDREN = {"default": {}, "counters": {"LIDARHIP_DEBUG_TSDF": "1"}, "one_wg": {"LIDARHIP_PIX_WGS": "1"},
            "three_wgs": {"LIDARHIP_PIX_WGS": "3"}, "counters_one_wg": {"LIDARHIP_DEBUG_TSDF": "1", "LIDARHIP_PIX_WGS": "1"}}
_REF_SKIP = "oracle/_ref/libref_tsdf_integrate.so not built (needs /root/reference + hipcc at build time)"
SMALL = [n for n in pc.NAMES if n not in pc.BIG]
INIT = np.array([0x3F800000, 0, 0, 0], np.int32)      # tsdf 1, weight 0, colour 0, remission 0


# ---- shared by the parent and the children ------------------------------------------------------------------------------

def _volume(name):
    from lidar_transfer_amd.fusion import TSDFVolume
    c = pc.case(name)
    vol = TSDFVolume(c["bnds"], c["voxel"], c["fov"][0], c["fov"][1], merge=True)
    assert tuple(int(x) for x in vol._vol_dim) == c["dims"]
    return vol


@functools.lru_cache(maxsize=None)
def _obs(name):
    return [tuple(np.array(a) for a in o) for o in pc.case(name)["obs"]]


def _records(vols):
    """[n, 4] int32 on the device: the four fields of every voxel, as bits."""
    import torch
    return torch.stack([v.reshape(-1) for v in vols], 1).contiguous().view(torch.int32)


def _sparse(rec):
    """(indices [m] int32, words [m, 4] int32) of the voxels that differ from the initial ones, as numpy arrays."""
    import torch
    init = torch.from_numpy(INIT).to(rec.device)
    idx = torch.nonzero((rec != init).any(1)).squeeze(1)
    return idx.to(torch.int32).cpu().numpy(), rec[idx].cpu().numpy()


def _oracle_records(name, which):
    """Generator: after each observation of the case, the [n, 4] int32 records of `which` = "dense" (oracle/lt_tsdf_dense.hip)
    or "ref" (the reference's kernel text, oracle/_ref) on the device."""
    import torch
    from oracle import binding as ob
    c = pc.case(name)
    dev = torch.device("cuda", 0)
    n = int(np.prod(c["dims"]))
    dims = (C.c_int * 3)(*c["dims"])
    org = (C.c_float * 3)(*[float(x) for x in c["origin"]])
    vp = C.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    # 64 spare floats behind each field: the reference kernel runs thread n (test_tsdf_ref_kernel_gpu.py)
    flat = [torch.ones(n + 64, device=dev)] + [torch.zeros(n + 64, device=dev) for _ in range(3)]
    vols = [t[:n] for t in flat]
    for label3, depth, rem in _obs(name):
        c3 = torch.from_numpy(label3).to(dev)
        folded = torch.floor(c3[:, :, 0] * 256 * 256 + c3[:, :, 1] * 256 + c3[:, :, 2]).contiguous()
        assert np.array_equal(folded.cpu().numpy(), pc.fold(label3))
        d, r = torch.from_numpy(depth).to(dev), torch.from_numpy(rem).to(dev)
        args = (dims, org, C.c_float(np.float32(c["voxel"])), C.c_float(np.float32(c["voxel"] * 5)), C.c_float(c["fov"][0]),
                C.c_float(c["fov"][1]), vp(folded.data_ptr()), vp(d.data_ptr()), vp(r.data_ptr()), c["H"], c["W"],
                C.c_float(1.0))
        if which == "ref":
            assert ob.ref_tsdf_lib(True).ref_tsdf_integrate(*[vp(t.data_ptr()) for t in vols], *args, st) == 0
        else:
            assert ob.dense_lib().lt_test_tsdf_integrate_dense(*[vp(t.data_ptr()) for t in vols], *args, 1, st) == 0
        torch.cuda.synchronize()
        yield _records(vols)


# ---- a child process: every case through the product, under one setting of the environment ----------------------------------

def _debug_calls():
    from lidar_transfer_amd import _lib
    lib = _lib.load()
    lib.lt_debug_tsdf_pix_paths.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    lib.lt_debug_tsdf_pix_paths.restype = C.c_int
    lib.lt_debug_tsdf_wedge.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    lib.lt_debug_tsdf_wedge.restype = C.c_int
    return lib


def _child_main(path):
    import torch
    sys.path.insert(0, os.path.dirname(HERE))
    lib = _debug_calls()
    counted = "LIDARHIP_DEBUG_TSDF" in os.environ
    out = {}

    def counters():
        buf = (C.c_ulonglong * pc.N_CNT)()
        assert lib.lt_debug_tsdf_pix_paths(buf, pc.N_CNT) == 0
        return np.array(list(buf), np.int64)

    for name in pc.NAMES:
        c, obs, big = pc.case(name), _obs(name), name in pc.BIG
        vol, other = _volume(name), _volume(name)
        init = torch.from_numpy(INIT).cuda()
        flags = {}
        oracles = {}
        if big:     # on the device, here: the oracles' records after every observation
            from oracle import binding as ob
            oracles["dense"] = list(_oracle_records(name, "dense"))
            if ob.ref_tsdf_available():
                oracles["ref"] = list(_oracle_records(name, "ref"))
        recs = []
        for rnd in range(2):
            if rnd:
                vol.reset()
                flags["reset_is_initial"] = bool((_records(vol.get_volume_tensors()) == init).all())
            for k, (l3, d, r) in enumerate(obs):
                vol.integrate(l3, d, r, np.eye(4))
                rec = _records(vol.get_volume_tensors())
                if rnd == 0:
                    recs.append(rec)
                    if counted:
                        out[f"{name}/cnt/{k}"] = counters()
                    if k == 0:
                        ws = (C.c_int * (c["W"] + 1))()
                        nq = C.c_int(-1)
                        assert lib.lt_debug_tsdf_wedge(vol._h, ws, c["W"] + 1, C.byref(nq)) == 0
                        out[f"{name}/wd_start"], out[f"{name}/n_quirk"] = np.array(list(ws), np.int64), np.int64(nq.value)
                    if big:
                        for which, o in oracles.items():
                            flags[f"equals_{which}/{k}"] = bool(torch.equal(o[k], rec))
                        out[f"{name}/n_written/{k}"] = np.int64(int((rec != init).any(1).sum()))
                    else:
                        out[f"{name}/idx/{k}"], out[f"{name}/val/{k}"] = _sparse(rec)
                else:
                    flags[f"second_round_equal/{k}"] = bool(torch.equal(recs[k], rec))
        for l3, d, r in obs:    # a second volume object of the case, after the first: the tables are per object
            other.integrate(l3, d, r, np.eye(4))
        flags["other_object_equal"] = bool(torch.equal(recs[-1], _records(other.get_volume_tensors())))
        if len(obs) >= 2:       # the fused pass
            for rnd in range(2):
                vol.reset()
                flags[f"reset_is_initial/multi{rnd}"] = bool((_records(vol.get_volume_tensors()) == init).all())
                vol.integrate_multi(obs)
                rec = _records(vol.get_volume_tensors())
                if rnd == 0:
                    first = rec
                    if counted:
                        out[f"{name}/cntm"] = counters()
                    flags["multi_equals_integrate"] = bool(torch.equal(recs[-1], rec))
                    if big:
                        flags["multi_equals_dense"] = bool(torch.equal(oracles["dense"][-1], rec))
                else:
                    flags["multi_second_round_equal"] = bool(torch.equal(first, rec))
        for key, val in flags.items():
            out[f"{name}/flag/{key}"] = np.bool_(val)
        vol.close()
        other.close()
        del recs, oracles
    np.savez(path, **out)


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """setting -> the child's results.  One child per setting, one after the other, each with a time limit of its own; after a
    child that a signal or the limit ended nothing more is started on the GPU: the session ends there."""
    root = tmp_path_factory.mktemp("tsdf_pix_paths")
    res = {}
    for mode, extra in CHILDREN.items():
        env = dict(os.environ)
        for k in ("LIDARHIP_TSDF_PIX", "LIDARHIP_TSDF_MULTI", "LIDARHIP_DEBUG_TSDF", "LIDARHIP_PIX_WGS"):
            env.pop(k, None)
        env.update(extra)
        path = str(root / f"{mode}.npz")
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True,
                               timeout=120)
        except subprocess.TimeoutExpired:
            pytest.exit(f"tsdf pixel-pass child '{mode}' did not end within its time limit: nothing more is run on the GPU", 1)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            pytest.exit(f"tsdf pixel-pass child '{mode}' ended with {r.returncode}: nothing more is run on the GPU\n"
                        + r.stderr[-2000:], 1)
        assert r.returncode == 0, f"child '{mode}':\n" + r.stderr[-2000:]
        res[mode] = dict(np.load(path))
    return res


# ---- the parent: oracles, comparisons ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracles(name):
    """(reference build's, dense restatement's): per observation prefix the sparse volume (indices, words); None where the
    reference build is absent."""
    from oracle import binding as ob
    D = [_sparse(rec) for rec in _oracle_records(name, "dense")]
    R = [_sparse(rec) for rec in _oracle_records(name, "ref")] if ob.ref_tsdf_available() else None
    return R, D


def _same(a, b, what):
    (ia, va), (ib, vb) = a, b
    if ia.shape == ib.shape and np.array_equal(ia, ib) and np.array_equal(va, vb):
        return
    sa, sb = {int(i): tuple(v) for i, v in zip(ia, va)}, {int(i): tuple(v) for i, v in zip(ib, vb)}
    bad = sorted(i for i in set(sa) | set(sb) if sa.get(i) != sb.get(i))
    assert not bad, f"{what}: {len(bad)} voxels differ (of {len(sa)} / {len(sb)} written), first at index {bad[0]}"


def _child_state(res, name, k):
    return res[f"{name}/idx/{k}"], res[f"{name}/val/{k}"]


def _cnt(res, name, k, word):
    return int(res[f"{name}/cnt/{k}"][pc.CNT[word]])


@pytest.mark.parametrize("name", SMALL)
def test_dense_restatement_equals_the_reference_kernel(name):
    from oracle import binding as ob
    if not ob.ref_tsdf_available():
        pytest.skip(_REF_SKIP)
    R, D = _oracles(name)
    for k in range(len(D)):
        _same(R[k], D[k], f"{name}, observation {k}: reference kernel source vs oracle/lt_tsdf_dense.hip")


@pytest.mark.parametrize("mode", list(CHILDREN))
@pytest.mark.parametrize("name", SMALL)
def test_integrate_equals_the_oracles(children, name, mode):
    """Every observation prefix against the dense restatement and the reference build; the second round after a reset, a
    second volume object and the fused pass against the first round's last prefix -- which equals the restatement here --
    (compared on the device in the child: its flags); after every reset all voxels are the initial ones, as bits (a column
    written but never stamped would survive: the direct marks and the LDS-merged ones each own that stamp)."""
    res = children[mode]
    R, D = _oracles(name)
    assert D[-1][0].size > 1000, "the oracle's volume is idle"
    for k in range(len(D)):
        _same(D[k], _child_state(res, name, k), f"{name}, observation {k}: oracle/lt_tsdf_dense.hip vs integrate ({mode})")
        if R is not None:
            _same(R[k], _child_state(res, name, k), f"{name}, observation {k}: reference kernel vs integrate ({mode})")
    flags = {k.split("/flag/")[1]: bool(v) for k, v in res.items() if k.startswith(f"{name}/flag/")}
    assert len(flags) >= 2 + len(D) and all(flags.values()), f"{name} ({mode}): {[k for k, v in flags.items() if not v]}"
    assert ("multi_equals_integrate" in flags) == (len(D) >= 2)


@pytest.mark.parametrize("mode", list(CHILDREN))
def test_beyond_2p24_equals_the_oracles_on_the_device(children, mode):
    """17.4 M voxels: compared by torch.equal on int32 views in the child; here its verdicts."""
    from oracle import binding as ob
    res, name = children[mode], "beyond_2p24"
    flags = {k.split("/flag/")[1]: bool(v) for k, v in res.items() if k.startswith(f"{name}/flag/")}
    n_obs = len(pc.case(name)["obs"])
    for k in range(n_obs):
        assert f"equals_dense/{k}" in flags and int(res[f"{name}/n_written/{k}"]) > 100000
        assert (f"equals_ref/{k}" in flags) == ob.ref_tsdf_available()
    assert "multi_equals_dense" in flags and "reset_is_initial" in flags and "other_object_equal" in flags
    assert all(flags.values()), f"{name} ({mode}): {[k for k, v in flags.items() if not v]}"


@pytest.mark.parametrize("mode", ["counters", "one_wg", "three_wgs", "counters_one_wg"])
def test_every_setting_equals_the_default(children, mode):
    """(Each is held to the oracles above as well; this names the pair.)"""
    for name in SMALL:
        for k in range(len(pc.case(name)["obs"])):
            _same(_child_state(children["default"], name, k), _child_state(children[mode], name, k),
                  f"{name}, observation {k}: default vs {mode}")
    for k in range(len(pc.case("beyond_2p24")["obs"])):
        assert int(children[mode][f"beyond_2p24/n_written/{k}"]) == int(children["default"][f"beyond_2p24/n_written/{k}"])


@pytest.mark.parametrize("name", pc.NAMES)
def test_wedge_table(children, name):
    """wd_n_quirk is the float32 count of the cases module, exactly; wd_start is non-decreasing from 0 to the number of table
    columns (with the quirk columns as the tail of the last wedge where the width is a power of two: k_wd_finish's bins), every
    wedge within its float64 bounds."""
    c, t = pc.case(name), pc.columns(name)
    n_cols, nq, W = c["dims"][0] * c["dims"][1], int(t["quirk"].sum()), c["W"]
    for mode in ("default", "counters"):
        ws, got_nq = children[mode][f"{name}/wd_start"], int(children[mode][f"{name}/n_quirk"])
        assert got_nq == nq, f"{name}: {got_nq} quirk columns, {nq} expected"
        assert ws.shape == (W + 1,) and ws[0] == 0 and (np.diff(ws) >= 0).all()
        assert ws[W] == (n_cols if pc.quirk_tail_in_last_wedge(W) else n_cols - nq)
        lo, hi = pc.wedge_bounds(name)
        size = np.diff(ws)
        assert ((size >= lo) & (size <= hi)).all(), f"{name}: wedge sizes {size} outside [{lo}, {hi}]"
    if name == "outside":
        assert ws[1] == 0 and ws[W - 1] == ws[W], "empty wedges at both ends"


@pytest.mark.parametrize("name", pc.NAMES)
def test_counters_show_the_intended_paths(children, name):
    res, c = children["counters"], pc.case(name)
    n_items, n_obs = -(-c["H"] * c["W"] // 64), len(c["obs"])
    total = {w: sum(_cnt(res, name, k, w) for k in range(n_obs)) for w in pc.CNT}
    print(name, {w: [_cnt(res, name, k, w) for k in range(n_obs)] for w in pc.CNT})
    if n_obs >= 2:
        print(name, "fused", {w: int(res[f"{name}/cntm"][i]) for w, i in pc.CNT.items()})
    keys = [("cnt", k) for k in range(n_obs)] + ([("cntm", None)] if n_obs >= 2 else [])
    for kind, k in keys:
        v = res[f"{name}/cnt/{k}"] if kind == "cnt" else res[f"{name}/cntm"]
        g = lambda w: int(v[pc.CNT[w]])     # noqa: E731
        assert g("items") == n_items
        assert g("staged") + g("unstaged") == n_items and g("t0") + g("agg") + g("direct") == n_items
        assert g("chunks_1") + g("chunks_n") == n_items - g("t0")
        assert g("max_items") == 1, "one workgroup per item by default"
        assert g("rounds") >= g("chunks") - g("v0") and g("sign_pos") + g("sign_neg") + g("sign_both") <= g("pairs")
        if c["expect"] == "staged":
            assert g("unstaged") == 0
        else:
            assert g("staged") == 0 and g("unstaged") == n_items
        clips = sum(g(w) for w in ("clip_all", "clip_lo", "clip_hi", "clip_hole", "clip_disj"))
        if kind == "cntm" or k == 0:
            assert clips == 0 and g("hole_skip") == 0, "no snapshot on a fresh volume"
        else:
            assert clips <= g("pairs") - g("empty"), "only a pair with an interval takes one of the five outcomes"
            assert clips >= g("chunks") - g("v0"), "a chunk with a voxel has a pair with an interval"
        assert g("clip_clean") <= g("clip_disj")
    one = children["counters_one_wg"]
    for k in range(n_obs):
        assert int(one[f"{name}/cnt/{k}"][pc.CNT["max_items"]]) == n_items, "LIDARHIP_PIX_WGS=1: one workgroup takes every item"
        for w in ("items", "staged", "unstaged", "agg", "direct", "t0", "pairs", "cand", "written", "empty", "clip_hole"):
            assert int(one[f"{name}/cnt/{k}"][pc.CNT[w]]) == _cnt(res, name, k, w), f"{w}: one workgroup vs one per item"
    if name == "staged_agg":
        assert total["direct"] == 0 and total["chunks_n"] > 0 and total["chunks_1"] > 0 and total["t0"] >= n_obs
        assert total["rounds_n"] > 0, "no chunk of several voxel rounds (V > 256)"
        assert _cnt(res, name, 2, "clip_all") > 0, "the repeated observation"
    if name == "unstaged_direct":
        assert total["unstaged"] == n_items * n_obs and all(_cnt(res, name, k, "direct") > 0 for k in range(n_obs))
        assert int(res[f"{name}/cntm"][pc.CNT["direct"]]) > 0
        # every item marks directly, and some pair holds two voxels or more: `z .. zend` is not `z .. z` here
        assert _cnt(res, name, 0, "direct") == n_items
        assert _cnt(res, name, 0, "cand") > 1.2 * (_cnt(res, name, 0, "pairs") - _cnt(res, name, 0, "empty"))
    if name == "two_wedges":
        assert all(_cnt(res, name, k, "two_cols") == n_items for k in range(n_obs))
    if name == "straddle_partial":
        assert n_items == 6 and all(_cnt(res, name, k, "two_cols") >= 5 for k in range(n_obs))
    if name == "holes":
        for w in ("clip_all", "clip_lo", "clip_hi", "clip_hole", "clip_disj"):
            assert total[w] >= 16, f"{w}: {total[w]} pairs"
        assert _cnt(res, name, 3, "clip_all") >= 16 and _cnt(res, name, 4, "clip_hole") >= 16
        assert _cnt(res, name, 4, "hole_skip") > 0
    if name == "outside":
        assert all(_cnt(res, name, k, "t0") >= 8 for k in range(n_obs))
        # the third observation: pairs, and not one voxel -- the case with pairs of an empty interval
        assert _cnt(res, name, 2, "pairs") > 0 and _cnt(res, name, 2, "empty") == _cnt(res, name, 2, "pairs")
        assert _cnt(res, name, 2, "v0") > 0 and _cnt(res, name, 2, "cand") == 0
    if name == "rows_level":
        assert min(total["sign_pos"], total["sign_neg"], total["sign_both"]) > 0
    if name == "rows_below":
        assert total["sign_pos"] == 0 and total["sign_both"] == 0 and total["sign_neg"] > 0
    if name == "rows_clamp":
        assert total["sign_both"] > 0 and total["sign_neg"] > 0
    if name.startswith("degenerate"):
        assert n_items == 1


@pytest.mark.parametrize("name", ["staged_agg", "holes", "axis_on"])
def test_mesh_from_the_kept_sign_bits(name):
    """extract_mesh reads the sign bits the pixel pass kept per voxel; marching cubes over contiguous copies of the oracle's
    tsdf / colour / remission reads the values: vertices, faces, colours, remissions element for element."""
    import torch
    from lidar_transfer_amd.fusion import DeviceMesh
    c = pc.case(name)
    vol = _volume(name)
    for l3, d, r in _obs(name):
        vol.integrate(l3, d, r, np.eye(4))
    got = [t.cpu().numpy() for t in vol.extract_mesh().renumber().tensors()]
    from oracle import binding as ob
    rec = list(_oracle_records(name, "ref" if ob.ref_tsdf_available() else "dense"))[-1].view(torch.float32)
    fields = [rec[:, k].contiguous().view(c["dims"]) for k in (0, 2, 3)]
    mesh = DeviceMesh()
    want = [t.cpu().numpy() for t in mesh.extract(*fields, c["voxel"], c["origin"]).renumber().tensors()]
    assert want[1].shape[0] > 1000, "hardly a mesh"
    for what, a, b in zip(("verts", "faces", "colors", "rem"), got, want):
        assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), f"{name}: {what} differ"
    mesh.close()
    vol.close()


if __name__ == "__main__":
    _child_main(sys.argv[1])
