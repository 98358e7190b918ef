"""Every path of the TSDF column walk (k_tsdf_colmax, k_tsdf_columns, k_tsdf_integrate_cols and k_tsdf_reset_cols of
lidar_transfer_amd/csrc/lt_tsdf.hip) driven on purpose, on the small inputs of tests/tsdf_walk_cases.py -- what they reach by
geometry alone is proven without a GPU in tests/test_tsdf_walk_cases_cpu.py; which branch the kernel took is read here from the
path counters of its debug instantiation (LIDARHIP_DEBUG_TSDF=1, lt_debug_tsdf_walk_paths) and from the tables of the walk
(lt_debug_tsdf_walk_table: colinfo, chunk_live, colz, colmax).

The counters do not steer control flow (`if constexpr (VCOUNT)` additions to a debug buffer the kernel never reads): what the
counted instantiation reports for an input is what the shipped VCOUNT = false kernel does on it, and the counted children's
volumes are held to the same oracles.

LIDARHIP_TSDF_PIX, LIDARHIP_TSDF_BLOCKS and LIDARHIP_DEBUG_TSDF are read once per process: one child process per setting, one
after the other.  Each runs every case through TSDFVolume.integrate (every observation prefix kept), resets, runs it again, and
runs it on a second volume object.
  walk                  LIDARHIP_TSDF_PIX=0: the column walk for every observation
  walk_counters         ... and LIDARHIP_DEBUG_TSDF=1: the counted instantiations
  walk_one_wg           LIDARHIP_TSDF_PIX=0, LIDARHIP_TSDF_BLOCKS=1: one workgroup takes every chunk in turn, the candidate queue
                        carries over from chunk to chunk
  walk_three_wgs        LIDARHIP_TSDF_BLOCKS=3
  walk_counters_one_wg  BLOCKS=1 and the counters: "the largest number of chunks one workgroup took" must be the number of chunks
  pix1                  LIDARHIP_TSDF_PIX=1: the pixel pass on the fresh volume, the walk afterwards -- on ranges and stamps the
                        pixel pass left with atomicMax
  default               nothing set: the walk for merge=False, touched volumes, the (80, -80) degree field of view and the wide
                        image; the pixel pass elsewhere (lt_debug_tsdf_wedge answers "no table" where it never ran)
(The children with LIDARHIP_TSDF_BLOCKS leave out big_ym2 -- one or three workgroups over 16.8 M live columns; how long that
takes has not been measured -- and are not parametrised for it.)
The oracles live in the parent: oracle/lt_tsdf_dense.hip with the case's merge flag and, where it was built, the reference's
own kernel text compiled for gfx950 (both variants).  All four fields, bit for bit, no tolerance anywhere.  A volume is carried
as its voxels that differ from the initial ones; the cases of tsdf_walk_cases.BIG are compared on the device, in the child."""
import ctypes as C
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tsdf_walk_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu
WALK = {"LIDARHIP_TSDF_PIX": "0"}
CHILDREN = {"walk": dict(WALK), "walk_counters": dict(WALK, LIDARHIP_DEBUG_TSDF="1"),
            "walk_one_wg": dict(WALK, LIDARHIP_TSDF_BLOCKS="1"), "walk_three_wgs": dict(WALK, LIDARHIP_TSDF_BLOCKS="3"),
            "walk_counters_one_wg": dict(WALK, LIDARHIP_TSDF_BLOCKS="1", LIDARHIP_DEBUG_TSDF="1"),
            "pix1": {"LIDARHIP_TSDF_PIX": "1"}, "default": {}}
ENV_KEYS = ("LIDARHIP_TSDF_PIX", "LIDARHIP_TSDF_MULTI", "LIDARHIP_DEBUG_TSDF", "LIDARHIP_PIX_WGS", "LIDARHIP_TSDF_BLOCKS")
SMALL = [n for n in wc.NAMES if n not in wc.BIG]
NO_BLOCKS = ("big_ym2",)
INIT = np.array([0x3F800000, 0, 0, 0], np.int32)      # tsdf 1, weight 0, colour 0, remission 0
TABLES = ("colinfo", "chunk_live", "colz", "colmax")


def _cases_of(mode):
    return [n for n in wc.NAMES if not ("LIDARHIP_TSDF_BLOCKS" in CHILDREN[mode] and n in NO_BLOCKS)]


# ---- shared by the parent and the children ------------------------------------------------------------------------------

def _volume(name):
    from lidar_transfer_amd.fusion import TSDFVolume
    c = wc.case(name)
    vol = TSDFVolume(c["bnds"], c["voxel"], c["fov"][0], c["fov"][1], merge=c["merge"])
    assert tuple(int(x) for x in vol._vol_dim) == c["dims"]
    return vol


@functools.lru_cache(maxsize=None)
def _obs(name):
    return [tuple(np.array(a) for a in o) for o in wc.case(name)["obs"]]


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


class _Oracle:
    """`which` = "dense" (oracle/lt_tsdf_dense.hip) or "ref" (the reference's kernel text, oracle/_ref) on the device, one
    observation at a time: four fields of n voxels."""

    def __init__(self, name, which):
        import torch
        self.c, self.which = wc.case(name), which
        n = int(np.prod(self.c["dims"]))
        dev = torch.device("cuda", 0)
        # 64 spare floats behind each field: the reference kernel runs thread n (test_tsdf_ref_kernel_gpu.py)
        self.flat = [torch.ones(n + 64, device=dev)] + [torch.zeros(n + 64, device=dev) for _ in range(3)]
        self.vols = [t[:n] for t in self.flat]

    def step(self, label3, depth, rem, weight=1.0):
        import torch
        from oracle import binding as ob
        c, dev, vp = self.c, self.vols[0].device, C.c_void_p
        c3 = torch.from_numpy(label3).to(dev)
        folded = torch.floor(c3[:, :, 0] * 256 * 256 + c3[:, :, 1] * 256 + c3[:, :, 2]).contiguous()
        d, r = torch.from_numpy(depth).to(dev), torch.from_numpy(rem).to(dev)
        args = ((C.c_int * 3)(*c["dims"]), (C.c_float * 3)(*[float(x) for x in c["origin"]]), C.c_float(np.float32(c["voxel"])),
                C.c_float(np.float32(c["voxel"] * 5)), C.c_float(c["fov"][0]), C.c_float(c["fov"][1]), vp(folded.data_ptr()),
                vp(d.data_ptr()), vp(r.data_ptr()), c["H"], c["W"], C.c_float(weight))
        st = vp(torch.cuda.current_stream().cuda_stream)
        ptrs = [vp(t.data_ptr()) for t in self.vols]
        if self.which == "ref":
            assert ob.ref_tsdf_lib(bool(c["merge"])).ref_tsdf_integrate(*ptrs, *args, st) == 0
        else:
            assert ob.dense_lib().lt_test_tsdf_integrate_dense(*ptrs, *args, 1 if c["merge"] else 0, st) == 0
        torch.cuda.synchronize()
        return self.vols


def _differ(a, b):
    """[n] bool on the device: the voxels in which four fields differ from four fields, as bits -- one field at a time (no
    packed copy of a big volume; the product's fields are strided views)."""
    import torch
    bad = None
    for x, y in zip(a, b):
        m = x.view(torch.int32).reshape(-1) != y.view(torch.int32).reshape(-1)
        bad = m if bad is None else bad | m
    return bad


def _fields_equal(a, b):
    return not bool(_differ(a, b).any())


def _fields_initial(a):
    import torch
    return all(bool((x.view(torch.int32) == int(w)).all()) for x, w in zip(a, INIT))


# ---- a child process: every case through the product, under one setting of the environment ----------------------------------

def _debug_calls():
    from lidar_transfer_amd import _lib
    lib = _lib.load()
    lib.lt_debug_tsdf_walk_paths.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    lib.lt_debug_tsdf_walk_paths.restype = C.c_int
    lib.lt_debug_tsdf_walk_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.lt_debug_tsdf_walk_table.restype = C.c_int
    lib.lt_debug_tsdf_wedge.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    lib.lt_debug_tsdf_wedge.restype = C.c_int
    return lib


def _tables(lib, vol, name):
    """{table: numpy array} of the volume's last walk, or None where it has not been walked."""
    c = wc.case(name)
    n_cols = c["dims"][0] * c["dims"][1]
    out = {}
    for what, (key, n, dt) in enumerate(zip(TABLES, (n_cols, (n_cols + 63) // 64, n_cols, c["W"]),
                                            (np.int32, np.int32, np.uint32, np.float32))):
        buf = np.zeros(n, dt)
        if lib.lt_debug_tsdf_walk_table(vol._h, what, buf.ctypes.data_as(C.c_void_p), n) != 0:
            return None
        out[key] = buf
    return out


def _mesh_check(vol, name):
    """(faces, equal): extract_mesh of the walked volume -- it reads the kept sign bits, stamps and ranges -- against marching
    cubes over contiguous copies of its downloaded fields."""
    import torch
    from lidar_transfer_amd.fusion import DeviceMesh
    c = wc.case(name)
    got = [t.clone() for t in vol.extract_mesh().renumber().tensors()]
    t, _, col, rem = vol.get_volume_tensors()
    mesh = DeviceMesh()
    want = mesh.extract(t.contiguous(), col.contiguous(), rem.contiguous(), c["voxel"], c["origin"]).renumber().tensors()
    same = all(a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want))
    n = int(got[1].shape[0])
    mesh.close()
    return n, same


def _child_main(path, mode):
    import torch
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import binding as ob
    lib = _debug_calls()
    counted = "LIDARHIP_DEBUG_TSDF" in os.environ
    keep_tables = mode in ("walk", "pix1", "default")
    out = {}

    def counters():
        buf = (C.c_ulonglong * wc.N_CNT)()
        return np.array(list(buf), np.int64) if lib.lt_debug_tsdf_walk_paths(buf, wc.N_CNT) == 0 else None

    for name in _cases_of(mode):
        t_case = time.perf_counter()
        c, obs, big = wc.case(name), _obs(name), name in wc.BIG
        weights = c["weights"]
        dz = c["dims"][2]
        vol = _volume(name)
        flags = {}
        cells = min(c["dims"]) >= 2     # (a volume one voxel thick has no cell for marching cubes: no mesh to compare)
        recs = []
        # a big case: the oracles run beside the product, observation by observation -- the dense restatement in the first
        # round, the reference build (where there is one) in the second: two copies of the volume at a time
        for rnd in range(2):
            oracle = None
            if big:
                which = "dense" if rnd == 0 else ("ref" if ob.ref_tsdf_available() else None)
                oracle = _Oracle(name, which) if which else None
            if rnd:
                vol.reset()
                flags["reset_is_initial"] = _fields_initial(vol.get_volume_tensors())
                if not big:
                    flags["reset_mesh_has_no_face"] = not cells or vol.extract_mesh().n_faces == 0
            if c["touch"]:
                vol.touch()
            for k, (l3, d, r) in enumerate(obs):
                # (soundness of the tables needs the oracle's volume before the observation: the third copy of a big volume)
                before = [t.clone() for t in oracle.vols] if oracle is not None and rnd == 0 else None
                vol.integrate(l3, d, r, np.eye(4), obs_weight=weights[k])
                if rnd == 0 and k == 0:
                    out[f"{name}/wedge_rc"] = np.int64(lib.lt_debug_tsdf_wedge(vol._h, None, 0, None))
                if rnd == 0 and counted:
                    cnt = counters()
                    if cnt is not None:
                        out[f"{name}/cnt/{k}"] = cnt
                tab = _tables(lib, vol, name) if rnd == 0 else None
                if rnd == 0:
                    out[f"{name}/walked/{k}"] = np.bool_(tab is not None)
                if big:
                    fields = vol.get_volume_tensors()
                    if rnd == 0:    # (the product's own count of voxels that are not the initial ones)
                        out[f"{name}/n_product/{k}"] = np.int64(int(((fields[1] != 0) | (fields[0] != 1) | (fields[2] != 0)).sum()))
                    if oracle is not None:
                        ovols = oracle.step(l3, d, r, weights[k])
                        bad = _differ(fields, ovols)
                        flags[f"equals_{oracle.which}/{k}"] = not bool(bad.any())
                        out[f"{name}/n_diff_{oracle.which}/{k}"] = np.int64(int(bad.sum()))
                        out[f"{name}/diff_idx_{oracle.which}/{k}"] = torch.nonzero(bad).squeeze(1)[:64].cpu().numpy()
                        if rnd == 0:
                            out[f"{name}/n_written/{k}"] = np.int64(int(((ovols[1] != 0) | (ovols[0] != 1) | (ovols[2] != 0)).sum()))
                        if before is not None and tab is not None:   # soundness of the tables, on the device
                            ch = torch.nonzero(_differ(before, ovols)).squeeze(1)
                            col, z = ch // dz, ch % dz
                            info = torch.from_numpy(tab["colinfo"]).cuda()[col]
                            cz = torch.from_numpy(tab["colz"].astype(np.int64)).cuda()[col]
                            live = torch.from_numpy(tab["chunk_live"]).cuda()[col >> 6]
                            flags[f"sound_colinfo/{k}"] = not bool((info == -1).any())
                            flags[f"sound_colz/{k}"] = bool(((z >= (cz & 0x7FFF)) & (z < ((cz >> 15) & 0xFFFF))).all())
                            flags[f"sound_chunk_live/{k}"] = bool((live == 1).all())
                        del before
                    if rnd == 0 and tab is not None:    # the tables of the columns that hold the misplaced voxels
                        m = wc.misplaced(name)
                        cols = m[:, 0] * c["dims"][1] + m[:, 1]
                        out[f"{name}/misplaced_info/{k}"], out[f"{name}/misplaced_colz/{k}"] = tab["colinfo"][cols], tab["colz"][cols]
                    if rnd == 0 and k == len(obs) - 1 and name not in wc.HUGE:
                        recs.append([f.clone() for f in fields])
                    if rnd == 1 and k == len(obs) - 1 and recs:
                        flags["second_round_equal"] = _fields_equal(recs[-1], fields)
                else:
                    rec = _records(vol.get_volume_tensors())
                    if rnd == 0:
                        recs.append(rec)
                        out[f"{name}/idx/{k}"], out[f"{name}/val/{k}"] = _sparse(rec)
                        if tab is not None and keep_tables:
                            for key, a in tab.items():
                                out[f"{name}/{key}/{k}"] = a
                        if k == len(obs) - 1:
                            out[f"{name}/mesh_faces"], flags["mesh_equals_marching_cubes_of_the_fields"] = \
                                _mesh_check(vol, name) if cells else (0, True)
                    else:
                        flags[f"second_round_equal/{k}"] = bool(torch.equal(recs[k], rec))
            del oracle
        # a second volume object of the case, after the first: the tables are per object
        if name in wc.HUGE:
            first = vol.get_volume_tensors()
        other = _volume(name)
        if c["touch"]:
            other.touch()
        for (l3, d, r), w in zip(obs, weights):
            other.integrate(l3, d, r, np.eye(4), obs_weight=w)
        if big:
            flags["other_object_equal"] = _fields_equal(first if name in wc.HUGE else recs[-1], other.get_volume_tensors())
        else:
            flags["other_object_equal"] = bool(torch.equal(recs[-1], _records(other.get_volume_tensors())))
        for key, val in flags.items():
            out[f"{name}/flag/{key}"] = np.bool_(val)
        vol.close()
        other.close()
        del recs, vol, other
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        out[f"{name}/seconds"] = np.float64(time.perf_counter() - t_case)
    np.savez(path, **out)


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """setting -> the child's results.  One child per setting, one after the other, each with a time limit of its own; after a
    child that a signal or the limit ended nothing more is started on the GPU: the session ends there."""
    root = tmp_path_factory.mktemp("tsdf_walk_paths")
    res = {}
    for mode, extra in CHILDREN.items():
        env = dict(os.environ)
        for k in ENV_KEYS:
            env.pop(k, None)
        env.update(extra)
        path = str(root / f"{mode}.npz")
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), path, mode], env=env, capture_output=True, text=True,
                               timeout=240)
        except subprocess.TimeoutExpired:
            pytest.exit(f"tsdf walk child '{mode}' did not end within its time limit: nothing more is run on the GPU", 1)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            pytest.exit(f"tsdf walk child '{mode}' ended with {r.returncode}: nothing more is run on the GPU\n"
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

    def run(which):
        o = _Oracle(name, which)
        return [_sparse(_records(o.step(*ob_, w))) for ob_, w in zip(_obs(name), wc.case(name)["weights"])]
    return (run("ref") if ob.ref_tsdf_available() else None), run("dense")


def _same(a, b, what):
    (ia, va), (ib, vb) = a, b
    if ia.shape == ib.shape and np.array_equal(ia, ib) and np.array_equal(va, vb):
        return
    sa, sb = {int(i): tuple(v) for i, v in zip(ia, va)}, {int(i): tuple(v) for i, v in zip(ib, vb)}
    bad = sorted(i for i in set(sa) | set(sb) if sa.get(i) != sb.get(i))
    assert not bad, f"{what}: {len(bad)} voxels differ (of {len(sa)} / {len(sb)} written), first at index {bad[0]}"


def _child_state(res, name, k):
    return res[f"{name}/idx/{k}"], res[f"{name}/val/{k}"]


def _flags(res, name):
    return {k.split("/flag/")[1]: bool(v) for k, v in res.items() if k.startswith(f"{name}/flag/")}


@pytest.mark.parametrize("name", [n for n in wc.OWN if n not in wc.BIG])
def test_dense_restatement_equals_the_reference_kernel(name):
    from oracle import binding as ob
    if not ob.ref_tsdf_available():
        pytest.skip("oracle/_ref/libref_tsdf_integrate.so not built (needs the reference's kernel text + hipcc at build time)")
    R, D = _oracles(name)
    for k in range(len(D)):
        _same(R[k], D[k], f"{name}, observation {k}: reference kernel source vs oracle/lt_tsdf_dense.hip")


@pytest.mark.parametrize("mode", list(CHILDREN))
@pytest.mark.parametrize("name", SMALL)
def test_integrate_equals_the_oracles(children, name, mode):
    """Every observation prefix against the dense restatement and the reference build; the second round after a reset and a
    second volume object against the first round (compared on the device in the child: its flags); after every reset all
    voxels are the initial ones, as bits, and the mesh has no face; the mesh of the walked volume is marching cubes over its
    fields."""
    res = children[mode]
    R, D = _oracles(name)
    assert D[-1][0].size > (40 if name in ("trips_dz1", "dead_ulp") else 300), "the oracle's volume is idle"
    for k in range(len(D)):
        _same(D[k], _child_state(res, name, k), f"{name}, observation {k}: oracle/lt_tsdf_dense.hip vs integrate ({mode})")
        if R is not None:
            _same(R[k], _child_state(res, name, k), f"{name}, observation {k}: reference kernel vs integrate ({mode})")
    flags = _flags(res, name)
    assert len(flags) == 4 + len(D) and all(flags.values()), f"{name} ({mode}): {[k for k, v in flags.items() if not v]}"


@pytest.mark.parametrize("name,mode", [(n, m) for n in wc.BIG for m in CHILDREN if n in _cases_of(m)])
def test_big_cases_equal_the_oracles_on_the_device(children, name, mode):
    """Beyond 2^24 voxels: compared field by field on the device in the child; here its verdicts and, where a comparison
    failed, how many voxels differ and the first of them."""
    from oracle import binding as ob
    res = children[mode]
    flags = _flags(res, name)
    n_obs = len(wc.case(name)["obs"])
    for k in range(n_obs):
        assert f"equals_dense/{k}" in flags and int(res[f"{name}/n_written/{k}"]) > 100000
        assert int(res[f"{name}/n_product/{k}"]) == int(res[f"{name}/n_written/{k}"])
        assert (f"equals_ref/{k}" in flags) == ob.ref_tsdf_available()
    assert "reset_is_initial" in flags and "other_object_equal" in flags
    if mode.startswith("walk"):
        assert all(f"sound_{t}/{k}" in flags for t in ("colinfo", "colz", "chunk_live") for k in range(n_obs))
    diffs = {k.split("/", 1)[1]: (int(v), res[k.replace("n_diff", "diff_idx")][:8].tolist())
             for k, v in res.items() if k.startswith(f"{name}/n_diff_") and int(v)}
    assert all(flags.values()) and not diffs, f"{name} ({mode}): {[k for k, v in flags.items() if not v]}; differing voxels {diffs}"


@pytest.mark.parametrize("name", ["beyond_2p24", "big_y0", "big_ym2"])
def test_columns_of_misplaced_voxels_are_walked_whole(children, name):
    """The columns whose first (or only) voxel the reference's float index gives to another x: dead by their own geometry in
    the constructed observations, and walked all the same (colinfo -2), from z = 0 to dim_z, not plain."""
    res = children["walk"]
    m = wc.misplaced(name)
    dz = wc.case(name)["dims"][2]
    for k in range(len(wc.case(name)["obs"])):
        info, colz = res[f"{name}/misplaced_info/{k}"], res[f"{name}/misplaced_colz/{k}"].astype(np.int64)
        assert info.shape[0] == m.shape[0] > 0
        assert (info != -1).all(), f"{name}, observation {k}: colinfo {info.tolist()}"
        assert ((colz & 0x7FFF) == 0).all() and (((colz >> 15) & 0xFFFF) == dz).all() and ((colz >> 31) == 0).all()
        if name != "beyond_2p24":
            assert (info == -2).all()


@pytest.mark.parametrize("mode", [m for m in CHILDREN if m != "walk"])
def test_every_child_equals_walk(children, mode):
    """(Each is held to the oracles above as well; this names the pair.)"""
    for name in SMALL:
        for k in range(len(wc.case(name)["obs"])):
            _same(_child_state(children["walk"], name, k), _child_state(children[mode], name, k),
                  f"{name}, observation {k}: walk vs {mode}")
    for name in wc.BIG:
        if name in _cases_of(mode):
            for k in range(len(wc.case(name)["obs"])):
                assert int(children[mode][f"{name}/n_product/{k}"]) == int(children["walk"][f"{name}/n_product/{k}"])


@pytest.mark.parametrize("name", wc.NAMES)
def test_which_kernel_ran(children, name):
    """lt_debug_tsdf_wedge answers "no table" for a volume the pixel pass never ran on; lt_debug_tsdf_walk_table likewise for
    one that was never walked."""
    c = wc.case(name)
    n_obs = len(c["obs"])
    pix = wc.pix_applies(c)
    for mode in CHILDREN:
        if name not in _cases_of(mode):
            continue
        res = children[mode]
        walked = [bool(res[f"{name}/walked/{k}"]) for k in range(n_obs)]
        if mode.startswith("walk"):
            assert int(res[f"{name}/wedge_rc"]) != 0 and all(walked), mode
        elif mode == "pix1":
            assert (int(res[f"{name}/wedge_rc"]) == 0) == pix and walked == [not pix] + [True] * (n_obs - 1), mode
        else:
            assert (int(res[f"{name}/wedge_rc"]) == 0) == pix and walked == [not pix] * n_obs, mode


def _unpack(colz):
    colz = colz.astype(np.int64)
    return colz & 0x7FFF, (colz >> 15) & 0xFFFF, (colz >> 31) != 0


@pytest.mark.parametrize("name", SMALL)
def test_tables_are_sound_and_equal_the_restatement(children, name):
    """Soundness: every voxel the dense oracle changed in observation k lies in a column with colinfo != -1, inside [z0, z1) of
    colz, in a chunk with chunk_live == 1 -- bit-equality implies it; this names the shortcut that failed.  And the tables are
    the ones the CPU proofs reason about: colmax exactly; colinfo, the z range and the plain flag on every column outside the
    restatement's margin."""
    c, g = wc.case(name), wc.geometry(name)
    dz = c["dims"][2]
    _, D = _oracles(name)
    prev = {}
    for k in range(len(c["obs"])):
        now = {int(i): tuple(v) for i, v in zip(*D[k])}
        changed = np.array(sorted(i for i in now if prev.get(i) != now[i]), np.int64)
        prev = now
        for mode in ("walk", "pix1", "default"):
            res = children[mode]
            if not bool(res[f"{name}/walked/{k}"]):
                continue
            info, live, colz, cm = (res[f"{name}/{t}/{k}"] for t in TABLES)
            z0, z1, plain = _unpack(colz)
            col, z = changed // dz, changed % dz
            what = f"{name}, observation {k} ({mode})"
            assert (info[col] != -1).all(), f"{what}: {(info[col] == -1).sum()} changed voxels in columns called dead"
            assert ((z >= z0[col]) & (z < z1[col])).all(), f"{what}: changed voxels outside the z range"
            assert (live[col >> 6] == 1).all(), f"{what}: changed voxels in chunks called dead"
            # the restatement
            T = wc.walk_tables(name, k)
            assert np.array_equal(cm.view(np.int32), T["colmax"].view(np.int32)), f"{what}: colmax"
            s = T["sure"] & (T["dead"] | (g["px_lo"] == g["px_hi"]))
            want = np.where(T["dead"], np.where(g["whole"], -2, -1), g["px_lo"])
            assert np.array_equal(info[s], want[s]), f"{what}: colinfo differs on {(info[s] != want[s]).sum()} columns"
            if name == "dead_ulp":
                tc = wc.DEAD_ULP_COL[0] * c["dims"][1] + wc.DEAD_ULP_COL[1]
                assert (info[tc] == -1) == (wc.DEAD_ULP_STEPS[k] < 0), f"{what}: the column decided by the last bit"
            sw = T["sure_walked"] & g["z_sure"] & (info != -1)
            assert np.array_equal(z0[sw], g["z0"][sw]) and np.array_equal(z1[sw], g["z1"][sw]), f"{what}: z ranges"
            ok = sw & s
            assert np.array_equal(plain[ok], (wc.plain_of(name) & (want >= 0))[ok]), f"{what}: plain flags"
            n_ch = g["n_chunks"]
            pad = lambda a, fill: np.concatenate([a, np.full(n_ch * 64 - a.size, fill, a.dtype)]).reshape(n_ch, 64)  # noqa: E731
            sure_ch = pad(T["sure_walked"], True).all(1)
            assert np.array_equal(live[:n_ch][sure_ch], pad(T["walked"], False).any(1)[sure_ch].astype(np.int32)), \
                f"{what}: chunk_live"


def _cnt(res, name, k, word):
    return int(res[f"{name}/cnt/{k}"][wc.CNT[word]])


@pytest.mark.parametrize("name", SMALL)
def test_counters_show_the_intended_paths(children, name):
    res, one = children["walk_counters"], children["walk_counters_one_wg"]
    c, g = wc.case(name), wc.geometry(name)
    n_obs, n_ch, dz = len(c["obs"]), g["n_chunks"], c["dims"][2]
    _, D = _oracles(name)
    band_on = wc.band_ok(c) and c["merge"] and not c["touch"]
    print(name, {w: [_cnt(res, name, k, w) for k in range(n_obs)] for w in wc.CNT})
    total = {w: sum(_cnt(res, name, k, w) for k in range(n_obs)) for w in wc.CNT}
    for k in range(n_obs):
        g_ = lambda w: _cnt(res, name, k, w)     # noqa: E731
        T = wc.walk_tables(name, k)
        assert g_("chunks") + g_("skipped") == n_ch
        assert g_("cols") == g_("cols_m2") + g_("cols_plain") + g_("cols_nonplain") == g_("cols_fresh") + g_("cols_written")
        assert g_("cols") == g_("cols_band") + g_("cols_direct")
        assert g_("chunks_max") == 1, "a workgroup per chunk by default"
        assert int(one[f"{name}/cnt/{k}"][wc.CNT["chunks_max"]]) == n_ch, "LIDARHIP_TSDF_BLOCKS=1: one workgroup takes every chunk"
        for w in ("chunks", "skipped", "cols", "cols_m2", "cols_plain", "cols_fresh", "cols_band", "band_vox", "band_cand",
                  "direct_vox", "code1", "code2", "stamp_fresh", "stamp_merged", "trips_max", "sign_hi", "mixed", "quads_idle"):
            assert int(one[f"{name}/cnt/{k}"][wc.CNT[w]]) == g_(w), f"{w}: one workgroup vs one per chunk"
        # the exact counts the CPU proof gives: walked columns, dead chunks, trips
        sure, walked = T["sure_walked"], T["walked"]
        lo = int((walked & sure).sum())
        assert lo <= g_("cols") <= lo + int((~sure).sum()), f"observation {k}: {g_('cols')} columns walked"
        m2 = int((T["info_m2"] & T["sure"]).sum())
        assert m2 <= g_("cols_m2") <= m2 + int((~T["sure"]).sum())
        pad = np.zeros(n_ch * 64, bool)
        pad[:g["n_cols"]] = walked | ~sure
        surely_dead = n_ch - int(pad.reshape(n_ch, 64).any(1).sum())
        pad[:g["n_cols"]] = walked & sure
        maybe_dead = n_ch - int(pad.reshape(n_ch, 64).any(1).sum())
        assert surely_dead <= g_("skipped") <= maybe_dead
        if sure.all() and g["z_sure"].all():
            assert g_("cols") == lo and g_("skipped") == surely_dead == maybe_dead
            trips = (g["z1"] - (g["z0"] & ~15) + 15) >> 4
            assert g_("trips_max") == int(trips[walked].max())
        # band or direct
        if not band_on:
            assert g_("cols_band") == g_("band_vox") == g_("band_cand") == g_("flush_full") == g_("flush_tail") == 0
            assert g_("direct_vox") > 0
        elif k == 0:
            assert g_("cols_fresh") == g_("cols") and g_("cols_band") == g_("cols_plain")
            assert g_("cols_direct") == g_("cols_m2") + g_("cols_nonplain") and g_("stamp_merged") == 0
            # every candidate is flushed once: the full flushes take 64 each, a tail flush fewer
            assert 64 * g_("flush_full") + g_("flush_tail") <= g_("band_cand")
            assert g_("band_cand") <= 64 * g_("flush_full") + g_("tail_max") * g_("flush_tail")
            if D[0][0].size:    # (degenerate_1x1: the first observation's only pixel has no depth)
                assert g_("cols_band") > 0 and g_("band_cand") > 0 and g_("flush_tail") > 0 and 0 < g_("tail_max") < 64
        if k == 0:  # what the first observation writes differs from the initial volume: the oracle's count, exactly
            idx, val = D[0]
            tsdf = val[:, 0].copy().view(np.float32)
            assert g_("code1") + g_("code2") == idx.size, f"{g_('code1')} + {g_('code2')} voxels written, {idx.size} by the oracle"
            assert g_("code2") == int((~(tsdf > 0)).sum())
        if c["touch"]:
            assert g_("cols_fresh") == 0 and g_("stamp_fresh") == 0 and g_("stamp_merged") > 0
        assert g_("band_cand") <= g_("band_vox") and g_("stamp_fresh") <= g_("cols_fresh")
        assert g_("sign_hi") == 0 or dz > 64, "sign words of index >= 1"
    if name == "wall0":
        assert _cnt(res, name, 0, "flush_full") >= 8 and _cnt(res, name, 0, "flush_tail") > 0
        assert _cnt(res, name, 0, "band_cand") > 0.5 * _cnt(res, name, 0, "band_vox")
    if name == "class_thin":
        assert total["flush_full"] == 0 and total["flush_tail"] > 0 and 0 < _cnt(res, name, 0, "tail_max") <= 48
        assert _cnt(one, name, 0, "flush_full") > 0, "one workgroup: the queue carries over from chunk to chunk and fills"
    if name == "mixed_waves":
        assert _cnt(res, name, 1, "mixed") >= 10 and _cnt(res, name, 1, "stamp_merged") > 100
        assert _cnt(res, name, 1, "cols_written") > 100 and _cnt(res, name, 1, "cols_band") > 100
    if name == "sparse_live":
        assert all(_cnt(res, name, k, "quads_idle") > 0 for k in range(n_obs))
    if name == "dead_partial":
        assert all(_cnt(res, name, k, "skipped") >= 35 for k in range(n_obs))
    if name.startswith("trips_dz"):
        assert all(_cnt(res, name, k, "trips_max") == wc.TRIPS[dz] for k in range(n_obs))
    if name in ("signs_dz65", "signs_dz130", "signs_nan"):
        assert all(_cnt(res, name, k, "sign_hi") > 0 for k in range(n_obs))
    if name in ("signs_dz37", "signs_dz64"):
        assert total["sign_hi"] == 0 and total["code2"] > 0
    if n_obs >= 2 and c["merge"] and name != "sparse_live":     # (sparse_live: another wedge every time)
        assert total["stamp_merged"] > 0 and total["cols_written"] > 0, "a later observation meets written columns"


def test_big_counters(children):
    """beyond_2p24's two columns with y = 0 are live and not plain; big_y0's fourteen and big_ym2's six are dead, walked whole."""
    res = children["walk_counters"]
    assert _cnt(res, "beyond_2p24", 0, "cols_nonplain") >= 2
    for name, n in (("big_y0", 14), ("big_ym2", 6)):
        T = wc.walk_tables(name, 0)
        m2 = int((T["info_m2"] & T["sure"]).sum())
        assert m2 >= n and m2 <= _cnt(res, name, 0, "cols_m2") <= m2 + int((~T["sure"]).sum())
        assert _cnt(res, name, 0, "skipped") > 0 and _cnt(res, name, 0, "chunks_max") == 1


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2])
