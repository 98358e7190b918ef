"""The values of the TSDF update pinned on the GPU: every update body of lidar_transfer_amd/csrc/lt_tsdf.hip off the
`obs_weight = 1` path, on the inputs of tests/tsdf_update_cases.py (what they reach is proven without a GPU in
tests/test_tsdf_update_cases_cpu.py): fractional and huge weights, the class-aware comparison against the weight volume
where it is live, rounding ties, the clamp, all three colour channels, a colour above 2^24, remissions 0 and -1.

Cases A - D: all four fields bit for bit between the reference's own kernel text compiled for gfx950
(oracle/_ref/libref_tsdf_integrate{,_plain}.so), the dense restatement (oracle/lt_tsdf_dense.hip), TSDFVolume.integrate in the
three modes of LIDARHIP_TSDF_PIX (read once per process: one child process per mode runs all cases) and
TSDFVolume.integrate_multi; every product volume is reset and run again.  The mesh read from the sign bits the update kept
against marching cubes over the oracle's fields.  Case E: mode="numpy" against the numpy restatement of the host-mode
contract.  The shapes that break the work-saving machinery are tests/test_tsdf_gpu.py's."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tsdf_update_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("tsdf", "weight", "color", "rem")
MODES = {"default": None, "walk": "0", "pix1": "1"}     # LIDARHIP_TSDF_PIX
_REF_SKIP = "oracle/_ref/libref_tsdf_integrate.so not built (needs /root/reference + hipcc at build time)"


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        bad = int((_bits(x) != _bits(y)).sum())
        assert bad == 0, f"{what}: {bad} of {x.size} voxels differ in {name}"


def _volume(case):
    from lidar_transfer_amd.fusion import TSDFVolume
    c = tc.CASES[case]
    vol = TSDFVolume(tc.BNDS, tc.VOXEL, tc.FOV_UP, tc.FOV_DOWN, merge=c["merge"], mode=c["mode"])
    assert tuple(int(x) for x in vol._vol_dim) == tc.DIMS
    return vol


def _two_rounds(vol, run):
    """`run(vol)`, the volumes, a reset, `run(vol)` again into the same object, the volumes."""
    out = []
    for rnd in range(2):
        if rnd:
            vol.reset()
        run(vol)
        out.append([t.cpu().numpy() for t in vol.get_volume_tensors()])
    return out


@functools.lru_cache(maxsize=None)
def _obs(case):
    """The case's observations as writable copies (the cases module shares read-only arrays; torch wraps writable ones)."""
    return [tuple(np.array(a) for a in o) for o in tc.observations(case)]


def _integrate_each(case):
    c = tc.CASES[case]

    def run(vol):
        for label3, depth, rem in _obs(case):
            vol.integrate(label3, depth, rem, np.eye(4), obs_weight=c["weight"])
    return run


# ---- the child process of one LIDARHIP_TSDF_PIX mode: every device case through TSDFVolume.integrate, twice ---------------

def _child_main(path):
    sys.path.insert(0, os.path.dirname(HERE))
    out = {}
    for case in tc.DEVICE_CASES:
        vol = _volume(case)
        for rnd, vols in enumerate(_two_rounds(vol, _integrate_each(case))):
            for name, a in zip(NAMES, vols):
                out[f"{case}/{rnd}/{name}"] = a
        vol.close()
    np.savez(path, **out)


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """mode -> the child's volumes.  One child per mode, one after the other, each with a time limit of its own; after a child
    that a signal or the limit ended nothing more is started on the GPU: the session ends there."""
    root = tmp_path_factory.mktemp("tsdf_update")
    res = {}
    for mode, value in MODES.items():
        env = dict(os.environ)
        env.pop("LIDARHIP_TSDF_PIX", None)
        env.pop("LIDARHIP_TSDF_MULTI", None)
        if value is not None:
            env["LIDARHIP_TSDF_PIX"] = value
        path = str(root / f"{mode}.npz")
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True,
                               timeout=120)
        except subprocess.TimeoutExpired:
            pytest.exit(f"tsdf update child '{mode}' did not end within its time limit: nothing more is run on the GPU", 1)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            pytest.exit(f"tsdf update child '{mode}' ended with {r.returncode}: nothing more is run on the GPU\n"
                        + r.stderr[-2000:], 1)
        assert r.returncode == 0, f"child '{mode}':\n" + r.stderr[-2000:]
        res[mode] = np.load(path)
    return res


# ---- the parent: the two oracles ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracles(case):
    """(reference kernel build's volumes or None, dense restatement's volumes) after the case, as numpy arrays."""
    import torch
    from oracle import binding as ob
    c = tc.CASES[case]
    dev = torch.device("cuda", 0)
    n = int(np.prod(tc.DIMS))
    dims = (C.c_int * 3)(*tc.DIMS)
    org = (C.c_float * 3)(*[float(x) for x in tc.ORIGIN])
    vp = C.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)

    def fresh():   # 64 spare floats behind each field: the reference kernel runs thread n (test_tsdf_ref_kernel_gpu.py)
        flat = [torch.ones(n + 64, device=dev)] + [torch.zeros(n + 64, device=dev) for _ in range(3)]
        return [t[:n].view(tc.DIMS) for t in flat]
    ref = ob.ref_tsdf_lib(c["merge"]) if ob.ref_tsdf_available() else None
    vr, vd = fresh(), fresh()
    for label3, depth, rem in _obs(case):
        folded_host = tc.fold(label3)
        c3 = torch.from_numpy(label3).to(dev)
        folded = torch.floor(c3[:, :, 0] * 256 * 256 + c3[:, :, 1] * 256 + c3[:, :, 2]).contiguous()
        assert np.array_equal(folded.cpu().numpy(), folded_host), "the device folds the colours as the cases module does"
        d, r = torch.from_numpy(depth).to(dev), torch.from_numpy(rem).to(dev)
        args = (dims, org, C.c_float(np.float32(tc.VOXEL)), C.c_float(np.float32(tc.VOXEL * 5)), C.c_float(tc.FOV_UP),
                C.c_float(tc.FOV_DOWN), vp(folded.data_ptr()), vp(d.data_ptr()), vp(r.data_ptr()), tc.H, tc.W,
                C.c_float(c["weight"]))
        if ref is not None:
            assert ref.ref_tsdf_integrate(*[vp(t.data_ptr()) for t in vr], *args, st) == 0
        assert ob.dense_lib().lt_test_tsdf_integrate_dense(*[vp(t.data_ptr()) for t in vd], *args, 1 if c["merge"] else 0,
                                                           st) == 0
        torch.cuda.synchronize()
    D = [t.cpu().numpy() for t in vd]
    R = [t.cpu().numpy() for t in vr] if ref is not None else None
    return R, D


def _not_idle(case, vols):
    """The oracle's volumes hold what the case is there for (counted in tests/test_tsdf_update_cases_cpu.py)."""
    c = tc.CASES[case]
    tsdf, weight, color, rem = vols
    n, w = tsdf.size, c["weight"]
    assert ((tsdf != 1) | (weight != 0)).sum() > 0.2 * n, "test volume barely touched"
    assert (tsdf < 0).sum() > 0.01 * n, "no surface crossing"
    if w != np.floor(w):
        assert (weight != np.floor(weight)).sum() > 0.01 * n, "no fractional weights"
    if w < 1:
        assert (tsdf > 1).sum() > 0.005 * n, "no tsdf above 1"
    b, g, r = tc.unfold(color)
    if w < tc.W24 or c["merge"]:
        assert ((g != 0) & (r != 0)).sum() > 0.01 * n, "no colour with g and r"
    assert (rem < 0).sum() > 0 and np.isfinite(tsdf).all()


@pytest.mark.parametrize("case", tc.DEVICE_CASES)
def test_dense_restatement_equals_the_reference_kernel(case):
    from oracle import binding as ob
    if not ob.ref_tsdf_available():
        pytest.skip(_REF_SKIP)
    R, D = _oracles(case)
    _not_idle(case, R)
    _same(R, D, f"{case}: reference kernel source vs restatement oracle/lt_tsdf_dense.hip")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", tc.DEVICE_CASES)
def test_integrate_equals_the_oracles(children, case, mode):
    """TSDFVolume.integrate, one call per observation, in one mode of LIDARHIP_TSDF_PIX (default: pixels, then the written
    ranges; walk: the column walk; pix1: pixels on the fresh volume, then the walk; the plain average walks in all three)."""
    R, D = _oracles(case)
    _not_idle(case, D)
    first, second = [[children[mode][f"{case}/{rnd}/{name}"] for name in NAMES] for rnd in range(2)]
    _same(D, first, f"{case}: oracle/lt_tsdf_dense.hip vs TSDFVolume.integrate ({mode})")
    _same(first, second, f"{case}: TSDFVolume.integrate ({mode}) after a reset vs the first round")
    if R is not None:   # (not built: test_dense_restatement_equals_the_reference_kernel skips and says so)
        _same(R, first, f"{case}: reference kernel source vs TSDFVolume.integrate ({mode})")


@pytest.mark.parametrize("case", tc.DEVICE_CASES)
def test_integrate_multi_equals_the_oracles(case):
    """TSDFVolume.integrate_multi: the fused pass for the class-aware cases (D: one pass of eight, the ninth alone on a volume
    with fractional weights), the loop for the plain average."""
    c = tc.CASES[case]
    R, D = _oracles(case)
    vol = _volume(case)
    first, second = _two_rounds(vol, lambda v: v.integrate_multi(_obs(case), obs_weight=c["weight"]))
    vol.close()
    _same(D, first, f"{case}: oracle/lt_tsdf_dense.hip vs TSDFVolume.integrate_multi")
    _same(first, second, f"{case}: TSDFVolume.integrate_multi after a reset vs the first round")
    if R is not None:
        _same(R, first, f"{case}: reference kernel source vs TSDFVolume.integrate_multi")


@pytest.mark.parametrize("how", ["integrate", "integrate_multi"])
@pytest.mark.parametrize("case", [k for k in tc.DEVICE_CASES if k.startswith("A-")])
def test_mesh_from_the_kept_sign_bits(case, how):
    """extract_mesh reads the sign bits the update kept per voxel (`!(tv > 0)`); marching cubes over contiguous copies of the
    oracle's tsdf / colour / remission reads the values: vertices, faces, colours, remissions element for element (both
    renumbered by first use in the face stream: the numbering that does not depend on the extraction's own order)."""
    import torch
    from lidar_transfer_amd.fusion import DeviceMesh
    c = tc.CASES[case]
    R, D = _oracles(case)
    O = R if R is not None else D
    assert np.isfinite(O[0]).all() and (O[0] < 0).sum() > 100
    if c["weight"] < 1:
        assert (O[0] > 1).sum() > 100, "no tsdf above 1 in the field"
    vol = _volume(case)
    if how == "integrate":
        _integrate_each(case)(vol)
    else:
        vol.integrate_multi(_obs(case), obs_weight=c["weight"])
    got = [t.cpu().numpy() for t in vol.extract_mesh().renumber().tensors()]
    fields = [torch.from_numpy(np.ascontiguousarray(O[k])).cuda() for k in (0, 2, 3)]
    mesh = DeviceMesh()
    want = [t.cpu().numpy() for t in mesh.extract(*fields, tc.VOXEL, tc.ORIGIN).renumber().tensors()]
    assert want[1].shape[0] > 1000, "hardly a mesh"
    for name, a, b in zip(("verts", "faces", "colors", "rem"), got, want):
        assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), f"{case} ({how}): {name} differ"
    mesh.close()
    vol.close()


@pytest.mark.parametrize("case", tc.HOST_CASES)
def test_host_mode_equals_its_restatement(case):
    """TSDFVolume(mode="numpy") against the numpy restatement of the LT_TSDF_HOST_MODE contract: tsdf bits, weight and colour
    but for max(2, 1e-5 n) voxels (within an ulp of a pixel boundary, where the float64 arctan2 / arcsin of numpy and of the
    device library decide by their last bit -- the allowance of test_numpy_mode_equals_the_reference_numpy_cpu_mode);
    remissions untouched."""
    c = tc.CASES[case]
    want = tc.host_case(case)[0]
    vol = _volume(case)
    first, second = _two_rounds(vol, _integrate_each(case))
    vol.close()
    _same(first, second, f"{case}: mode='numpy' after a reset vs the first round")
    tsdf, weight, color, rem = first
    n = tsdf.size
    diff = (_bits(tsdf) != _bits(want[0])) | (weight != want[1]) | (color != want[2])
    assert diff.sum() <= max(2, 1e-5 * n), f"{case}: {diff.sum()} of {n} voxels differ"
    assert float(np.abs(rem).max()) == 0.0
    assert (weight > 0).sum() > 0.2 * n
    if c["weight"] != np.floor(c["weight"]):
        assert (weight != np.floor(weight)).sum() > 0.01 * n


if __name__ == "__main__":
    _child_main(sys.argv[1])
