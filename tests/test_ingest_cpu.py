"""The ingest stage's host side and its contract, without a GPU (golden F17, tests/golden/make_golden_ingest.py: the
reference's `parse_calibration` / `parse_poses` / `open_multiple_scans` / `deform` run from the files of a synthetic sequence).

This file also holds THE numpy restatement of the five rules of `lt_ingest_scans_dev` (include/lidarhip.h) -- plain order, no
matmul -- which tests/test_ingest_gpu.py compares the device with bit for bit."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("LT_REFERENCE", "/root/reference")
U = 2.0 ** -53


def gold():
    return np.load(os.path.join(HERE, "golden", "f17_ingest.npz"))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def raw_scans(g):
    """[(xyzr [n,4] f32, label [n] u32)] of the fixture's eight file pairs"""
    return [(g[f"scan{k}"].view(np.float32).reshape(-1, 4), g[f"label{k}"].view(np.uint32)) for k in range(int(g["n_scans_seq"]))]


def case_of(g, tag):
    return dict(tag=tag, adaption=str(g[f"{tag}_adaption"]), nscans=int(g[f"{tag}_nscans"]), idx=int(g[f"{tag}_idx"]),
                slots=[int(x) for x in g[f"{tag}_slots"]], back=g[f"{tag}_back"], ignore=[int(x) for x in g[f"{tag}_ignore"]],
                moving=[int(x) for x in g[f"{tag}_moving"]], merged=str(g[f"{tag}_adaption"]) != "mesh")


def cases(g):
    return [case_of(g, str(t)) for t in g["cases"]]


# ---- the restatement: rules 1-5 of lt_ingest_scans_dev -------------------------------------------------------------------
def plain_transform(M, p):
    """rule 5: every row as ((m0*x + m1*y) + m2*z) + m3 -- numpy's elementwise products and sums round one by one"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], 1)


def restate(raw, poses, slots, back, ignore, moving, merged, world=False):
    """[(points f64, rem f32, label u32)] per slot, or the one merged cloud; ``world``: also the stage-one coordinates"""
    out, qs, hs = [], [], []
    for i, s in enumerate(slots):
        xyzr, label = raw[s]
        l = label & 0xFFFF                                     # rule 1
        drop = np.isin(l, ignore)                              # rule 2
        if i != 0:
            drop |= np.isin(l, moving)
        keep = ~drop                                           # rule 3: a boolean mask keeps the file order
        h = xyzr[keep, :3].astype(np.float64)
        q = plain_transform(poses[s], h)                       # rule 4: two transforms, each rounded
        out.append((plain_transform(back, q), xyzr[keep, 3].copy(), l[keep].astype(np.uint32)))
        qs.append(q)
        hs.append((h, np.broadcast_to(np.abs(poses[s]), (len(h), 4, 4))))
    if merged:
        out = [tuple(np.concatenate([c[j] for c in out]) for j in range(3))]
        qs = [np.concatenate(qs)]
        hs = [(np.concatenate([h for h, _ in hs]), np.concatenate([a for _, a in hs]))]
    return (out, qs, hs) if world else out


def reference_points(g, tag, plain):
    """The reference's prepared points of a case: the fixture stores their distance (int64 views subtracted) from the plain
    order, and the digest of their own bytes -- what comes out here IS the reference's array, or the assertion fails."""
    ulp = g[f"{tag}_prep_ulp"]
    n = [int(x) for x in g[f"{tag}_prep_n"]]
    assert [len(c[0]) for c in plain] == n, (tag, [len(c[0]) for c in plain], n)   # the kept set's size
    out, at = [], 0
    for k, (p, _, _) in enumerate(plain):
        ref = (np.ascontiguousarray(p).view(np.int64) + ulp[at:at + len(p)]).view(np.float64)
        at += len(p)
        assert sha(ref) == str(g[f"{tag}_prep_sha"][k][0]), f"{tag}: cloud {k}: not the reference's points"
        out.append(ref)
    return out


def transform_bound(h, absA, q, back):
    """What two correctly rounded evaluations of the two chained 4-term dot products may differ by, per coordinate (any
    order, fused or not): with gamma = 4u / (1 - 4u), stage one b1_i = 2 gamma sum_j |A_ij| |h_j| (h = [x, y, z, 1]), stage
    two sum_{j<3} |B_ij| b1_j + 2 gamma sum_j |B_ij| |[q, 1]_j|; twice that for the second-order terms."""
    gam = 4 * U / (1 - 4 * U)
    h1 = np.concatenate([np.abs(h), np.ones((len(h), 1))], 1)
    b1 = 2 * gam * np.einsum("nij,nj->ni", absA[:, :3, :], h1)
    q1 = np.concatenate([np.abs(q), np.ones((len(q), 1))], 1)
    aB = np.abs(back)
    b2 = b1 @ aB[:3, :3].T + 2 * gam * (q1 @ aB[:3, :].T)
    return 2 * b2


# ---- tests ----------------------------------------------------------------------------------------------------------------
def test_relative_indices_are_the_slot_order_of_open_multiple_scans():
    from lidar_transfer_amd.ingest import relative_indices
    g = gold()
    for n in range(1, 7):
        assert relative_indices(n) == [int(x) for x in g[f"relative_{n}"]], n
    assert relative_indices(3) == [0, -1, 1] and relative_indices(4) == [0, -2, -1, 1] and relative_indices(1) == [0]
    for c in cases(g):
        assert [c["idx"] + r for r in relative_indices(c["nscans"])] == c["slots"], c["tag"]
    with pytest.raises(ValueError):
        relative_indices(0)


def _write_text_files(g, d):
    calib, poses = os.path.join(d, "calib.txt"), os.path.join(d, "poses.txt")
    g["calib_txt"].tofile(calib)
    g["poses_txt"].tofile(poses)
    return calib, poses


def test_parsed_poses_equal_the_golden_poses(tmp_path):
    """The generator ran under another interpreter and BLAS build, which reorder the sums of Tr^-1 (pose Tr): two chained
    4-term products cost at most 4 * 2^-53 * sum |a||b| each, under 64 * 2^-53 * max|pose| together for a Tr whose rows sum
    to less than 3 in magnitude (translation below 1 m), plus the inverse of a well-conditioned rigid Tr; 256 leaves a factor
    of four."""
    from lidar_transfer_amd.ingest import parse_calibration, parse_poses
    g = gold()
    calib_path, poses_path = _write_text_files(g, str(tmp_path))
    calib = parse_calibration(calib_path)
    assert sorted(calib) == ["P0", "Tr"] and calib["Tr"].shape == (4, 4) and calib["Tr"].dtype == np.float64
    assert np.abs(calib["Tr"][:3, 3]).max() < 1.0 and np.abs(calib["Tr"][:3]).sum(1).max() < 3.0
    poses = parse_poses(poses_path, calib)
    want = g["poses"]
    assert len(poses) == len(want) == 8 and all(p.shape == (4, 4) and p.dtype == np.float64 for p in poses)
    atol = 256 * U * float(np.abs(want).max())
    assert np.allclose(np.stack(poses), want, rtol=0, atol=atol)
    assert not np.array_equal(want, want.astype(np.float32))        # true float64 poses
    assert np.abs(want - np.eye(4)).max() > 1.0                     # ... of a drive, not identities


_LIVE = r"""
import sys, types
import numpy as np
ref, calib, poses, out = sys.argv[1:5]
for name in ("auxiliary", "auxiliary.laserscan", "auxiliary.laserscanvis"):   # the parsers need neither
    sys.modules[name] = types.ModuleType(name)
sys.modules["auxiliary.laserscanvis"].LaserScanVis = None
try:
    import yaml
except ImportError:
    sys.modules["yaml"] = types.ModuleType("yaml")
sys.path.insert(0, ref)
import lidar_deform as ld
c = ld.parse_calibration(calib)
np.savez(out, poses=np.stack(ld.parse_poses(poses, c)), **{"calib_" + k: v for k, v in c.items()})
"""


def test_parsers_are_bit_identical_to_the_live_reference(tmp_path):
    """same interpreter, same numpy: the reference's own functions on the fixture's text files"""
    if not os.path.isfile(os.path.join(REF, "lidar_deform.py")):
        pytest.skip("the reference checkout is absent (LT_REFERENCE)")
    from lidar_transfer_amd.ingest import parse_calibration, parse_poses
    g = gold()
    calib_path, poses_path = _write_text_files(g, str(tmp_path))
    out = str(tmp_path / "live.npz")
    res = subprocess.run([sys.executable, "-c", _LIVE, REF, calib_path, poses_path, out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    live = np.load(out)
    calib = parse_calibration(calib_path)
    assert sorted("calib_" + k for k in calib) == sorted(k for k in live.files if k.startswith("calib_"))
    for k, v in calib.items():
        assert np.array_equal(v.view(np.int64), live["calib_" + k].view(np.int64)), k
    poses = np.stack(parse_poses(poses_path, calib))
    assert poses.shape == live["poses"].shape and np.array_equal(poses.view(np.int64), live["poses"].view(np.int64))


def test_the_five_rules_restated_in_numpy_give_the_references_prepared_clouds():
    """kept set, order, remissions and labels exactly; points within the bound of transform_bound"""
    g = gold()
    raw, poses = raw_scans(g), g["poses"]
    for k, (xyzr, label) in enumerate(raw):   # what the fixture promises
        l = label & 0xFFFF
        assert (label >> 16).min() > 0 and all(int((l == c).sum()) >= 100 for c in (0, 1, 252, 253)), k
    n_diff = n_all = 0
    for c in cases(g):
        tag = c["tag"]
        assert np.allclose(np.linalg.inv(poses[c["idx"]]), c["back"], rtol=0, atol=1e-12)
        plain, qs, hs = restate(raw, poses, c["slots"], c["back"], c["ignore"], c["moving"], c["merged"], world=True)
        assert len(plain) == (1 if c["merged"] else c["nscans"])
        ref = reference_points(g, tag, plain)
        for k, ((p, r, l), want, q, (h, absA)) in enumerate(zip(plain, ref, qs, hs)):
            assert sha(r) == str(g[f"{tag}_prep_sha"][k][1]), f"{tag}: remissions of cloud {k}"
            assert sha(l) == str(g[f"{tag}_prep_sha"][k][2]), f"{tag}: labels of cloud {k}"
            assert l.max() <= 0xFFFF and not np.isin(l, c["ignore"]).any()
            bound = transform_bound(h, absA, q, c["back"])
            err = np.abs(p - want)
            assert (err <= bound).all(), (tag, k, float((err / bound).max()))
            n_diff += int((p.view(np.int64) != want.view(np.int64)).any(1).sum())
            n_all += len(p)
        if c["nscans"] > 1 and not c["merged"]:   # moving classes stay in the primary scan only
            assert np.isin(plain[0][2], c["moving"]).any() and not any(np.isin(cl[2], c["moving"]).any() for cl in plain[1:])
    assert n_all > 100000 and n_diff > 0.4 * n_all   # the reference's dgemm does round differently: the bound is not idle


def test_long_class_lists_case_drops_classes_present_in_the_scans():
    g = gold()
    c = case_of(g, "cp3L")
    assert len(c["moving"]) == 40 and len(c["ignore"]) > 16 and 65535 in c["ignore"]
    short = case_of(g, "mm2")
    assert c["slots"] == short["slots"]
    assert int(g["cp3L_prep_n"][0]) < int(g["mm2_prep_n"][0]) - 1000   # class 50 of the secondary scans is gone


def test_native_entry_point_rejects_bad_arguments():
    """the C ABI itself: class values, slot count, missing pointers -- LT_ERR_INVALID_ARG with a message, nothing launched"""
    import ctypes as C
    from lidar_transfer_amd import _lib
    lib = _lib.load()
    rs, io = (_lib.RawScan * 1)(), (_lib.IngestOut * 1)()
    pose = (C.c_double * 16)(*np.eye(4).reshape(-1))
    one = (C.c_int * 1)(70000)
    dummy = C.c_void_p(256)   # (never dereferenced: every call below is refused before its first launch)
    assert lib.lt_ingest_scans_dev(1, rs, pose, None, one, 1, None, 0, 0, io, dummy, dummy, None) == -1
    assert b"65535" in lib.lt_last_error()
    assert lib.lt_ingest_scans_dev(0, rs, pose, None, None, 0, None, 0, 0, io, dummy, dummy, None) == -1
    assert lib.lt_ingest_scans_dev(17, rs, pose, None, None, 0, None, 0, 0, io, dummy, dummy, None) == -1
    rs[0].n = 10                                                  # points announced, no buffers
    assert lib.lt_ingest_scans_dev(1, rs, pose, None, None, 0, None, 0, 0, io, dummy, dummy, None) == -1
    assert lib.lt_ingest_scans_dev(1, rs, pose, None, None, 0, None, 0, 2, io, dummy, dummy, None) == -1   # unknown flag
