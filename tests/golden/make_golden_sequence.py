#!/usr/bin/env python3
"""Generate golden F18 -- the reference's batch loop body (lidar_deform.py:396-418 + `write`) for EVERY index of the batch
list of the synthetic sequence make_golden_ingest.py writes (the same bytes: asserted against F17 by SHA-256, so they are not
stored twice), in one process:

    number_of_scans 3, batch_interval 1, offset 0  ->  output scans 1..5 of the 8
    adaptions cp, mesh, mergemesh (ONE voxel_bounds array per run, handed to every MultiSemLaserScan as lidar_deform.py:397-401
    does), fusion in the reference's numpy mode
    targets: F17's (32, 512, +10, -30) ["t"] and the source sensor itself ["s"]

    /opt/conda/bin/python3.9 tests/golden/make_golden_sequence.py      (scikit-image 0.18.x, as make_golden_ingest.py)

Per output scan: digests and byte counts of velodyne/N.bin and labels/N.label, what `compare(scan, scans)` returns (m_iou,
m_acc, MSE) and the per-class iou of its iouEval, and the bounds array after the scan.  For all eight files the source
reference scan of lidar_deform.py:403-409 (digests of proj_range / proj_remissions / proj_label and of the black mask
`sum(proj_color) == 0`; the arrays themselves for scans 1 and 4).  nclasses is 300 as in F17's generator.  Data only.

The script ASSERTS that the fixture is fit for a bit-exact test: the reference's source image equals
oracle.projection.range_projection(method="old", remove=True) and no cell's two nearest points tie (numpy's argsort leaves
equal depths unspecified); at most 64 label values present per compared scan.  If a seed fails that, change the seed."""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden  # noqa: E402
import make_golden_deform_mesh as gm  # noqa: E402
import make_golden_ingest as gi  # noqa: E402
from oracle import projection as op  # noqa: E402

NSCANS, INTERVAL, NCLASSES = 3, 1, 300
TARGETS = dict(t=gi.TARGET, s=gi.SOURCE)
ADAPTIONS = ("cp", "mesh", "mergemesh")
STORED_SOURCE = (1, 4)


def source_scan(ls, scan_name, label_name):
    """lidar_deform.py:396, :403-409"""
    H, W, fu, fd = gi.SOURCE
    scan = ls.SemLaserScan(H, W, NCLASSES, gi.COLOR_DICT)
    scan.open_scan(scan_name, fu, fd)
    scan.open_label(label_name)
    scan.colorize()
    scan.remove_classes(gi.IGNORE)
    scan.do_range_projection(fu, fd, remove=True)
    scan.do_label_projection()
    return scan


def fit_source(tag, scan, scan_name, label_name):
    H, W, fu, fd = gi.SOURCE
    xyzr = np.fromfile(scan_name, np.float32).reshape(-1, 4)
    l = np.fromfile(label_name, np.uint32) & 0xFFFF
    keep = ~np.isin(l, gi.IGNORE)
    o = op.range_projection(xyzr[keep, :3], xyzr[keep, 3], H, W, fu, fd, remove=True, method="old")
    assert np.array_equal(o["index"], scan.proj_idx) and np.array_equal(o["range"].view(np.int32), scan.proj_range.view(np.int32)), \
        f"{tag}: change the seed"
    cell = o["py"].astype(np.int64) * W + o["px"]
    order = np.lexsort((o["unproj_range"], cell))
    c, d = cell[order], o["unproj_range"][order]
    tie = (c[1:] == c[:-1]) & (d[1:] == d[:-1])
    first = np.r_[True, c[1:] != c[:-1]]
    assert not (tie & first[:-1]).any(), f"{tag}: the two nearest points of a cell tie: change the seed"
    assert np.array_equal(scan.proj_label, op.label_projection(o["index"], l[keep][o["kept"]]))


def main():
    try:
        from skimage import measure
    except ImportError:
        raise SystemExit("make_golden_sequence.py needs scikit-image 0.18.x: /opt/conda/bin/python3.9 has it")
    if not hasattr(measure, "marching_cubes_lewiner"):
        measure.marching_cubes_lewiner = lambda vol, level=0.0, **kw: measure.marching_cubes(vol, level=level, method="lewiner", **kw)
    ls, fl = make_golden.import_reference(stub_skimage=False)
    assert fl.FUSION_GPU_MODE == 0, "the fixture is made by the reference's numpy fusion mode"
    vis = types.ModuleType("auxiliary.laserscanvis")
    vis.LaserScanVis = None
    sys.modules["auxiliary.laserscanvis"] = vis
    import lidar_deform as ld
    orig_integrate = fl.TSDFVolume.integrate
    fl.TSDFVolume.integrate = lambda self, c, d, r, pose, obs_weight=1.: orig_integrate(self, c, d, r, np.eye(4), obs_weight=obs_weight)
    ious = []
    orig_iou = ls.iouEval.getIoU

    def spy_iou(self):
        m, iou = orig_iou(self)
        ious.append(np.array(iou))
        return m, iou
    ls.iouEval.getIoU = spy_iou
    sha = gm.sha
    f17 = np.load(os.path.join(HERE, "f17_ingest.npz"))
    H, W, fu, fd = gi.SOURCE
    out = dict(nscans=NSCANS, batch_interval=INTERVAL, nclasses=NCLASSES, source=np.array(gi.SOURCE), targets=np.array(list(TARGETS)),
               ignore=np.array(gi.IGNORE), moving=np.array(gi.MOVING), mesh_bnds=gi.MESH_BNDS.copy(), mesh_voxel=gi.MESH_VOXEL,
               mm_bnds=gi.MM_BNDS.copy(), mm_voxel=gi.MM_VOXEL, stored_source=np.array(STORED_SOURCE))
    for k, t in TARGETS.items():
        out[f"target_{k}"] = np.array(t)
    with tempfile.TemporaryDirectory() as d:
        seq = gi.write_sequence(ls, d)
        scan_names = sorted(os.path.join(dp, f) for dp, dn, fn in os.walk(os.path.join(seq, "velodyne")) for f in fn)
        label_names = sorted(os.path.join(dp, f) for dp, dn, fn in os.walk(os.path.join(seq, "labels")) for f in fn)
        poses = ld.parse_poses(os.path.join(seq, "poses.txt"), ld.parse_calibration(os.path.join(seq, "calib.txt")))
        n = len(scan_names)
        assert n == gi.N_SCANS_SEQ == int(f17["n_scans_seq"])
        for k in range(n):   # the input IS F17's
            assert sha(np.fromfile(scan_names[k], np.uint8)) == sha(f17[f"scan{k}"]) and \
                sha(np.fromfile(label_names[k], np.uint8)) == sha(f17[f"label{k}"]), "the sequence differs from F17's: regenerate F17 first"
        assert np.array_equal(np.stack(poses), f17["poses"])
        indices = list(range(NSCANS // 2, n - (NSCANS - 1), INTERVAL))   # lidar_deform.py:385-390, :457-459
        assert indices == [1, 2, 3, 4, 5]
        out["indices"] = np.array(indices)
        sources = []
        for k in range(n):
            scan = source_scan(ls, scan_names[k], label_names[k])
            fit_source(f"source scan {k}", scan, scan_names[k], label_names[k])
            black = (np.sum(scan.proj_color, axis=2) == 0).astype(np.uint8)
            imgs = (np.asarray(scan.proj_range, np.float32), np.asarray(scan.proj_remissions, np.float32),
                    np.asarray(scan.proj_label, np.int32), black)
            out[f"src{k}_sha"] = np.array([sha(a) for a in imgs])
            if k in STORED_SOURCE:
                for name, a in zip(("range", "rem", "label", "black"), imgs):
                    out[f"src{k}_{name}"] = a
            sources.append(scan)
        cwd = os.getcwd()
        for tkey, (tH, tW, tfu, tfd) in TARGETS.items():
            for adaption in ADAPTIONS:
                bnds = gi.MM_BNDS.copy() if adaption == "mergemesh" else gi.MESH_BNDS.copy()   # ONE array per run
                voxel = gi.MM_VOXEL if adaption == "mergemesh" else gi.MESH_VOXEL
                for idx in indices:
                    tag = f"{tkey}_{adaption}_{idx}"
                    scan = source_scan(ls, scan_names[idx], label_names[idx])   # (compare() does not modify it: overwrite = False)
                    ms = ls.MultiSemLaserScan(gm.sensor("src", H, W, fu, fd), gm.sensor("tgt", tH, tW, tfu, tfd), NSCANS, NCLASSES,
                                              list(gi.IGNORE), list(gi.MOVING), color_dict=gi.COLOR_DICT, transformation=None,
                                              preserve_float=False, voxel_size=voxel, vol_bnds=bnds)
                    ms.open_multiple_scans(scan_names, label_names, poses, idx)
                    with tempfile.TemporaryDirectory() as w:
                        os.chdir(w)
                        try:
                            ms.deform(adaption, poses, idx)
                        finally:
                            os.chdir(cwd)
                        assert tH == H and tW == W                              # lidar_deform.py:416
                        tl = ms.merged.proj_label if adaption == "cp" else ms.label_image
                        n_present = len(np.union1d(np.unique(scan.proj_label), np.unique(tl)))
                        assert n_present <= 64, f"{tag}: {n_present} label values: change the seed"
                        del ious[:]
                        _, _, _, m_iou, m_acc, MSE = ls.compare(scan, ms)
                        os.makedirs(os.path.join(w, "velodyne"))
                        os.makedirs(os.path.join(w, "labels"))
                        ms.write(w, idx)
                        b = np.fromfile(os.path.join(w, "velodyne", str(idx).zfill(6) + ".bin"), np.uint8)
                        l = np.fromfile(os.path.join(w, "labels", str(idx).zfill(6) + ".label"), np.uint8)
                    out[f"{tag}_bin_sha"], out[f"{tag}_label_sha"] = sha(b), sha(l)
                    out[f"{tag}_n_bin"], out[f"{tag}_n_label"] = b.size, l.size
                    out[f"{tag}_m_iou"], out[f"{tag}_m_acc"], out[f"{tag}_MSE"] = float(m_iou), float(m_acc), float(MSE)
                    out[f"{tag}_iou"] = ious[-1]
                    out[f"{tag}_n_present"] = n_present
                    out[f"{tag}_bnds_after"] = np.array(bnds)
                    print(f"## {tag}: IoU {float(m_iou)!r} Acc {float(m_acc)!r} MSE {float(MSE)!r} present {n_present} points "
                          f"{b.size // 16} bounds after {np.array(bnds).reshape(-1).tolist()}", flush=True)
    path = os.path.join(HERE, "f18_sequence.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("f18_sequence.npz", size, "bytes")
    assert size <= 1 << 20, "a committed file stays below 1 MiB"


if __name__ == "__main__":
    main()
