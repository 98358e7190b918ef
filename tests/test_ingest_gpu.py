"""The device ingest stage (lt_ingest_scans_dev, lidar_transfer_amd.ingest) against golden F17 -- the reference's
`open_multiple_scans` + `deform` + `write` run from the files of a synthetic sequence (tests/golden/make_golden_ingest.py).
Reads tests/golden/ only; the numpy restatement of the kernel's five rules lives in tests/test_ingest_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_ingest_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu


def _source(g, **kw):
    from lidar_transfer_amd.ingest import SequenceSource
    raw = cpu.raw_scans(g)
    return SequenceSource(scans=[x for x, _ in raw], labels=[l for _, l in raw], poses=g["poses"], **kw)


def _ingest(g, src, c):
    from lidar_transfer_amd.ingest import ScanIngest
    return ScanIngest(src, (c["nscans"], c["ignore"], c["moving"]))


def _np(cloud):
    p, r, l = cloud
    return p.cpu().numpy(), r.cpu().numpy(), l.cpu().numpy().view(np.uint32)


def _sensors(g):
    s, t = g["source"], g["target"]
    return (int(s[0]), int(s[1]), float(s[2]), float(s[3])), (int(t[0]), int(t[1]), float(t[2]), float(t[3]))


def _write_sequence(g, d):
    seq = os.path.join(d, "sequences", "00")
    os.makedirs(os.path.join(seq, "velodyne"))
    os.makedirs(os.path.join(seq, "labels"))
    g["calib_txt"].tofile(os.path.join(seq, "calib.txt"))
    g["poses_txt"].tofile(os.path.join(seq, "poses.txt"))
    for k in range(int(g["n_scans_seq"])):
        g[f"scan{k}"].tofile(os.path.join(seq, "velodyne", f"{k:06d}.bin"))
        g[f"label{k}"].tofile(os.path.join(seq, "labels", f"{k:06d}.label"))
    return d


@pytest.mark.parametrize("merged", [True, False])
def test_prepare_equals_the_restatement_bit_for_bit_and_the_reference_within_the_bound(merged):
    """every case of the fixture, as one merged cloud and per slot, fed the golden's poses and inv(poses[idx]): points,
    remissions, labels, order and counts equal the plain-order numpy restatement exactly (points as int64 views); against the
    REFERENCE's prepared points (where the fixture holds them in this form) within test_ingest_cpu.transform_bound"""
    import torch
    g = cpu.gold()
    raw, poses = cpu.raw_scans(g), g["poses"]
    src = _source(g)
    n_ref = 0
    for c in cpu.cases(g):
        ing = _ingest(g, src, c)
        want, qs, hs = cpu.restate(raw, poses, c["slots"], c["back"], c["ignore"], c["moving"], merged, world=True)
        got = ing.prepare(c["idx"], merged=merged, exact=True, back=c["back"])
        torch.cuda.synchronize()
        assert len(got) == len(want) == (1 if merged else c["nscans"])
        for k, (gc, wc) in enumerate(zip(got, want)):
            p, r, l = _np(gc)
            assert p.shape == wc[0].shape and p.dtype == np.float64, (c["tag"], k, p.shape, wc[0].shape)
            assert np.array_equal(p.view(np.int64), wc[0].view(np.int64)), (c["tag"], k)
            assert np.array_equal(r.view(np.int32), wc[1].view(np.int32)) and np.array_equal(l, wc[2]), (c["tag"], k)
        if merged == c["merged"]:
            ref = cpu.reference_points(g, c["tag"], want)
            for k, (gc, rp, q, (h, absA)) in enumerate(zip(got, ref, qs, hs)):
                p = gc[0].cpu().numpy()
                bound = cpu.transform_bound(h, absA, q, c["back"])
                assert (np.abs(p - rp) <= bound).all(), (c["tag"], k)
                n_ref += len(p)
        # world coordinates: the first transform alone
        if c["tag"] in ("cp3", "mesh3"):
            world = ing.prepare(c["idx"], merged=merged, exact=True, back=False)
            for gc, q in zip(world, qs):
                assert np.array_equal(gc[0].cpu().numpy().view(np.int64), q.view(np.int64)), c["tag"]
    assert n_ref > 30000
    src.close()


def test_padded_clouds_carry_origin_points_behind_the_kept_ones():
    """exact=False: capacity-length tensors, the kept points first, then (0, 0, 0) / remission 0 / label 0"""
    import torch
    g = cpu.gold()
    src = _source(g)
    for tag, merged in (("cp3", True), ("mesh4", False), ("cp3L", True)):
        c = cpu.case_of(g, tag)
        ing = _ingest(g, src, c)
        exact = ing.prepare(c["idx"], merged=merged, exact=True, back=c["back"])
        padded = ing.prepare(c["idx"], merged=merged, back=c["back"])
        torch.cuda.synchronize()
        caps = [sum(len(g[f"label{s}"]) // 4 for s in c["slots"])] if merged else [len(g[f"label{s}"]) // 4 for s in c["slots"]]
        for e, p, cap in zip(exact, padded, caps):
            n = e[0].shape[0]
            assert p[0].shape[0] == cap > n
            for a, b in zip(e, p):
                assert torch.equal(a, b[:n]) and float(b[n:].abs().sum()) == 0.0
    src.close()


def _restated_reference_check(got, g, tag):
    """the criteria of tests/test_deform_gpu.py::_check_against_reference_scan on the fixture's digests"""
    import torch
    torch.cuda.synchronize()
    assert got["n_verts"] == int(g[f"{tag}_n_verts"]) and got["n_faces"] == int(g[f"{tag}_n_faces"]), \
        (tag, got["n_verts"], got["n_faces"], int(g[f"{tag}_n_verts"]), int(g[f"{tag}_n_faces"]))
    assert np.array_equal(got["range"].cpu().numpy().view(np.int32), g[f"{tag}_proj_range"].view(np.int32)), tag
    assert cpu.sha(got["range"].cpu().numpy()) == str(g[f"{tag}_img_sha"][0]), tag
    assert cpu.sha(got["rem"].cpu().numpy()) == str(g[f"{tag}_img_sha"][1]), tag
    assert cpu.sha(got["label"].cpu().numpy().astype(np.int32)) == str(g[f"{tag}_img_sha"][2]), tag
    assert cpu.sha(got["endpoints"].cpu().numpy()) == str(g[f"{tag}_back_points_sha"]), tag
    assert got["bin"].shape[0] == int(g[f"{tag}_n_written"]), tag
    assert cpu.sha(got["bin"].cpu().numpy()) == str(g[f"{tag}_bin_sha"]), tag
    assert cpu.sha(got["label_file"].cpu().numpy()) == str(g[f"{tag}_label_sha"]), tag
    assert int(g[f"{tag}_n_written"]) > 1500 and (g[f"{tag}_proj_range"] > 0).sum() > 1500


def test_deform_from_the_raw_bytes_equals_the_references_run_from_the_same_files(tmp_path):
    """`DeviceDeform(fusion="numpy").deform(adaption, ingest, idx)` from the sequence's FILES: mesh sizes, range / label /
    remission / endpoint images and the bytes of velodyne/N.bin and labels/N.label identical to the reference's
    `open_multiple_scans` + `deform` + `write`; `vol_bnds` after every mergemesh scan identical in value and dtype; cp:
    index, range, bytes.  The kept counts never visit the host (padded clouds)."""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest, SequenceSource
    g = cpu.gold()
    source, target = _sensors(g)
    src = SequenceSource(_write_sequence(g, str(tmp_path)), "00", poses=g["poses"])
    assert [os.path.basename(n) for n in src.scan_names] == [f"{k:06d}.bin" for k in range(8)]
    mm_bnds = g["mm_bnds"].copy()
    dds = dict(cp=DeviceDeform(source, target, None, fusion="numpy"),
               mesh=DeviceDeform(source, target, g["mesh_bnds"].copy(), float(g["mesh_voxel"]), fusion="numpy"),
               mergemesh=DeviceDeform(source, target, mm_bnds, float(g["mm_voxel"]), fusion="numpy", mesh_volume=False))
    for c in cpu.cases(g):
        tag, dd = c["tag"], dds[c["adaption"]]
        ing = ScanIngest(src, (c["nscans"], c["ignore"], c["moving"]))
        got = dd.deform(c["adaption"], ing, c["idx"])
        torch.cuda.synchronize()
        if c["adaption"] == "cp":
            assert cpu.sha(got["index"].cpu().numpy()) == str(g[f"{tag}_index_sha"]), tag
            assert np.array_equal(got["range"].cpu().numpy().view(np.int32), g[f"{tag}_proj_range"].view(np.int32)), tag
            assert got["bin"].shape[0] == int(g[f"{tag}_n_written"]) > 1500, tag
            assert cpu.sha(got["bin"].cpu().numpy()) == str(g[f"{tag}_bin_sha"]), tag
            assert cpu.sha(got["label_file"].cpu().numpy()) == str(g[f"{tag}_label_sha"]), tag
            continue
        if c["adaption"] == "mergemesh":
            assert got["vol_dim"] == tuple(int(x) for x in g[f"{tag}_vol_dim"]), (tag, got["vol_dim"])
            assert np.array_equal(mm_bnds, g[f"{tag}_bnds_after"]) and mm_bnds.dtype == g[f"{tag}_bnds_after"].dtype, tag
        _restated_reference_check(got, g, tag)
        v, f, cc, r = dd.mesh_obj.renumber().tensors()
        assert [cpu.sha(v.cpu().numpy()), cpu.sha(f.cpu().numpy()), cpu.sha(cc.cpu().numpy().astype(np.uint8)),
                cpu.sha(r.cpu().numpy())] == [str(x) for x in g[f"{tag}_mesh_sha"]], tag
    for dd in dds.values():
        dd.close()
    src.close()


def test_padded_and_exact_clouds_give_identical_scans():
    """`mergemesh` and `cp` fed the exact-length clouds and the capacity-length ones (depth-0 tail): byte-identical"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    g = cpu.gold()
    source, target = _sensors(g)
    src = _source(g)
    c = cpu.case_of(g, "mm0")
    ing = _ingest(g, src, c)
    outs = []
    for exact in (True, False):
        clouds = ing.prepare(c["idx"], merged=True, exact=exact)
        with DeviceDeform(source, target, g["mm_bnds"].copy(), float(g["mm_voxel"]), mesh_volume=False) as dd:
            got = dd.mergemesh(clouds)
            torch.cuda.synchronize()
            outs.append({k: got[k].cpu().numpy() for k in ("range", "rem", "label", "endpoints", "tri", "bin", "label_file")})
            outs[-1]["dim"] = np.array(got["vol_dim"])
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    assert outs[0]["bin"].shape[0] > 1500
    for tag in ("cp4", "cp3L"):
        c = cpu.case_of(g, tag)
        ing = _ingest(g, src, c)
        res = []
        with DeviceDeform(source, target, None) as dd:
            for exact in (True, False):
                got = dd.cp(ing.prepare(c["idx"], merged=True, exact=exact))
                torch.cuda.synchronize()
                res.append({k: got[k].cpu().numpy() for k in ("index", "range", "rem", "label", "back_points", "bin", "label_file")})
        for k in res[0]:
            assert res[0][k].tobytes() == res[1][k].tobytes(), (tag, k)
        assert cpu.sha(res[1]["bin"]) == str(g[f"{tag}_bin_sha"])
    src.close()


def test_mergemesh_scans_in_flight_equal_the_serial_run():
    """the three consecutive output scans through FusionScanPipeline.submit_mergemesh(ingest.prepare(idx, merged=True)),
    all submitted before the first is collected, against DeviceDeform.deform scan after scan"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.pipeline import FusionScanPipeline
    g = cpu.gold()
    source, target = _sensors(g)
    src = _source(g)
    tags = ("mm0", "mm1", "mm2")
    c0 = cpu.case_of(g, tags[0])
    ing = _ingest(g, src, c0)
    serial, b = [], g["mm_bnds"].copy()
    with DeviceDeform(source, target, b, float(g["mm_voxel"]), mesh_volume=False) as dd:
        for tag in tags:
            got = dd.deform("mergemesh", ing, int(g[f"{tag}_idx"]), pack=False)
            torch.cuda.synchronize()
            serial.append(({k: got[k].cpu().numpy() for k in ("range", "rem", "label", "endpoints", "tri")}, got["vol_dim"], b.copy()))
            assert got["vol_dim"] == tuple(int(x) for x in g[f"{tag}_vol_dim"]) and np.array_equal(b, g[f"{tag}_bnds_after"])
    b2 = g["mm_bnds"].copy()
    rays = create_rays_device(target[2], target[3], target[0], target[1], device=0)
    with FusionScanPipeline(b2, float(g["mm_voxel"]), target[2], target[3], rays, target[0], chains=3, device=0,
                            label_image=True, source_hw=(source[0], source[1]), fixed_volume=False) as pipe:
        tickets = [pipe.submit_mergemesh(ing.prepare(int(g[f"{tag}_idx"]), merged=True)) for tag in tags]
        for (want, dim, after), t in zip(serial, tickets):
            got = pipe.wait(t)
            assert tuple(got["vol_dim"]) == tuple(dim)
            assert np.array_equal(np.array(got["vol_bnds_after"]).reshape(3, 2), after.astype(np.float64))
            for k, name in (("range", "range"), ("rem", "endrem"), ("label", "endcolors"), ("endpoints", "endpoints"), ("tri", "tri")):
                assert got[name].cpu().numpy().reshape(-1).tobytes() == want[k].reshape(-1).tobytes(), k
        pipe.flush()
        assert np.array_equal(b2, serial[-1][2]) and b2.dtype == b.dtype
    src.close()


def test_every_raw_file_is_uploaded_once_over_consecutive_output_scans(tmp_path):
    """counted, not timed: output scans 1, 3, 5 with three scans each read scans 0..6 -- seven uploads, two cache hits, and a
    second pass over the same output scans uploads nothing; a cache of ONE scan has to upload again"""
    import torch
    from lidar_transfer_amd.ingest import ScanIngest, SequenceSource
    g = cpu.gold()
    src = SequenceSource(_write_sequence(g, str(tmp_path)), "00", poses=g["poses"])
    ing = ScanIngest(src, (3, [0, 1], [252, 253]))
    for idx in (1, 3, 5):
        ing.prepare(idx, merged=True)
    torch.cuda.synchronize()
    assert src.stats["uploads"] == 7 and src.stats["hits"] == 2, src.stats
    assert sorted(src.upload_counts) == list(range(7)) and set(src.upload_counts.values()) == {1}
    assert src.stats["bytes"] == sum(g[f"scan{k}"].size + g[f"label{k}"].size for k in range(7))
    first = [ing.prepare(idx, merged=True, exact=True) for idx in (1, 3, 5)]
    assert src.stats["uploads"] == 7 and src.stats["hits"] == 11
    src.close()
    small = SequenceSource(_write_sequence(g, str(tmp_path / "again")), "00", poses=g["poses"], cache_scans=1)
    ing2 = ScanIngest(small, (3, [0, 1], [252, 253]))
    second = [ing2.prepare(idx, merged=True, exact=True) for idx in (1, 3, 5)]
    torch.cuda.synchronize()
    assert small.stats["uploads"] > 7          # (scans evicted while still needed: correct, only slower)
    for a, b in zip(first, second):
        for x, y in zip(a[0], b[0]):
            assert torch.equal(x, y)
    small.close()


def test_error_paths_raise_before_any_device_work():
    from lidar_transfer_amd.ingest import ScanIngest, SequenceSource
    g = cpu.gold()
    raw = cpu.raw_scans(g)
    scans, labels = [x for x, _ in raw], [l for _, l in raw]
    labels[3] = labels[3][:-5]                                   # scan 3: five labels short
    src = SequenceSource(scans=scans, labels=labels, poses=g["poses"])
    ing = ScanIngest(src, (3, [0, 1], [252, 253]))
    with pytest.raises(ValueError, match="same number of points"):
        ing.prepare(2, merged=True)                              # slots 2, 1, 3
    with pytest.raises(ValueError, match="same number of points"):
        ing.prepare(4, merged=False)
    assert src.stats["uploads"] == 0
    for idx in (0, 7, -1, 8):                                    # a neighbour before the first / after the last scan
        with pytest.raises(IndexError):
            ing.prepare(idx, merged=True)
    ing4 = ScanIngest(src, (4, [], []))
    with pytest.raises(IndexError):
        ing4.prepare(1, merged=True)                             # needs scan -1
    assert src.stats["uploads"] == 0
    for bad in ([65536], [-1], [0, 1, 70000]):
        with pytest.raises(ValueError, match="0..65535"):
            ScanIngest(src, (3, bad, []))
        with pytest.raises(ValueError, match="0..65535"):
            ScanIngest(src, (3, [], bad))
    with pytest.raises(ValueError):
        ScanIngest(src, (0, [], []))
    ing.prepare(6, merged=True)                                  # slots 6, 5, 7: fine
    assert src.stats["uploads"] == 3
    src.close()
