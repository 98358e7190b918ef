"""`SequenceTransfer` and `python -m lidar_transfer_amd` against golden F18 -- the reference's own loop body (source scan,
`open_multiple_scans`, `deform`, `compare`, `write`) over the batch list of F17's synthetic sequence, made by
tests/golden/make_golden_sequence.py in the reference's numpy fusion mode -- and, in the default `cuda` fusion mode (for which
no reference-made golden can exist on this hardware), three runs against each other: three chains, one chain, and a loop
written here from the parent's public calls."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_evaluate_cpu as ev  # noqa: E402
import test_ingest_cpu as cpu  # noqa: E402
import test_sequence_cpu as sc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(g17, **kw):
    from lidar_transfer_amd.ingest import SequenceSource
    raw = cpu.raw_scans(g17)
    return SequenceSource(scans=[x for x, _ in raw], labels=[l for _, l in raw], poses=g17["poses"], **kw)


def _target(g18, tkey):
    t = g18[f"target_{tkey}"]
    return int(t[0]), int(t[1]), float(t[2]), float(t[3])


def _file_sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _files(out_dir, idx, seq="00"):
    from lidar_transfer_amd.sequence import output_paths
    return output_paths(str(out_dir), seq, idx)


def _check_files(g18, tag, out_dir, idx):
    b, l = _files(out_dir, idx)
    assert os.path.getsize(b) == int(g18[f"{tag}_n_bin"]) and os.path.getsize(l) == int(g18[f"{tag}_n_label"]), tag
    assert _file_sha(b) == str(g18[f"{tag}_bin_sha"]) and _file_sha(l) == str(g18[f"{tag}_label_sha"]), tag


def _run(g17, g18, adaption, tkey, out_dir, chains=1, fusion="numpy", **run_kw):
    from lidar_transfer_amd.sequence import SequenceTransfer
    src = _source(g17)
    with SequenceTransfer(src, sc.approach_for(g18, adaption), ev.SOURCE, _target(g18, tkey), out_dir=str(out_dir) if out_dir else None,
                          chains=chains, fusion=fusion, nclasses=int(g18["nclasses"])) as tr:
        recs = list(tr.run(**run_kw))
        summary = tr.summary
    src.close()
    return recs, summary


def test_source_scans_of_the_sequence_are_bit_identical_to_the_references():
    import torch
    from lidar_transfer_amd.evaluate import Evaluator
    g17, g18 = cpu.gold(), sc.gold18()
    src = _source(g17)
    with Evaluator(ev.SOURCE, [int(x) for x in g18["ignore"]], ev.color_lut(ev.COLOR_DICT)) as e:
        for k in range(8):
            im = e.source_scan(*src.raw(k))
            torch.cuda.synchronize()
            got = [cpu.sha(im[n].cpu().numpy()) for n in ("range", "rem", "label", "black")]
            assert got == [str(x) for x in g18[f"src{k}_sha"]], k
            assert int(im["bad_labels"][0]) == 0
    src.close()


@pytest.mark.parametrize("tkey", ["t", "s"])
@pytest.mark.parametrize("adaption", ["cp", "mesh", "mergemesh"])
def test_one_chain_in_numpy_mode_reproduces_the_references_sequence(adaption, tkey, tmp_path):
    """every written file byte-identical (SHA-256), m_iou / m_acc within 1e-12 and MSE within 1e-6 * MSE + 1e-9 of the
    reference's `compare()`, mergemesh's bounds after every scan equal"""
    g17, g18 = cpu.gold(), sc.gold18()
    recs, summary = _run(g17, g18, adaption, tkey, tmp_path)
    assert [r["idx"] for r in recs] == [1, 2, 3, 4, 5] and summary["scans"] == 5 and not any(r["skipped"] for r in recs)
    for r in recs:
        tag = f"{tkey}_{adaption}_{r['idx']}"
        _check_files(g18, tag, tmp_path, r["idx"])
        assert r["n_points"] * 16 == int(g18[f"{tag}_n_bin"])
        sc.metrics_close(r, g18, tag)
        if adaption == "mergemesh":
            assert np.array_equal(r["bnds_after"], g18[f"{tag}_bnds_after"].astype(np.float64)), tag
    if adaption == "mergemesh":
        assert summary["mm_stats"]["scans"] == 5


@pytest.mark.parametrize("adaption", ["mesh", "mergemesh"])
def test_three_chains_in_numpy_mode_reproduce_the_references_sequence(adaption, tmp_path):
    g17, g18 = cpu.gold(), sc.gold18()
    recs, summary = _run(g17, g18, adaption, "t", tmp_path, chains=3)
    assert [r["idx"] for r in recs] == [1, 2, 3, 4, 5] and summary["chains"] == 3
    for r in recs:
        tag = f"t_{adaption}_{r['idx']}"
        _check_files(g18, tag, tmp_path, r["idx"])
        sc.metrics_close(r, g18, tag)
        if adaption == "mergemesh":
            assert np.array_equal(r["bnds_after"], g18[f"{tag}_bnds_after"].astype(np.float64)), tag


@pytest.mark.parametrize("adaption", ["mesh", "mergemesh"])
def test_default_fusion_three_chains_one_chain_and_the_hand_written_loop_agree_byte_for_byte(adaption, tmp_path):
    """the loop below uses the parent's public calls only (ScanIngest.prepare + DeviceDeform.mesh / mergemesh + write), which
    tests/test_default_chain_gpu.py pins to tests/oracle_chain.py"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    g17, g18 = cpu.gold(), sc.gold18()
    target = _target(g18, "t")
    a = sc.approach_for(g18, adaption)
    hand = tmp_path / "hand" / "sequences" / "00"
    src = _source(g17)
    ing = ScanIngest(src, a)
    with DeviceDeform(ev.SOURCE, target, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=adaption == "mesh") as dd:
        for idx in a.scan_indices(len(src)):
            clouds = ing.prepare(idx, merged=adaption != "mesh")
            out = dd.mesh(clouds) if adaption == "mesh" else dd.mergemesh(clouds)
            torch.cuda.synchronize()
            DeviceDeform.write(out, str(hand), idx)
    src.close()
    r3, s3 = _run(g17, g18, adaption, "t", tmp_path / "c3", chains=3, fusion="cuda")
    r1, s1 = _run(g17, g18, adaption, "t", tmp_path / "c1", chains=1, fusion="cuda")
    for idx in (1, 2, 3, 4, 5):
        want = [_file_sha(p) for p in _files(tmp_path / "hand", idx)]
        assert [_file_sha(p) for p in _files(tmp_path / "c3", idx)] == want, idx
        assert [_file_sha(p) for p in _files(tmp_path / "c1", idx)] == want, idx
        assert os.path.getsize(_files(tmp_path / "hand", idx)[0]) > 16 * 1500
    for a3, a1 in zip(r3, r1):                      # the records too, bit for bit
        assert a3["idx"] == a1["idx"] and a3["n_points"] == a1["n_points"]
        assert a3["m_iou"] == a1["m_iou"] and a3["m_acc"] == a1["m_acc"] and a3["MSE"] == a1["MSE"]
    if adaption == "mergemesh":
        assert s3["mm_stats"]["scans"] == s1["mm_stats"]["scans"] == 5   # (waited / rerun may differ: no byte depends on them)


@pytest.mark.parametrize("adaption", ["mesh", "mergemesh"])
def test_resume_rewrites_only_the_missing_scans(adaption, tmp_path):
    g17, g18 = cpu.gold(), sc.gold18()
    _run(g17, g18, adaption, "t", tmp_path)
    gone = (2, 4)
    for idx in gone:
        os.remove(_files(tmp_path, idx)[0] if idx == 2 else _files(tmp_path, idx)[1])      # one file of the pair is enough
    before = {idx: [os.stat(p).st_mtime_ns for p in _files(tmp_path, idx)] for idx in (1, 3, 5)}
    recs, _ = _run(g17, g18, adaption, "t", tmp_path, resume=True)
    assert [r["skipped"] for r in recs] == [True, False, True, False, True]
    for idx in (1, 2, 3, 4, 5):
        _check_files(g18, f"t_{adaption}_{idx}", tmp_path, idx)      # mergemesh: scans 2 and 4 saw the replayed bounds
    assert {idx: [os.stat(p).st_mtime_ns for p in _files(tmp_path, idx)] for idx in (1, 3, 5)} == before
    assert recs[0]["n_points"] * 16 == int(g18[f"t_{adaption}_1_n_bin"]) and recs[0]["m_iou"] is None
    sc.metrics_close(recs[1], g18, f"t_{adaption}_2")


def test_small_source_cache_is_refused_with_a_clear_error():
    from lidar_transfer_amd.sequence import SequenceTransfer
    g17, g18 = cpu.gold(), sc.gold18()
    src = _source(g17, cache_scans=4)
    with pytest.raises(ValueError, match="cache_scans"):
        SequenceTransfer(src, sc.approach_for(g18, "mesh"), ev.SOURCE, _target(g18, "t"), chains=3)
    src.close()


def test_cli_in_a_child_process_writes_the_references_files_and_prints_its_lines(tmp_path):
    import yaml
    g17, g18 = cpu.gold(), sc.gold18()
    ds, out = tmp_path / "ds", tmp_path / "out"
    seq = ds / "sequences" / "00"
    os.makedirs(seq / "velodyne")
    os.makedirs(seq / "labels")
    os.makedirs(out)
    g17["calib_txt"].tofile(str(seq / "calib.txt"))
    g17["poses_txt"].tofile(str(seq / "poses.txt"))
    for k in range(8):
        g17[f"scan{k}"].tofile(str(seq / "velodyne" / f"{k:06d}.bin"))
        g17[f"label{k}"].tofile(str(seq / "labels" / f"{k:06d}.label"))
    sensor = lambda name, s: dict(name=name, beams=int(s[0]), fov_hor=360.0, angle_res_hor=360.0 / int(s[1]), fov_up=float(s[2]),   # noqa: E731
                                  fov_down=float(s[3]))
    (ds / "config.yaml").write_text(yaml.safe_dump(sensor("src", ev.SOURCE)))
    (tmp_path / "target.yaml").write_text(yaml.safe_dump(sensor("tgt", _target(g18, "t"))))
    a = sc.approach_for(g18, "cp")
    (tmp_path / "approach.yaml").write_text(yaml.safe_dump(dict(
        adaption="cp", preserve_float=False, voxel_size=a.voxel_size, voxel_bounds=[float(x) for x in a.voxel_bounds.reshape(-1)],
        number_of_scans=3, batch_interval=1, ignore=a.ignore, moving=a.moving, transformation=[], color_map=ev.COLOR_DICT)))
    res = subprocess.run([sys.executable, "-m", "lidar_transfer_amd", "-d", str(ds), "-c", str(tmp_path / "approach.yaml"), "-t",
                          str(tmp_path / "target.yaml"), "-w", "-p", str(out), "-b", "--log", str(tmp_path / "log.jsonl")],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    vals = {k: [float(line.split(":", 1)[1]) for line in res.stdout.splitlines() if line.startswith(k + ": ")] for k in ("IoU", "Acc", "MSE")}
    rows = [json.loads(line) for line in open(tmp_path / "log.jsonl")]
    assert [r["idx"] for r in rows[:-1]] == [1, 2, 3, 4, 5] and rows[-1]["summary"]["scans"] == 5
    for k, idx in enumerate((1, 2, 3, 4, 5)):
        tag = f"t_cp_{idx}"
        _check_files(g18, tag, out, idx)
        assert vals["IoU"][k] == rows[k]["m_iou"] and vals["Acc"][k] == rows[k]["m_acc"] and vals["MSE"][k] == rows[k]["MSE"]
        sc.metrics_close(dict(m_iou=vals["IoU"][k], m_acc=vals["Acc"][k], MSE=vals["MSE"][k], iou=g18[f"{tag}_iou"]), g18, tag)
    base = out / "sequences" / "00"
    assert (base / "target.yaml").is_file() and (base / "approach.yaml").is_file()        # lidar_deform.py:446-452
