"""`SequenceTransfer` and the command line with an approach that has a `rig`, on golden F17's synthetic sequence
built as tests/test_sequence_gpu.py builds its source.  A two-head `mesh` rig writes one folder per head whose files are byte
for byte those of two single-target runs; the merged scan is the concatenation of the heads' rows in the primary scan's
frame; `--resume` redoes a scan of which one head's file is gone; a rig of ONE head is that head's single run, in its files,
its records and its totals; a rig is not evaluated and takes no target sensor."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mount_common as mc  # noqa: E402
import test_evaluate_cpu as ev  # noqa: E402
import test_ingest_cpu as cpu  # noqa: E402
import test_sequence_cpu as sc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_FRONT = mc.transformation_of(mc.POSE_EXAMPLE)


def _sensors():
    """head `roof`: golden F18's target as a sensor mapping; head `front`: a table head with a return model, mounted"""
    t = sc.gold18()["target_t"]
    H, W, fu, fd = int(t[0]), int(t[1]), float(t[2]), float(t[3])
    roof = dict(name="roof sensor", fov_up=fu, fov_down=fd, beams=H, angle_res_hor=360.0 / W, fov_hor=360)
    angles = [float(x) for x in np.round(np.linspace(fu - 1.0, fd + 1.0, 8) + np.array([0, .4, -.3, .2, 0, -.5, .3, 0]), 3)]
    front = dict(name="front sensor", fov_up=fu, fov_down=fd, beams=8, angle_res_hor=360.0 / 128, fov_hor=360, beam_model="table",
                 beam_angles=angles, return_model=dict(min_range=1.0, max_range=30.0, max_incidence=80.0, remission="lambert",
                                                       drop_rate=0.05, seed=7))
    return roof, front


def _approach(adaption="mesh", rig=True, merged=False, transformation=(), heads=("roof", "front")):
    a = sc.approach_for(sc.gold18(), adaption)
    a.transformation = list(transformation)
    if rig:
        roof, front = _sensors()
        block = dict(roof=dict(name="roof", sensor=roof), front=dict(name="front", sensor=front, transformation=T_FRONT))
        a.rig_block = [block[name] for name in heads]
        a.rig_merged = bool(merged)
    return a


def _source():
    from lidar_transfer_amd.ingest import SequenceSource
    raw = cpu.raw_scans(cpu.gold())
    return SequenceSource(scans=[x for x, _ in raw], labels=[l for _, l in raw], poses=cpu.gold()["poses"])


def _run(a, target, out_dir, chains=1, **run_kw):
    from lidar_transfer_amd.sequence import SequenceTransfer
    src = _source()
    try:
        with SequenceTransfer(src, a, ev.SOURCE, target, out_dir=str(out_dir), chains=chains,
                              nclasses=int(sc.gold18()["nclasses"])) as tr:
            recs = list(tr.run(**run_kw))
            return recs, tr.summary
    finally:
        src.close()


def _read(out_dir, idx, sub="00"):
    from lidar_transfer_amd.sequence import output_paths
    b, l = output_paths(str(out_dir), sub, idx)
    return open(b, "rb").read(), open(l, "rb").read()


_SINGLE = {}


def _singles(tmp_path_factory):
    """the two single-target runs of the heads' sensors, once for the module: name -> (out_dir, records, summary)"""
    from lidar_transfer_amd.config import load_sensor
    if not _SINGLE:
        roof, front = _sensors()
        for name, sensor, t in (("roof", roof, ()), ("front", front, T_FRONT)):
            out = tmp_path_factory.mktemp("single_" + name)
            recs, summary = _run(_approach(rig=False, transformation=t), load_sensor(sensor), out)
            _SINGLE[name] = (out, recs, summary)
    return _SINGLE


@pytest.mark.parametrize("chains", [1, 3])
def test_a_two_head_mesh_rig_writes_the_files_of_two_single_runs(chains, tmp_path, tmp_path_factory):
    single = _singles(tmp_path_factory)
    a = _approach()
    assert [h.sensor.W for h in a.rig()] == [int(sc.gold18()["target_t"][1]), 128]
    recs, summary = _run(a, None, tmp_path, chains=chains)
    indices = [r["idx"] for r in recs]
    assert summary["chains"] == chains and len(indices) >= 3 and indices == [r["idx"] for r in single["roof"][1]]
    for k, rec in enumerate(recs):
        assert not rec["skipped"] and rec["m_iou"] is None and set(rec["sensors"]) == {"roof", "front"}
        for name in ("roof", "front"):
            out, srecs, _ = single[name]
            got = _read(tmp_path, rec["idx"], os.path.join("00", name))
            assert got == _read(out, rec["idx"]), (name, rec["idx"])
            assert rec["sensors"][name]["n_points"] == srecs[k]["n_points"] == len(got[0]) // 16 > 50
        assert rec["n_points"] == sum(v["n_points"] for v in rec["sensors"].values())
    # no merged scan was asked for: the standard pair does not exist
    assert not os.path.exists(os.path.join(str(tmp_path), "sequences", "00", "velodyne"))
    # the tallies are kept per head: the front head's return model against its single run's, none for the roof head
    assert summary["return_totals"] is None
    assert summary["sensors"]["front"]["return_totals"] == single["front"][2]["return_totals"]
    assert summary["sensors"]["roof"]["return_totals"] is None and sum(summary["sensors"]["front"]["return_totals"][1:]) > 0


def test_the_merged_files_are_the_concatenation(tmp_path, tmp_path_factory):
    single = _singles(tmp_path_factory)
    recs, _ = _run(_approach(merged=True), None, tmp_path)
    T = np.array(T_FRONT).reshape(4, 4)
    for rec in recs:
        bins, labs = zip(*[_read(tmp_path, rec["idx"], os.path.join("00", n)) for n in ("roof", "front")])
        assert (bins[0], labs[0]) == _read(single["roof"][0], rec["idx"])
        mb, ml = _read(tmp_path, rec["idx"])
        assert ml == labs[0] + labs[1] and len(mb) == len(bins[0]) + len(bins[1]) and rec["n_points"] == len(mb) // 16
        assert mb[:len(bins[0])] == bins[0]                       # the roof head stands at the source pose
        rows = np.frombuffer(mb[len(bins[0]):], np.float32).reshape(-1, 4)
        front = np.frombuffer(bins[1], np.float32).reshape(-1, 4)
        assert rows[:, 3].tobytes() == front[:, 3].tobytes()
        assert rows[:, :3].tobytes() != front[:, :3].tobytes()    # the primary scan's frame, not the head's own
        assert mc.to_frame(rows[:, :3], T).tobytes() == np.ascontiguousarray(front[:, :3]).tobytes()


def test_resume_redoes_a_scan_of_which_one_heads_file_is_gone(tmp_path):
    from lidar_transfer_amd.sequence import output_paths
    a = _approach(merged=True)
    recs, _ = _run(a, None, tmp_path)
    victim = recs[1]["idx"]
    path = output_paths(str(tmp_path), os.path.join("00", "front"), victim)[1]
    before = {r["idx"]: [_read(tmp_path, r["idx"], s) for s in ("00", "00/roof", "00/front")] for r in recs}
    os.remove(path)
    again, _ = _run(a, None, tmp_path, resume=True)
    assert [r["skipped"] for r in again] == [r["idx"] != victim for r in recs]
    for r, r0 in zip(again, recs):
        assert r["sensors"] == r0["sensors"] and r["n_points"] == r0["n_points"]
        assert [_read(tmp_path, r["idx"], s) for s in ("00", "00/roof", "00/front")] == before[r["idx"]]


TOTALS = ("return_totals", "noise_totals", "range_error_rms", "echo_totals", "echo_fraction_mean", "second_returns")


def test_a_rig_of_one_head_is_that_heads_single_run(tmp_path, tmp_path_factory):
    out, srecs, ssummary = _singles(tmp_path_factory)["front"]
    recs, summary = _run(_approach(heads=("front",)), None, tmp_path)
    assert [r["idx"] for r in recs] == [r["idx"] for r in srecs] and len(recs) >= 3
    for rec, srec in zip(recs, srecs):
        assert _read(tmp_path, rec["idx"], os.path.join("00", "front")) == _read(out, rec["idx"]), rec["idx"]
        assert set(rec["sensors"]) == {"front"}
        assert rec["sensors"]["front"]["n_points"] == rec["n_points"] == srec["n_points"] > 50
    assert not os.path.exists(os.path.join(str(tmp_path), "sequences", "00", "velodyne"))
    assert set(summary["sensors"]) == {"front"} and set(summary["sensors"]["front"]) == set(TOTALS)
    for key in TOTALS:
        assert summary["sensors"]["front"][key] == ssummary[key], key
        assert summary[key] is None, key
    assert sum(ssummary["return_totals"][1:]) > 0


def test_a_merged_rig_of_one_head_writes_the_single_run_twice_and_resumes_by_either(tmp_path, tmp_path_factory):
    from lidar_transfer_amd.sequence import output_paths
    out, srecs, _ = _singles(tmp_path_factory)["roof"]
    a = _approach(heads=("roof",), merged=True)
    recs, _ = _run(a, None, tmp_path)
    assert [r["idx"] for r in recs] == [r["idx"] for r in srecs] and len(recs) >= 3
    for rec, srec in zip(recs, srecs):
        want = _read(out, rec["idx"])
        assert _read(tmp_path, rec["idx"], os.path.join("00", "roof")) == want == _read(tmp_path, rec["idx"]), rec["idx"]
        assert rec["n_points"] == rec["sensors"]["roof"]["n_points"] == srec["n_points"] == len(want[0]) // 16 > 50
    # --resume: a scan whose MERGED label file is gone is redone, and no other
    victim = recs[1]["idx"]
    before = {r["idx"]: [_read(tmp_path, r["idx"], s) for s in ("00", "00/roof")] for r in recs}
    os.remove(output_paths(str(tmp_path), "00", victim)[1])
    again, _ = _run(a, None, tmp_path, resume=True)
    assert [r["skipped"] for r in again] == [r["idx"] != victim for r in recs] and sum(r["skipped"] for r in again) == len(recs) - 1
    for r, r0 in zip(again, recs):
        assert r["sensors"] == r0["sensors"] and r["n_points"] == r0["n_points"]
        assert [_read(tmp_path, r["idx"], s) for s in ("00", "00/roof")] == before[r["idx"]]


def test_what_a_rig_refuses():
    from lidar_transfer_amd.config import load_sensor
    from lidar_transfer_amd.sequence import SequenceTransfer
    roof, _ = _sensors()
    cases = [(_approach(), None, dict(evaluate=True), "rig evaluation"), (_approach(), None, dict(evaluate="target"), "rig evaluation"),
             (_approach(), load_sensor(roof), {}, "takes no target sensor"), (_approach("cp"), None, {}, "cp renders no ray"),
             (_approach(rig=False), None, {}, "target sensor")]
    tall = _approach("mergemesh")
    tall.rig_block = [tall.rig_block[0], dict(name="tall", sensor=dict(roof, fov_up=roof["fov_up"] + 2.0))]
    cases.append((tall, None, {}, "widest first"))
    for a, target, kw, say in cases:
        src = _source()
        try:
            with pytest.raises(ValueError, match=say):
                SequenceTransfer(src, a, ev.SOURCE, target, **kw)
        finally:
            src.close()
    # evaluate=None resolves to no comparison
    src = _source()
    try:
        with SequenceTransfer(src, _approach(), ev.SOURCE, None) as tr:
            assert tr.evaluate is False and tr.evaluate_mode is None
    finally:
        src.close()


def test_cli_writes_one_folder_per_head_and_refuses_a_target(tmp_path):
    import yaml
    g17, a = cpu.gold(), _approach(merged=True)
    data = tmp_path / "data"
    seq = data / "sequences" / "00"
    (seq / "velodyne").mkdir(parents=True)
    (seq / "labels").mkdir()
    for k, (xyzr, lab) in enumerate(cpu.raw_scans(g17)):
        xyzr.tofile(seq / "velodyne" / f"{k:06d}.bin")
        lab.tofile(seq / "labels" / f"{k:06d}.label")
    g17["calib_txt"].tofile(seq / "calib.txt")
    g17["poses_txt"].tofile(seq / "poses.txt")
    H, W, fu, fd = ev.SOURCE
    (data / "config.yaml").write_text(f"name: src\nfov_up: {fu}\nfov_down: {fd}\nbeams: {H}\nangle_res_hor: {360.0 / W!r}\nfov_hor: 360.0\n")
    roof, front = _sensors()
    (tmp_path / "front.yaml").write_text(yaml.safe_dump(front))
    cfg = tmp_path / "rig.yaml"
    cfg.write_text(yaml.safe_dump(dict(
        adaption="mesh", preserve_float=False, number_of_scans=int(a.number_of_scans), batch_interval=int(a.batch_interval),
        voxel_size=float(a.voxel_size), voxel_bounds=[float(x) for x in np.asarray(a.voxel_bounds).reshape(-1)], transformation=[],
        ignore=[int(x) for x in a.ignore], moving=[int(x) for x in a.moving],
        color_map={int(k): [int(x) for x in v] for k, v in ev.COLOR_DICT.items()}, rig_merged=True,
        rig=[dict(name="roof", sensor=roof), dict(name="front", sensor="front.yaml", transformation=[float(x) for x in T_FRONT])])))
    out = tmp_path / "out"
    out.mkdir()
    log = tmp_path / "log.jsonl"
    base = [sys.executable, "-m", "lidar_transfer_amd", "-d", str(data), "-c", str(cfg), "-s", "00", "-w", "-p", str(out), "--one_scan"]
    res = subprocess.run(base + ["--log", str(log)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    rows = [json.loads(x) for x in log.read_text().splitlines()]
    idx = rows[0]["idx"]
    assert set(rows[0]["sensors"]) == {"roof", "front"} and "IoU:" not in res.stdout and "front: Returns: kept" in res.stdout
    sizes = {s: len(_read(out, idx, s)[0]) // 16 for s in ("00", "00/roof", "00/front")}
    assert sizes["00/roof"] == rows[0]["sensors"]["roof"]["n_points"] > 50 and sizes["00/front"] == rows[0]["sensors"]["front"]["n_points"]
    assert sizes["00"] == sizes["00/roof"] + sizes["00/front"] == rows[0]["n_points"]
    assert rows[-1]["summary"]["sensors"]["front"]["return_totals"] is not None
    res = subprocess.run(base + ["-t", str(tmp_path / "front.yaml")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 1 and "-t / --target cannot be given" in res.stdout
    res = subprocess.run(base + ["--evaluate", "target"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 1 and "rig is not evaluated" in res.stdout
