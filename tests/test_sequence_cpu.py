"""Golden F18 (tests/golden/make_golden_sequence.py: the reference's loop body lidar_deform.py:396-418 + write over the batch
list of F17's sequence) against the written contracts, and the host side of `SequenceTransfer` / the CLI, without a GPU:
the numpy restatements of `lt_source_scan_dev` and `lt_compare_record_dev` (tests/test_evaluate_cpu.py) reproduce the
reference's source images and -- for `cp`, whose target image the restated projection gives on the CPU -- its IoU / Acc / MSE
from the file bytes F17 holds; scan list, `resume`'s file test, output layout, the writer, CLI parsing and exit statuses."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_evaluate_cpu as ev  # noqa: E402
import test_ingest_cpu as cpu  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def gold18():
    return np.load(os.path.join(HERE, "golden", "f18_sequence.npz"))


def approach_for(g18, adaption):
    from lidar_transfer_amd.config import Approach
    mm = adaption == "mergemesh"
    return Approach(adaption=adaption, preserve_float=False, voxel_size=float(g18["mm_voxel"] if mm else g18["mesh_voxel"]),
                    voxel_bounds=(g18["mm_bnds"] if mm else g18["mesh_bnds"]).copy(), number_of_scans=int(g18["nscans"]),
                    ignore=[int(x) for x in g18["ignore"]], moving=[int(x) for x in g18["moving"]], transformation=[],
                    batch_interval=int(g18["batch_interval"]), color_map=dict(ev.COLOR_DICT), labels={})


def metrics_close(got, g18, tag):
    """the tolerances tests/test_post_gpu.py:74-77 uses for the same quantities"""
    mse = float(g18[f"{tag}_MSE"])
    assert abs(got["m_iou"] - float(g18[f"{tag}_m_iou"])) < 1e-12, tag
    assert abs(got["m_acc"] - float(g18[f"{tag}_m_acc"])) < 1e-12, tag
    assert abs(got["MSE"] - mse) < 1e-6 * mse + 1e-9, (tag, got["MSE"], mse)
    assert np.allclose(got["iou"], g18[f"{tag}_iou"], rtol=0, atol=1e-12), tag


def test_f18_is_the_batch_list_of_f17s_sequence_and_holds_the_issues_sample_values():
    g18, g17 = gold18(), cpu.gold()
    from lidar_transfer_amd.dist import scan_indices
    assert [int(x) for x in g18["indices"]] == scan_indices(int(g17["n_scans_seq"]), 3, 0, 1) == [1, 2, 3, 4, 5]
    assert tuple(g18["source"]) == tuple(g17["source"]) and tuple(g18["target_t"]) == tuple(g17["target"])
    assert tuple(g18["target_s"]) == tuple(g17["source"]) and int(g18["nclasses"]) == 300
    assert float(g18["t_cp_1_m_iou"]) == 0.5131937215150113 and float(g18["t_cp_1_m_acc"]) == 0.9248046875
    assert float(g18["s_mergemesh_5_m_iou"]) == 0.5600166969756221 and float(g18["s_mergemesh_5_MSE"]) == 0.2502092123031616
    for t in ("t", "s"):
        for a in ("cp", "mesh", "mergemesh"):
            for i in range(1, 6):
                tag = f"{t}_{a}_{i}"
                assert int(g18[f"{tag}_n_bin"]) == 4 * int(g18[f"{tag}_n_label"]) > 16 * 1500 and int(g18[f"{tag}_n_present"]) <= 64
    assert np.array_equal(g18["t_mergemesh_5_bnds_after"], [[1, 11], [-7, 11], [-2, 1]])


def test_source_contract_restated_reproduces_the_references_source_scans():
    g18, g17 = gold18(), cpu.gold()
    H, W, fu, fd = ev.SOURCE
    lut = ev.color_lut(ev.COLOR_DICT)
    for k, (xyzr, label) in enumerate(cpu.raw_scans(g17)):
        got = ev.restate_source(xyzr, label, ev.IGNORE, H, W, fu, fd, lut)
        digests = [cpu.sha(got["range"]), cpu.sha(got["rem"]), cpu.sha(got["label"]), cpu.sha(got["black"])]
        assert digests == [str(x) for x in g18[f"src{k}_sha"]], k
        if k in [int(x) for x in g18["stored_source"]]:
            assert np.array_equal(got["range"].view(np.int32), g18[f"src{k}_range"].view(np.int32))
            assert np.array_equal(got["label"], g18[f"src{k}_label"]) and np.array_equal(got["black"], g18[f"src{k}_black"])


@pytest.mark.parametrize("tkey", ["t", "s"])
def test_compare_contract_restated_reproduces_the_references_metrics_for_cp(tkey):
    """the `cp` target image is the restated projection of the restated merged cloud (both pinned by F17): source image +
    record + `post.confusion_metrics` give the reference's IoU / Acc / MSE / per-class iou of `compare(scan, scans)`"""
    from lidar_transfer_amd.post import confusion_metrics
    from oracle import projection as op
    g18, g17 = gold18(), cpu.gold()
    H, W, fu, fd = ev.SOURCE
    tH, tW, tfu, tfd = (int(g18[f"target_{tkey}"][0]), int(g18[f"target_{tkey}"][1]), float(g18[f"target_{tkey}"][2]),
                        float(g18[f"target_{tkey}"][3]))
    lut = ev.color_lut(ev.COLOR_DICT)
    raw, poses = cpu.raw_scans(g17), g17["poses"]
    ignore, moving = [int(x) for x in g18["ignore"]], [int(x) for x in g18["moving"]]
    for idx in (1, 5):
        src = ev.restate_source(*raw[idx], ignore, H, W, fu, fd, lut)
        slots = [idx, idx - 1, idx + 1]
        (p, r, l), = cpu.restate(raw, poses, slots, np.linalg.inv(poses[idx]), ignore, moving, True)
        t = op.range_projection(p, r, tH, tW, tfu, tfd, remove=True, method="new")
        tl = op.label_projection(t["index"], l[t["kept"]])
        rec = ev.restate_compare(src["label"], src["black"], tl, src["range"], t["range"])
        assert rec["status"] == 0 and len(rec["present"]) <= int(g18[f"{tkey}_cp_{idx}_n_present"])   # (F18 counts before the masks)
        _, m_iou, m_acc, iou = confusion_metrics(rec["present"], rec["counts"], int(g18["nclasses"]))
        metrics_close(dict(m_iou=m_iou, m_acc=m_acc, MSE=rec["sq_sum"] / rec["n_cells"], iou=iou), g18, f"{tkey}_cp_{idx}")


def test_scan_list_layout_and_the_resume_file_test(tmp_path):
    from lidar_transfer_amd import sequence as sq
    g18 = gold18()
    assert approach_for(g18, "mesh").scan_indices(8, 0) == [1, 2, 3, 4, 5] and approach_for(g18, "cp").scan_indices(8, 3) == [3, 4, 5]
    b, l = sq.output_paths(str(tmp_path), "07", 12)
    assert b == str(tmp_path / "sequences" / "07" / "velodyne" / "000012.bin") and l.endswith(os.path.join("labels", "000012.label"))
    assert not sq.plausible_output(str(tmp_path), "07", 12)
    os.makedirs(os.path.dirname(b))
    os.makedirs(os.path.dirname(l))
    open(b, "wb").write(b"\0" * 160)
    assert not sq.plausible_output(str(tmp_path), "07", 12)              # no label file
    open(l, "wb").write(b"\0" * 36)
    assert not sq.plausible_output(str(tmp_path), "07", 12)              # not a quarter
    open(l, "wb").write(b"\0" * 40)
    assert sq.plausible_output(str(tmp_path), "07", 12)
    open(b, "wb").write(b"\0" * 150)
    assert not sq.plausible_output(str(tmp_path), "07", 12)              # not whole points
    assert sq.cache_scans_needed(5, 3, 1) == 8 and sq.cache_scans_needed(3, 1, 10) == 13
    assert sq.sensor_tuple((32, 512, 3, -25)) == (32, 512, 3.0, -25.0)
    from lidar_transfer_amd.config import load_sensor
    assert sq.sensor_tuple(load_sensor(os.path.join(ROOT, "config", "vlp32_1024.yaml"))) == (32, 1024, 10.0, -30.0)


def test_writer_thread_writes_the_two_files_behind_the_event_and_reports_failures(tmp_path):
    import torch
    from lidar_transfer_amd import sequence as sq

    class Ev:
        def __init__(self):
            self.waited = False

        def synchronize(self):
            self.waited = True

    w = sq._Writer()
    hb = torch.arange(40, dtype=torch.float32).reshape(10, 4)
    hl = torch.arange(10, dtype=torch.int32) - 3                          # negative labels travel as uint32 bits
    job, e = dict(written=threading.Event(), error=None), Ev()
    paths = sq.output_paths(str(tmp_path), "00", 3)
    w.q.put((job, [(paths, hb, hl, 7)], e))
    assert job["written"].wait(30) and job["error"] is None and e.waited
    assert np.array_equal(np.fromfile(paths[0], np.float32), np.arange(28, dtype=np.float32))
    assert np.array_equal(np.fromfile(paths[1], np.uint32), (np.arange(7) - 3).astype(np.int32).view(np.uint32))
    blocked = tmp_path / "file"
    blocked.write_text("x")
    job2 = dict(written=threading.Event(), error=None)
    w.q.put((job2, [(sq.output_paths(str(blocked), "00", 3), hb, hl, 7)], Ev()))
    assert job2["written"].wait(30) and isinstance(job2["error"], OSError)
    w.close()
    assert not w.thread.is_alive()


def test_cli_flag_surface_and_exit_statuses(tmp_path, capsys):
    from lidar_transfer_amd import __main__ as cli
    a = cli.build_parser().parse_args(["-d", "D", "-c", "C", "-s", "05", "-t", "T", "-o", "4", "-p", "P", "-b", "-w", "--one_scan",
                                       "--chains", "3", "--fusion", "numpy", "--resume", "--log", "L"])
    assert (a.dataset, a.config, a.sequence, a.target, a.offset, a.output) == ("D", "C", "05", "T", 4, "P")
    assert a.batch and a.write and a.one_scan and a.chains == 3 and a.fusion == "numpy" and a.resume and a.log == "L"
    d = cli.build_parser().parse_args(["--dataset", "D"])
    assert (d.sequence, d.target, d.offset, d.output, d.chains, d.fusion) == ("00", "", 0, "output/", 1, "cuda")
    assert not (d.batch or d.write or d.one_scan or d.resume) and os.path.isfile(os.path.join(ROOT, d.config))
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args([])                                 # --dataset is required
    ds = tmp_path / "ds"
    assert cli.main(["-d", str(ds)]) == 1 and "Sequence folder doesn't exist" in capsys.readouterr().out
    os.makedirs(ds / "sequences" / "00" / "velodyne")
    assert cli.main(["-d", str(ds)]) == 1 and "Labels folder doesn't exist" in capsys.readouterr().out
    os.makedirs(ds / "sequences" / "00" / "labels")
    assert cli.main(["-d", str(ds), "-w", "-p", str(tmp_path / "nowhere")]) == 1 and "Output folder doesn't exist" in capsys.readouterr().out
    assert cli.main(["-d", str(ds)]) == 1 and "config.yaml" in capsys.readouterr().out
    (ds / "config.yaml").write_text("name: x\n")
    assert cli.main(["-d", str(ds), "-c", str(tmp_path / "none.yaml")]) == 1 and "approach yaml" in capsys.readouterr().out
    assert cli.main(["-d", str(ds), "-c", os.path.join(ROOT, "config", "approach_mergemesh.yaml")]) == 1   # KeyError: fov_up
    assert "Error opening yaml file" in capsys.readouterr().out


def test_shipped_approach_yaml_loads():
    from lidar_transfer_amd.config import load_approach
    a = load_approach(os.path.join(ROOT, "config", "approach_mergemesh.yaml"))
    assert a.adaption == "mergemesh" and a.number_of_scans == 5 and a.voxel_bounds.shape == (3, 2) and len(a.color_map) == 34
    assert a.color_lut().shape == (360, 3) and a.scan_indices(20) == list(range(2, 16))


def test_closing_lines_are_the_format_functions_lines_in_order_with_the_lead():
    from lidar_transfer_amd import sequence as sq
    totals = dict(return_totals=[5, 4, 3, 2, 1, 0], noise_totals=[7, 8, 9], range_error_rms=0.0125, echo_totals=[1, 20, 3],
                  echo_fraction_mean=0.75, second_returns=11, scans=2, chains=1)
    for lead in ("", "front: "):
        assert sq.format_closing_lines(totals, lead) == [
            lead + sq.format_return_totals([5, 4, 3, 2, 1, 0]), lead + sq.format_noise_totals([7, 8, 9], 0.0125),
            lead + sq.format_echo_totals([1, 20, 3], 0.75), lead + "Second returns: %d" % 11]
    assert sq.format_closing_lines(totals, "front: ")[0] == \
        "front: Returns: kept 5, no hit 4, below min_range 3, beyond max_range 2, beyond max_incidence 1, dropped at random 0"
    assert sq.format_closing_lines(totals)[3] == "Second returns: 11"
    # each line only when its model was on; a noise model that noised nothing still has its line
    only = dict(return_totals=None, noise_totals=[4, 0, 0], range_error_rms=None, echo_totals=None, echo_fraction_mean=None,
                second_returns=None)
    assert sq.format_closing_lines(only, "a: ") == ["a: " + sq.format_noise_totals([4, 0, 0], None)]
    nothing = dict(return_totals=None, noise_totals=None, range_error_rms=None, echo_totals=None, echo_fraction_mean=None,
                   second_returns=None)
    assert sq.format_closing_lines(nothing) == [] and sq.format_closing_lines(nothing, "front: ") == []


CP_SENTENCES = dict(
    return_model="adaption cp renders no surface: the target sensor's return_model cannot be applied (use mesh or mergemesh).",
    noise_model="adaption cp renders no ray: the target sensor's noise_model cannot be applied (use mesh or mergemesh).",
    echo_model="adaption cp renders no ray: the target sensor's echo_model cannot be applied (use mesh or mergemesh).",
    dual_return="adaption cp renders no ray: the target sensor's dual_return cannot be applied (use mesh or mergemesh).")


@pytest.mark.parametrize("key, name", [("return_model", "vlp32c_table_returns_1024.yaml"), ("noise_model", "vlp32c_table_noise_1024.yaml"),
                                       ("echo_model", "vlp32c_table_echo_1024.yaml"), ("dual_return", "vlp32c_table_dual_1024.yaml")])
def test_cli_refuses_cp_with_each_shipped_model_file_in_the_order_return_noise_echo_dual(tmp_path, capsys, monkeypatch, key, name):
    """The shipped file of a model also holds the blocks of the models before it, so as shipped every one of the four is
    refused for its ``return_model``.  With the blocks before its own key taken out, each is refused for its own -- but a
    ``dual_return`` cannot be loaded without its ``echo_model``, which comes first: its own sentence is reached with a target
    that answers for the dual return alone."""
    import yaml
    from lidar_transfer_amd import __main__ as cli
    from lidar_transfer_amd import config
    ds = tmp_path / "ds"
    os.makedirs(ds / "sequences" / "00" / "velodyne")
    os.makedirs(ds / "sequences" / "00" / "labels")
    with open(os.path.join(ROOT, "config", "hdl64_1024.yaml")) as f:
        (ds / "config.yaml").write_text(f.read())
    with open(os.path.join(ROOT, "config", "approach_mergemesh.yaml")) as f:
        text = f.read()
    assert text.count('adaption: "mergemesh"') == 1
    (tmp_path / "cp.yaml").write_text(text.replace('adaption: "mergemesh"', 'adaption: "cp"'))
    args = ["-d", str(ds), "-c", str(tmp_path / "cp.yaml"), "-t"]
    shipped = os.path.join(ROOT, "config", name)
    with open(shipped) as f:
        sensor = yaml.safe_load(f)
    order = list(CP_SENTENCES)
    before = order[:order.index(key)]
    assert key in sensor and all(k in sensor for k in before)
    assert cli.main(args + [shipped]) == 1
    assert capsys.readouterr().out == CP_SENTENCES["return_model"] + "\n"
    for k in before[:2]:
        del sensor[k]
    (tmp_path / "own.yaml").write_text(yaml.safe_dump(sensor))
    assert cli.main(args + [str(tmp_path / "own.yaml")]) == 1
    assert capsys.readouterr().out == CP_SENTENCES["echo_model" if key == "dual_return" else key] + "\n"
    if key == "dual_return":
        real = config.load_sensor
        dual = real(shipped).dual_return()
        assert dual is not None

        class OnlyDual:
            return_model = noise_model = echo_model = staticmethod(lambda: None)
            dual_return = staticmethod(lambda: dual)
        monkeypatch.setattr(config, "load_sensor", lambda path: OnlyDual() if path == shipped else real(path))
        assert cli.main(args + [shipped]) == 1
        assert capsys.readouterr().out == CP_SENTENCES["dual_return"] + "\n"
