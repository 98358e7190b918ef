#!/usr/bin/env python3
"""What a whole sequence costs per output scan (lidar_transfer_amd/sequence.py), at user size, against the loop a caller had
to write before it existed.

    python tools/bench_sequence.py --out profiles/sequence/bench_sequence.json                     # the timings (needs a GPU)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o seq -- python tools/bench_sequence.py --trace-only
    python tools/bench_sequence.py --kernel-stats DIR --out profiles/sequence/bench_sequence.json  # kernel times into the JSON

The seeded sequence of tools/bench_ingest.py (64 x 2048 sensor, ~120 k points per scan), `number_of_scans` 5, source = target
= 64 x 2048, the default adaption `mergemesh` on the reference's default volume (+-50 / +-50 / +-5 m, 0.05 m voxels),
config/approach_mergemesh.yaml.  Every variant is warmed up with one pass over the sequence; a timed window is whole passes
until at least `--window` seconds have gone by (host clock, ending in a device synchronise and -- where files are written --
in the writer thread having written them); `--reps` repetitions with the variants alternating inside one command; median
(min - max) in ms per OUTPUT scan.

baseline_plain   the parent's public calls: DeviceDeform.deform('mergemesh', ingest, idx) per scan, nothing else
baseline_full    ... + the source reference scan the only way the parent offers (numpy class removal on the host, upload,
                 Projector in the old float32 mode with the colour table) + post.compare on downloaded images + DeviceDeform.write
st1_plain / st1_eval / st1_write / st1_full      SequenceTransfer(chains=1), evaluation and writing each off / on
st3_plain / st3_full                             SequenceTransfer(chains=3)

Without a device the tool fails; it prints no numbers."""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_ingest as bi  # noqa: E402

SENSOR = (bi.H, bi.W, bi.FOV_UP, bi.FOV_DOWN)
KERNELS = ("k_src_project", "k_src_resolve", "k_cmp_pairs", "k_cmp_record", "k_compare")


def stat(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--raw-scans", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--trace-only", action="store_true", help="one pass of st1_full and baseline_full, for the profiler")
    ap.add_argument("--kernel-stats", default="", help="directory of a rocprofv3 --kernel-trace --stats run: merge into --out")
    args = ap.parse_args()
    if args.kernel_stats:
        rows = {}
        for path in glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                for k in KERNELS:
                    if k in r["Name"]:
                        rows[k] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3)
        doc = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        doc["kernels"] = rows
        json.dump(doc, open(args.out, "w"), indent=1)
        print(json.dumps(rows))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sequence.py needs a GPU")
    from lidar_transfer_amd.config import load_approach
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest, SequenceSource
    from lidar_transfer_amd.laserscan import Projector
    from lidar_transfer_amd.post import compare
    from lidar_transfer_amd.sequence import SequenceTransfer
    dev = torch.device("cuda", 0)
    approach = load_approach(os.path.join(ROOT, "config", "approach_mergemesh.yaml"))
    scans, poses = bi.make_sequence(args.raw_scans, 7)
    indices = approach.scan_indices(len(scans))
    nclasses = len(approach.color_map)
    lut_np = approach.color_lut()
    tmp = tempfile.mkdtemp(prefix="bench_sequence_")

    def source():
        return SequenceSource(scans=[s for s, _ in scans], labels=[l for _, l in scans], poses=poses, cache_scans=32)

    # ---- the baseline: the parent's public calls only ------------------------------------------------------------------------
    b_src = source()
    b_ing = ScanIngest(b_src, approach)
    b_dd = DeviceDeform(SENSOR, SENSOR, approach.voxel_bounds.copy(), approach.voxel_size, mesh_volume=False)
    b_pj = Projector(0)
    lut = torch.from_numpy(lut_np).to(dev)
    h = lambda t: t.cpu().numpy()   # noqa: E731

    def baseline(full):
        b_dd.reset_bounds(approach.voxel_bounds)
        for idx in indices:
            out = b_dd.deform("mergemesh", b_ing, idx)
            if full:
                xyzr, label = scans[idx]
                l = label & 0xFFFF
                keep = ~np.isin(l, approach.ignore)
                cloud = (torch.from_numpy(np.ascontiguousarray(xyzr[keep, :3])).to(dev), torch.from_numpy(np.ascontiguousarray(xyzr[keep, 3])).to(dev),
                         torch.from_numpy(l[keep].astype(np.int32)).to(dev))
                s = b_pj.project([cloud], SENSOR[2], SENSOR[3], SENSOR[0], SENSOR[1], new=False, remove=True, color_lut=lut,
                                 outputs=("range", "rem", "label", "color"))[0]
                m = compare(h(s["label"]), h(s["color"]), h(out["label"]), h(s["range"]), h(out["range"]), h(s["rem"]), h(out["rem"]), nclasses)
                DeviceDeform.write(out, os.path.join(tmp, "base", "sequences", "00"), idx)
                last["base"] = (m["m_iou"], m["m_acc"], m["MSE"])
        torch.cuda.synchronize()
        return len(indices)

    last = {}
    runners = {}

    def make(name, chains, evaluate, write):
        tr = SequenceTransfer(source(), approach, SENSOR, SENSOR, out_dir=os.path.join(tmp, name) if write else None, chains=chains,
                              evaluate=evaluate)

        def run():
            n = 0
            for rec in tr.run():
                n += 1
                if rec["m_iou"] is not None:
                    last[name] = (rec["m_iou"], rec["m_acc"], rec["MSE"])
            torch.cuda.synchronize()
            return n
        runners[name] = (tr, run)

    variants = {"baseline_plain": lambda: baseline(False), "baseline_full": lambda: baseline(True)}
    wanted = [("st1_full", 1, True, True)] if args.trace_only else \
        [("st1_plain", 1, False, False), ("st1_eval", 1, True, False), ("st1_write", 1, False, True), ("st1_full", 1, True, True),
         ("st3_plain", 3, False, False), ("st3_full", 3, True, True)]
    for name, chains, evaluate, write in wanted:
        make(name, chains, evaluate, write)
        variants[name] = runners[name][1]
    for name, fn in variants.items():      # warm-up: every shape, every volume
        fn()
    if args.trace_only:
        variants["st1_full"]()
        variants["baseline_full"]()
        print("trace pass done")
    else:
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for name, fn in variants.items():
                n, t0 = 0, time.perf_counter()
                while time.perf_counter() - t0 < args.window:
                    n += fn()
                times[name].append((time.perf_counter() - t0) * 1e3 / n)
        doc = dict(workload=dict(raw_scans=len(scans), points_per_scan=int(np.mean([len(l) for _, l in scans])), output_scans=len(indices),
                                 number_of_scans=approach.number_of_scans, sensor=list(SENSOR), adaption=approach.adaption,
                                 voxel_size=approach.voxel_size, nclasses=nclasses, window_s=args.window, reps=args.reps),
                   ms_per_output_scan={k: stat(v) for k, v in times.items()},
                   last_metrics={k: [float(x) for x in v] for k, v in last.items()},
                   mm_stats={k: tr.summary.get("mm_stats") for k, (tr, _) in runners.items()})
        m = doc["ms_per_output_scan"]
        doc["derived"] = dict(baseline_compare_and_write_ms=m["baseline_full"]["median"] - m["baseline_plain"]["median"],
                              st1_evaluation_ms=m["st1_eval"]["median"] - m["st1_plain"]["median"],
                              st1_writing_ms=m["st1_write"]["median"] - m["st1_plain"]["median"],
                              st1_plain_minus_baseline_plain_ms=m["st1_plain"]["median"] - m["baseline_plain"]["median"],
                              baseline_plain_spread_ms=m["baseline_plain"]["max"] - m["baseline_plain"]["min"])
        print(json.dumps(doc))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(doc, open(args.out, "w"), indent=1)
    for tr, _ in runners.values():
        tr.close()
    b_dd.close()
    b_pj.close()
    b_src.close()


if __name__ == "__main__":
    main()
