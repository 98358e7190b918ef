#!/usr/bin/env python3
"""What per-beam azimuth offsets (`beam_azimuth_offsets`) cost a table target over the plain table: the render alone with the
scatter's counters, and a whole `mergemesh` sequence per output scan -- the method of tools/bench_beam_table.py.

    python tools/bench_beam_azimuth.py --out profiles/beam_azimuth/bench.json                              # this tree
    python tools/bench_beam_azimuth.py --table-only --root PARENT --out profiles/beam_azimuth/parent.json  # a checkout of the parent commit

render     `lt_stats.ms_trace` of `lt_scene_render_dev` (Scene.render(stats=True)) against the 1 M-triangle synthetic scene of
           workload C2: the VLP-32C table of config/vlp32c_table_1024.yaml at 32 x 1024 beside the same table with the offsets
           of config/vlp32c_table_az_1024.yaml; `--reps` repetitions of `--renders` renders each after a warm-up, the cases
           alternating; median (min - max) of the repetitions' means, ms.  Counters: one `LT_TRACE_COUNT` render per case
           (`lt_stats`: nodes_visited = candidate bins, tris_tested, entries_culled, n_hits) and the ray set's grid.
sequence   `SequenceTransfer(chains=1)`, nothing evaluated, nothing written: the seeded sequence of tools/bench_ingest.py with
           config/approach_mergemesh.yaml, target config/vlp32c_table_1024.yaml against config/vlp32c_table_az_1024.yaml; whole
           passes for at least `--window` seconds, `--reps` repetitions alternating; ms per output scan.

`--table-only` runs the plain table alone and uses nothing the parent commit lacks; `--root` names the tree whose package and
tools are imported.  Without a device the tool fails; it prints no numbers."""
import argparse
import json
import os
import sys

import bench_beam_table as bbt   # this tree's: the two measurement bodies (imported before `--root` goes on the path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--table-only", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--renders", type=int, default=20)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--raw-scans", type=int, default=16)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_azimuth.py needs a GPU")
    import lidar_transfer_amd
    from lidar_transfer_amd.config import load_sensor
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.synth import WORKLOADS
    assert os.path.abspath(lidar_transfer_amd.__file__).startswith(root + os.sep), lidar_transfer_amd.__file__
    doc = dict(root=os.path.relpath(root), table_only=bool(args.table_only))
    plain = load_sensor(os.path.join(root, "config", "vlp32c_table_1024.yaml"))
    fu, fd, H, W = plain.fov_up, plain.fov_down, plain.H, plain.W
    rays = {"vlp32c 32x1024": create_rays_device(fu, fd, H, W, beam_table=plain.beam_table())}
    targets = {"vlp32c_table_1024.yaml": plain}
    if not args.table_only:   # (the parent has neither the file nor the keyword, and is not asked)
        az = load_sensor(os.path.join(here, "config", "vlp32c_table_az_1024.yaml"))
        rays["vlp32c az 32x1024"] = create_rays_device(fu, fd, H, W, beam_table=az.beam_table(), beam_azimuth=az.beam_azimuth())
        targets["vlp32c_table_az_1024.yaml"] = az
    doc["render"] = bbt.render_cases(rays, H, WORKLOADS["C2"]["tris"], args.reps, args.renders)
    del rays
    doc["sequence"] = bbt.sequence_targets(root, targets, args.raw_scans, args.window, args.reps)
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
