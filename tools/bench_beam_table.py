#!/usr/bin/env python3
"""What a target sensor with a beam table (`beam_model: table`) costs over an evenly spaced sensor of the same shape: the
render alone with the scatter's counters, and a whole `mergemesh` sequence per output scan.

    python tools/bench_beam_table.py --out profiles/beam_table/bench.json                          # this tree
    python tools/bench_beam_table.py --linear-only --root PARENT --out profiles/beam_table/parent.json   # a checkout of the parent commit

render     `lt_stats.ms_trace` of `lt_scene_render_dev` (Scene.render(stats=True)) against the 1 M-triangle synthetic scene of
           workload C2: the two-block table (32 beams from 2 degrees down at 1/3 degree, 32 from -8.83 at 1/2 degree) at
           64 x 2048 and the VLP-32C table of config/vlp32c_table_1024.yaml at 32 x 1024, each beside the evenly spaced sensor
           of the same shape and field of view; `--reps` repetitions of `--renders` renders each after a warm-up, the cases
           alternating; median (min - max) of the repetitions' means, ms.  Counters: one `LT_TRACE_COUNT` render per case
           (`lt_stats`: nodes_visited = candidate bins, tris_tested, entries_culled, n_hits) and the ray set's grid.
sequence   `SequenceTransfer(chains=1)`, nothing evaluated, nothing written: the seeded sequence of tools/bench_ingest.py with
           config/approach_mergemesh.yaml, target config/vlp32_1024.yaml against config/vlp32c_table_1024.yaml; whole passes
           for at least `--window` seconds, `--reps` repetitions alternating; ms per output scan.

`--linear-only` runs the evenly spaced cases alone and uses nothing the parent commit lacks; `--root` names the tree whose
package and tools are imported.  Without a device the tool fails; it prints no numbers."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

VLP32C = [15.0, 10.333, 7.0, 4.667, 3.333, 2.333, 1.667, 1.333, 1.0, 0.667, 0.333, 0.0, -0.333, -0.667, -1.0, -1.333, -1.667,
          -2.0, -2.333, -2.667, -3.0, -3.333, -3.667, -4.0, -4.667, -5.333, -6.148, -7.254, -8.843, -11.31, -15.639, -25.0]
TWO_BLOCK = [2.0 - k / 3 for k in range(32)] + [-8.83 - 0.5 * k for k in range(32)]


def stat(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), n=len(xs))


def grid(rs):
    lib = rs._lib
    lib.lt_debug_rayset_params.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.lt_debug_rayset_params.restype = C.c_int
    nb, p = (C.c_int * 2)(), (C.c_float * 6)()
    lib.lt_debug_rayset_params(rs._h, nb, p)
    return dict(nb_az=int(nb[0]), nb_el=int(nb[1]), dev_az=float(p[4]), dev_el=float(p[5]))


def render_cases(rays, H, tris, reps, renders):
    """`rays`: name -> [H * W, 3] device rays of one image height.  The render part of the docstring: returns the `render` record"""
    import torch
    from lidar_transfer_amd.raytracer import RaySet, Scene
    from lidar_transfer_amd.synth import synth_scene
    dev = torch.device("cuda", 0)
    scn = Scene(0)
    mesh = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in synth_scene(0, tris)]
    scn.set_mesh(*mesh)
    sets, outs, counters = {}, {}, {}
    for name, r in rays.items():
        h = H[name] if isinstance(H, dict) else H
        sets[name] = RaySet(r, h)
        outs[name] = scn.alloc_outputs(r.shape[0])
    for name, rs in sets.items():          # warm-up, counters
        for _ in range(3):
            o = scn.render(rs, (0.0, 0.0, 0.0), out=outs[name], count=True)
        s = o["stats"]
        counters[name] = dict(grid(rs), n_rays=int(s["n_rays"]), n_hits=int(s["n_hits"]), candidate_bins=int(s["nodes_visited"]),
                              tris_tested=int(s["tris_tested"]), tris_tested_per_ray=float(s["tris_tested"]) / max(int(s["n_rays"]), 1),
                              entries_culled=int(s["entries_culled"]))
    ms = {k: [] for k in sets}
    for _ in range(reps):
        for name, rs in sets.items():
            acc = 0.0
            for _ in range(renders):
                acc += scn.render(rs, (0.0, 0.0, 0.0), out=outs[name], stats=True)["stats"]["ms_trace"]
            ms[name].append(acc / renders)
    doc = dict(tris=int(mesh[1].shape[0]), renders_per_rep=renders, reps=reps, ms_trace={k: stat(v) for k, v in ms.items()},
               counters=counters)
    for rs in sets.values():
        rs.close()
    scn.close()
    return doc


def sequence_targets(root, targets, raw_scans, window, reps):
    """`targets`: name -> target SensorModel.  The sequence part of the docstring: returns the `sequence` record"""
    import bench_ingest as bi
    import torch
    from lidar_transfer_amd.config import load_approach
    from lidar_transfer_amd.ingest import SequenceSource
    from lidar_transfer_amd.sequence import SequenceTransfer
    sensor = (bi.H, bi.W, bi.FOV_UP, bi.FOV_DOWN)
    scans, poses = bi.make_sequence(raw_scans, 7)
    a = load_approach(os.path.join(root, "config", "approach_mergemesh.yaml"))
    runners = {}
    for name, t in targets.items():
        src = SequenceSource(scans=[s for s, _ in scans], labels=[l for _, l in scans], poses=poses, cache_scans=32)
        runners[name] = SequenceTransfer(src, a, sensor, t, out_dir=None, chains=1, evaluate=False)

    def one_pass(tr):
        n = sum(1 for _ in tr.run())
        torch.cuda.synchronize()
        return n

    for tr in runners.values():
        one_pass(tr)
    times = {k: [] for k in runners}
    for _ in range(reps):
        for name, tr in runners.items():
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < window:
                n += one_pass(tr)
            times[name].append((time.perf_counter() - t0) * 1e3 / n)
    doc = dict(workload=dict(raw_scans=len(scans), source=list(sensor), adaption="mergemesh", chains=1,
                             number_of_scans=a.number_of_scans, window_s=window, reps=reps),
               ms_per_output_scan={k: stat(v) for k, v in times.items()},
               mm_stats={k: tr.summary.get("mm_stats") for k, tr in runners.items()})
    for tr in runners.values():
        tr.source.close()
        tr.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--linear-only", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--renders", type=int, default=20)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--raw-scans", type=int, default=16)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_table.py needs a GPU")
    import lidar_transfer_amd
    from lidar_transfer_amd.config import load_sensor
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.synth import WORKLOADS
    assert os.path.abspath(lidar_transfer_amd.__file__).startswith(root + os.sep), lidar_transfer_amd.__file__
    doc = dict(root=os.path.relpath(root), linear_only=bool(args.linear_only))
    cases = {"linear 64x2048": (2.0, -24.8, 64, 2048, None), "linear 32x1024": (15.0, -25.0, 32, 1024, None)}
    if not args.linear_only:
        cases["two_block 64x2048"] = (2.0, -24.8, 64, 2048, np.array(TWO_BLOCK))
        cases["vlp32c 32x1024"] = (15.0, -25.0, 32, 1024, np.array(VLP32C))
    rays = {name: (create_rays_device(fu, fd, H, W) if table is None else create_rays_device(fu, fd, H, W, beam_table=table))
            for name, (fu, fd, H, W, table) in cases.items()}
    doc["render"] = render_cases(rays, {name: c[2] for name, c in cases.items()}, WORKLOADS["C2"]["tris"], args.reps, args.renders)
    del rays
    targets = {"vlp32_1024.yaml": load_sensor(os.path.join(root, "config", "vlp32_1024.yaml"))}
    if not args.linear_only:
        targets["vlp32c_table_1024.yaml"] = load_sensor(os.path.join(root, "config", "vlp32c_table_1024.yaml"))
    doc["sequence"] = sequence_targets(root, targets, args.raw_scans, args.window, args.reps)
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
