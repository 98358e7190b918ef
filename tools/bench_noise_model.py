#!/usr/bin/env python3
"""What the target sensor's noise model (`noise_model`) costs: its kernel beside the return model's by HIP events
(and, under the profiler, in one trace), and a whole `mergemesh` sequence per output scan with and without the key -- the
method of tools/bench_return_model.py.

    python tools/bench_noise_model.py --out profiles/noise_model/bench.json          # this tree
    python tools/bench_return_model.py --out profiles/noise_model/parent.json        # in a checkout of the parent commit: its own
                                                                                     # tool, the same sequence body

kernel     `lt_return_model_dev` and then `lt_noise_model_dev` with the models of config/vlp32c_table_noise_1024.yaml behind
           `lt_scene_render_dev` against the 1 M-triangle synthetic scene of workload C2, at 64 x 2048 (the reference's rays) and
           at 32 x 1024 (the VLP-32C table): every iteration renders the scan again (both models are read-modify-write) and
           times each call alone between two HIP events on the stream; `--reps` repetitions of `--renders` iterations after a
           warm-up, the cases alternating; median (min - max) of the repetitions' means, microseconds.  Run under
           `rocprofv3 --kernel-trace --stats` with `--kernel-only` the same loop gives `k_return_model` and `k_noise_model` side
           by side in one trace (`--case`: one shape per trace).
sequence   `SequenceTransfer(chains=1)`, nothing evaluated, nothing written: the seeded sequence of tools/bench_ingest.py with
           config/approach_mergemesh.yaml, targets config/vlp32c_table_1024.yaml, config/vlp32c_table_returns_1024.yaml and
           config/vlp32c_table_noise_1024.yaml (the second plus the noise block); whole passes for at least `--window` seconds,
           `--reps` repetitions alternating; ms per output scan.

Without a device the tool fails; it prints no numbers."""
import argparse
import json
import os
import sys

import bench_beam_table as bbt   # stat() and the sequence body


def kernel_cases(cases, returns, noise, tris, reps, renders):
    """`cases`: name -> (rays [H * W, 3] device, H).  The kernel part of the docstring: returns the `kernel` record"""
    import numpy as np
    import torch
    from lidar_transfer_amd import post
    from lidar_transfer_amd.raytracer import RaySet, Scene
    from lidar_transfer_amd.synth import synth_scene
    dev = torch.device("cuda", 0)
    scn = Scene(0)
    mesh = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in synth_scene(0, tris)]
    scn.set_mesh(*mesh)
    st = torch.cuda.current_stream(dev)
    sets, outs, extra, more, totals = {}, {}, {}, {}, {}
    for name, (r, h) in cases.items():
        n = r.shape[0]
        sets[name] = RaySet(r, h)
        outs[name] = scn.alloc_outputs(n, label_image=True)
        extra[name] = dict(incidence=torch.empty(n, dtype=torch.float32, device=dev), drop=torch.empty(n, dtype=torch.uint8, device=dev))
        more[name] = dict(range_error=torch.empty(n, dtype=torch.float32, device=dev), state=torch.empty(n, dtype=torch.uint8, device=dev))

    def one(name, k):
        scn.render(sets[name], (0.0, 0.0, 0.0), out=outs[name], label_image=True)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record(st)
        post.return_model(scn, cases[name][0], returns, k, outs[name], stream=st, **extra[name])
        e[1].record(st)
        post.noise_model((0.0, 0.0, 0.0), noise, k, outs[name], gate=returns, stream=st, **more[name])
        e[2].record(st)
        e[2].synchronize()
        return e[0].elapsed_time(e[1]) * 1e3, e[1].elapsed_time(e[2]) * 1e3

    for name in cases:   # warm-up, totals
        for k in range(5):
            one(name, k)
        err = more[name]["range_error"].double()
        on = more[name]["state"] == 1
        totals[name] = dict(cells_per_state=torch.bincount(more[name]["state"].long(), minlength=3).cpu().tolist(),
                            range_error_rms=float(err[on].square().mean().sqrt()) if bool(on.any()) else None)
    ret_us, noise_us = {k: [] for k in cases}, {k: [] for k in cases}
    for _ in range(reps):
        for name in cases:
            got = [one(name, k) for k in range(renders)]
            ret_us[name].append(sum(g[0] for g in got) / renders)
            noise_us[name].append(sum(g[1] for g in got) / renders)
    doc = dict(tris=int(mesh[1].shape[0]), iterations_per_rep=renders, reps=reps, return_model=returns.fields(),
               noise_model=noise.fields(), return_model_us={k: bbt.stat(v) for k, v in ret_us.items()},
               noise_model_us={k: bbt.stat(v) for k, v in noise_us.items()}, scans=totals)
    for rs in sets.values():
        rs.close()
    scn.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--sequence-only", action="store_true")
    ap.add_argument("--case", default="", help="the kernel part at this shape alone (64x2048 or 'vlp32c 32x1024'): one shape per trace")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--renders", type=int, default=20)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--raw-scans", type=int, default=16)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_noise_model.py needs a GPU")
    from lidar_transfer_amd.config import load_sensor
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.synth import WORKLOADS
    names = ("vlp32c_table_1024.yaml", "vlp32c_table_returns_1024.yaml", "vlp32c_table_noise_1024.yaml")
    targets = {n: load_sensor(os.path.join(root, "config", n)) for n in names}
    full = targets[names[2]]
    doc = {}
    if not args.sequence_only:
        c2 = WORKLOADS["C2"]
        cases = {"64x2048": (create_rays_device(c2["fov_up"], c2["fov_down"], c2["H"], c2["W"]), c2["H"]),
                 "vlp32c 32x1024": (create_rays_device(full.fov_up, full.fov_down, full.H, full.W, beam_table=full.beam_table()), full.H)}
        if args.case:
            cases = {args.case: cases[args.case]}
        doc["kernel"] = kernel_cases(cases, full.return_model(), full.noise_model(), c2["tris"], args.reps, args.renders)
        del cases
    if not args.kernel_only:
        doc["sequence"] = bbt.sequence_targets(root, targets, args.raw_scans, args.window, args.reps)
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
