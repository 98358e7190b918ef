#!/usr/bin/env python3
"""What the target sensor's echo model (`echo_model`) costs: its two kernels and the render of the sub-ray set
beside the plain render by HIP events (and, under the profiler, the two kernels in one trace), the bin grids tried for the
sub-ray set, and a whole `mergemesh` sequence per output scan with and without the key -- the method of
tools/bench_noise_model.py.

    python tools/bench_echo_model.py --out profiles/echo_model/bench.json            # this tree
    python tools/bench_noise_model.py --sequence-only --out profiles/echo_model/parent.json   # in a checkout of the parent
                                                                                      # commit: its own tool, the same sequence body

kernel     with the model of config/vlp32c_table_echo_1024.yaml (S = 5) against the 1 M-triangle synthetic scene of workload
           C2, at 64 x 2048 (the reference's rays) and at 32 x 1024 (the VLP-32C table): `lt_create_subrays_dev`, then per
           iteration the plain render (`lt_scene_render_dev` of the H x W ray set), the render of the S * H x W sub-ray set
           under each bin grid tried, and `lt_echo_resolve_dev` on the sub-images, each alone between two HIP events on the
           stream; `--reps` repetitions of `--renders` iterations after a warm-up, the cases alternating; median (min - max) of
           the repetitions' means, microseconds.  The grids: `central` -- the central set's azimuth rule and H elevation rows,
           what `_chain.Echoes.grid_of` makes; `image` -- the image's own rule for the taller set, S * H rows; `az2` -- the
           central grid with the azimuth bins doubled.  Every grid renders the same image: the tool checks it.  Run under
           `rocprofv3 --kernel-trace --stats` with `--kernel-only` the same loop gives `k_subrays` and `k_echo_resolve` beside
           `k_sc_resolve` in one trace (`--case`: one shape per trace).
sequence   `SequenceTransfer(chains=1)`, nothing evaluated, nothing written: the seeded sequence of tools/bench_ingest.py with
           config/approach_mergemesh.yaml, targets config/vlp32c_table_noise_1024.yaml and config/vlp32c_table_echo_1024.yaml
           (the first plus the echo block); whole passes for at least `--window` seconds, `--reps` repetitions alternating; ms
           per output scan.

Without a device the tool fails; it prints no numbers."""
import argparse
import json
import os
import sys

import bench_beam_table as bbt   # stat(), grid() and the sequence body


def kernel_cases(cases, echo, tris, reps, renders):
    """`cases`: name -> (rays [H * W, 3] device, H).  The kernel part of the docstring: returns the `kernel` record"""
    import numpy as np
    import torch
    from lidar_transfer_amd import _chain, post
    from lidar_transfer_amd.raytracer import RaySet, Scene
    from lidar_transfer_amd.synth import synth_scene
    dev = torch.device("cuda", 0)
    scn = Scene(0)
    mesh = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in synth_scene(0, tris)]
    scn.set_mesh(*mesh)
    st = torch.cuda.current_stream(dev)
    S = echo.subrays
    org = (0.0, 0.0, 0.0)
    state, info = {}, {}
    for name, (r, h) in cases.items():
        n, w = r.shape[0], r.shape[0] // h
        sub = post.create_subrays(r, echo)
        plain = RaySet(r, h)
        az = bbt.grid(plain)["nb_az"]
        grids = dict(central=_chain.Echoes.grid_of(None, h), image=None, az2=(2 * az, h))
        sets = {g: RaySet(sub, S * h, grid=grids[g]) for g in grids}
        state[name] = dict(rays=r, sub=sub, plain=plain, sets=sets, out=scn.alloc_outputs(n, label_image=True),
                           subout={g: scn.alloc_outputs(S * n, label_image=True) for g in grids},
                           more=dict(n_echoes=torch.empty(n, dtype=torch.uint8, device=dev), fraction=torch.empty(n, dtype=torch.float32, device=dev)))
        info[name] = dict(H=h, W=w, plain_grid=bbt.grid(plain), sub_grids={g: bbt.grid(rs) for g, rs in sets.items()})

    def timed(f):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record(st)
        f()
        e[1].record(st)
        e[1].synchronize()
        return e[0].elapsed_time(e[1]) * 1e3

    def one(name):
        s = state[name]
        t = dict(subrays=timed(lambda: post.create_subrays(s["rays"], echo, stream=st)),
                 plain_render=timed(lambda: scn.render(s["plain"], org, out=s["out"], label_image=True)))
        for g, rs in s["sets"].items():
            t["sub_render_" + g] = timed(lambda: scn.render(rs, org, out=s["subout"][g], label_image=True))
        t["resolve"] = timed(lambda: post.echo_resolve(s["rays"], org, echo, s["subout"]["central"], s["out"], stream=st, **s["more"]))
        return t

    for name in cases:   # warm-up, the grids render one image, totals
        for _ in range(5):
            one(name)
        s = state[name]
        for g in s["sets"]:
            for k in ("range", "endcolors", "endrem", "tri"):
                assert torch.equal(s["subout"][g][k], s["subout"]["central"][k]), (name, g, k)
        ne = s["more"]["n_echoes"]
        info[name]["cells_none_one_several"] = torch.bincount(ne.clamp(max=2).long(), minlength=3).cpu().tolist()
        info[name]["mean_fraction"] = float(s["more"]["fraction"][ne > 0].double().mean())
    us = {name: {} for name in cases}
    for _ in range(reps):
        for name in cases:
            got = [one(name) for _ in range(renders)]
            for k in got[0]:
                us[name].setdefault(k, []).append(sum(g[k] for g in got) / renders)
    doc = dict(tris=int(mesh[1].shape[0]), iterations_per_rep=renders, reps=reps, echo_model=echo.fields(),
               us={name: {k: bbt.stat(v) for k, v in d.items()} for name, d in us.items()}, scans=info)
    for name, d in us.items():
        plain = bbt.stat(d["plain_render"])["median"]
        doc["scans"][name]["sub_render_over_plain"] = {g: bbt.stat(d["sub_render_" + g])["median"] / plain for g in state[name]["sets"]}
    for s in state.values():
        s["plain"].close()
        for rs in s["sets"].values():
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
        raise SystemExit("bench_echo_model.py needs a GPU")
    from lidar_transfer_amd.config import load_sensor
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.synth import WORKLOADS
    names = ("vlp32c_table_noise_1024.yaml", "vlp32c_table_echo_1024.yaml")
    targets = {n: load_sensor(os.path.join(root, "config", n)) for n in names}
    full = targets[names[1]]
    doc = {}
    if not args.sequence_only:
        c2 = WORKLOADS["C2"]
        cases = {"64x2048": (create_rays_device(c2["fov_up"], c2["fov_down"], c2["H"], c2["W"]), c2["H"]),
                 "vlp32c 32x1024": (create_rays_device(full.fov_up, full.fov_down, full.H, full.W, beam_table=full.beam_table()), full.H)}
        if args.case:
            cases = {args.case: cases[args.case]}
        doc["kernel"] = kernel_cases(cases, full.echo_model(), c2["tris"], args.reps, args.renders)
        del cases
    if not args.kernel_only:
        doc["sequence"] = bbt.sequence_targets(root, targets, args.raw_scans, args.window, args.reps)
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
