#!/usr/bin/env python3
"""What a dual-return target sensor (`dual_return`) costs: the dual resolve beside the single one in one kernel
trace, and a whole `mergemesh` sequence per output scan with and without the block -- the method of tools/bench_echo_model.py,
whose `--kernel-only` trace and `--sequence-only` pass measure the parent commit and the single resolve of this tree.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o s -- python tools/bench_dual_return.py --kernel-only --case 64x2048
    python tools/bench_dual_return.py --sequence-only --out profiles/dual_return/seq_tree.json

kernel     with the models of config/vlp32c_table_dual_1024.yaml (S = 5, strongest, second: last) against the 1 M-triangle
           synthetic scene of workload C2, at 64 x 2048 (the reference's rays) or at 32 x 1024 (the VLP-32C table; `--case`:
           one shape per trace): the sub-ray set is rendered once, then `lt_echo_resolve_dev` and `lt_echo_resolve_dual_dev`
           run `--launches` times each on its sub-images, alternating, after a warm-up of five; the trace's `k_echo_resolve`
           and `k_echo_resolve_dual` rows are the result.  The tool prints the cells per number of echoes and the second
           returns, and checks that the dual call's primary images are the single call's.
sequence   `SequenceTransfer(chains=1)`, nothing evaluated, nothing written: the seeded sequence of tools/bench_ingest.py with
           config/approach_mergemesh.yaml, targets config/vlp32c_table_echo_1024.yaml and config/vlp32c_table_dual_1024.yaml
           (the first plus the block); whole passes for at least `--window` seconds, `--reps` repetitions alternating; ms per
           output scan.

Without a device the tool fails; it prints no numbers."""
import argparse
import json
import os
import sys

import bench_beam_table as bbt   # stat() and the sequence body


def kernel_case(rays, h, echo, dual, tris, launches):
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
    n, S, org = rays.shape[0], echo.subrays, (0.0, 0.0, 0.0)
    sub = post.create_subrays(rays, echo)
    rs = RaySet(sub, S * h, grid=_chain.Echoes.grid_of(None, h))
    subout = scn.render(rs, org, out=scn.alloc_outputs(S * n, label_image=True), label_image=True)
    one, two, ref = (scn.alloc_outputs(n, label_image=True) for _ in range(3))
    more = dict(n_echoes=torch.empty(n, dtype=torch.uint8, device=dev), fraction=torch.empty(n, dtype=torch.float32, device=dev))
    more2 = dict(more, fraction2=torch.empty(n, dtype=torch.float32, device=dev))
    for k in range(5 + launches):
        post.echo_resolve(rays, org, echo, subout, ref, stream=st, **more)
        post.echo_resolve_dual(rays, org, echo, dual, subout, one, two, stream=st, **more2)
    torch.cuda.synchronize()
    for k in ("endpoints", "endcolors", "range", "endrem", "tri"):
        assert torch.equal(one[k].view(torch.int32), ref[k].view(torch.int32)), k
    ne = more["n_echoes"]
    doc = dict(tris=int(mesh[1].shape[0]), H=h, W=n // h, launches_each=5 + launches, echo_model=echo.fields(), dual_return=dual.fields(),
               cells_none_one_several=torch.bincount(ne.clamp(max=2).long(), minlength=3).cpu().tolist(),
               second_returns=int((two["tri"] >= 0).sum()))
    rs.close()
    scn.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--sequence-only", action="store_true")
    ap.add_argument("--case", default="64x2048", help="the kernel part's shape: 64x2048 or 'vlp32c 32x1024'")
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--raw-scans", type=int, default=16)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dual_return.py needs a GPU")
    from lidar_transfer_amd.config import load_sensor
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.synth import WORKLOADS
    names = ("vlp32c_table_echo_1024.yaml", "vlp32c_table_dual_1024.yaml")
    targets = {n: load_sensor(os.path.join(root, "config", n)) for n in names}
    full = targets[names[1]]
    doc = {}
    if not args.sequence_only:
        c2 = WORKLOADS["C2"]
        if args.case == "64x2048":
            rays, h = create_rays_device(c2["fov_up"], c2["fov_down"], c2["H"], c2["W"]), c2["H"]
        else:
            rays, h = create_rays_device(full.fov_up, full.fov_down, full.H, full.W, beam_table=full.beam_table()), full.H
        doc["kernel"] = {args.case: kernel_case(rays, h, full.echo_model(), full.dual_return(), c2["tris"], args.launches)}
    if not args.kernel_only:
        doc["sequence"] = bbt.sequence_targets(root, targets, args.raw_scans, args.window, args.reps)
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
