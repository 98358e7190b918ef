#!/usr/bin/env python3
"""What a target sensor at a pose of its own (`transformation` of the approach file) costs: the render alone, and a whole
sequence per output scan -- and that the identity path costs what it cost before.

    python tools/bench_mount.py --out profiles/mount/bench_mount.json                            # this tree
    python tools/bench_mount.py --identity-only --root PARENT --out profiles/mount/parent.json   # a checkout of the parent commit

render     `lt_stats.ms_trace` of `lt_scene_render_dev` (Scene.render(stats=True)): workload C2, a 64 x 2048 sensor against the
           1 M-triangle synthetic scene; rays of the identity, of a translation only (0.4 m lower) and of the pose of
           config/approach_mount_example.yaml (0.4 m lower, pitched 5 degrees down); `--reps` repetitions of `--renders`
           renders each after a warm-up, the cases alternating; median (min - max) of the repetitions' means, ms.
sequence   `SequenceTransfer(chains=1)`, nothing evaluated, nothing written: the seeded sequence of tools/bench_ingest.py,
           config/approach_mergemesh.yaml against config/approach_mount_example.yaml; whole passes for at least `--window`
           seconds, `--reps` repetitions alternating; ms per output scan.

`--identity-only` runs the identity cases alone and uses nothing the parent commit lacks; `--root` names the tree whose
package and tools are imported.  Without a device the tool fails; it prints no numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np


def stat(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--identity-only", action="store_true")
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
        raise SystemExit("bench_mount.py needs a GPU")
    import bench_ingest as bi
    import lidar_transfer_amd
    from lidar_transfer_amd.config import load_approach
    from lidar_transfer_amd.ingest import SequenceSource
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.raytracer import RaySet, Scene
    from lidar_transfer_amd.sequence import SequenceTransfer
    from lidar_transfer_amd.synth import WORKLOADS, synth_scene
    assert os.path.abspath(lidar_transfer_amd.__file__).startswith(root + os.sep), lidar_transfer_amd.__file__
    dev = torch.device("cuda", 0)
    doc = dict(root=os.path.relpath(root), identity_only=bool(args.identity_only))

    # ---- the render alone ----------------------------------------------------------------------------------------------------
    wl = WORKLOADS["C2"]
    H, W, fu, fd = wl["H"], wl["W"], wl["fov_up"], wl["fov_down"]
    cases = {"identity": (None, (0.0, 0.0, 0.0))}
    if not args.identity_only:
        example = load_approach(os.path.join(root, "config", "approach_mount_example.yaml")).mount()[1]
        org = tuple(float(np.float32(x)) for x in example[:3, 3])
        cases["translation"] = (None, org)
        cases["example"] = (example[:3, :3], org)
    scn = Scene(0)
    mesh = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in synth_scene(0, wl["tris"])]
    scn.set_mesh(*mesh)
    sets = {}
    for name, (rot, org) in cases.items():
        rays = create_rays_device(fu, fd, H, W) if rot is None else create_rays_device(fu, fd, H, W, rot=rot)
        sets[name] = (RaySet(rays, H), org, rays)
    out = scn.alloc_outputs(H * W)
    hits = {}
    for name, (rs, org, _) in sets.items():          # warm-up
        for _ in range(3):
            o = scn.render(rs, org, out=out, count=True)
        hits[name] = int(o["stats"]["n_hits"])
    ms = {k: [] for k in sets}
    for _ in range(args.reps):
        for name, (rs, org, _) in sets.items():
            acc = 0.0
            for _ in range(args.renders):
                acc += scn.render(rs, org, out=out, stats=True)["stats"]["ms_trace"]
            ms[name].append(acc / args.renders)
    doc["render"] = dict(workload=dict(H=H, W=W, fov_up=fu, fov_down=fd, tris=int(mesh[1].shape[0]), renders_per_rep=args.renders,
                                       reps=args.reps),
                         ms_trace={k: stat(v) for k, v in ms.items()}, n_hits=hits)
    for rs, _, _ in sets.values():
        rs.close()
    scn.close()
    del mesh, out

    # ---- a whole sequence ------------------------------------------------------------------------------------------------------
    sensor = (bi.H, bi.W, bi.FOV_UP, bi.FOV_DOWN)
    scans, poses = bi.make_sequence(args.raw_scans, 7)
    approaches = {"identity": load_approach(os.path.join(root, "config", "approach_mergemesh.yaml"))}
    if not args.identity_only:
        approaches["example"] = load_approach(os.path.join(root, "config", "approach_mount_example.yaml"))
    runners = {}
    for name, a in approaches.items():
        src = SequenceSource(scans=[s for s, _ in scans], labels=[l for _, l in scans], poses=poses, cache_scans=32)
        runners[name] = SequenceTransfer(src, a, sensor, sensor, out_dir=None, chains=1, evaluate=False)

    def one_pass(tr):
        n = sum(1 for _ in tr.run())
        torch.cuda.synchronize()
        return n

    for tr in runners.values():
        one_pass(tr)
    times = {k: [] for k in runners}
    for _ in range(args.reps):
        for name, tr in runners.items():
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < args.window:
                n += one_pass(tr)
            times[name].append((time.perf_counter() - t0) * 1e3 / n)
    doc["sequence"] = dict(workload=dict(raw_scans=len(scans), sensor=list(sensor), adaption="mergemesh", chains=1,
                                         number_of_scans=approaches["identity"].number_of_scans, window_s=args.window, reps=args.reps),
                           ms_per_output_scan={k: stat(v) for k, v in times.items()},
                           mm_stats={k: tr.summary.get("mm_stats") for k, tr in runners.items()})
    for tr in runners.values():
        tr.source.close()
        tr.close()
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
