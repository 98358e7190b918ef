#!/usr/bin/env python3
"""What a target sensor with a horizontal sector (`azimuth_model: sector`) costs, and what the ray set's bin grid at the
sector's resolution saves: the render alone with the scatter's counters, and a whole `mergemesh` sequence per output scan.

    python tools/bench_sector.py --out profiles/sector/bench.json                          # this tree
    python tools/bench_sector.py --full-only --root PARENT --out profiles/sector/parent.json   # a checkout of the parent commit

render     `lt_stats.ms_trace` of `lt_scene_render_dev` (Scene.render(stats=True)) against the 1 M-triangle synthetic scene of
           workload C2: the 120 degree x 64 x 1024 sector of config/front120_64x1024.yaml on the default bin grid (`RaySet`
           without `grid`: 1024 azimuth bins over the circle, three rays of a row in every occupied one) and on the fitted
           grid (`sector_grid`: 3072 bins, a ray on every occupied bin's centre); the evenly spaced 64 x 3072 full-circle
           sensor, which has the same angular resolution; and the evenly spaced 64 x 2048 sensor, the unchanged path;
           `--reps` repetitions of `--renders` renders each after a warm-up, the cases alternating; median (min - max) of
           the repetitions' means, ms.  Counters: one `LT_TRACE_COUNT` render per case (`lt_stats`: nodes_visited =
           candidate bins, tris_tested, entries_culled, n_hits) and the ray set's grid.
sequence   `SequenceTransfer(chains=1)`, nothing evaluated, nothing written: the seeded sequence of tools/bench_ingest.py with
           config/approach_mergemesh.yaml, target config/vlp32_1024.yaml against config/front120_64x1024.yaml; whole passes
           for at least `--window` seconds, `--reps` repetitions alternating; ms per output scan.

`--full-only` runs the full-circle cases alone and uses nothing the parent commit lacks; `--root` names the tree whose
package and tools are imported.  Without a device the tool fails; it prints no numbers."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

FOV = (2.0, -24.8)
SECTOR = (0.0, 120.0)


def stat(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), n=len(xs))


def grid(rs):
    lib = rs._lib
    lib.lt_debug_rayset_params.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.lt_debug_rayset_params.restype = C.c_int
    nb, p = (C.c_int * 2)(), (C.c_float * 6)()
    lib.lt_debug_rayset_params(rs._h, nb, p)
    return dict(nb_az=int(nb[0]), nb_el=int(nb[1]), dev_az=float(p[4]), dev_el=float(p[5]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--full-only", action="store_true")
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
        raise SystemExit("bench_sector.py needs a GPU")
    import bench_ingest as bi
    import lidar_transfer_amd
    from lidar_transfer_amd.config import load_approach, load_sensor
    from lidar_transfer_amd.ingest import SequenceSource
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.raytracer import RaySet, Scene
    from lidar_transfer_amd.sequence import SequenceTransfer
    from lidar_transfer_amd.synth import WORKLOADS, synth_scene
    assert os.path.abspath(lidar_transfer_amd.__file__).startswith(root + os.sep), lidar_transfer_amd.__file__
    dev = torch.device("cuda", 0)
    doc = dict(root=os.path.relpath(root), full_only=bool(args.full_only))

    # ---- the render alone ----------------------------------------------------------------------------------------------------
    # (H, W, sector, fitted grid?)
    cases = {"full 64x2048": (64, 2048, None, False), "full 64x3072": (64, 3072, None, False)}
    if not args.full_only:
        from lidar_transfer_amd.raytracer import sector_grid
        cases["sector 120 64x1024, default grid"] = (64, 1024, SECTOR, False)
        cases["sector 120 64x1024, fitted grid"] = (64, 1024, SECTOR, True)
    scn = Scene(0)
    mesh = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in synth_scene(0, WORKLOADS["C2"]["tris"])]
    scn.set_mesh(*mesh)
    sets, outs, counters = {}, {}, {}
    for name, (H, W, sector, fitted) in cases.items():
        rays = create_rays_device(FOV[0], FOV[1], H, W) if sector is None else create_rays_device(FOV[0], FOV[1], H, W, sector=sector)
        sets[name] = (RaySet(rays, H, sector=sector, grid=sector_grid(W, sector)) if fitted else RaySet(rays, H), rays)
        outs[name] = scn.alloc_outputs(H * W)
    for name, (rs, _) in sets.items():          # warm-up, counters
        for _ in range(3):
            o = scn.render(rs, (0.0, 0.0, 0.0), out=outs[name], count=True)
        s = o["stats"]
        counters[name] = dict(grid(rs), n_rays=int(s["n_rays"]), n_hits=int(s["n_hits"]), candidate_bins=int(s["nodes_visited"]),
                              tris_tested=int(s["tris_tested"]), tris_tested_per_ray=float(s["tris_tested"]) / max(int(s["n_rays"]), 1),
                              entries_culled=int(s["entries_culled"]))
    ms = {k: [] for k in sets}
    for _ in range(args.reps):
        for name, (rs, _) in sets.items():
            acc = 0.0
            for _ in range(args.renders):
                acc += scn.render(rs, (0.0, 0.0, 0.0), out=outs[name], stats=True)["stats"]["ms_trace"]
            ms[name].append(acc / args.renders)
    doc["render"] = dict(tris=int(mesh[1].shape[0]), renders_per_rep=args.renders, reps=args.reps,
                         ms_trace={k: stat(v) for k, v in ms.items()}, counters=counters)
    for rs, _ in sets.values():
        rs.close()
    scn.close()
    del mesh, outs

    # ---- a whole sequence ------------------------------------------------------------------------------------------------------
    sensor = (bi.H, bi.W, bi.FOV_UP, bi.FOV_DOWN)
    scans, poses = bi.make_sequence(args.raw_scans, 7)
    a = load_approach(os.path.join(root, "config", "approach_mergemesh.yaml"))
    targets = {"vlp32_1024.yaml": load_sensor(os.path.join(root, "config", "vlp32_1024.yaml"))}
    if not args.full_only:
        targets["front120_64x1024.yaml"] = load_sensor(os.path.join(root, "config", "front120_64x1024.yaml"))
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
    for _ in range(args.reps):
        for name, tr in runners.items():
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < args.window:
                n += one_pass(tr)
            times[name].append((time.perf_counter() - t0) * 1e3 / n)
    doc["sequence"] = dict(workload=dict(raw_scans=len(scans), source=list(sensor), adaption="mergemesh", chains=1,
                                         number_of_scans=a.number_of_scans, window_s=args.window, reps=args.reps),
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
