#!/usr/bin/env python3
"""What a rig of K sensors costs to render from one scene, by HIP events:

    python tools/rig_time.py --out profiles/rig/render.json

scene     the 1 M-triangle synthetic scene of workload C2 (`synth_scene(0, 1_000_000)`), K = 1, 2, 4, 8 heads of 64 x 2048 at
          distinct poses (each head yawed and pitched a little and moved by some decimetres: a ray set of its own per head).
cases     `single`  K successive `lt_scene_render_dev` calls (what exists without the rig call);
          `rig`     one `lt_scene_render_rig_dev` call (k_sc_tris, k_sc_rest, k_sc_resolve over K jobs that share the mesh).
          The images of the two cases are compared bit for bit before anything is timed.  (profiles/rig/README.md also holds
          the figures of a kernel that looped over the sensors inside a triangle block; it lost and left the sources.)
timing    every case between two HIP events on the stream, `--renders` calls per timing; `--reps` series, the cases
          alternating inside every series after a warm-up; per case the median of the series' means and their min - max (the
          spread between series), microseconds per rig.
chain     `--chain`: a `mesh` and a `mergemesh` output scan of config/approach_rig_example.yaml as a `RigDeform` against the
          sum of the single-sensor `DeviceDeform` scans of its heads, on synthetic clouds; ms per output scan.

Without a device the tool fails; it prints no numbers."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])


def heads_of(K, H, W, dev):
    import numpy as np
    import torch
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.raytracer import RaySet
    sets, origins = [], []
    for k in range(K):
        y, p = np.deg2rad(11.0 * k), np.deg2rad(1.5 * k)
        Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1.0]])
        Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1.0, 0], [-np.sin(p), 0, np.cos(p)]])
        rays = create_rays_device(3.0, -25.0, H, W, device=dev.index, rot=(Rz @ Ry) if k else None)
        sets.append(RaySet(rays, H))
        origins.append((0.3 * k, -0.2 * k, 0.05 * k))
    torch.cuda.synchronize()
    return sets, origins


def render_cases(tris, H, W, reps, renders):
    import numpy as np
    import torch
    from lidar_transfer_amd.raytracer import Scene
    from lidar_transfer_amd.synth import synth_scene
    dev = torch.device("cuda", 0)
    scn = Scene(0)
    mesh = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in synth_scene(0, tris)]
    scn.set_mesh(*mesh)
    st = torch.cuda.current_stream(dev)
    record = {}
    sets, origins = heads_of(8, H, W, dev)
    cases = ("single", "rig")
    outs = {c: [scn.alloc_outputs(H * W, label_image=True) for _ in range(8)] for c in cases}

    def run(case, K):
        if case == "single":
            for k in range(K):
                scn.render(sets[k], origins[k], out=outs[case][k], label_image=True)
        else:
            scn.render_rig(sets[:K], origins[:K], outs=outs[case][:K], label_image=True)

    for K in (1, 2, 4, 8):
        for c in cases:
            run(c, K)
        torch.cuda.synchronize()
        for c in cases[1:]:   # the same images
            for k in range(K):
                for key in ("endpoints", "endcolors", "range", "endrem", "tri"):
                    assert torch.equal(outs[c][k][key].view(torch.int32), outs["single"][k][key].view(torch.int32)), (c, K, k, key)
        for c in cases:    # warm-up
            for _ in range(renders):
                run(c, K)
        torch.cuda.synchronize()
        series = {c: [] for c in cases}
        for _ in range(reps):
            for c in cases:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(renders):
                    run(c, K)
                e1.record(st)
                e1.synchronize()
                series[c].append(1000.0 * e0.elapsed_time(e1) / renders)
        record[str(K)] = {c: stat(v) for c, v in series.items()}
        print("K=%d  " % K + "  ".join("%s %.1f (%.1f - %.1f) us" % (c, s["median"], s["min"], s["max"])
                                        for c, s in record[str(K)].items()), flush=True)
    scn.status()
    return record


def chain_cases(reps, scans):
    import numpy as np
    import torch
    from lidar_transfer_amd.config import load_approach
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.rig import RigDeform, head_keywords
    from lidar_transfer_amd.synth import synth_cloud
    dev = torch.device("cuda", 0)
    ap = load_approach(os.path.join(ROOT, "config", "approach_rig_example.yaml"))
    heads = ap.rig()
    source = (64, 2048, 3.0, -25.0)
    st = torch.cuda.current_stream(dev)
    clouds = [[tuple(torch.from_numpy(np.ascontiguousarray(a if i else a.astype(np.float32))).to(dev) if i != 2 else
                     torch.from_numpy(a.astype(np.int32)).to(dev) for i, a in enumerate(synth_cloud(100 + 7 * s + k)))
               for k in range(ap.number_of_scans)] for s in range(scans)]
    record = {}
    for adaption in ("mesh", "mergemesh"):
        if adaption == "mergemesh" and any(h.sensor.fov_up > heads[0].sensor.fov_up or h.sensor.fov_down < heads[0].sensor.fov_down
                                           for h in heads[1:]):
            continue
        bnds = np.array(ap.voxel_bounds, dtype=np.float64)
        rig = RigDeform(source, heads, bnds.copy(), ap.voxel_size, mesh_volume=adaption == "mesh")
        singles = []
        for h in heads:
            target, kw = head_keywords(h.sensor)
            singles.append(DeviceDeform(source, target, bnds.copy(), ap.voxel_size, transformation=h.mount,
                                        mesh_volume=adaption == "mesh", **kw))

        def run(what):
            for s in range(scans):
                if what == "rig":
                    getattr(rig, adaption)(clouds[s], scan_index=s)
                else:
                    for dd in singles:
                        getattr(dd, adaption)(clouds[s], scan_index=s)

        for what in ("rig", "singles"):
            run(what)
        torch.cuda.synchronize()
        series = {"rig": [], "singles": []}
        for _ in range(reps):
            for what in series:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                run(what)
                e1.record(st)
                e1.synchronize()
                series[what].append(e0.elapsed_time(e1) / scans)
        record[adaption] = {c: stat(v) for c, v in series.items()}
        print(adaption + "  " + "  ".join("%s %.3f (%.3f - %.3f) ms" % (c, s["median"], s["min"], s["max"])
                                          for c, s in record[adaption].items()), flush=True)
        rig.close()
        for dd in singles:
            dd.close()
    return record


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--renders", type=int, default=20)
    ap.add_argument("--chain", action="store_true")
    ap.add_argument("--scans", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = dict(render=render_cases(a.tris, 64, 2048, a.reps, a.renders))
    if a.chain:
        rec["chain"] = chain_cases(a.reps, a.scans)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
