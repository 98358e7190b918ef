#!/usr/bin/env python3
"""Host + device time of one DeviceDeform.cp() call (pack=True: the call ends in the read-back of the packed count, a device
synchronise) for three targets at 32 x 1024: evenly spaced, the VLP-32C table, the table with the offsets of
config/vlp32c_table_az_1024.yaml.  Cloud: synth_cloud(3, 120000, fov_up=15) as float64.  Per case: warm-up of 50 calls, then
`--reps` windows of at least `--window` seconds, the cases alternating; microseconds per call, median (min - max).
    python profiles/target_model/cp_call.py --root TREE --out FILE.json   # TREE: a built checkout"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True)
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cp_call.py needs a GPU")
    import lidar_transfer_amd
    from lidar_transfer_amd.config import load_sensor
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.synth import synth_cloud
    assert os.path.abspath(lidar_transfer_amd.__file__).startswith(root + os.sep), lidar_transfer_amd.__file__
    p, rm, lb = synth_cloud(3, 120000, dtype=np.float64, fov_up=15.0)
    cloud = (torch.from_numpy(p).cuda(), torch.from_numpy(rm).cuda(), torch.from_numpy(lb.astype(np.int32)).cuda())
    az = load_sensor(os.path.join(root, "config", "vlp32c_table_az_1024.yaml"))
    tgt = (az.H, az.W, az.fov_up, az.fov_down)
    src = (64, 2048, 3.0, -25.0)
    cases = {"linear 32x1024": {}, "vlp32c table": dict(t_beam_table=az.beam_table()),
             "vlp32c table + offsets": dict(t_beam_table=az.beam_table(), t_beam_azimuth=az.beam_azimuth())}
    dds = {k: DeviceDeform(src, tgt, None, **kw) for k, kw in cases.items()}
    kept = {}
    for k, dd in dds.items():
        for _ in range(50):
            out = dd.cp([cloud])
        torch.cuda.synchronize()
        kept[k] = int(out["bin"].shape[0])
    res = {k: [] for k in dds}
    for _ in range(args.reps):
        for k, dd in dds.items():
            n, t0 = 0, time.perf_counter()
            while True:
                for _ in range(100):
                    dd.cp([cloud])
                n += 100
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= args.window:
                    break
            res[k].append(dt / n * 1e6)
    doc = dict(root=os.path.relpath(root), points=int(p.shape[0]), target=list(tgt),
               cp_us_per_call={k: dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v, packed_points=kept[k])
                               for k, v in res.items()})
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
