#!/usr/bin/env python3
"""What evaluating through the target view (`lt_target_view_dev`) costs: its call alone by HIP events beside the
calls it stands next to, and a whole `mergemesh` sequence per output scan with `evaluate="target"` and with no evaluation --
the method of tools/bench_beam_table.py.

    python tools/bench_target_view.py --out profiles/target_eval/bench.json

calls      on ONE resident raw scan of the seeded sequence of tools/bench_ingest.py (about 120 k points), the example
           mounting of config/approach_mount_example.yaml, `ignore` of config/approach_mergemesh.yaml:
             view vlp32c_az   `Evaluator.target_view` for config/vlp32c_table_az_1024.yaml (table + offsets, 32 x 1024)
             view 64x2048     ... for a linear 64 x 2048 target with another field of view (10 .. -30)
             source 64x2048   `Evaluator.source_scan`, the source reference scan
             composed ...     the route the view replaces: `lt_ingest_scans_dev` of the one scan with poses[0] = T, then
                              `Projector.project` (range, remission, label) under the same model
           `--iters` calls between two HIP events on the stream, `--reps` repetitions after a warm-up, the cases alternating;
           median (min - max) of the repetitions' means, microseconds per call.  The Python wrapper's allocation of the five
           output images is inside every figure, for all cases alike.
sequence   `SequenceTransfer(chains=1)`, nothing written, target config/vlp32c_table_az_1024.yaml, the example mounting:
           `evaluate="target"` against `evaluate=False`; whole passes for at least `--window` seconds, `--reps` repetitions
           alternating; ms per output scan.

Without a device the tool fails; it prints no numbers."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stat(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), n=len(xs))


def call_cases(scan, approach, T, targets, source, iters, reps):
    import torch
    from lidar_transfer_amd import _lib
    from lidar_transfer_amd.evaluate import Evaluator
    from lidar_transfer_amd.laserscan import Projector
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    lib = _lib.load()
    xyzr, label = torch.from_numpy(scan[0]).to(dev), torch.from_numpy(scan[1].view(np.int32)).to(dev)
    n = int(label.shape[0])
    lut = approach.color_lut()
    ign = (C.c_int * max(len(approach.ignore), 1))(*approach.ignore)
    pose = np.ascontiguousarray(T, np.float64).reshape(1, 16)
    pts, rem, lab = (torch.empty((n, 3), dtype=torch.float64, device=dev), torch.empty(n, device=dev),
                     torch.empty(n, dtype=torch.int32, device=dev))
    n_kept = torch.empty(2, dtype=torch.int32, device=dev)
    work = torch.empty(_lib.ingest_work_ints(n, 1), dtype=torch.int32, device=dev)
    rs = (_lib.RawScan * 1)(_lib.RawScan(xyzr.data_ptr(), label.data_ptr(), n))
    io = (_lib.IngestOut * 1)(_lib.IngestOut(pts.data_ptr(), rem.data_ptr(), lab.data_ptr()))
    pj = Projector(0)
    cases, keep = {}, [pj]
    for name, (t, model) in targets.items():
        e = Evaluator(source, approach.ignore, lut, target=t, target_model=model, transformation=T)
        keep.append(e)
        cases["view " + name] = lambda e=e: e.target_view(xyzr, label, stream=st)

        def composed(t=t, model=model):
            _lib.check(lib.lt_ingest_scans_dev(1, rs, pose.ctypes.data_as(C.POINTER(C.c_double)), None, ign, len(approach.ignore),
                                               None, 0, _lib.LT_INGEST_MERGED, io, C.c_void_p(n_kept.data_ptr()),
                                               C.c_void_p(work.data_ptr()), C.c_void_p(st.cuda_stream)), "lt_ingest_scans_dev")
            pj._project([(pts, rem, lab)], t[2], t[3], t[0], t[1], model, new=True, remove=True, stream=st)
        cases["composed " + name] = composed
    src_ev = Evaluator(source, approach.ignore, lut)
    keep.append(src_ev)
    cases[f"source {source[0]}x{source[1]}"] = lambda: src_ev.source_scan(xyzr, label, stream=st)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(iters):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    for fn in cases.values():
        timed(fn)
    us = {k: [] for k in cases}
    for _ in range(reps):
        for name, fn in cases.items():
            us[name].append(timed(fn))
    for o in keep:
        o.close()
    return dict(points=n, iters_per_rep=iters, reps=reps, us_per_call={k: stat(v) for k, v in us.items()})


def sequence_modes(scans, poses, approach, source, target, window, reps):
    import torch
    from lidar_transfer_amd.ingest import SequenceSource
    from lidar_transfer_amd.sequence import SequenceTransfer
    runners = {}
    for name, mode in (("evaluate target", "target"), ("evaluate off", False)):
        src = SequenceSource(scans=[s for s, _ in scans], labels=[l for _, l in scans], poses=poses, cache_scans=32)
        runners[name] = SequenceTransfer(src, approach, source, target, out_dir=None, chains=1, evaluate=mode)

    def one_pass(tr):
        recs = list(tr.run())
        torch.cuda.synchronize()
        return recs

    first = {k: one_pass(tr) for k, tr in runners.items()}
    times = {k: [] for k in runners}
    for _ in range(reps):
        for name, tr in runners.items():
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < window:
                n += len(one_pass(tr))
            times[name].append((time.perf_counter() - t0) * 1e3 / n)
    r = first["evaluate target"]
    doc = dict(workload=dict(raw_scans=len(scans), source=list(source), adaption=approach.adaption, chains=1,
                             number_of_scans=approach.number_of_scans, window_s=window, reps=reps, output_scans=len(r)),
               ms_per_output_scan={k: stat(v) for k, v in times.items()},
               first_pass=dict(m_iou=[x["m_iou"] for x in r], n_compared=[x["n_compared"] for x in r],
                               MSE_compared=[x["MSE_compared"] for x in r]))
    for tr in runners.values():
        tr.source.close()
        tr.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--raw-scans", type=int, default=16)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_target_view.py needs a GPU")
    import bench_ingest as bi
    from lidar_transfer_amd.config import TargetModel, load_approach, load_sensor
    source = (bi.H, bi.W, bi.FOV_UP, bi.FOV_DOWN)
    scans, poses = bi.make_sequence(args.raw_scans, 7)
    a = load_approach(os.path.join(ROOT, "config", "approach_mount_example.yaml"))
    T = a.mount()[0]
    vlp = load_sensor(os.path.join(ROOT, "config", "vlp32c_table_az_1024.yaml"))
    targets = {"vlp32c_az 32x1024": ((vlp.H, vlp.W, vlp.fov_up, vlp.fov_down), vlp.target_model()),
               "linear 64x2048": ((64, 2048, 10.0, -30.0), TargetModel())}
    doc = dict(calls=call_cases(scans[0], a, T, targets, source, args.iters, args.reps),
               sequence=sequence_modes(scans, poses, a, source, vlp, args.window, args.reps))
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
