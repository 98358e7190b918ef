#!/usr/bin/env python3
"""What the ingest stage (lidar_transfer_amd/ingest.py, csrc/lt_ingest.hip) costs and saves, at user size.

    python tools/bench_ingest.py --out profiles/ingest/bench_ingest.json                      # the timings (needs a GPU)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ingest -- python tools/bench_ingest.py --trace-only   # a run of its own
    python tools/bench_ingest.py --kernel-stats DIR --out profiles/ingest/bench_ingest.json  # kernel times into the JSON

A seeded sequence: a 64 x 2048 sensor driving a curve through a static world (ground plane + walls), ~120 k points per scan,
`number_of_scans` 5, 128 output scans by default (132 raw scans = 317 MB of file bytes, 2.5 GB of prepared clouds: the inputs
of the timed loops cycle far beyond the chip's 256 MiB last-level cache).  Reported per OUTPUT scan, median / min / max over
`--reps` repetitions in which the routes alternate:

host_route_ms     what a caller had to do before this stage existed: the reference's statements (laserscan.py:776-817 +
                  :949) in numpy on the host -- label & 0xFFFF, two float64 4x4 transforms, the boolean-mask copies of
                  remove_classes, np.concatenate -- plus the upload of the float64 clouds; host clock, ends in a synchronise.
                  The files are in memory already in BOTH routes (reading them depends on the page cache).
device_route_ms   ScanIngest.prepare(idx, merged=True): `warm` = every raw scan resident (HIP events, and the host clock to a
                  synchronise); `streaming` = consecutive output scans with a small cache, ONE new scan uploaded per output
                  scan (the steady state of a batch_interval-1 run); `cold` = the cache emptied before every call, all five
                  scans uploaded.
chain_ms          DeviceDeform.mergemesh fed pre-made clouds against DeviceDeform.deform('mergemesh', ingest, idx) =
                  prepare() + the same chain, on the reference's default volume (+-50 / +-50 / +-5 m, 0.05 m voxels).
kernels           (--kernel-stats) bytes the two kernels must move, from the point counts, over their traced time, as a
                  share of the HBM peak.

Without a device the tool fails; it prints no numbers."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12       # bytes/s (spec); a float4 copy measures 6.29e12 on this chip
H, W, FOV_UP, FOV_DOWN = 64, 2048, 3.0, -25.0
IGNORE, MOVING = [0, 1], [252, 253, 254, 255, 256, 257, 258, 259]


def pose(k):
    yaw = 0.01 * k + 0.00005 * k * k
    c, s = np.cos(yaw), np.sin(yaw)
    p = np.zeros(3)
    for j in range(k):
        yj = 0.01 * j + 0.00005 * j * j
        p += 0.3 * np.array([np.cos(yj), np.sin(yj), 0.0])
    M = np.eye(4)
    M[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    M[:3, 3] = p - np.array([15.0, 10.0, 0.0])
    return M


def make_sequence(n_raw, seed):
    """[(xyzr f32 [n,4], label u32 [n])], poses: the sensor sees a ground plane at z = -1.73 and walls at |x|, |y| = 45 m"""
    from lidar_transfer_amd.laserscan import create_rays
    rng = np.random.default_rng(seed)
    d = create_rays(FOV_UP, FOV_DOWN, H, W).reshape(-1, 3).astype(np.float64)
    scans, poses = [], []
    for k in range(n_raw):
        M = pose(k)
        dw, o = d @ M[:3, :3].T, M[:3, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.stack([(-1.73 - o[2]) / dw[:, 2], (45.0 - o[0]) / dw[:, 0], (-45.0 - o[0]) / dw[:, 0],
                          (45.0 - o[1]) / dw[:, 1], (-45.0 - o[1]) / dw[:, 1]], 1)
        t[~(t > 0)] = np.inf
        which = t.argmin(1)
        tt = t.min(1) * (1.0 + rng.normal(0, 0.001, len(t)))
        keep = np.isfinite(tt) & (rng.random(len(tt)) > 0.08)
        pts = (d[keep] * tt[keep, None]).astype(np.float32)
        lab = np.where(which[keep] == 0, 40, 50).astype(np.uint32)
        r = rng.random(len(lab))
        lab[r < 0.03] = rng.integers(0, 2, int((r < 0.03).sum()))
        m = (r >= 0.03) & (r < 0.08)
        lab[m] = rng.integers(252, 260, int(m.sum()))
        lab |= rng.integers(1, 500, len(lab)).astype(np.uint32) << 16
        rem = (rng.integers(0, 100, len(lab)) / 100).astype(np.float32)
        scans.append((np.ascontiguousarray(np.concatenate([pts, rem[:, None]], 1)), lab))
        poses.append(M)
    return scans, poses


def host_route(scans, poses, slots, idx, torch, dev):
    """open_multiple_scans + the merge and inverse pose of deform('mergemesh') as the reference states them, then the upload"""
    pts_l, rem_l, lab_l = [], [], []
    for i, s in enumerate(slots):
        scan, label = scans[s]
        points, rem = scan[:, 0:3], scan[:, 3]
        label = label & 0xFFFF
        hom = np.ones((points.shape[0], 4))
        hom[:, 0:3] = points
        points = np.matmul(poses[s], hom.T).T[:, 0:3]
        for classes in ((MOVING, IGNORE) if i != 0 else (IGNORE,)):
            remove = np.full((len(points),), False)
            for c in classes:
                remove += label == c
            keepi = np.invert(remove)
            points, rem, label = points[keepi], rem[keepi], label[keepi]
        pts_l.append(points)
        rem_l.append(rem)
        lab_l.append(label)
    points, rem, label = np.concatenate(pts_l), np.concatenate(rem_l), np.concatenate(lab_l)
    hom = np.ones((points.shape[0], 4))
    hom[:, 0:3] = points
    points = np.ascontiguousarray(np.matmul(np.linalg.inv(poses[idx]), hom.T).T[:, 0:3])
    out = (torch.from_numpy(points).to(dev), torch.from_numpy(rem).to(dev), torch.from_numpy(label.astype(np.int32)).to(dev))
    torch.cuda.synchronize()
    return out


def stat(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), n=len(xs))


def kernel_stats(trace_dir, points_per_call, n_scans):
    """rocprofv3 --kernel-trace --stats: *_kernel_stats.csv -> per kernel the traced time and the share of the HBM peak"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {trace_dir}")
    rows = list(csv.DictReader(open(files[0])))
    n, nb = points_per_call, points_per_call // 256 + n_scans
    need = {"k_ingest_count": 4 * n + 4 * nb,                 # the labels in, one count per workgroup out
            "k_ingest_write": 20 * n + 32 * n + 4 * nb}       # xyzr + label in; every raw point writes one 32-byte output cell
    out = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        for k, nbytes in need.items():
            if k in name:
                calls = int(r["Calls"])
                avg_ns = float(r["TotalDurationNs"]) / calls
                out[k] = dict(calls=calls, avg_us=avg_ns / 1e3, bytes_per_call=nbytes, gbytes_per_s=nbytes / avg_ns,
                              share_of_hbm_peak=nbytes / (avg_ns * 1e-9) / HBM_PEAK)
    other = sorted(((float(r["TotalDurationNs"]), r.get("Name") or r.get("KernelName")) for r in rows), reverse=True)[:6]
    out["top_kernels_of_the_trace_us"] = [[round(t / 1e3, 1), nme[:80]] for t, nme in other]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest", "bench_ingest.json"))
    ap.add_argument("--outputs", type=int, default=128, help="distinct output scans")
    ap.add_argument("--nscans", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--trace-only", action="store_true", help="warm prepare() calls only (to run under rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run")
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("--reps: at least five")
    if args.kernel_stats:
        rec = json.load(open(args.out))
        rec["kernels"] = kernel_stats(args.kernel_stats, rec["sequence"]["raw_points_per_output_scan"], args.nscans)
        json.dump(rec, open(args.out, "w"), indent=1)
        print(json.dumps(rec["kernels"]))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest.py measures on a GPU and found none: no numbers")
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest, SequenceSource, relative_indices
    dev = torch.device("cuda", 0)
    rel = relative_indices(args.nscans)
    first = -min(rel)
    n_raw = args.outputs + args.nscans - 1
    scans, poses = make_sequence(n_raw, args.seed)
    idxs = list(range(first, first + args.outputs))
    raw_pts = float(np.mean([sum(len(scans[i + r][1]) for r in rel) for i in idxs]))
    src = SequenceSource(scans=[s for s, _ in scans], labels=[l for _, l in scans], poses=poses, cache_scans=n_raw + 1, cache_bytes=4 << 30)
    ing = ScanIngest(src, (args.nscans, IGNORE, MOVING))
    for i in idxs:                       # warm-up: every raw scan resident, every shape launched once
        ing.prepare(i, merged=True)
    torch.cuda.synchronize()
    if args.trace_only:
        for _ in range(2):
            for i in idxs:
                ing.prepare(i, merged=True)
        torch.cuda.synchronize()
        print("trace-only: %d warm prepare() calls" % (2 * len(idxs)))
        return
    # the two routes give the same clouds (points within the rounding of the reference's dgemm)
    hp, hr, hl = host_route(scans, poses, [idxs[3] + r for r in rel], idxs[3], torch, dev)
    dp, dr, dl = ing.prepare(idxs[3], merged=True, exact=True)[0]
    assert hp.shape == dp.shape and torch.equal(hr, dr) and torch.equal(hl, dl) and float((hp - dp).abs().max()) < 1e-9
    del hp, hr, hl, dp, dr, dl
    host_idx = idxs[:: max(1, len(idxs) // 16)][:16]
    small = SequenceSource(scans=[s for s, _ in scans], labels=[l for _, l in scans], poses=poses, cache_scans=args.nscans + 3)
    ing_small = ScanIngest(small, (args.nscans, IGNORE, MOVING))
    for i in idxs[:8]:
        ing_small.prepare(i, merged=True)
    host_route(scans, poses, [idxs[0] + r for r in rel], idxs[0], torch, dev)
    torch.cuda.synchronize()
    t_host, t_warm_ev, t_warm_clock, t_stream, t_cold = [], [], [], [], []
    for rep in range(args.reps):
        t0 = time.perf_counter()
        for i in host_idx:
            host_route(scans, poses, [i + r for r in rel], i, torch, dev)
        t_host.append((time.perf_counter() - t0) * 1e3 / len(host_idx))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for i in idxs:
            ing.prepare(i, merged=True)
        e1.record()
        torch.cuda.synchronize()
        t_warm_clock.append((time.perf_counter() - t0) * 1e3 / len(idxs))
        t_warm_ev.append(e0.elapsed_time(e1) / len(idxs))
        small._cache.clear()
        small._cached_bytes = 0
        ing_small.prepare(idxs[0], merged=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in idxs[1:]:
            ing_small.prepare(i, merged=True)
        torch.cuda.synchronize()
        t_stream.append((time.perf_counter() - t0) * 1e3 / (len(idxs) - 1))
        t0 = time.perf_counter()
        for i in host_idx:
            small._cache.clear()
            small._cached_bytes = 0
            ing_small.prepare(i, merged=True)
        torch.cuda.synchronize()
        t_cold.append((time.perf_counter() - t0) * 1e3 / len(host_idx))
    # the mergemesh chain with and without the ingest stage in front of it
    chain_idx = idxs[8:20]
    premade = {i: ing.prepare(i, merged=True) for i in chain_idx}
    bnds = np.array([-50, 50, -50, 50, -5, 5]).reshape(3, 2)
    sensor = (H, W, FOV_UP, FOV_DOWN)
    dd = DeviceDeform(sensor, sensor, bnds, 0.05, mesh_volume=False)
    same = True
    for i in chain_idx[:4]:
        a = dd.mergemesh(premade[i])["bin"].clone()
        b = dd.deform("mergemesh", ing, i)["bin"]
        torch.cuda.synchronize()
        same = same and bool(torch.equal(a, b))
    t_fed, t_ingest = [], []
    for rep in range(args.reps):
        for ts, fn in ((t_fed, lambda i: dd.mergemesh(premade[i])), (t_ingest, lambda i: dd.deform("mergemesh", ing, i))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in chain_idx:
                fn(i)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / len(chain_idx))
    mm_stats = dict(dd._mm_state.stats)
    dd.close()
    rec = {
        "what": "ingest stage per output scan: merged cloud of %d scans, 64 x 2048 source, MI355X" % args.nscans,
        "device": torch.cuda.get_device_name(0), "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count(),
        "sequence": {"output_scans": len(idxs), "raw_scans": n_raw, "number_of_scans": args.nscans,
                     "raw_points_per_output_scan": int(raw_pts), "raw_bytes_total": int(sum(20 * len(l) for _, l in scans)),
                     "prepared_bytes_per_output_scan": int(32 * raw_pts), "seed": args.seed, "ignore": IGNORE, "moving": MOVING},
        "host_route_ms": dict(stat(t_host), output_scans_per_rep=len(host_idx),
                              note="reference statements in numpy + upload of float64 clouds; host clock ending in a synchronise"),
        "device_route_ms": {"warm_events": stat(t_warm_ev), "warm_host_clock": stat(t_warm_clock),
                            "streaming_one_new_scan_host_clock": stat(t_stream), "cold_all_scans_uploaded_host_clock": stat(t_cold)},
        "speedup_host_over_device_warm_host_clock": float(np.median(t_host) / np.median(t_warm_clock)),
        "speedup_host_over_device_streaming": float(np.median(t_host) / np.median(t_stream)),
        "chain_ms": {"mergemesh_fed_premade_clouds": stat(t_fed), "mergemesh_with_prepare_in_front": stat(t_ingest),
                     "added_ms_per_output_scan": float(np.median(t_ingest) - np.median(t_fed)), "same_bytes": same,
                     "output_scans_per_rep": len(chain_idx), "mm_stats": mm_stats,
                     "volume": "+-50 / +-50 / +-5 m int bounds, 0.05 m voxels, source = target = 64 x 2048"},
        "kernels": "not measured (run rocprofv3 --kernel-trace --stats on --trace-only, then --kernel-stats)",
        "uploads": dict(src.stats),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps({k: rec[k] for k in ("host_route_ms", "device_route_ms", "chain_ms")}))
    assert np.median(t_warm_clock) < np.median(t_host), "the device route is not faster than the host route"


if __name__ == "__main__":
    main()
