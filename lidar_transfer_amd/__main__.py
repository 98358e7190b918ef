"""``python -m lidar_transfer_amd`` -- the reference's ``lidar_deform.py`` in batch mode (its flag surface, :78-137) on the device:

    python -m lidar_transfer_amd -d DATASET -c config/approach_mergemesh.yaml -s 00 -t config/vlp32_1024.yaml -w -p output/

``DATASET/config.yaml`` is the source sensor, ``--target`` the target sensor (default: the source), ``--config`` the approach
YAML -- its ``transformation`` (16 numbers, ``x_target = T . x_source``) mounts the target sensor at a pose of its own: the
output is then in the target's frame, no metrics are printed and every row of ``--log`` carries ``"mounted": true``.  A
target YAML with ``beam_model: table`` (config/vlp32c_table_1024.yaml) switches on the target's real beam geometry: rays and
image rows at the angles of its ``beam_angles``; no metrics are printed and every row of ``--log`` carries
``"beam_model": "table"``.  A target YAML with ``azimuth_model: sector`` (config/front120_64x1024.yaml) gives the target a
horizontal field of view of ``fov_hor`` degrees around ``azimuth_center``: rays and image columns cover that sector alone; no
metrics are printed and every row of ``--log`` carries ``"azimuth_model": "sector"``.  A table target with
``beam_azimuth_offsets`` (config/vlp32c_table_az_1024.yaml) shears rays and columns row by row by its beams' azimuth offsets;
every row of ``--log`` then carries ``"beam_azimuth": true`` as well.  A target YAML with a ``return_model`` block
(config/vlp32c_table_returns_1024.yaml) applies the sensor's range gate, incidence limit and random dropout to every output scan
of ``mesh`` / ``mergemesh`` (``cp`` is refused); the run closes with one line ``Returns: kept N, no hit N, ...``, the cells per
code over all its scans, which the ``--log`` summary carries as ``return_totals``.  A target YAML with a ``noise_model`` block
(config/vlp32c_table_noise_1024.yaml) gives every output scan of ``mesh`` / ``mergemesh`` (``cp`` is refused) the sensor's
measurement error -- range jitter and grid, remission jitter and levels --; the run closes with one line ``Noise: untouched N,
noised N, lost N, range error RMS X m``, which the ``--log`` summary carries as ``noise_totals`` and ``range_error_rms``.  The
metrics of such a run, under ``--evaluate auto`` and under ``--evaluate target`` alike, compare the NOISY output with a
reference that has no noise: their MSE contains the noise.  A target YAML with an ``echo_model`` block
(config/vlp32c_table_echo_1024.yaml) gives the beams of ``mesh`` / ``mergemesh`` (``cp`` is refused) a divergence: every cell
is rendered with several sub-rays whose hits are grouped into echoes, one of which is reported -- with a blended range where
two surfaces lie within one pulse --; the run closes with one line ``Echoes: none N, one N, several N, mean fraction X``,
which the ``--log`` summary carries as ``echo_totals`` and ``echo_fraction_mean``, and every row of ``--log`` carries
``"echo_model": true``; ``--evaluate auto`` treats the key as it treats ``return_model``: nothing is switched off.  The tool
is always headless (``--batch`` is accepted).  Per compared scan it prints the reference's three lines
``IoU:  <m_iou>``, ``Acc:  <m_acc>``, ``MSE:  <MSE>`` (laserscan.py:1233-1234, :1262).  ``--evaluate target`` compares for
every target -- mounted, with a table, a sector, offsets, a return model, another image size -- against the source scan seen
through the target's model from its pose: the three lines are printed per scan and every row of ``--log`` carries
``"evaluate": "target"``, ``n_compared`` and ``MSE_compared``; ``--evaluate off`` compares nothing.  A missing dataset, labels
or output folder ends with a message and exit status 1.  An approach file with a ``rig`` (config/approach_rig_example.yaml, DESIGN
7i) names SEVERAL target sensors: ``-t`` is refused with it, every output scan is written once per head into
``OUT/sequences/SS/NAME/velodyne|labels`` (and, with ``rig_merged``, as one scan into the standard pair), nothing is compared,
every row of ``--log`` carries ``sensors: {NAME: {n_points}}`` and the closing lines are printed per head, led by ``NAME: ``."""
from __future__ import annotations

import argparse
import json
import os
import sys


def build_parser():
    p = argparse.ArgumentParser("python -m lidar_transfer_amd")
    p.add_argument("--dataset", "-d", type=str, required=True, help="Dataset to adapt. No Default")
    p.add_argument("--config", "-c", type=str, default="config/approach_mergemesh.yaml", help="Approach config file. Defaults to %(default)s")
    p.add_argument("--sequence", "-s", type=str, default="00", help="Sequence to transfer. Defaults to %(default)s")
    p.add_argument("--target", "-t", type=str, default="", help="Target sensor config file. Defaults to the dataset's config.yaml")
    p.add_argument("--offset", "-o", type=int, default=0, help="Scan to start at. Defaults to %(default)s")
    p.add_argument("--output", "-p", type=str, default="output/", help="Output folder to write bin files to. Defaults to %(default)s")
    p.add_argument("--batch", "-b", action="store_true", help="Run in batch mode (always on: there is no visualiser).")
    p.add_argument("--write", "-w", action="store_true", help="Write new dataset to file.")
    p.add_argument("--one_scan", action="store_true", help="Run only once.")
    p.add_argument("--chains", type=int, default=1, help="Output scans in flight (mesh adaptions). Defaults to %(default)s")
    p.add_argument("--fusion", choices=("cuda", "numpy"), default="cuda", help="Arithmetic of the TSDF fusion. Defaults to %(default)s")
    p.add_argument("--resume", action="store_true", help="Skip scans whose two output files exist.")
    p.add_argument("--log", type=str, default="", help="Write one JSON object per scan to this file.")
    p.add_argument("--evaluate", choices=("auto", "target", "off"), default="auto",
                   help="auto: compare with the source scan when both images have one size and the target has no model of its "
                        "own; target: compare with the source scan seen through the target's model, for every target; off: "
                        "compare nothing. Defaults to %(default)s")
    return p


def check_paths(args):
    """The reference's existence tests (lidar_deform.py:163-219), as messages: ``None`` when all is well"""
    if args.write and not os.path.isdir(args.output):
        return "Output folder doesn't exist! Exiting..."
    seq = os.path.join(args.dataset, "sequences", args.sequence)
    if not os.path.isdir(os.path.join(seq, "velodyne")):
        return "Sequence folder doesn't exist! Exiting..."
    if not os.path.isdir(os.path.join(seq, "labels")):
        return "Labels folder doesn't exist! Exiting..."
    if not os.path.isfile(os.path.join(args.dataset, "config.yaml")):
        return "Error opening source config.yaml file %s." % os.path.join(args.dataset, "config.yaml")
    for name, path in (("approach", args.config), ("target", args.target)):
        if path and not os.path.isfile(path):
            return "Error opening %s yaml file %s." % (name, path)
    return None


def main(argv=None):
    args, _ = build_parser().parse_known_args(argv)
    problem = check_paths(args)
    if problem:
        print(problem)
        return 1
    from .config import load_approach, load_sensor, refuse_source_models
    source_path = os.path.join(args.dataset, "config.yaml")
    target_path = args.target or source_path
    try:
        approach, source = load_approach(args.config), load_sensor(source_path)
        rig = approach.rig()   # (a rig that cannot be used: said here; None without the key)
        if rig is not None and args.target:
            print("The approach file has a rig, which names its target sensors: -t / --target cannot be given with it.")
            return 1
        if rig is not None and approach.adaption == "cp":
            print("adaption cp renders no ray: a rig needs mesh or mergemesh.")
            return 1
        if rig is not None and args.evaluate == "target":
            print("--evaluate target: a rig is not evaluated (rig evaluation is a follow-up); use auto or off.")
            return 1
        target = load_sensor(target_path) if rig is None else rig[0].sensor
        approach.mount()   # (a transformation that is not a rigid motion: said here, not half way into the run)
        refuse_source_models(source)
    except Exception as e:  # noqa: BLE001  (a YAML that cannot be read: message and status, as the reference's quit())
        print(e)
        print("Error opening yaml file.")
        return 1
    from ._chain import CP_REFUSALS
    from .sequence import SequenceTransfer, format_closing_lines
    if approach.adaption == "cp":   # (a rig was refused above; mesh and mergemesh take every model of every head)
        for name in ("returns", "noise", "echoes", "dual"):
            key, _, what, _ = CP_REFUSALS[name]
            if getattr(target, key)() is not None:
                print(f"adaption cp renders no {what}: the target sensor's {key} cannot be applied (use mesh or mergemesh).")
                return 1
    log = open(args.log, "w") if args.log else None
    try:
        with SequenceTransfer((args.dataset, args.sequence), approach, source, target if rig is None else None,
                              out_dir=args.output if args.write else None, chains=args.chains, fusion=args.fusion,
                              copy_files=(target_path, args.config) if rig is None else (args.config,),
                              evaluate={"auto": None, "target": "target", "off": False}[args.evaluate]) as tr:
            n_files = len(tr.source)
            for rec in tr.run(offset=args.offset, one_scan=args.one_scan, resume=args.resume):
                if rec["m_iou"] is not None:
                    print("IoU: ", float(rec["m_iou"]))
                    print("Acc: ", float(rec["m_acc"]))
                    print("MSE: ", float(rec["MSE"]))
                print("#" * 30, args.sequence, "-", rec["idx"], "/", n_files, "#" * 30, flush=True)
                if log is not None:
                    row = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in rec.items()}
                    if rig is not None:      # (`sensors` is in the record; the single-target marks below describe no rig)
                        log.write(json.dumps(row) + "\n")
                        continue
                    if tr.evaluate_mode == "target":
                        row["evaluate"] = "target"
                    if tr.mounted:
                        row["mounted"] = True
                    if tr.beam_model != "linear":
                        row["beam_model"] = tr.beam_model
                    if tr.azimuth_model != "full":
                        row["azimuth_model"] = tr.azimuth_model
                    if tr.beam_azimuth is not None:
                        row["beam_azimuth"] = True
                    if tr.echoes is not None:
                        row["echo_model"] = True
                    if tr.dual is not None:
                        row["dual_return"] = True
                    log.write(json.dumps(row) + "\n")
            heads = [(name + ": ", totals) for name, totals in (tr.summary.get("sensors") or {}).items()]   # a rig: per head
            for lead, totals in heads + [("", tr.summary)]:
                for line in format_closing_lines(totals, lead):
                    print(line, flush=True)
            if log is not None:
                log.write(json.dumps(dict(summary=tr.summary)) + "\n")
    finally:
        if log is not None:
            log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
