"""A whole sequence: the reference's batch loop (lidar_deform.py:385-462) from a SemanticKITTI sequence on disk to the
transferred sequence on disk, with the metrics ``compare()`` prints per scan.

    tr = SequenceTransfer((dataset, "00"), approach, source_sensor, target_sensor, out_dir="output", chains=3)
    for rec in tr.run():                                   # records in scan order
        rec["idx"], rec["n_points"], rec["m_iou"], rec["m_acc"], rec["MSE"], rec["iou"]
    tr.close()

Per output scan, all queued without the host waiting in between: ``ScanIngest.prepare`` (raw scans -> clouds) on the
submitting thread's stream; an event orders the chain's stream behind it; on the chain's stream ``DeviceDeform.cp / mesh /
mergemesh``, then -- when source and target images have one size -- the source reference scan and ``compare()`` into a
pinned record (:mod:`lidar_transfer_amd.evaluate`), then ``write``'s packing, an asynchronous copy of the packed bytes into
pinned memory and an event; ONE writer thread waits for that event and writes ``velodyne/N.bin`` / ``labels/N.label``.
``chains > 1`` (mesh adaptions): every chain owns a ``DeviceDeform``, an ``Evaluator``, a HIP stream and a host thread; scans
are dealt to the chains in turn; ``mergemesh``'s bounds statements run in scan order whichever chain a scan lands on
(``MergeMeshState``, shared).  Thread counts are ``chains`` + 1, never derived from the machine's CPU count.  There is no CPU
path: everything ends in ``liblidarhip.so``."""
from __future__ import annotations

import collections
import os
import queue
import shutil
import threading

import numpy as np

from ._chain import CP_REFUSALS
from .deform import DeviceDeform, MergeMeshState
from .evaluate import Evaluator
from .ingest import ScanIngest, SequenceSource
from .rig import RigDeform, head_keywords

ADAPTIONS = ("cp", "mesh", "mergemesh")
#: what the codes of a return model's ``drop`` image mean, in code order (``return_totals``, the CLI's closing line)
RETURN_CODES = ("kept", "no hit", "below min_range", "beyond max_range", "beyond max_incidence", "dropped at random")


def format_return_totals(totals):
    """the CLI's closing line of a run with a return model: ``Returns: kept N, no hit N, ...`` in code order"""
    return "Returns: " + ", ".join(f"{name} {int(n)}" for name, n in zip(RETURN_CODES, totals))


#: what the states of a noise model's ``noise_state`` image mean, in state order (``noise_totals``, the CLI's closing line)
NOISE_STATES = ("untouched", "noised", "lost")


def format_noise_totals(totals, rms):
    """the CLI's closing line of a run with a noise model: ``Noise: untouched N, noised N, lost N, range error RMS X m`` (the
    root mean square of ``range_error`` over the noised cells; ``None``: there was none)"""
    return "Noise: " + ", ".join(f"{name} {int(n)}" for name, n in zip(NOISE_STATES, totals)) + \
        ", range error RMS " + ("n/a" if rms is None else f"{float(rms):.6f} m")


#: how many echoes a cell of an echo model's ``n_echoes`` image detected (``echo_totals``, the CLI's closing line)
ECHO_COUNTS = ("none", "one", "several")


def format_echo_totals(totals, fraction):
    """the CLI's closing line of a run with an echo model: ``Echoes: none N, one N, several N, mean fraction X`` (the cells per
    number of detected echoes, and the mean of ``echo_fraction`` over the cells that detected one; ``None``: there was none)"""
    return "Echoes: " + ", ".join(f"{name} {int(n)}" for name, n in zip(ECHO_COUNTS, totals)) + \
        ", mean fraction " + ("n/a" if fraction is None else f"{float(fraction):.6f}")


def format_closing_lines(totals, lead=""):
    """the CLI's closing lines of a run, or of one head of a rig: one per model that is on in ``totals`` (:attr:`summary`, or
    its ``sensors[NAME]``) -- returns, noise, echoes, second returns --, each led by ``lead`` (``""`` or ``"NAME: "``)"""
    lines = []
    if totals.get("return_totals") is not None:
        lines.append(format_return_totals(totals["return_totals"]))
    if totals.get("noise_totals") is not None:
        lines.append(format_noise_totals(totals["noise_totals"], totals["range_error_rms"]))
    if totals.get("echo_totals") is not None:
        lines.append(format_echo_totals(totals["echo_totals"], totals["echo_fraction_mean"]))
    if totals.get("second_returns") is not None:
        lines.append("Second returns: %d" % totals["second_returns"])
    return [lead + line for line in lines]


def sensor_tuple(s):
    """``(H, W, fov_up, fov_down)`` of a :class:`lidar_transfer_amd.config.SensorModel` (or such a tuple itself)"""
    if hasattr(s, "fov_up"):
        return int(s.H), int(s.W), float(s.fov_up), float(s.fov_down)
    return int(s[0]), int(s[1]), float(s[2]), float(s[3])


def output_paths(out_dir, sequence, idx):
    """``<out_dir>/sequences/<seq>/velodyne/NNNNNN.bin`` and ``.../labels/NNNNNN.label`` (lidar_deform.py:166-168, laserscan.py:1162-1173)"""
    base = os.path.join(out_dir, "sequences", str(sequence))
    name = str(int(idx)).zfill(6)
    return os.path.join(base, "velodyne", name + ".bin"), os.path.join(base, "labels", name + ".label")


def plausible_output(out_dir, sequence, idx):
    """``resume``'s test: both files exist, the ``.bin`` is a whole number of 16-byte points and the ``.label`` a quarter of it"""
    b, l = output_paths(out_dir, sequence, idx)
    try:
        sb, sl = os.path.getsize(b), os.path.getsize(l)
    except OSError:
        return False
    return sb % 16 == 0 and sl * 4 == sb


def cache_scans_needed(number_of_scans, chains, batch_interval):
    """raw scans that must stay resident: those of one output scan plus what the scans in flight have moved on by"""
    return int(number_of_scans) + int(chains) * max(int(batch_interval), 1)


class _Tally:
    """Cells per code (uint8, ``0 .. n_codes - 1``) plus one float64 sum, kept on ``device`` without a read-back: what a run
    sums per chain for a model that is on.  Nothing is allocated before the first :meth:`add`, which runs on the chain's
    stream; :meth:`read` is called once per run, behind a synchronise of that stream."""

    def __init__(self, n_codes, device):
        self.n_codes, self.device = int(n_codes), device
        self.codes = self.counts = self.sum = None

    def add(self, codes_u8, value_f64=None):
        """one scan's ``codes_u8`` [n] and ``value_f64`` (a float64 scalar tensor, or ``None``), on the current stream"""
        if self.counts is None:
            import torch
            if self.codes is None:
                self.codes = torch.arange(self.n_codes, dtype=torch.uint8, device=self.device)
            self.counts = torch.zeros(self.n_codes, dtype=torch.int64, device=self.device)
        self.counts += (codes_u8.unsqueeze(1) == self.codes).sum(0)
        if value_f64 is not None:
            self.sum = value_f64 if self.sum is None else self.sum + value_f64

    def read(self):
        """``(cells per code as ints, the sum as a float)``; waits for the current stream"""
        counts = [0] * self.n_codes if self.counts is None else [int(x) for x in self.counts.cpu().tolist()]
        return counts, 0.0 if self.sum is None else float(self.sum)

    def reset(self):
        """the next :meth:`add` starts from zero (on ITS stream: nothing is launched here)"""
        self.counts = self.sum = None


class _Writer:
    """ONE thread: waits for a scan's event, writes its files"""

    def __init__(self):
        self.q = queue.Queue()
        self.thread = threading.Thread(target=self._loop, daemon=True)
        self.thread.start()

    def _loop(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            job, files, event = item         # files: (paths, points, labels, n) per file pair -- one, or one per head [+ merged]
            try:
                event.synchronize()
                for paths, hb, hl, n in files:
                    for p in paths:
                        os.makedirs(os.path.dirname(p), exist_ok=True)
                    hb.numpy()[:n].tofile(paths[0])
                    hl.numpy()[:n].view(np.uint32).tofile(paths[1])
            except BaseException as e:  # noqa: BLE001  (handed to the generator as this scan's exception)
                job["error"] = e
            job["written"].set()

    def close(self):
        self.q.put(None)
        self.thread.join()


def _chain_worker(runner_work, q):
    while True:
        item = q.get()
        if item is None:
            return
        runner_work(*item)


class SequenceTransfer:
    """See the module docstring.  ``source_seq``: a :class:`SequenceSource` (then ``sequence`` names the output folder) or
    ``(dataset, sequence)``; ``approach``: :class:`lidar_transfer_amd.config.Approach`; sensors: ``SensorModel`` or ``(H, W,
    fov_up, fov_down)``.  ``out_dir=None``: nothing is written.  ``evaluate=None``: compare when source and target images
    have one size, as lidar_deform.py:416 does.  ``fusion``: ``"cuda"`` or ``"numpy"`` (the reference's two fusion modes).
    ``nclasses``: default ``len(approach.color_map)`` (lidar_deform.py:359).  ``copy_files``: paths (the target and approach
    YAML) copied next to the output once (lidar_deform.py:446-452).  A non-identity ``approach.transformation`` mounts the
    target sensor at a pose of its own (``Approach.mount()``; ``DeviceDeform(transformation=...)``): the output is in the
    target's frame, ``compare()`` against the source scan would mean nothing, so ``evaluate=None`` resolves to ``False`` and
    ``evaluate=True`` raises; ``mounted`` tells.  A target ``SensorModel`` brings its ``TargetModel``
    (``SensorModel.target_model()``, kept as ``target_model``; its fields ``beam_table``, ``sector`` and ``beam_azimuth`` are
    attributes here too, ``None``: none) to every chain's ``DeviceDeform``.  With a beam table (``beam_model`` tells) the source
    scan, projected by the evenly spaced model, cannot be compared row for row, with a sector (``azimuth_model`` tells) not
    column for column: ``evaluate`` then behaves as for a mounted target.  A source sensor with any of the three is refused.
    ``evaluate="target"`` compares for EVERY target and adaption instead: each chain's evaluator makes the TARGET VIEW of the
    primary raw scan -- the scan seen through the target's model from the target's pose (``Evaluator.target_view``, DESIGN
    7f) -- on the chain's stream and compares it with the chain's ``label`` / ``range``, behind the return model and the
    frame change; the records then also carry ``n_compared`` (cells that are not background) and ``MSE_compared`` (``sq_sum
    / n_compared``, ``None`` when 0).  ``evaluate_mode`` tells ``"source"``, ``"target"`` or ``None``; ``evaluate`` is then
    ``True``.
    A target ``SensorModel`` with a ``return_model`` block (kept as ``returns``; ``None``: none) has it applied to every
    output scan of ``mesh`` / ``mergemesh`` behind its render, with the scan's FILE index as the random rule's ``scan`` --
    evaluation and the written files see what the target sensor sees --; the cells per code are summed on the device and
    read once at the end of :meth:`run` (``summary["return_totals"]``, six numbers in :data:`RETURN_CODES`' order).  ``cp``
    renders no surface: with such a target it raises ``ValueError``; so does a source sensor with the key.
    A target ``SensorModel`` with a ``noise_model`` block (kept as ``noise``; ``None``: none) has it applied in the same way
    and with the same ``scan``, behind the return model and about the target's position in the scene: evaluation
    -- either mode; the target view itself is never noised, so its MSE contains the noise -- and the written files see what
    the target sensor reports.  The cells per state and the squared ``range_error`` are summed on the device and read once
    at the end of :meth:`run` (``summary["noise_totals"]``, three numbers in :data:`NOISE_STATES`' order, and
    ``summary["range_error_rms"]`` over the noised cells).  ``cp`` renders no ray: with such a target it raises
    ``ValueError``; so does a source sensor with the key.
    A target ``SensorModel`` with an ``echo_model`` block (kept as ``echoes``; ``None``: none) has its beams widened (DESIGN
    7h): every chain renders the one shared sub-ray set and resolves it ahead of the two other models; evaluation and the
    written files see the resolved scan.  The cells per number of detected echoes and the reported share of the beam are
    summed on the device and read once at the end of :meth:`run` (``summary["echo_totals"]``, three numbers in
    :data:`ECHO_COUNTS`' order, and ``summary["echo_fraction_mean"]`` over the cells with an echo).  ``cp`` renders no ray:
    with such a target it raises ``ValueError``; so does a source sensor with the key.
    A target ``SensorModel`` with a ``dual_return`` block that is on (kept as ``dual``; ``None``: none) has every chain resolve
    a SECOND echo per cell: each file holds the primary's points, as without the block, followed by the second
    returns'; a record's ``n_points`` is the file's count; evaluation sees the primary alone.  The second returns that stand
    behind the models are summed on the device and read once at the end of :meth:`run` (``summary["second_returns"]``).
    ``cp`` renders no ray: with such a target it raises ``ValueError``; so does a source sensor with the key.
    An approach with a ``rig`` (``Approach.rig()``) names SEVERAL target sensors: ``target_sensor`` is ``None`` (one
    given raises), every chain is a ``rig.RigDeform`` -- the later ones share the first one's ray sets --, ``mesh`` and
    ``mergemesh`` only.  The files of head ``NAME`` go to ``<out_dir>/sequences/SS/NAME/velodyne|labels``, with ``rig_merged`` the
    merged scan to the standard pair; a record gains ``sensors: {NAME: {n_points}}`` and its ``n_points`` is the merged scan's
    (else the heads' sum); ``resume`` skips a scan only when EVERY file of it is plausible; the tallies above are kept per head
    under ``summary["sensors"][NAME]`` (the top-level ones stay ``None``).  A rig is not evaluated: ``evaluate=None`` resolves
    to no comparison, ``True`` and ``"target"`` raise ``ValueError`` naming the follow-up.  The single-target attributes
    (``target_sensor``, ``beam_model``, ...) then describe head 0."""

    def __init__(self, source_seq, approach, source_sensor, target_sensor, out_dir=None, chains=1, fusion="cuda", evaluate=None,
                 device=None, sequence="00", nclasses=None, copy_files=()):
        import torch
        self._torch = torch
        if approach.adaption not in ADAPTIONS:
            raise ValueError(f"adaption {approach.adaption!r} (cp, mesh or mergemesh)")
        if int(chains) < 1:
            raise ValueError("chains: at least one")
        self.approach, self.adaption = approach, approach.adaption
        from .config import TargetModel, refuse_source_models
        refuse_source_models(source_sensor)
        # a rig: the approach names the target sensors, every chain is a RigDeform, nothing is compared
        self.rig = approach.rig()
        self.rig_names = None if self.rig is None else [h.name for h in self.rig]
        self.merged = self.rig is not None and bool(approach.rig_merged)
        if self.rig is not None:
            if target_sensor is not None:
                raise ValueError("rig: the approach file names its target sensors (rig) -- SequenceTransfer takes no target sensor "
                                 "with it (target_sensor=None)")
            if self.adaption == "cp":
                raise ValueError("rig: adaption cp renders no ray -- a rig needs mesh or mergemesh")
            if evaluate is True or isinstance(evaluate, str):
                raise ValueError(f"evaluate: {evaluate!r} -- a rig is not evaluated (which head is compared with the source scan, "
                                 "and how a merged scan is, is the follow-up 'rig evaluation'); use None or False")
            evaluate = False
            target_sensor = self.rig[0].sensor   # (what the single-target attributes below describe: head 0)
        elif target_sensor is None:
            raise ValueError("SequenceTransfer: a target sensor, or an approach with a rig")
        self.source_sensor, self.target_sensor = sensor_tuple(source_sensor), sensor_tuple(target_sensor)
        # (sensor_tuple drops the model; ValueError on one that cannot be used; a plain tuple has none: the empty model)
        m = self.target_model = getattr(target_sensor, "target_model", TargetModel)()
        self.beam_table, self.sector, self.beam_azimuth = m.beam_table, m.sector, m.beam_azimuth
        self.beam_model = "linear" if m.beam_table is None else "table"
        self.azimuth_model = "full" if m.sector is None else "sector"
        for name in ("returns", "noise", "echoes", "dual"):
            key, _, what, why = CP_REFUSALS[name]
            setattr(self, name, getattr(target_sensor, key, lambda: None)())
            if getattr(self, name) is not None and self.adaption == "cp":
                raise ValueError(f"adaption cp renders no {what} ({why}): the target sensor's {key} cannot be applied -- use "
                                 "mesh or mergemesh, or a target file without the key")
        self.chains = 1 if self.adaption == "cp" else int(chains)     # `cp` always runs on one chain
        self.fusion, self.out_dir = fusion, out_dir
        self.nclasses = int(nclasses) if nclasses is not None else len(approach.color_map)
        self.copy_files = [p for p in copy_files if p]
        same = self.source_sensor[:2] == self.target_sensor[:2]
        if isinstance(evaluate, str) and evaluate != "target":
            raise ValueError(f"evaluate: {evaluate!r} (None, True, False or \"target\")")
        target_view = isinstance(evaluate, str)
        if target_view:                              # every target can see the source scan through its own model
            evaluate = None
        if evaluate and not same:
            raise ValueError("evaluate: source and target images differ in size (lidar_deform.py:416)")
        self.mount = approach.mount()                # (raises ValueError on a transformation that is not rigid)
        self.mounted = self.mount is not None
        if evaluate and self.mounted:
            raise ValueError("evaluate: the target sensor is mounted at its own pose (approach.transformation): its scan "
                             "cannot be compared with the source scan cell by cell")
        if evaluate and self.beam_table is not None:
            raise ValueError("evaluate: the target sensor has a beam table (beam_model: table): its rows are not the source "
                             "scan's evenly spaced rows, the two cannot be compared cell by cell")
        if evaluate and self.sector is not None:
            raise ValueError("evaluate: the target sensor has a horizontal sector (azimuth_model: sector): its columns are not "
                             "the source scan's full-circle columns, the two cannot be compared cell by cell")
        self.evaluate = (same and not self.mounted and self.beam_table is None and self.sector is None) \
            if evaluate is None else bool(evaluate)
        if target_view:
            self.evaluate = True
        self.evaluate_mode = "target" if target_view else ("source" if self.evaluate else None)
        need = cache_scans_needed(approach.number_of_scans, self.chains, approach.batch_interval)
        idx = torch.cuda.current_device() if device is None else int(device)
        if isinstance(source_seq, SequenceSource):
            self.source, self._own_source, self.sequence = source_seq, False, str(sequence)
            if self.source.cache_scans < need:
                raise ValueError(f"SequenceSource(cache_scans={self.source.cache_scans}) is too small: number_of_scans "
                                 f"{approach.number_of_scans} with {self.chains} scan(s) in flight needs {need}")
        else:
            dataset, self.sequence = source_seq[0], str(source_seq[1])
            self.source, self._own_source = SequenceSource(dataset, self.sequence, device=idx, cache_scans=max(16, need)), True
        self.device = self.source.device
        self.ingest = ScanIngest(self.source, approach)
        beams = getattr(source_sensor, "beam_angles", None)
        self._configured_bnds = np.array(approach.voxel_bounds).copy() if self.adaption != "cp" else None
        self._mm = None
        self._chains = []
        self._writer = None
        self._copied = False
        self.summary = {}
        try:
            if self.adaption == "mergemesh":
                self.vol_bnds = self._configured_bnds.copy()   # the ONE array of the sequence, kept current
                self._mm = MergeMeshState(self.vol_bnds, approach.voxel_size, idx)
            # the heads of a chain by name -- ``None``: the one target sensor -- and what every chain's constructor takes
            heads = {None: target_sensor} if self.rig is None else {h.name: h.sensor for h in self.rig}
            self._names = list(heads)
            every = dict(beam_angles=beams, preserve_float=approach.preserve_float, device=idx, fusion=fusion,
                         mesh_volume=self.adaption == "mesh", mm_state=self._mm)
            single = dict(head_keywords(target_sensor)[1], transformation=self.mount)
            for c in range(self.chains):
                bnds = None if self._mm is not None or self.adaption == "cp" else self._configured_bnds.copy()
                if self.rig is not None:
                    dd = RigDeform(self.source_sensor, self.rig, bnds, approach.voxel_size, merged=self.merged,
                                   share=self._chains[0]["dd"] if self._chains else None, **every)
                    if self.adaption == "mergemesh":
                        try:
                            dd.check_mergemesh()     # (a later head that looks past head 0: said here, not at the first scan)
                        except BaseException:
                            dd.close()
                            raise
                else:
                    dd = DeviceDeform(self.source_sensor, self.target_sensor, bnds, approach.voxel_size, **every, **single)
                    # (the first chain's ray set and sub-ray set are shared by the later ones)
                    single.update(rayset=dd.rayset, echoes=dd.bound_echoes or single["echoes"])
                ch = dict(dd=dd, ev=None, q=None, thread=None,
                          tally={name: self._tallies(sensor) for name, sensor in heads.items()},
                          stream=torch.cuda.Stream(self.device) if self.chains > 1 else torch.cuda.current_stream(self.device))
                if target_view:
                    ch["ev"] = Evaluator(self.source_sensor, approach.ignore, approach.color_lut(), device=idx,
                                         target=self.target_sensor, target_model=m, transformation=self.mount)
                elif self.evaluate:
                    ch["ev"] = Evaluator(self.source_sensor, approach.ignore, approach.color_lut(), device=idx)
                if self.chains > 1:
                    ch["q"] = queue.Queue()
                    ch["thread"] = threading.Thread(target=_chain_worker, args=(self._work, ch["q"]), daemon=True)
                    ch["thread"].start()
                self._chains.append(ch)
            if out_dir is not None:
                self._writer = _Writer()
        except BaseException:
            self.close()
            raise

    def _tallies(self, sensor):
        """one head's accumulators on a chain: a :class:`_Tally` per model of ``sensor`` that is on"""
        n = dict(returns=len(RETURN_CODES), noise=len(NOISE_STATES), echoes=len(ECHO_COUNTS), dual=2)
        return {name: _Tally(n[name], self.device) for name in n
                if getattr(sensor, CP_REFUSALS[name][0], lambda: None)() is not None}

    def _read_tallies(self, name, head):
        """``(cells per code, sum)`` of model ``name`` of head ``head`` (``None``: the one target sensor) over the chains, read
        and reset; ``(None, 0.0)`` when it is off, or the run has no such head"""
        if not self._chains or name not in self._chains[0]["tally"].get(head, {}):
            return None, 0.0
        counts, value = None, 0.0
        for ch in self._chains:
            ch["stream"].synchronize()
            c, v = ch["tally"][head][name].read()
            counts, value = c if counts is None else [a + b for a, b in zip(counts, c)], value + v
            ch["tally"][head][name].reset()
        return counts, value

    def _totals(self, head):
        """what a run sums of the models that are on of head ``head`` (``None``: the one target sensor; all ``None`` for a rig,
        which has no such head): the summary's keys"""
        totals, _ = self._read_tallies("returns", head)
        noise_totals, sq_sum = self._read_tallies("noise", head)
        echo_totals, share = self._read_tallies("echoes", head)
        second, _ = self._read_tallies("dual", head)
        rms = float(np.sqrt(sq_sum / noise_totals[1])) if noise_totals and noise_totals[1] else None
        echo_mean = share / (echo_totals[1] + echo_totals[2]) if echo_totals and echo_totals[1] + echo_totals[2] else None
        return dict(return_totals=totals, noise_totals=noise_totals, range_error_rms=rms, echo_totals=echo_totals,
                    echo_fraction_mean=echo_mean, second_returns=second[1] if second else None)

    @staticmethod
    def _add_tallies(tally, out):
        """one scan's result ``out`` into the accumulators ``tally`` of its sensor, on the current stream"""
        import torch
        if "returns" in tally:               # cells per code
            tally["returns"].add(out["drop"])
        if "noise" in tally:                 # cells per state and the squared range error (float64)
            tally["noise"].add(out["noise_state"], torch.linalg.vector_norm(out["range_error"], dtype=torch.float64) ** 2)
        if "echoes" in tally:                # cells per number of echoes (two stand for several), the reported shares
            tally["echoes"].add(out["n_echoes"].clamp(max=2), out["echo_fraction"].sum(dtype=torch.float64))
        if "dual" in tally:                  # second returns that stand after the models (code 1) and those that do not
            tally["dual"].add((out["second"]["tri"].reshape(-1) >= 0).to(torch.uint8))

    # ---- the files of an output scan ----------------------------------------------------------------------------------------
    def file_sets(self):
        """the folders of an output scan's file pairs, relative to ``<out_dir>/sequences``: the sequence's own -- or, with a
        rig, ``SS/NAME`` per head, and ``SS`` for the merged scan when the approach says ``rig_merged``"""
        if self.rig is None:
            return [self.sequence]
        return [os.path.join(self.sequence, n) for n in self.rig_names] + ([self.sequence] if self.merged else [])

    def _count(self, job, counts):
        """a scan's ``n_points`` from the points of its file pairs (in :meth:`file_sets`' order), made or found by ``resume``:
        per head, and of the scan -- the merged scan's, else the heads' sum"""
        job["sensors"] = {name: dict(n_points=int(c)) for name, c in zip(self._names, counts)}
        job["n_points"] = int(counts[-1]) if self.merged else sum(int(c) for c in counts)

    def _host_copy(self, b, l):
        """the packed rows on their way into pinned memory, on the current stream -> ``(points, labels, n)``"""
        torch = self._torch
        n = int(b.shape[0])
        hb = torch.empty((max(n, 1), 4), dtype=torch.float32, pin_memory=True)
        hl = torch.empty((max(n, 1),), dtype=torch.int32, pin_memory=True)
        if n:
            hb[:n].copy_(b, non_blocking=True)
            hl[:n].copy_(l, non_blocking=True)
        return hb, hl, n

    # ---- the scan list -------------------------------------------------------------------------------------------------
    def scan_indices(self, offset=0, one_scan=False):
        idx = self.approach.scan_indices(len(self.source), offset)
        return idx[:1] if one_scan else idx

    # ---- one scan on its chain (the chain's thread, or the caller's with one chain) ---------------------------------------
    def _work(self, ch, job):
        torch = self._torch
        dd, st = ch["dd"], ch["stream"]
        try:
            with torch.cuda.device(self.device), torch.cuda.stream(st):
                if job["ready"] is not None:
                    st.wait_event(job["ready"])      # the ingest was queued on the submitting thread's stream
                clouds = job["clouds"]
                if job["skipped"]:                   # resume: only mergemesh's bounds are replayed
                    dd.mergemesh_bounds(clouds, seq=job["k"])
                    return
                if self.adaption == "cp":
                    outs = dd.cp(clouds, pack=False)
                elif self.adaption == "mesh":
                    outs = dd.mesh(clouds, pack=False, scan_index=job["idx"])
                else:
                    outs = dd.mergemesh(clouds, pack=False, seq=job["k"], scan_index=job["idx"])
                if self.rig is None:                 # one result per head: a rig's call returns the list
                    outs = [outs]
                if self.adaption == "mergemesh":
                    job["bnds_after"] = np.array(outs[0]["vol_bnds_after"]).reshape(3, 2)
                for name, out in zip(self._names, outs):
                    self._add_tallies(ch["tally"][name], out)   # summed on the chain's stream: read once, in run()
                if ch["ev"] is not None:             # behind the render, before the packing's read-back: in flight too
                    scan = ch["ev"].target_view if self.evaluate_mode == "target" else ch["ev"].source_scan
                    src = scan(*job["raw"], stream=st)
                    job["record"] = ch["ev"].compare(src, outs[0]["label"], outs[0]["range"], stream=st)
                    job["images"] = (src, outs[0])
                if self.rig is None:
                    packed = [dd.pack_result(outs[0], st)]
                else:
                    packed = [dd.pack_head(out, k, st) for k, out in enumerate(outs)]
                if self.merged:
                    packed.append(dd.merged_rows(outs, st))
                self._count(job, [b.shape[0] for b, _ in packed])
                if self._writer is not None:
                    files = [(output_paths(self.out_dir, d, job["idx"]),) + self._host_copy(b, l)
                             for d, (b, l) in zip(self.file_sets(), packed)]
                    ev = torch.cuda.Event()
                    ev.record(st)
                    job["keep"] = (packed, outs)
                    self._writer.q.put((job, files, ev))
                else:
                    job["written"].set()
        except BaseException as e:  # noqa: BLE001  (handed to the generator as this scan's exception)
            job["error"] = e
            if self._mm is not None:
                self._mm.skip(job["k"])              # (no-op when the scan's geometry call was made after all)
            job["written"].set()
        finally:
            job["done"].set()

    def _submit(self, k, idx, resume):
        torch = self._torch
        job = dict(k=k, idx=int(idx), done=threading.Event(), written=threading.Event(), error=None, record=None, skipped=False,
                   n_points=None, bnds_after=None)
        sets = self.file_sets()
        if resume and self.out_dir is not None and all(plausible_output(self.out_dir, d, idx) for d in sets):
            job["skipped"] = True                    # (a rig: only when EVERY file of the scan is plausible)
            self._count(job, [os.path.getsize(output_paths(self.out_dir, d, idx)[0]) // 16 for d in sets])
            job["written"].set()
            if self._mm is None:
                job["done"].set()
                return job
        st = torch.cuda.current_stream(self.device)
        back = self._chains[0]["dd"].cp_back(self.source.poses[int(idx)]) if self.adaption == "cp" else None
        job["clouds"] = self.ingest.prepare(idx, merged=self.adaption != "mesh", stream=st, back=back)
        if self.evaluate and not job["skipped"]:
            job["raw"] = self.source.raw(idx, st)
        ch = self._chains[k % len(self._chains)]
        job["ready"] = None                          # (one chain: the same stream, already in order)
        if ch["q"] is not None:
            job["ready"] = torch.cuda.Event()
            job["ready"].record(st)
            ch["q"].put((ch, job))
        else:
            self._work(ch, job)
        return job

    def _collect(self, job):
        job["done"].wait()
        job["written"].wait()
        if job["error"] is not None:
            raise job["error"]
        rec = dict(idx=job["idx"], n_points=job["n_points"], m_iou=None, m_acc=None, MSE=None, iou=None, skipped=job["skipped"])
        if job["bnds_after"] is not None:
            rec["bnds_after"] = job["bnds_after"]
        if self.rig is not None:
            rec["sensors"] = job.get("sensors")
        compared = self.evaluate_mode == "target"    # a sparse reference image: how many cells were compared at all
        if compared:
            rec.update(n_compared=None, MSE_compared=None)
        if job["record"] is not None:
            try:
                rec.update(job["record"].metrics(self.nclasses, compared=compared))
            except OverflowError:        # more label values than a record holds: this scan through post.compare
                from .post import compare
                src, out = job["images"]
                h = lambda t: t.cpu().numpy()   # noqa: E731
                color = np.where(h(src["black"])[:, :, None] != 0, 0.0, 1.0) * np.ones((1, 1, 3))
                m = compare(h(src["label"]), color, h(out["label"]), h(src["range"]), h(out["range"]), h(src["rem"]), h(out["rem"]),
                            self.nclasses)
                rec.update(m_iou=m["m_iou"], m_acc=m["m_acc"], MSE=m["MSE"], iou=m["iou"])
                if compared:             # (background: black or label 0 in the source image, as the record counts it)
                    nc = int(((h(src["black"]) == 0) & (h(src["label"]) != 0)).sum())
                    rec.update(n_compared=nc, MSE_compared=float(m["range_diff"].astype(np.float64).sum()) / nc if nc else None)
        if self.out_dir is not None and not self._copied and not job["skipped"]:
            base = os.path.join(self.out_dir, "sequences", self.sequence)
            os.makedirs(base, exist_ok=True)         # (a rig without a merged scan writes into its heads' folders only)
            for p in self.copy_files:
                shutil.copy2(p, base)
            self._copied = True
        for key in ("clouds", "raw", "images", "keep", "record"):
            job.pop(key, None)
        return rec

    def run(self, offset=0, one_scan=False, resume=False):
        """Generator of one record per output scan, in scan order: ``idx``, ``n_points``, ``m_iou`` / ``m_acc`` / ``MSE`` /
        ``iou`` (``None`` when the run does not compare), ``skipped`` (``resume`` found both output files), ``bnds_after``
        (mergemesh), ``n_compared`` / ``MSE_compared`` (``evaluate="target"`` only).  A failed scan or a failed write surfaces
        as that scan's exception; later scans are not started."""
        indices = self.scan_indices(offset, one_scan)
        if self._mm is not None:
            self._mm.reset(self._configured_bnds)        # a run is one sequence: it starts from the configured bounds
        pending = collections.deque()
        n_done = 0
        try:
            for k, idx in enumerate(indices):
                pending.append(self._submit(k, idx, resume))
                while len(pending) >= self.chains:
                    rec = self._collect(pending.popleft())
                    n_done += 1
                    yield rec
            while pending:
                rec = self._collect(pending.popleft())
                n_done += 1
                yield rec
        finally:
            for job in pending:                          # (a failure or an abandoned generator: let what is queued finish)
                job["done"].wait()
                job["written"].wait()
            self.summary = dict(**self._totals(None), scans=n_done,
                                chains=self.chains, adaption=self.adaption, fusion=self.fusion,
                                mounted=self.mounted, beam_model=self.beam_model, azimuth_model=self.azimuth_model,
                                beam_azimuth=self.beam_azimuth is not None,
                                mm_stats=dict(self._mm.stats) if self._mm is not None else None,
                                source_stats=dict(self.source.stats))
            if self.rig is not None:                     # the tallies are kept per head
                self.summary["sensors"] = {name: self._totals(name) for name in self.rig_names}

    def close(self):
        for ch in getattr(self, "_chains", []):
            if ch["q"] is not None:
                ch["q"].put(None)
        for ch in getattr(self, "_chains", []):
            if ch["thread"] is not None:
                ch["thread"].join()
            if ch["ev"] is not None:
                ch["ev"].close()
        if getattr(self, "_writer", None) is not None:
            self._writer.close()
            self._writer = None
        chains, self._chains = getattr(self, "_chains", []), []
        for ch in reversed(chains):                      # (the first chain owns the shared ray set)
            ch["dd"].close()
        if getattr(self, "_mm", None) is not None:
            self._mm.close()
            self._mm = None
        if getattr(self, "_own_source", False) and getattr(self, "source", None) is not None:
            self.source.close()
            self._own_source = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
