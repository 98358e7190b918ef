"""From a SemanticKITTI sequence on disk to the clouds ``DeviceDeform`` projects -- on the device.

What the reference does between its files and ``deform``'s first projection (``MultiSemLaserScan.open_multiple_scans``,
auxiliary/laserscan.py:776-817, and the first statement of each ``deform`` branch, :845 / :878 / :949):

    read velodyne/N.bin + labels/N.label -> label & 0xFFFF -> apply_pose (float64) -> drop the *moving* classes from all
    but the primary scan and the *ignore* classes from every scan -> back into the primary scan's frame with inv(pose)

Here the file bytes are uploaded ONCE per scan (:class:`SequenceSource` keeps the last raw scans resident: consecutive
output scans share all but ``batch_interval`` of their source scans) and everything after that is one native call,
``lt_ingest_scans_dev`` (csrc/lt_ingest.hip), asynchronous on the caller's stream:

    src = SequenceSource(dataset, "00")
    ing = ScanIngest(src, approach)                      # number_of_scans, ignore, moving of config/lidar_transfer.yaml
    out = dd.deform("mergemesh", ing, idx)               # = dd.mergemesh(ing.prepare(idx, merged=True))

The text files (``calib.txt``, ``poses.txt``) and ``inv(poses[idx])`` are numpy on the host, statement for statement the
reference's.  There is no CPU path for the clouds: everything ends in ``liblidarhip.so``.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np

from . import _lib


# ---- lidar_deform.py:13-74 ---------------------------------------------------------------------------------------------
def parse_calibration(path):
    """``parse_calibration`` (lidar_deform.py:13-38): ``{key: 4x4 float64}`` of ``calib.txt``."""
    calib = {}
    with open(path) as f:
        for line in f:
            key, content = line.strip().split(":")
            values = [float(v) for v in content.strip().split()]
            pose = np.zeros((4, 4))
            pose[0, 0:4] = values[0:4]
            pose[1, 0:4] = values[4:8]
            pose[2, 0:4] = values[8:12]
            pose[3, 3] = 1.0
            calib[key] = pose
    return calib


def parse_poses(path, calib):
    """``parse_poses`` (lidar_deform.py:41-74) without its ``print``: the list of ``Tr^-1 . pose . Tr`` (4x4 float64)."""
    poses = []
    Tr = calib["Tr"]
    Tr_inv = np.linalg.inv(Tr)
    with open(path) as f:
        for line in f:
            if len(line.strip()) == 0:
                continue
            values = [float(v) for v in line.strip().split()]
            pose = np.zeros((4, 4))
            pose[0, 0:4] = values[0:4]
            pose[1, 0:4] = values[4:8]
            pose[2, 0:4] = values[8:12]
            pose[3, 3] = 1.0
            poses.append(np.matmul(Tr_inv, np.matmul(pose, Tr)))
    return poses


def relative_indices(nscans):
    """The slot order of ``open_multiple_scans`` (laserscan.py:783-790): the primary scan first, then the previous and the
    next ones in file order -- 1 -> [0], 3 -> [0, -1, 1], 4 -> [0, -2, -1, 1]."""
    nscans = int(nscans)
    if nscans < 1:
        raise ValueError("number_of_scans: at least one")
    if nscans == 1:
        return [0]
    n_prev = nscans // 2
    rel = [r for r in range(-n_prev, nscans - n_prev) if r != 0]
    return [0] + rel


def _check_classes(name, classes):
    out = []
    for c in classes:
        if int(c) != c or not 0 <= int(c) <= 65535:
            raise ValueError(f"{name}: class {c!r} is outside 0..65535 (labels are masked to their lower 16 bits)")
        out.append(int(c))
    return out


class _Pinned:
    """One ``lt_host_alloc`` buffer, seen as a numpy byte array."""

    def __init__(self, lib, nbytes):
        self._lib = lib
        self.nbytes = max(int(nbytes), 16)
        p = C.c_void_p()
        _lib.check(lib.lt_host_alloc(C.byref(p), self.nbytes), "lt_host_alloc")
        self.ptr = p
        self.array = np.ctypeslib.as_array((C.c_ubyte * self.nbytes).from_address(p.value))

    def free(self):
        if self.ptr is not None:
            self.array = None
            self._lib.lt_host_free(self.ptr)
            self.ptr = None


class SequenceSource:
    """The scans, labels and poses of one sequence, and a device cache of its RAW scans.

        SequenceSource(dataset, "00")                               # <dataset>/sequences/00/{velodyne,labels,calib.txt,poses.txt}
        SequenceSource(scans=[xyzr ...], labels=[u32 ...], poses=[4x4 ...])   # arrays of the caller's own loader

    ``scan_names`` / ``label_names`` are the sorted file lists of lidar_deform.py:208-227.  :meth:`raw` returns the device
    tensors holding a scan's file bytes (``xyzr`` [n,4] float32, ``label`` [n] int32: the uint32 words, unmasked): each file
    is read once into pinned memory (``lt_host_alloc``) and uploaded once; the last ``cache_scans`` raw scans (and at most
    ``cache_bytes``) stay resident.  ``cache_scans`` must cover ``number_of_scans`` plus the scans of the output scans still
    in flight.  A scan whose label file holds another number of points raises ``ValueError`` (laserscan.py:587-590) before
    anything is uploaded.  ``stats``: ``uploads`` / ``hits`` / ``bytes``; ``upload_counts[i]``: uploads of scan ``i``."""

    def __init__(self, dataset=None, sequence=None, scans=None, labels=None, poses=None, device=None, cache_scans=16,
                 cache_bytes=256 << 20):
        import torch
        self._torch = torch
        self._lib = _lib.load()
        if dataset is not None:
            seq = os.path.join(dataset, "sequences", str(sequence))
            scan_dir, label_dir = os.path.join(seq, "velodyne"), os.path.join(seq, "labels")
            if not os.path.isdir(scan_dir):
                raise FileNotFoundError(f"sequence folder {scan_dir} does not exist")
            if not os.path.isdir(label_dir):
                raise FileNotFoundError(f"labels folder {label_dir} does not exist")
            self.scan_names = sorted(os.path.join(dp, f) for dp, dn, fn in os.walk(os.path.expanduser(scan_dir)) for f in fn)
            self.label_names = sorted(os.path.join(dp, f) for dp, dn, fn in os.walk(os.path.expanduser(label_dir)) for f in fn)
            if len(self.scan_names) != len(self.label_names):
                raise ValueError(f"{len(self.scan_names)} scans but {len(self.label_names)} label files")   # lidar_deform.py:227
            if poses is None:
                calib = parse_calibration(os.path.join(seq, "calib.txt"))
                poses = parse_poses(os.path.join(seq, "poses.txt"), calib)
            self._arrays = None
        else:
            if scans is None or labels is None or poses is None:
                raise ValueError("SequenceSource: a dataset path, or scans + labels + poses")
            if len(scans) != len(labels):
                raise ValueError(f"{len(scans)} scans but {len(labels)} label arrays")
            self.scan_names = self.label_names = None
            self._arrays = (list(scans), list(labels))
        self.poses = [np.array(p, dtype=np.float64).reshape(4, 4) for p in poses]
        self.n_scans = len(self.scan_names) if self._arrays is None else len(self._arrays[0])
        idx = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", idx)
        self.cache_scans, self.cache_bytes = int(cache_scans), int(cache_bytes)
        self._cache = collections.OrderedDict()   # scan index -> (xyzr, label, n), least recently used first
        self._cached_bytes = 0
        self._staging = []                        # [_Pinned, event of the upload that read it | None]
        self.stats = dict(uploads=0, hits=0, bytes=0)
        self.upload_counts = collections.Counter()

    def __len__(self):
        return self.n_scans

    # ---- the file bytes -------------------------------------------------------------------------------------------------
    def _sizes(self, i):
        """(points, label words) of scan ``i`` -- from the files' sizes / the arrays' shapes, nothing is read"""
        if self._arrays is None:
            sb, lb = os.path.getsize(self.scan_names[i]), os.path.getsize(self.label_names[i])
            if sb % 16:
                raise ValueError(f"{self.scan_names[i]}: {sb} bytes is not a whole number of (x, y, z, remission) float32 records")
            return sb // 16, lb // 4
        s, l = self._arrays[0][i], self._arrays[1][i]
        return int(np.asarray(s).size // 4), int(np.asarray(l).size)

    def check(self, i):
        """``open_label``'s test (laserscan.py:587-590), without reading the scan"""
        n, nl = self._sizes(i)
        if n != nl:
            raise ValueError("Scan and Label don't contain same number of points "
                             f"(scan {i}: {n} points, {nl} labels)")
        return n

    def _stage(self, nbytes):
        for ent in self._staging:
            if ent[0].nbytes >= nbytes and (ent[1] is None or ent[1].query()):
                ent[1] = None
                return ent
        ent = [_Pinned(self._lib, nbytes), None]
        self._staging.append(ent)
        return ent

    def raw(self, i, stream=None):
        """Device tensors of scan ``i``'s file bytes: ``(xyzr [n,4] f32, label [n] i32, n)``, uploaded on ``stream`` (default:
        the current one) unless resident."""
        torch = self._torch
        i = int(i)
        if not 0 <= i < self.n_scans:
            raise IndexError(f"scan {i} is outside the sequence (0..{self.n_scans - 1})")
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        hit = self._cache.get(i)
        if hit is not None:
            self._cache.move_to_end(i)
            self.stats["hits"] += 1
            if hit[3] is not None and hit[3].cuda_stream != st.cuda_stream:
                ev = hit[4]
                st.wait_event(ev)                 # (uploaded on another stream)
                hit[0].record_stream(st)
                hit[1].record_stream(st)
            return hit[0], hit[1], hit[2]
        n = self.check(i)
        ent = self._stage(20 * n)
        host = ent[0].array
        if self._arrays is None:
            with open(self.scan_names[i], "rb") as f:
                got = f.readinto(memoryview(host[:16 * n]))
            with open(self.label_names[i], "rb") as f:
                got += f.readinto(memoryview(host[16 * n:20 * n]))
            if got != 20 * n:
                raise IOError(f"scan {i}: short read ({got} of {20 * n} bytes)")
        else:
            host[:16 * n] = np.ascontiguousarray(self._arrays[0][i], dtype=np.float32).reshape(-1).view(np.uint8)
            host[16 * n:20 * n] = np.ascontiguousarray(self._arrays[1][i]).astype(np.uint32, copy=False).reshape(-1).view(np.uint8)
        with torch.cuda.stream(st):
            dev = torch.empty(max(20 * n, 16), dtype=torch.uint8, device=self.device)
            if n:
                dev[:20 * n].copy_(torch.from_numpy(host[:20 * n]), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st)
        ent[1] = ev
        xyzr = dev[:16 * n].view(torch.float32).view(n, 4)
        label = dev[16 * n:20 * n].view(torch.int32)
        self.stats["uploads"] += 1
        self.stats["bytes"] += 20 * n
        self.upload_counts[i] += 1
        self._cache[i] = (xyzr, label, n, st, ev)
        self._cached_bytes += 20 * n
        while len(self._cache) > 1 and (len(self._cache) > self.cache_scans or self._cached_bytes > self.cache_bytes):
            _, old = self._cache.popitem(last=False)
            self._cached_bytes -= 20 * old[2]
        return xyzr, label, n

    def close(self):
        self._cache.clear()
        self._cached_bytes = 0
        for ent in self._staging:
            if ent[1] is not None:
                ent[1].synchronize()
            ent[0].free()
        self._staging = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ScanIngest:
    """``open_multiple_scans`` + the inverse pose of ``deform`` as one native call per output scan.

    ``approach_or_lists``: a :class:`lidar_transfer_amd.config.Approach` (its ``number_of_scans`` / ``ignore`` / ``moving``)
    or a ``(number_of_scans, ignore, moving)`` tuple.  Class values outside 0..65535 raise ``ValueError`` here."""

    def __init__(self, source, approach_or_lists, device=None):
        import torch
        self._torch = torch
        self._lib = _lib.load()
        self.source = source
        if hasattr(approach_or_lists, "number_of_scans"):
            a = approach_or_lists
            nscans, ignore, moving = a.number_of_scans, a.ignore, a.moving
        else:
            nscans, ignore, moving = approach_or_lists
        self.number_of_scans = int(nscans)
        self.relative = relative_indices(self.number_of_scans)
        if self.number_of_scans > _lib.LT_INGEST_MAX_SCANS:
            raise ValueError(f"number_of_scans: at most {_lib.LT_INGEST_MAX_SCANS}")
        self.ignore = _check_classes("ignore", ignore)
        self.moving = _check_classes("moving", moving)
        self.device = source.device if device is None else torch.device("cuda", int(device))
        if self.device != source.device:
            raise ValueError("ScanIngest: the source's raw scans live on another device")
        self._ign = (C.c_int * max(len(self.ignore), 1))(*self.ignore)
        self._mov = (C.c_int * max(len(self.moving), 1))(*self.moving)

    def scan_indices(self, idx):
        """The scans of output scan ``idx`` in slot order (laserscan.py:792-793).  The reference lets a negative index wrap
        round to the end of the sequence and fails past its end; here both raise ``IndexError``."""
        out = [int(idx) + r for r in self.relative]
        for s in out:
            if not 0 <= s < len(self.source):
                raise IndexError(f"output scan {idx} needs scan {s}, outside the sequence (0..{len(self.source) - 1})")
        return out

    def prepare(self, idx, merged, exact=False, stream=None, back=None):
        """The clouds of output scan ``idx`` as ``deform`` sees them just before its projection: a list of ``(points [n,3]
        f64, remissions [n] f32, label [n] i32)`` CUDA triples -- ONE with ``merged`` (``cp`` / ``mergemesh``), one per slot
        otherwise (``mesh``) -- fresh tensors per call, queued on ``stream`` (default: the current one); the host reads
        nothing back.  The tensors have the raw scans' capacity: behind the kept points sit points at (0, 0, 0), which
        ``do_range_projection_new`` removes (laserscan.py:307-309) and which change no kept point's number.  ``exact=True``
        waits for the kept counts (pinned memory + an event) and returns tensors of exactly the kept lengths.
        ``back``: the second transform -- default ``np.linalg.inv(poses[idx])``, computed here with numpy as the reference does;
        a 4x4 array replaces it; ``False``: stay in world coordinates."""
        torch, src = self._torch, self.source
        slots = self.scan_indices(idx)                      # (raises before any device work)
        for s in slots:
            src.check(s)
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        raws = [src.raw(s, st) for s in slots]
        n_scans = len(slots)
        ns = [r[2] for r in raws]
        total = sum(ns)
        poses = np.ascontiguousarray(np.stack([src.poses[s] for s in slots]), dtype=np.float64)
        if back is None:
            binv = np.ascontiguousarray(np.linalg.inv(src.poses[int(idx)]), dtype=np.float64)
        elif back is False:
            binv = None
        else:
            binv = np.ascontiguousarray(back, dtype=np.float64)
            if binv.shape != (4, 4):
                raise ValueError("back: a 4x4 transform")
        dp = C.POINTER(C.c_double)
        with torch.cuda.stream(st):
            caps = [total] if merged else ns
            outs = [(torch.empty((c, 3), dtype=torch.float64, device=self.device),
                     torch.empty((c,), dtype=torch.float32, device=self.device),
                     torch.empty((c,), dtype=torch.int32, device=self.device)) for c in caps]
            n_kept = torch.empty((n_scans + 1,), dtype=torch.int32, device=self.device)
            work = torch.empty((_lib.ingest_work_ints(total, n_scans),), dtype=torch.int32, device=self.device)
            rs = (_lib.RawScan * n_scans)()
            for k, (xyzr, label, n) in enumerate(raws):
                rs[k].xyzr, rs[k].label, rs[k].n = xyzr.data_ptr(), label.data_ptr(), n
            io = (_lib.IngestOut * len(outs))()
            for k, (p, r, l) in enumerate(outs):
                io[k].points, io[k].rem, io[k].label = p.data_ptr(), r.data_ptr(), l.data_ptr()
            with torch.cuda.device(self.device):
                _lib.check(self._lib.lt_ingest_scans_dev(n_scans, rs, poses.ctypes.data_as(dp),
                                                         binv.ctypes.data_as(dp) if binv is not None else None,
                                                         self._ign, len(self.ignore), self._mov, len(self.moving),
                                                         _lib.LT_INGEST_MERGED if merged else 0, io,
                                                         C.c_void_p(n_kept.data_ptr()), C.c_void_p(work.data_ptr()),
                                                         C.c_void_p(st.cuda_stream)), "lt_ingest_scans_dev")
            if not exact:
                return outs
            host = torch.empty((n_scans + 1,), dtype=torch.int32, pin_memory=True)
            host.copy_(n_kept, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st)
        ev.synchronize()
        kept = [int(x) for x in host.tolist()]
        lens = [kept[n_scans]] if merged else kept[:n_scans]
        return [(p[:k], r[:k], l[:k]) for (p, r, l), k in zip(outs, lens)]
