"""The evaluation of one output scan without a host round trip (csrc/lt_evaluate.hip).

What ``lidar_deform.py`` does around ``deform`` when source and target images have one size (:396-409, :416-418): open the
primary scan alone as a ``SemLaserScan`` -- ``label & 0xFFFF``, ``remove_classes(ignore)``, ``do_range_projection(fov,
remove=True)`` on the float32 file points, ``do_label_projection`` -- and ``compare(scan, scans)``.  Here the source image
comes from the raw scan that ``SequenceSource.raw`` keeps resident (``lt_source_scan_dev``), and ``compare()`` +
``iouEval.addBatch`` leave the device as a 16 KB record (``lt_compare_record_dev``): the label values present and the dense
counts over them, the sum of squared range differences.  Both calls are asynchronous on the caller's stream; the class
renumbering and ``getIoU`` / ``getacc`` are :func:`lidar_transfer_amd.post.confusion_metrics` on the tiny matrix.

    ev = Evaluator(source=(H, W, fov_up, fov_down), ignore=approach.ignore, color_lut=approach.color_lut())
    src = ev.source_scan(*sequence_source.raw(idx))          # dict of [H, W] CUDA images + 'bad_labels'
    rec = ev.compare(src, out["label"], out["range"])        # queued; out: what DeviceDeform.cp / mesh / mergemesh return
    m = rec.metrics(nclasses)                                # waits for the record's event: m_iou, m_acc, MSE, iou

A target with a pose, rows or columns of its own cannot be compared with that image cell by cell.  ``Evaluator(target=...,
target_model=..., transformation=...)`` and ``target_view`` make the image to compare with instead: the same raw scan seen
through the target sensor's model from the target's pose (``lt_target_view_dev``), in the target's shape:

    src = ev.target_view(*sequence_source.raw(idx))
    m = ev.compare(src, out["label"], out["range"]).metrics(nclasses, compared=True)   # + n_compared, MSE_compared
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .post import confusion_metrics


class CompareRecord:
    """One queued ``lt_compare_record_dev`` call: the pinned record and the event behind it."""

    def __init__(self, buf, event, keep):
        self._buf, self._event, self._keep = buf, event, keep

    def ready(self):
        return self._event.query()

    def __del__(self):
        # the copy into the pinned buffer is queued by the library: the buffer must not return to its pool before it landed
        try:
            if self._keep is not None:
                self._event.synchronize()
        except Exception:
            pass

    def raw(self):
        """The record as a :class:`lidar_transfer_amd._lib.CompareRecord` (waits for its event, nothing else)."""
        self._event.synchronize()
        self._keep = None
        return _lib.CompareRecord.from_buffer_copy(self._buf.numpy().tobytes())

    def counts(self):
        """``(status, present [P] int64, counts [P, P] int64, sq_sum, n_cells, src_bad_labels)``"""
        r = self.raw()
        P = min(int(r.n_present), _lib.LT_COMPARE_MAX_PRESENT) if r.status == 0 else 0
        present = np.array(r.present[:P], np.int64)
        counts = np.array(r.counts[:P * P], np.int64).reshape(P, P)
        return int(r.status), present, counts, float(r.sq_sum), int(r.n_cells), int(r.src_bad_labels)

    def metrics(self, nclasses, compared=False):
        """``dict(m_iou, m_acc, MSE, iou)`` as ``compare()`` prints / returns them; with ``compared`` also ``n_compared``, the
        cells that are not background (``n_cells`` minus the cells whose masked source label is 0), and ``MSE_compared`` =
        ``sq_sum / n_compared`` (``None`` when 0): what a sparse reference image needs.  ``IndexError`` where the reference raises
        one: a source label outside the colour table (``colorize``, laserscan.py:642) or a renumbered class index
        ``>= nclasses`` (np_ioueval.py:47).  ``OverflowError`` when the record could not hold the scan (more than 64 label
        values present, or a label outside ``0 .. n_labels - 1``): evaluate that scan with ``post.compare``."""
        status, present, counts, sq_sum, n_cells, bad = self.counts()
        if bad:
            raise IndexError(f"source scan: {bad} points carry a label outside the colour table (colorize, laserscan.py:642)")
        if status != 0:
            raise OverflowError("compare record: " + ("more than 64 label values present" if status == _lib.LT_COMPARE_OVERFLOW
                                                      else "a label outside 0 .. n_labels - 1"))
        _, m_iou, m_acc, iou = confusion_metrics(present, counts, nclasses)
        m = dict(m_iou=m_iou, m_acc=m_acc, MSE=sq_sum / n_cells, iou=iou)
        if compared:   # background cells hold source label 0 (rule 1 of lt_compare_record_dev) and add 0 to sq_sum
            n_bg = int(counts[:, 0].sum()) if len(present) and present[0] == 0 else 0
            m["n_compared"] = n_cells - n_bg
            m["MSE_compared"] = sq_sum / (n_cells - n_bg) if n_cells > n_bg else None
        return m


class Evaluator:
    """Owns an ``lt_evaluator`` (the workspaces of both calls).  One per stream / host thread: calls on one evaluator are
    queued in stream order.  ``source``: the source sensor ``(H, W, fov_up, fov_down)``; ``ignore``: the approach's
    ``ignore`` classes; ``color_lut``: ``Approach.color_lut()`` ([n, 3] float32).  ``n_labels``: label values the pair-count
    workspace spans (a multiple of 256; 512 covers SemanticKITTI's)."""

    def __init__(self, source, ignore, color_lut, n_labels=512, device=None, target=None, target_model=None, transformation=None):
        """``target``: the TARGET sensor ``(H, W, fov_up, fov_down)`` of :meth:`target_view` (``None``: that method raises),
        ``target_model`` its :class:`~lidar_transfer_amd.config.TargetModel` (``None``: the evenly spaced full circle),
        ``transformation`` its mounting, what ``DeviceDeform(transformation=...)`` accepts (``None``, empty or the identity:
        the source's frame).  None of the three changes :meth:`source_scan`."""
        import torch
        self._torch = torch
        self._view = self._view_T = None
        if target is not None:
            from ._chain import Mount
            from .config import TargetModel
            m = target_model if target_model is not None else TargetModel()
            if not isinstance(m, TargetModel):
                raise ValueError("Evaluator: target_model= takes a lidar_transfer_amd.config.TargetModel or None")
            self.t_H, self.t_W, self.t_fov_up, self.t_fov_down = int(target[0]), int(target[1]), float(target[2]), float(target[3])
            self.t_model = m.validate(self.t_H, (self.t_fov_up, self.t_fov_down), "Evaluator")
            sec = m.sector_rad if m.sector_rad is not None else (0.0, 0.0)
            az = m.azimuth_rad
            self._view = _lib.ViewModel(self.t_fov_up, self.t_fov_down, self.t_H, self.t_W, m.proj_flags, m.rows_ptr,
                                        None if az is None else az.ctypes.data_as(C.c_void_p), float(sec[0]), float(sec[1]))
            T = Mount(transformation).T          # (the model keeps `rows` and `az` alive, the evaluator the model and T)
            self._view_T = None if T is None else np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        elif target_model is not None or transformation is not None:
            raise ValueError("Evaluator: target_model= and transformation= describe the sensor of target=, which is missing")
        self._lib = _lib.load()
        idx = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", idx)
        self.H, self.W, self.fov_up, self.fov_down = int(source[0]), int(source[1]), float(source[2]), float(source[3])
        self.ignore = [int(c) for c in ignore]
        for c in self.ignore:
            if not 0 <= c <= 65535:
                raise ValueError(f"ignore: class {c!r} is outside 0..65535 (labels are masked to their lower 16 bits)")
        self._ign = (C.c_int * max(len(self.ignore), 1))(*self.ignore)
        lut = np.ascontiguousarray(color_lut, dtype=np.float32).reshape(-1, 3)
        self.lut = torch.from_numpy(lut).to(self.device)
        self.n_labels = int(n_labels)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.lt_evaluator_create(C.byref(h), self.n_labels, idx), "lt_evaluator_create")
        self._h = h

    def _scan_images(self, xyzr, label, n, stream, H, W, call, what):
        """the images both scan calls fill: allocated on ``stream``, handed to ``call(raw scan, images, stream pointer)``"""
        torch = self._torch
        n = int(xyzr.shape[0]) if n is None else int(n)
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        with torch.cuda.stream(st), torch.cuda.device(self.device):
            out = dict(range=torch.empty((H, W), dtype=torch.float32, device=self.device),
                       rem=torch.empty((H, W), dtype=torch.float32, device=self.device),
                       label=torch.empty((H, W), dtype=torch.int32, device=self.device),
                       black=torch.empty((H, W), dtype=torch.uint8, device=self.device),
                       bad_labels=torch.empty((1,), dtype=torch.int32, device=self.device))
            rs = _lib.RawScan(xyzr.data_ptr() if n else None, label.data_ptr() if n else None, n)
            im = _lib.SourceImages(*[out[k].data_ptr() for k in ("range", "rem", "label", "black", "bad_labels")])
            _lib.check(call(C.byref(rs), C.byref(im), C.c_void_p(st.cuda_stream)), what)
        out["_keep"] = (xyzr, label)   # (the kernels are queued, not finished)
        return out

    def source_scan(self, xyzr, label, n=None, stream=None):
        """The source reference image of lidar_deform.py:403-409 from a raw scan's device tensors (``SequenceSource.raw``):
        ``range`` / ``rem`` [H, W] f32 (empty -1), ``label`` [H, W] i32 (empty 0), ``black`` [H, W] u8 (``sum(proj_color) ==
        0``), ``bad_labels`` [1] i32 (points whose label is outside the colour table).  Queued on ``stream``."""
        def call(rs, im, st):
            return self._lib.lt_source_scan_dev(self._h, rs, self._ign, len(self.ignore), self.fov_up, self.fov_down, self.H,
                                                self.W, self.lut.data_ptr(), int(self.lut.shape[0]), im, st)
        return self._scan_images(xyzr, label, n, stream, self.H, self.W, call, "lt_source_scan_dev")

    def target_view(self, xyzr, label, n=None, stream=None):
        """The TARGET VIEW of a raw scan's device tensors (``lt_target_view_dev``): the scan seen through the target sensor's
        model from the target's pose -- what ``cp`` with one scan would put into the target image.  The dict
        :meth:`source_scan` returns, in the target's shape [t_H, t_W]; :meth:`compare` takes it as ``src``.  Queued on
        ``stream``; needs ``Evaluator(target=...)``."""
        if self._view is None:
            raise ValueError("Evaluator.target_view: constructed without target=")
        T = None if self._view_T is None else self._view_T.ctypes.data_as(C.POINTER(C.c_double))

        def call(rs, im, st):
            return self._lib.lt_target_view_dev(self._h, rs, self._ign, len(self.ignore), T, C.byref(self._view),
                                                self.lut.data_ptr(), int(self.lut.shape[0]), im, st)
        return self._scan_images(xyzr, label, n, stream, self.t_H, self.t_W, call, "lt_target_view_dev")

    def compare(self, src, tgt_label, tgt_range, stream=None):
        """Queue ``compare()`` + ``addBatch`` of one output scan: ``src`` from :meth:`source_scan` or :meth:`target_view`,
        ``tgt_label`` i32 and ``tgt_range`` f32 in the shape of ``src``'s images, as ``DeviceDeform`` returns them.  Returns a
        :class:`CompareRecord`."""
        torch = self._torch
        H, W = self.H, self.W                        # the shape of `src`: the source's, or this evaluator's target view's
        if self._view is not None and tuple(src["label"].shape) == (self.t_H, self.t_W):
            H, W = self.t_H, self.t_W
        if tuple(src["label"].shape) != (H, W) or tuple(tgt_label.shape) != (H, W) or tuple(tgt_range.shape) != (H, W):
            raise ValueError(f"compare: the target images must be {H} x {W} like the source's (lidar_deform.py:416)")
        if tgt_label.dtype != torch.int32 or tgt_range.dtype != torch.float32:
            raise TypeError("compare: tgt_label int32, tgt_range float32")
        tl, tr = tgt_label.contiguous(), tgt_range.contiguous()
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        buf = torch.empty((C.sizeof(_lib.CompareRecord),), dtype=torch.uint8, pin_memory=True)
        with torch.cuda.stream(st), torch.cuda.device(self.device):
            _lib.check(self._lib.lt_compare_record_dev(self._h, src["label"].data_ptr(), src["black"].data_ptr(), tl.data_ptr(),
                                                       src["range"].data_ptr(), tr.data_ptr(), H * W,
                                                       src["bad_labels"].data_ptr(), buf.data_ptr(),
                                                       C.c_void_p(st.cuda_stream)), "lt_compare_record_dev")
            ev = torch.cuda.Event()
            ev.record(st)
        return CompareRecord(buf, ev, (src, tl, tr))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lt_evaluator_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
