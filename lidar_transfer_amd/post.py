"""What the reference does with the rendered images right after the hot path:
back-projection, SemanticKITTI packing / writing, and the source-vs-target comparison -- computed by
``liblidarhip.so`` (lt_post.hip); torch is used for device buffers only."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _device():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("lidar_transfer_amd.post needs a GPU (there is no CPU implementation)")
    return torch.device("cuda", torch.cuda.current_device())


def do_reverse_projection_new(range_image, proj_x, proj_y, fov_up, fov_down, preserve_float=False):
    """``LaserScan.do_reverse_projection_new`` (auxiliary/laserscan.py:475-501).

    ``range_image [H,W] f32``; ``proj_x / proj_y [H,W]``: the integer pixel coordinates of the winning point of
    each cell (``scan.proj_x``), or the float ones (``scan.proj_x_float``) with ``preserve_float``.  Returns
    ``back_points [H*W, 3] float64``.
    """
    import torch
    lib = _lib.load()
    dev = _device()
    H, W = range_image.shape
    rng = _dev(np.asarray(range_image, np.float32), dev)
    dt = np.float64 if preserve_float else np.int32
    px, py = _dev(np.asarray(proj_x, dt), dev), _dev(np.asarray(proj_y, dt), dev)
    out = torch.empty((H * W, 3), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    _lib.check(lib.lt_reverse_projection_dev(rng.data_ptr(), px.data_ptr(), py.data_ptr(), int(preserve_float),
                                             float(fov_up), float(fov_down), H, W, out.data_ptr(),
                                             C.c_void_p(st.cuda_stream)), "lt_reverse_projection_dev")
    return out.cpu().numpy()


def points_to_frame(points, T, tri=None, out=None, stream=None):
    """``points`` ([n, 3] float32 CUDA tensor, contiguous) into the frame ``T`` (4x4, row-major, host) maps to:
    ``float32(((m0 * x + m1 * y) + m2 * z) + m3)`` per row of ``T``, in float64 from the float32 point
    (``lt_points_to_frame_dev``; asynchronous on ``stream``, default the current one).  ``tri`` ([n] int32 CUDA): rows with
    ``tri < 0`` -- rays that missed -- are copied unchanged.  ``out``: where the result goes (``points`` itself is allowed);
    default a fresh tensor."""
    import torch
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32 or not points.is_contiguous():
        raise ValueError("points: contiguous float32 CUDA tensor [n, 3]")
    n = points.numel() // 3
    m = np.ascontiguousarray(T, dtype=np.float64)
    if m.size != 16:
        raise ValueError("T: a 4x4 transform")
    if tri is not None and (tri.dtype != torch.int32 or not tri.is_contiguous() or tri.numel() != n or tri.device != points.device):
        raise ValueError("tri: contiguous int32 CUDA tensor [n] on the points' device")
    if out is None:
        out = torch.empty_like(points)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != points.numel() or out.device != points.device:
        raise ValueError("out: contiguous float32 CUDA tensor of the points' shape and device")
    st = torch.cuda.current_stream(points.device) if stream is None else stream
    with torch.cuda.device(points.device):
        _lib.check(_lib.load().lt_points_to_frame_dev(points.data_ptr(), tri.data_ptr() if tri is not None else None, n,
                                                      m.ctypes.data_as(C.POINTER(C.c_double)), out.data_ptr(),
                                                      C.c_void_p(st.cuda_stream)), "lt_points_to_frame_dev")
    return out


def _image_ptrs(images, n, dev, what="out", label_image=True, endpoints=True):
    """the pointers of a scan's ``images`` of ``n`` cells under the render's keys (``None``: absent or ``None``), each image
    checked against its dtype, its element count and the device ``dev``; ``what`` names the argument in the message"""
    import torch
    want = dict(endcolors=(torch.int32, n if label_image else 3 * n), range=(torch.float32, n), endrem=(torch.float32, n),
                tri=(torch.int32, n))
    if endpoints:
        want = dict(endpoints=(torch.float32, 3 * n), **want)
    ptr = {}
    for key, (dt, numel) in want.items():
        t = images.get(key)
        if t is not None and (not t.is_cuda or t.dtype != dt or not t.is_contiguous() or t.numel() != numel or t.device != dev):
            raise ValueError(f"{what}[{key!r}]: contiguous {dt} CUDA tensor with {numel} elements on the device of `tri`")
        ptr[key] = t.data_ptr() if t is not None else None
    return ptr


def _extra_outputs(asked, n, dev):
    """``(dict, pointers)`` of a model's extra [n] outputs, ``asked`` as ``(key, value, dtype)``: ``True`` gives a fresh
    tensor, a tensor is used as given (and checked), ``None`` / ``False`` gives none"""
    import torch
    extra = {}
    for key, t, dt in asked:
        if t is True:
            t = torch.empty((n,), dtype=dt, device=dev)
        elif t is False:
            t = None
        if t is not None and (not t.is_cuda or t.dtype != dt or not t.is_contiguous() or t.numel() != n or t.device != dev):
            raise ValueError(f"{key}: contiguous {dt} CUDA tensor [n] on the device of `tri`")
        extra[key] = t
    return extra, [t.data_ptr() if t is not None else None for t in extra.values()]


def _check_rays(rays, n, dev, message):
    """``rays``: the contiguous float32 CUDA tensor of at least ``n`` rays on ``dev``, else ``ValueError(message)``"""
    import torch
    if not isinstance(rays, torch.Tensor) or not rays.is_cuda or rays.dtype != torch.float32 or not rays.is_contiguous() \
            or rays.numel() < 3 * n or rays.device != dev:
        raise ValueError(message)


def return_model(scene, rays, model, scan, out, incidence=True, drop=True, label_image=True, stream=None, seed_xor=0):
    """The target sensor's return model (``lt_return_model_dev``) on a rendered scan, in place and asynchronous
    on ``stream`` (default the current one): a return outside the range gate, seen beyond ``max_incidence`` or dropped at
    random (``hash(seed, scan, cell)``) becomes the miss the render writes -- end point (0, 0, 0), label 0, remission 0,
    range 0, ``tri`` -1 --, and with ``remission: lambert`` the remission of one that stands is multiplied by the cosine of
    its incidence angle.  ``scene``: the :class:`~lidar_transfer_amd.raytracer.Scene` that rendered (its CURRENT mesh is
    read); ``rays``: the [n, 3] float32 CUDA tensor the ray set was built from; ``model``: a
    :class:`~lidar_transfer_amd.config.ReturnModel`; ``scan``: the output scan's index in its sequence; ``out``: the render's
    images (``Scene.alloc_outputs``' keys; ``tri`` and ``range`` are needed, the others may be absent or ``None``);
    ``label_image``: whether ``endcolors`` is the [n] label image or [n, 3].  ``incidence`` / ``drop``: ``True`` -- a fresh
    [n] float32 / uint8 tensor, a tensor -- that one, ``None`` -- not wanted.  Returns ``dict(incidence=..., drop=...)``:
    the cosine of every standing return (-1 elsewhere) and every cell's code (0 stands, 1 no hit, 2 too near, 3 too far,
    4 incidence, 5 random).  ``seed_xor`` (uint32, default 0: the model's own seed) is xor-ed into the model's seed for this
    call: a second return of the same cells draws for itself."""
    import torch

    from .config import ReturnModel
    if not isinstance(model, ReturnModel):
        raise ValueError("model: a lidar_transfer_amd.config.ReturnModel")
    tri, rng = out.get("tri"), out.get("range")
    if tri is None or rng is None:
        raise ValueError("out: the render's `tri` and `range` images are needed")
    n = tri.numel()
    dev = tri.device
    _check_rays(rays, n, dev, "rays: contiguous float32 CUDA tensor [n, 3] on the images' device")
    ptr = _image_ptrs(out, n, dev, label_image=label_image)
    extra, more = _extra_outputs((("incidence", incidence, torch.float32), ("drop", drop, torch.uint8)), n, dev)
    st = torch.cuda.current_stream(dev) if stream is None else stream
    args = model.args()
    if seed_xor:
        args.seed = (args.seed ^ int(seed_xor)) & 0xFFFFFFFF
    with torch.cuda.device(dev):
        _lib.check(_lib.load().lt_return_model_dev(
            scene._h, rays.data_ptr(), n, C.byref(args), int(scan) & 0xFFFFFFFF, ptr["endpoints"], ptr["endcolors"], ptr["range"],
            ptr["endrem"], ptr["tri"], *more, _lib.LT_TRACE_LABEL_IMAGE if label_image else 0, C.c_void_p(st.cuda_stream)),
            "lt_return_model_dev")
    return extra


def noise_model(origin, model, scan, out, gate=None, range_error=True, state=True, label_image=True, stream=None,
                seed_xor=0):
    """The target sensor's noise model (``lt_noise_model_dev``) on a rendered scan, in place and asynchronous on
    ``stream`` (default the current one).  Per return (``tri >= 0`` and ``range > 0``): the range is jittered by ``(range_sigma
    + range_sigma_rel * range) * z`` and put on the ``range_resolution`` grid, the end point is scaled about ``origin`` to
    the new range, the remission is jittered by ``remission_sigma * z'``, clamped to [0, 1] and put on ``remission_levels``
    levels; ``z``, ``z'``: sums of twelve 16-bit uniforms, a pure function of ``(seed, scan, cell)``.  A return whose new
    range is not positive or lies outside ``gate`` becomes the miss the render writes; every other cell is not touched.  The
    call is read-modify-write: ONCE per rendered scan, behind the return model, before the frame change, evaluation and
    packing.  ``origin``: three numbers, where the scan's rays start in the scene; ``model``: a
    :class:`~lidar_transfer_amd.config.NoiseModel`; ``scan``: the output scan's index in its sequence; ``out``: the render's
    images (``Scene.alloc_outputs``' keys; ``tri`` and ``range`` are needed, the others may be absent or ``None``); ``gate``:
    the sensor's :class:`~lidar_transfer_amd.config.ReturnModel` or ``None``; ``label_image``: whether ``endcolors`` is the
    [n] label image or [n, 3].  ``range_error`` / ``state``: ``True`` -- a fresh [n] float32 / uint8 tensor, a tensor -- that
    one, ``None`` -- not wanted.  Returns ``dict(range_error=..., noise_state=...)``: ``float32(new - old)`` of every noised
    return (0 elsewhere) and every cell's state (0 untouched, 1 noised, 2 lost).  ``seed_xor``: as for
    :func:`return_model`."""
    import torch

    from .config import NoiseModel, ReturnModel
    if not isinstance(model, NoiseModel):
        raise ValueError("model: a lidar_transfer_amd.config.NoiseModel")
    if gate is not None and not isinstance(gate, ReturnModel):
        raise ValueError("gate: a lidar_transfer_amd.config.ReturnModel or None")
    tri, rng = out.get("tri"), out.get("range")
    if tri is None or rng is None:
        raise ValueError("out: the render's `tri` and `range` images are needed")
    n = tri.numel()
    dev = tri.device
    ptr = _image_ptrs(out, n, dev, label_image=label_image)
    extra, more = _extra_outputs((("range_error", range_error, torch.float32), ("noise_state", state, torch.uint8)), n, dev)
    st = torch.cuda.current_stream(dev) if stream is None else stream
    args = model.args(gate)
    if seed_xor:
        args.seed = (args.seed ^ int(seed_xor)) & 0xFFFFFFFF
    o = (C.c_float * 3)(*[float(x) for x in origin])
    with torch.cuda.device(dev):
        _lib.check(_lib.load().lt_noise_model_dev(
            o, n, C.byref(args), int(scan) & 0xFFFFFFFF, ptr["endpoints"], ptr["endcolors"], ptr["range"], ptr["endrem"],
            ptr["tri"], *more, _lib.LT_TRACE_LABEL_IMAGE if label_image else 0, C.c_void_p(st.cuda_stream)), "lt_noise_model_dev")
    return extra


def create_subrays(rays, model, stream=None):
    """The sub-rays of a target sensor with a beam divergence (``lt_create_subrays_dev``), asynchronous on
    ``stream`` (default the current one): ``rays`` [n, 3] float32 (CUDA, contiguous; the finished ray tensor, whatever pose,
    table, sector or offsets made it) -> [S * n, 3] float32, PLANE BY PLANE: sub-ray ``k`` of cell ``i`` is row ``k * n + i``.
    Plane 0 is ``rays`` byte for byte; plane ``k >= 1`` leaves at ``model.offsets()[k]`` from the central ray, ``a`` to the
    left and ``b`` upwards in units of its length, not normalised (the ray set does that).  ``model``: a
    :class:`~lidar_transfer_amd.config.EchoModel`."""
    import torch

    from .config import EchoModel
    if not isinstance(model, EchoModel) or model.is_default:
        raise ValueError("model: a lidar_transfer_amd.config.EchoModel with a divergence and at least two sub-rays")
    if not isinstance(rays, torch.Tensor) or not rays.is_cuda or rays.dtype != torch.float32 or not rays.is_contiguous() \
            or rays.numel() % 3:
        raise ValueError("rays: contiguous float32 CUDA tensor [n, 3]")
    n = rays.numel() // 3
    dev = rays.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    args = model.args()
    with torch.cuda.device(dev), torch.cuda.stream(st):
        sub = torch.empty((model.subrays * n, 3), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().lt_create_subrays_dev(rays.data_ptr(), n, C.byref(args), sub.data_ptr(),
                                                     C.c_void_p(st.cuda_stream)), "lt_create_subrays_dev")
    return sub


def echo_resolve(rays, origin, model, sub, out, n_echoes=True, fraction=True, stream=None):
    """The target sensor's echo model (``lt_echo_resolve_dev``): the ``S`` sub-images ``sub`` of a render of
    :func:`create_subrays`' rays resolved into the scan ``out``, asynchronous on ``stream`` (default the current one).  Per
    cell the sub-hits (``tri >= 0`` and ``range > 0``) are walked in ``(range, k)`` order and grouped into echoes -- a sub-hit
    more than ``separation`` behind an echo's first one opens the next --; an echo of at least ``min_subrays`` sub-hits is
    detected; ``mode`` picks one of them; the cell gets the mean range of its sub-hits, ``1 / S`` of the sum of their
    remissions, the label and triangle of its member with the smallest ``k`` and an end point on the CENTRAL ray at that
    range.  A cell without a detected echo becomes the miss the render writes.  ``rays``: the central rays [n, 3] float32;
    ``origin``: three numbers, where they start in the scene; ``model``: a :class:`~lidar_transfer_amd.config.EchoModel`;
    ``sub``: the sub-render's images, ``range`` and ``tri`` [S * n] (needed), ``endcolors`` (the [S * n] label image) and
    ``endrem`` (absent or ``None``: read as 0); ``out``: the scan's images (``Scene.alloc_outputs``' keys with the label image;
    ``range`` and ``tri`` are needed, the others may be absent or ``None``), every cell of each written.  ``n_echoes`` /
    ``fraction``: ``True`` -- a fresh [n] uint8 / float32 tensor, a tensor -- that one, ``None`` -- not wanted.  Returns
    ``dict(n_echoes=..., echo_fraction=...)``: the number of detected echoes of every cell and the share ``c / S`` of the
    beam's sub-rays in the reported one (0 for a miss)."""
    import torch

    from .config import EchoModel
    if not isinstance(model, EchoModel) or model.is_default:
        raise ValueError("model: a lidar_transfer_amd.config.EchoModel with a divergence and at least two sub-rays")
    tri, rng = out.get("tri"), out.get("range")
    if tri is None or rng is None:
        raise ValueError("out: the scan's `tri` and `range` images are needed")
    if sub.get("tri") is None or sub.get("range") is None:
        raise ValueError("sub: the sub-render's `tri` and `range` images are needed")
    n = tri.numel()
    S = model.subrays
    dev = tri.device
    o = _image_ptrs(out, n, dev)
    s = _image_ptrs(sub, S * n, dev, "sub", endpoints=False)
    _check_rays(rays, n, dev, "rays: contiguous float32 CUDA tensor [n, 3], the central rays, on the device of `tri`")
    extra, more = _extra_outputs((("n_echoes", n_echoes, torch.uint8), ("echo_fraction", fraction, torch.float32)), n, dev)
    st = torch.cuda.current_stream(dev) if stream is None else stream
    args = model.args()
    org = (C.c_float * 3)(*[float(x) for x in origin])
    with torch.cuda.device(dev):
        _lib.check(_lib.load().lt_echo_resolve_dev(
            rays.data_ptr(), org, n, C.byref(args), s["range"], s["endcolors"], s["endrem"], s["tri"], o["endpoints"],
            o["endcolors"], o["range"], o["endrem"], o["tri"], *more, C.c_void_p(st.cuda_stream)), "lt_echo_resolve_dev")
    return extra


def echo_resolve_dual(rays, origin, model, second, sub, out, out2, n_echoes=True, fraction=True, fraction2=True, stream=None):
    """The dual-return resolve (``lt_echo_resolve_dual_dev``): :func:`echo_resolve` into ``out``, bit for bit, and
    in the same launch a SECOND echo of every cell into ``out2``.  ``second``: a
    :class:`~lidar_transfer_amd.config.DualReturn` that is on; its rule picks among the cell's detected echoes other than the
    primary -- ``first`` the earliest of the rest, ``last`` the latest, ``strongest`` the largest remission sum (a tie to
    the larger count, then to the earlier).  The second echo's range, remission, label, triangle and end point (on the
    CENTRAL ray) are the primary's expressions on its own sub-hits; a cell with fewer than two detected echoes gets the miss
    the render writes.  ``out2``: images under ``out``'s keys (``range`` and ``tri`` are needed, the others may be absent or
    ``None``), overlapping nothing of ``out`` or ``sub``.  ``fraction2``: as ``fraction``, for the second echo.  Returns
    ``dict(n_echoes=..., echo_fraction=..., echo_fraction2=...)``."""
    import torch

    from .config import DualReturn, EchoModel
    if not isinstance(model, EchoModel) or model.is_default:
        raise ValueError("model: a lidar_transfer_amd.config.EchoModel with a divergence and at least two sub-rays")
    if not isinstance(second, DualReturn) or second.is_default:
        raise ValueError("second: a lidar_transfer_amd.config.DualReturn whose `second` is first, strongest or last")
    tri, rng = out.get("tri"), out.get("range")
    if tri is None or rng is None:
        raise ValueError("out: the scan's `tri` and `range` images are needed")
    if out2.get("tri") is None or out2.get("range") is None:
        raise ValueError("out2: the second return's `tri` and `range` images are needed")
    if sub.get("tri") is None or sub.get("range") is None:
        raise ValueError("sub: the sub-render's `tri` and `range` images are needed")
    n = tri.numel()
    S = model.subrays
    dev = tri.device
    o = _image_ptrs(out, n, dev)
    o2 = _image_ptrs(out2, n, dev, "out2")
    s = _image_ptrs(sub, S * n, dev, "sub", endpoints=False)
    _check_rays(rays, n, dev, "rays: contiguous float32 CUDA tensor [n, 3], the central rays, on the device of `tri`")
    extra, more = _extra_outputs((("n_echoes", n_echoes, torch.uint8), ("echo_fraction", fraction, torch.float32),
                                  ("echo_fraction2", fraction2, torch.float32)), n, dev)
    st = torch.cuda.current_stream(dev) if stream is None else stream
    args = model.args()
    org = (C.c_float * 3)(*[float(x) for x in origin])
    with torch.cuda.device(dev):
        _lib.check(_lib.load().lt_echo_resolve_dual_dev(
            rays.data_ptr(), org, n, C.byref(args), second.mode, s["range"], s["endcolors"], s["endrem"], s["tri"],
            o["endpoints"], o["endcolors"], o["range"], o["endrem"], o["tri"], more[0], more[1], o2["endpoints"], o2["endcolors"],
            o2["range"], o2["endrem"], o2["tri"], more[2], C.c_void_p(st.cuda_stream)), "lt_echo_resolve_dual_dev")
    return extra


def pack_scan(back_points, label_image, remissions, index=None):
    """Filtering + packing of ``MultiSemLaserScan.write`` (auxiliary/laserscan.py:1133-1160): returns
    ``(bin [N,4] float32, label [N] uint32)`` -- byte-for-byte what the reference writes to
    ``velodyne/NNNNNN.bin`` and ``labels/NNNNNN.label``.  ``index`` is the ``merged.index`` image of the
    ``cp`` adaption (cells with ``index <= 0`` are dropped there), ``None`` for the mesh adaptions."""
    import torch
    lib = _lib.load()
    dev = _device()
    pts = np.ascontiguousarray(np.asarray(back_points).reshape(-1, 3))
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float64)
    n = pts.shape[0]
    lab = np.asarray(label_image).reshape(-1)
    lab = np.where(np.isfinite(lab.astype(np.float64)), lab, -1).astype(np.int32) if lab.dtype.kind == "f" \
        else lab.astype(np.int32)
    rem = np.asarray(remissions, np.float32).reshape(-1)
    tp, tr, tl = _dev(pts, dev), _dev(rem, dev), _dev(lab, dev)
    ti = _dev(np.asarray(index, np.int32).reshape(-1), dev) if index is not None else None
    out_bin = torch.empty((n, 4), dtype=torch.float32, device=dev)
    out_lab = torch.empty((n,), dtype=torch.int32, device=dev)
    kept = C.c_int(0)
    st = torch.cuda.current_stream(dev)
    _lib.check(lib.lt_pack_scan_dev(tp.data_ptr(), int(pts.dtype == np.float64), tr.data_ptr(), tl.data_ptr(),
                                    ti.data_ptr() if ti is not None else None, n, out_bin.data_ptr(),
                                    out_lab.data_ptr(), C.byref(kept), C.c_void_p(st.cuda_stream)),
               "lt_pack_scan_dev")
    k = kept.value
    return out_bin[:k].cpu().numpy(), out_lab[:k].cpu().numpy().view(np.uint32)


def write_scan(out_dir, idx, back_points, label_image, remissions, index=None):
    """Write ``velodyne/NNNNNN.bin`` and ``labels/NNNNNN.label`` like laserscan.py:1162-1178."""
    b, l = pack_scan(back_points, label_image, remissions, index)
    os.makedirs(os.path.join(out_dir, "velodyne"), exist_ok=True)
    os.makedirs(os.path.join(out_dir, "labels"), exist_ok=True)
    b.tofile(os.path.join(out_dir, "velodyne", str(idx).zfill(6) + ".bin"))
    l.tofile(os.path.join(out_dir, "labels", str(idx).zfill(6) + ".label"))
    return b.shape[0]


def confusion_metrics(value, counts, nclasses):
    """The host tail of ``compare()`` on the tiny matrix: ``value`` -- the label values present, ascending; ``counts[t, s]`` --
    cells whose masked target label is ``value[t]`` and source label ``value[s]``.  The reference renumbers IN PLACE on the
    arrays it scans (laserscan.py:1216-1222: label[label == value] = i for the sorted values present).  For non-negative
    labels that is the rank (u_i >= i: no rank meets a value still to come); with negative labels a rank can equal a later
    value and the two classes MERGE ({-1, 0, 3}: -1 -> 0, then every 0 -> 1) -- replayed here on the list of values, not on
    the images.  Then ``iouEval`` (np_ioueval.py:45-70) with the empty classes ignored.  Returns ``(final, m_iou, m_acc,
    iou)``; ``final[j]`` = class of the pixels whose raw label is ``value[j]``.  Both :func:`compare` and the device records
    of ``lt_compare_record_dev`` (:mod:`lidar_transfer_amd.evaluate`) end here."""
    value = np.asarray(value)
    counts = np.asarray(counts, np.int64)
    cur = value.copy()
    for i, v in enumerate(value):
        cur[cur == v] = i
    final = cur
    if len(final) and int(final.max()) >= nclasses:
        # np.add.at would raise IndexError in the reference (np_ioueval.py:47)
        raise IndexError(f"compare: class index {int(final.max())} after renumbering but nclasses = {nclasses}")
    cm = np.zeros((nclasses, nclasses), np.int64)
    np.add.at(cm, (final[:, None], final[None, :]), counts)
    used = np.unique(final)
    ignore = np.setdiff1d(np.arange(nclasses), used)
    include = np.array([c for c in range(nclasses) if c not in set(ignore.tolist())], dtype=np.int64)
    c2 = cm.copy()
    c2[ignore] = 0
    c2[:, ignore] = 0
    tp = np.diag(c2)
    fp = c2.sum(axis=1) - tp
    fn = c2.sum(axis=0) - tp
    union = tp + fp + fn + 1e-15
    iou = tp / union
    m_iou = (tp[include] / union[include]).mean()
    m_acc = tp.sum() / (tp[include].sum() + fp[include].sum() + 1e-15)
    return final, m_iou, m_acc, iou


def compare(source_label, source_color, target_label, source_range, target_range, source_rem, target_rem, nclasses):
    """Array part of ``compare()`` (auxiliary/laserscan.py:1181-1301) + ``iouEval`` (np_ioueval.py).

    Images ``[H,W]`` (colour ``[H,W,3]``).  Returns ``dict(range_diff, rem_diff, m_iou, m_acc, MSE, iou,
    source_label, target_label)`` with the reference's masking, class compaction (labels are renumbered by
    rank among the values present, laserscan.py:1216-1222) and ignore-empty-classes rule.
    """
    import torch
    lib = _lib.load()
    dev = _device()
    H, W = np.asarray(source_label).shape
    n = H * W
    src_l = np.asarray(source_label, np.int32).reshape(-1)
    tgt_l = np.asarray(target_label, np.int32).reshape(-1)
    mx = int(max(np.max(src_l), np.max(tgt_l), 0)) + 1
    lo = int(min(np.min(src_l), np.min(tgt_l), 0))
    if lo < 0:
        # The reference renumbers the labels among the values present (np.unique, laserscan.py:1216-1222) BEFORE
        # they index the confusion matrix (in place -- see the replay below: negative labels can merge classes).  The
        # histogram kernel counts non-negative codes: negatives travel as codes above the largest label (mx - 1 - v)
        # -- raw 0 stays 0, which is what the background rule tests -- and are put back in value order below.
        src_l = np.where(src_l < 0, mx - 1 - src_l, src_l).astype(np.int32)
        tgt_l = np.where(tgt_l < 0, mx - 1 - tgt_l, tgt_l).astype(np.int32)
    NL = 1
    while NL < mx - lo:
        NL <<= 1
    sl, tl = _dev(src_l, dev), _dev(tgt_l, dev)
    sc = _dev(np.asarray(source_color, np.float32).reshape(-1, 3), dev)
    sr, tr = _dev(np.asarray(source_range, np.float32).reshape(-1), dev), _dev(np.asarray(target_range, np.float32).reshape(-1), dev)
    sm, tm = _dev(np.asarray(source_rem, np.float32).reshape(-1), dev), _dev(np.asarray(target_rem, np.float32).reshape(-1), dev)
    conf = torch.empty((NL, NL), dtype=torch.int64, device=dev)
    rd = torch.empty(n, dtype=torch.float32, device=dev)
    md = torch.empty(n, dtype=torch.float32, device=dev)
    slm = torch.empty(n, dtype=torch.int32, device=dev)
    tlm = torch.empty(n, dtype=torch.int32, device=dev)
    sq = torch.zeros(1, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    _lib.check(lib.lt_compare_dev(sl.data_ptr(), sc.data_ptr(), tl.data_ptr(), sr.data_ptr(), tr.data_ptr(),
                                  sm.data_ptr(), tm.data_ptr(), n, NL, conf.data_ptr(), rd.data_ptr(), md.data_ptr(),
                                  slm.data_ptr(), tlm.data_ptr(), sq.data_ptr(), C.c_void_p(st.cuda_stream)),
               "lt_compare_dev")
    conf = conf.cpu().numpy()          # conf[target, source] over raw labels
    # class compaction + iouEval on the (tiny) confusion matrix: host bookkeeping, no image work
    present = np.nonzero(conf.sum(0) + conf.sum(1))[0]
    # codes of negative labels back to values: code c >= mx stands for mx - 1 - c
    value = np.where(present >= mx, mx - 1 - present, present) if lo < 0 else present.copy()
    order = np.argsort(value, kind="stable")
    present, value = present[order], value[order]
    final, m_iou, m_acc, iou = confusion_metrics(value, conf[np.ix_(present, present)], nclasses)
    remap = np.full(NL, -1, np.int32)
    remap[present] = final.astype(np.int32)
    return dict(range_diff=rd.cpu().numpy().reshape(H, W), rem_diff=md.cpu().numpy().reshape(H, W), m_iou=m_iou,
                m_acc=m_acc, MSE=float(sq.item()) / n, iou=iou,
                source_label=remap[slm.cpu().numpy()].reshape(H, W), target_label=remap[tlm.cpu().numpy()].reshape(H, W))
