"""``MultiSemLaserScan.deform`` + ``write`` from point clouds without leaving HBM.

The loop body of the reference per output scan (lidar_deform.py:393-462) for its two adaptions, composed from the
library's device entry points on ONE HIP stream:

``mesh``  (auxiliary/laserscan.py:863-918, :1121-1178)
    per source scan ``do_range_projection_new(fov, remove=True)`` + ``do_label_projection_new`` (:874-881)
    -> fresh ``TSDFVolume``, ``integrate(proj_label3, proj_range, proj_remissions)`` per scan (:886-897)
    -> ``throw_rays_at_mesh`` = marching cubes + ray cast of the target sensor (:899-907), unpack (:909-914)
    -> ``write``: filter + pack ``velodyne/N.bin`` / ``labels/N.label`` (:1133-1178)
    =  ``lt_range_projection_batch_dev`` -> ``lt_fusion_scan_dev`` -> ``lt_pack_scan_dev``

``mergemesh``  (:921-1012, the adaption config/lidar_transfer.yaml selects)
    the scans merged into ONE cloud (:939-949), ``do_range_projection_new`` with the TARGET field of view onto the SOURCE
    H x W (:929-931, :952-954), ``vol_bnds`` clipped IN PLACE by the rounded bounds of the kept points (:957-962), a fresh
    ``TSDFVolume`` of the TARGET field of view (:968), one ``integrate``, rays of the target sensor, ray cast, ``write``
    =  ``lt_range_projection_batch_dev`` (+ the kept points' bounds, left on the device) -> ``lt_mm_geometry_dev`` (the five
       numpy statements on the device-resident bounds, record mirrored to pinned memory) -> ``lt_fusion_scan_dev`` on the
       PREVIOUS scan's geometry (checked afterwards, re-run when the bounds moved) -> ``lt_pack_scan_dev``

``cp``    (:827-861, :1121-1178)
    the merged cloud through ``do_range_projection_new(target fov, remove=True)`` + ``do_label_projection_new`` +
    ``do_reverse_projection_new`` (:841-845), then ``write`` with ``index > 0`` (:1133-1144)
    =  ``lt_range_projection_batch_dev`` -> ``lt_reverse_projection_dev`` -> ``lt_pack_scan_dev``

The clouds are CUDA tensors in the frame the reference projects them in -- made from a sequence's files by
``lidar_transfer_amd.ingest`` (``open_multiple_scans`` + the inverse pose on the device; :meth:`DeviceDeform.deform` puts
it in front of the three adaptions) or by the caller; the host is touched twice per output scan: the mesh sizes inside marching cubes and the number
of packed points.  There is no CPU path: everything ends in ``liblidarhip.so``.
"""
from __future__ import annotations

import ctypes as C

from . import _chain, _lib
from .raytracer import Scene


class MergeMeshState:
    """The ONE ``voxel_bounds`` array ``deform('mergemesh')`` clips output scan after output scan (laserscan.py:957-962 +
    fusion_lidar.py:33-37 on the array lidar_deform.py:321 passes to every ``MultiSemLaserScan``), as device-resident state
    (``lt_mm_state``): a scan's volume geometry depends on EVERY earlier scan of its sequence, so the scans of a sequence
    go through :meth:`geometry` in order -- ``seq`` numbers them when several chains (host threads, streams) share the state
    -- and a job that is cut into blocks (``lidar_transfer_amd.dist``) starts every block at a sequence boundary or replays
    the bounds of the scans before it (:func:`lidar_transfer_amd.dist.mergemesh_blocks`).  ``vol_bnds``: the caller's
    [3, 2] numpy array; it is kept current (``bnds_after`` of the latest scan) like the reference's.  :meth:`reset` = a
    new sequence (the reference starts a new process with the configured bounds per sequence)."""

    def __init__(self, vol_bnds, voxel_size, device):
        import threading

        import numpy as np
        self._lib = _lib.load()
        self._np = np
        self.vol_bnds = vol_bnds if isinstance(vol_bnds, np.ndarray) else np.array(vol_bnds)
        if self.vol_bnds.shape != (3, 2):
            raise ValueError("vol_bnds is [3, 2] (rows x, y, z; columns min, max)")
        self.voxel_size = float(voxel_size)
        self.device = int(device)
        self.is_int = bool(np.issubdtype(self.vol_bnds.dtype, np.integer))
        h = C.c_void_p()
        b = (C.c_double * 6)(*[float(x) for x in self.vol_bnds.reshape(-1)])
        _lib.check(self._lib.lt_mm_state_create(C.byref(h), b, int(self.is_int), self.voxel_size, self.device), "lt_mm_state_create")
        self._h = h
        self._turn = threading.Lock()
        self.pred = None         # bnds_given of the latest VERIFIED scan: what the next chain is launched on
        self._settled_ticket = -1
        self.stats = dict(scans=0, waited=0, rerun=0)

    def reset(self, vol_bnds=None, stream=None):
        """Sequence boundary: the bounds go back to ``vol_bnds`` (default: what the array held at construction is NOT
        remembered -- pass the configured bounds) and the next scan waits for its geometry instead of assuming the last one."""
        np = self._np
        if vol_bnds is not None:
            self.vol_bnds[...] = np.asarray(vol_bnds).reshape(3, 2)
        b = (C.c_double * 6)(*[float(x) for x in self.vol_bnds.reshape(-1)])
        with self._turn:
            _lib.check(self._lib.lt_mm_state_reset(self._h, b, C.c_void_p(stream.cuda_stream if stream is not None else 0)),
                       "lt_mm_state_reset")
            self.pred = None   # (the caller has completed the scans of the previous sequence: FusionScanPipeline.reset_bounds flushes)

    def geometry(self, bnds, stream, seq=None):
        """Queue the bounds statements for one scan behind its projection (``bnds``: the projector's device [3, 2] float64);
        with ``seq`` (the scan's number in its sequence, from 0 since construction / :meth:`reset`) the call waits on the host
        until scans 0 .. seq - 1 have queued theirs (several chains share the state)."""
        t = C.c_int(0)
        _lib.check(self._lib.lt_mm_geometry_dev(self._h, C.c_void_p(bnds.data_ptr()), -1 if seq is None else int(seq), C.byref(t),
                                                C.c_void_p(stream.cuda_stream)), "lt_mm_geometry_dev")
        return t.value

    def skip(self, seq):
        """a scan that failed before its geometry call gives up its turn (no-op when the call was made after all)"""
        t = C.c_int(0)
        self._lib.lt_mm_geometry_dev(self._h, None, int(seq), C.byref(t), None)

    def get(self, ticket):
        g = _lib.MMGeometry()
        _lib.check(self._lib.lt_mm_geometry_get(self._h, int(ticket), C.byref(g)), "lt_mm_geometry_get")
        return g

    def settle(self, ticket, geo):
        """The scan's record is in: mirror the bounds it left behind into the caller's array (the latest scan wins) and make
        its geometry the prediction for the chains launched from now on."""
        np = self._np
        with self._turn:
            if ticket > self._settled_ticket:
                self._settled_ticket = ticket
                if geo.status != 1:
                    self.vol_bnds[...] = np.array(list(geo.bnds_after)).reshape(3, 2)   # (exact: ints are ints already)
                if geo.status == 0:
                    self.pred = tuple(geo.bnds_given)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lt_mm_state_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceDeform:
    """One chain of device objects (projector, TSDF volume, mesh, scene, ray set of the target sensor) that turns the
    source scans of one output scan into the target sensor's scan.

        dd = DeviceDeform(source=(H, W, fov_up, fov_down), target=(t_H, t_W, t_fov_up, t_fov_down),
                          vol_bnds=[[-50, 50], [-50, 50], [-5, 5]], voxel_size=0.05)
        out = dd.mesh([(points, rem, label), ...])     # CUDA tensors, one triple per source scan
        out["bin"], out["label_file"]                  # [N,4] f32 / [N] i32: the bytes of velodyne/N.bin, labels/N.label
        out = dd.cp([(points, rem, label), ...])       # the scans of the merged cloud (concatenated here)
    """

    def __init__(self, source, target, vol_bnds=None, voxel_size=0.1, beam_angles=None, t_beam_angles=None,
                 preserve_float=False, device=None, merge=True, fusion="cuda", mesh_volume=True, rayset=None, mm_state=None,
                 transformation=None, t_beam_table=None, t_sector=None, t_beam_azimuth=None, returns=None, noise=None,
                 echoes=None, dual=None):
        """``fusion``: ``"cuda"`` -- the arithmetic of the reference's CUDA kernel (class-aware with ``merge``), or ``"numpy"`` --
        that of its numpy branch (``FUSION_GPU_MODE == 0``, fusion_lidar.py:290-388; what goldens F13 / F14 are made by).
        ``vol_bnds``: [3,2]; for :meth:`mergemesh` it is STATE, clipped in place call after call exactly as the reference
        clips the one ``voxel_bounds`` array it hands every ``MultiSemLaserScan`` (lidar_deform.py:321-401,
        laserscan.py:960-962, fusion_lidar.py:36) -- pass a numpy array to see it.  ``mesh_volume=False``: do not allocate the
        fixed volume of :meth:`mesh` (a caller that only runs ``mergemesh``).  ``rayset`` / ``mm_state``: a shared target ray set
        (read-only) and a shared :class:`MergeMeshState` -- several chains of one sequence (``FusionScanPipeline``).
        ``transformation``: the approach file's key (16 numbers, ``x_target = T . x_source``; or ``Approach.mount()``'s pair)
        -- the target sensor stands at ``P = inv(T) = [Rp | tp]`` in the primary scan's frame: its rays are ``Rp . d`` cast
        from ``float32(tp)`` into the scene, which is still fused in the primary scan's frame, and the hits' ``endpoints``
        are brought into the target's frame by ``T`` (``endpoints_scene``: as rendered); ``cp`` takes its cloud into the
        target frame on ingest (:meth:`deform`).  Empty, ``None`` or the identity: none of this runs.  A shared ``rayset``
        must have been built for the same pose (a ``RaySet`` with ``pose=P``; ``_chain.TargetHead`` checks it).
        ``t_beam_table``, ``t_sector``, ``t_beam_azimuth``: the fields of the TARGET sensor's
        :class:`~lidar_transfer_amd.config.TargetModel` (``SensorModel.target_model()``; kept as ``t_model``, validated against
        ``target``; each ``None``: nothing of it runs).  The target's rays are the model's (turned by the pose of a
        ``transformation``), so ``mesh`` and ``mergemesh`` change by their rays alone -- and, for a sector, by the ray set's bin
        grid (``TargetModel.grid``; ``mergemesh`` still fuses what the source origin sees inside the target's vertical field of
        view).  ``cp`` projects into the model's rows and columns (``Projector``) and re-projects along the winner's ray (the
        ``lt_reverse_projection*_dev`` entry point of the model).  A shared ``rayset`` must have been built for an equal model.
        ``returns``: the TARGET sensor's :class:`~lidar_transfer_amd.config.ReturnModel` (``SensorModel.return_model()``;
        ``None`` or all-default: nothing of it runs) -- ``mesh`` and ``mergemesh`` then take ``scan_index``, the output scan's
        index in its sequence, apply the model once to the render that stands (range gate, incidence, dropout: such cells
        become misses) before the hits go into the target's frame and before packing, and return ``incidence`` and ``drop``
        as well; ``cp`` renders no surface and raises.
        ``noise``: the TARGET sensor's :class:`~lidar_transfer_amd.config.NoiseModel` (``SensorModel.noise_model()``; ``None``
        or all-default: nothing of it runs) -- ``mesh`` and ``mergemesh`` take ``scan_index`` for it too and apply it once to
        the render that stands, BEHIND the return model (whose range gate a measured range must stay inside) and before the
        frame change and packing: ranges are jittered and put on a grid, the end points follow along their rays about the
        ray origin, remission is jittered and put on levels; the result holds ``range_error`` and
        ``noise_state`` [n] as well.  ``cp`` renders no ray and has no origin: it raises.
        ``echoes``: the TARGET sensor's :class:`~lidar_transfer_amd.config.EchoModel` (``SensorModel.echo_model()``; ``None``
        or off: nothing of it runs) -- a beam with a divergence: ``mesh`` and ``mergemesh`` render ``S`` sub-rays
        per cell (one read-only ray set over them, made here or shared: a bound ``_chain.Echoes`` of another chain) into
        scratch images and resolve them into the scan -- echoes along the range, one reported, a blended range where two
        surfaces are closer than ``separation`` -- on the render that stands, AHEAD of the return and noise models, which see
        the resolved scan; the result holds ``n_echoes`` [n] uint8 and ``echo_fraction`` [n] as well.  No ``scan_index`` is
        needed: nothing is drawn.  ``cp`` renders no ray: it raises.
        ``dual``: the TARGET sensor's :class:`~lidar_transfer_amd.config.DualReturn` (``SensorModel.dual_return()``; ``None``
        or ``second: none``: nothing of it runs; it needs ``echoes``) -- ``mesh`` and ``mergemesh`` resolve TWO echoes per cell
        in the one resolve launch; the primary's images are bit for bit those without the setting; the second return goes
        through the return and noise models with draws of its own and comes back under ``second`` (``range`` / ``rem`` /
        ``label`` images, ``endpoints``, ``endpoints_scene``, ``tri``, ``echo_fraction`` and the models' images); ``bin`` /
        ``label_file`` hold the primary's packed rows followed by the second returns' (DESIGN 7h).  A caller's ``out`` then
        has its five images replaced by views of the scan's two-plane allocations.  ``cp`` renders no ray: it raises."""
        import numpy as np
        import torch

        from .fusion import DeviceMesh, TSDFVolume
        from .laserscan import Projector
        self._torch = torch
        self._lib = _lib.load()
        idx = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", idx)
        self.H, self.W, self.fov_up, self.fov_down = int(source[0]), int(source[1]), float(source[2]), float(source[3])
        self.beam_angles = sorted(beam_angles) if beam_angles else None      # laserscan.py:732-735
        # the reference reads the TARGET's beam angles from the source config (laserscan.py:744)
        self.t_beam_angles = sorted(t_beam_angles) if t_beam_angles else self.beam_angles
        self.preserve_float = bool(preserve_float)
        self.projector = Projector(idx)
        self._merge = _lib.LT_TSDF_MERGE if merge else 0
        self.vol = self.mesh_obj = self.scene = self.rayset = None
        self._merge_flag, self._fusion, self._voxel_size, self._idx = bool(merge), fusion, voxel_size, idx
        self._mm_vols = {}   # mergemesh: geometry -> TSDFVolume (the clipped bounds settle after a few output scans)
        self.vol_bnds = None
        self._mm_state, self._mm_own = mm_state, mm_state is None
        if mm_state is not None and vol_bnds is None:
            vol_bnds = mm_state.vol_bnds
        # the target sensor: shape, model, what stands between the render and the result, rays (with a scene to cast at), origin
        h = self.head = _chain.TargetHead(target, transformation, returns, noise, echoes, dual, "DeviceDeform", idx, t_beam_table,
                                          t_sector, t_beam_azimuth, rayset=rayset, cast=vol_bnds is not None)
        s = self._sensing = h.sensing
        self.t_H, self.t_W, self.t_fov_up, self.t_fov_down, self.n_rays = h.t_H, h.t_W, h.t_fov_up, h.t_fov_down, h.n_rays
        self._mounting, self._returns, self._noise, self._echoes = s.mounting, s.returns, s.noise, s.echoes
        self.returns, self.noise, self.echoes, self.dual = s.returns.model, s.noise.model, s.echoes.model, s.dual.setting
        m = self.t_model = h.t_model
        # what the reverse projection reads on the device: the table and the offsets in radians
        self._t_brad = None if m.rows is None else torch.from_numpy(m.rows[:self.t_H].copy()).to(self.device)
        self._t_az_dev = None if m.azimuth_rad is None else torch.from_numpy(m.azimuth_rad.copy()).to(self.device)
        self.mount, self.origin, self.rayset = s.mount, h.origin, h.rayset
        if vol_bnds is not None:
            self.vol_bnds = vol_bnds if isinstance(vol_bnds, np.ndarray) else np.array(vol_bnds)
            if self.vol_bnds.shape != (3, 2):
                raise ValueError("DeviceDeform: vol_bnds is [3, 2] (rows x, y, z; columns min, max)")
            # the volume is the SOURCE sensor's (laserscan.py:886-887), the rays the TARGET's (:899-900)
            if mesh_volume:
                self.vol = TSDFVolume(self.vol_bnds, voxel_size, self.fov_up, self.fov_down, device=idx, merge=merge, mode=fusion)
                self._merge = self.vol._flags
            self.mesh_obj = DeviceMesh(idx)
            self.scene = Scene(idx)

    t_beam_table = property(lambda self: self.t_model.beam_table)
    t_sector = property(lambda self: self.t_model.sector)
    t_beam_azimuth = property(lambda self: self.t_model.beam_azimuth)

    def _stream(self):
        """The caller's current stream -- ordered behind the stream of the previous call when that was another one: the
        projector re-arms its z-min keys, and the volume / mesh / scene are reused, in stream order."""
        torch = self._torch
        st = torch.cuda.current_stream(self.device)
        last = getattr(self, "_last_stream", None)
        if last is not None and last.cuda_stream != st.cuda_stream:
            ev = torch.cuda.Event()
            ev.record(last)
            st.wait_event(ev)
        self._last_stream = st
        return st

    def cp_back(self, pose):
        """``cp`` with a mounted target: the second transform of the ingest, ``T . inv(pose of the primary scan)`` (float64,
        host) -- the merged cloud arrives in the target's frame; ``None`` (the ingest's default) without a mounting"""
        import numpy as np
        if self.mount is None:
            return None
        return np.matmul(self.mount[0], np.linalg.inv(pose))

    # ---- write(): filter + pack (laserscan.py:1133-1178) -------------------------------------------------------------
    def _pack(self, points, is_f64, rem, label, index, n, st):
        """``lt_pack_scan_dev`` on this chain's device: every packing of this chain's target goes through here"""
        return _chain.pack_rows(points, is_f64, rem, label, index, n, st, self.device)

    def pack_result(self, out, stream=None, scene_frame=False):
        """``write``'s packing for a result of :meth:`cp`, :meth:`mesh` or :meth:`mergemesh` made with ``pack=False``:
        ``(bin [N,4] f32, label_file [N] i32)``.  ``cp`` packs its float64 ``back_points`` where ``index > 0``
        (laserscan.py:1133-1144); the mesh adaptions their float32 ``endpoints``, no index filter (:1145-1148).  A dual-return
        result packs both of its planes in the ONE call: the primary's rows in cell order, then the second returns'
        (``_chain.pack_result``, the one packing of every head)."""
        return self.head.pack(out, stream if stream is not None else self._stream(), scene_frame, self._pack)

    @property
    def last_stream(self):
        """the stream of this chain's last call (``None`` before the first): what a caller that continues the scan on the
        same scene -- a rig's further heads -- queues its work on"""
        return getattr(self, "_last_stream", None)

    @property
    def bound_echoes(self):
        """this chain's bound ``_chain.Echoes`` (falsy when the echo model is off): what ``echoes=`` of a further chain of
        the same sensor takes, so that the sub-ray set is shared"""
        return self._echoes

    @property
    def mm_state(self):
        """the :class:`MergeMeshState` of this chain's ``mergemesh`` calls (``None`` before the first without a shared one)"""
        return self._mm_state

    # ---- deform('mesh') + write ---------------------------------------------------------------------------------------
    def mesh(self, clouds, origin=None, pack=True, timing=None, scan_index=None):
        """``clouds``: one (points [n,3] f32|f64, remissions [n] f32, label [n] i32) triple of CUDA tensors per source scan,
        already in the primary scan's frame (laserscan.py:876-879).  Returns the target scan: ``range`` / ``rem`` [t_H,t_W]
        f32, ``label`` [t_H,t_W] i32 (``label_image``, :912), ``endpoints`` [t_H*t_W,3] f32 (``back_points``), ``tri``, the
        source images per scan under ``source``, and -- with ``pack`` -- ``bin`` [N,4] f32 + ``label_file`` [N] i32, the
        bytes ``write`` puts into ``velodyne/N.bin`` and ``labels/N.label``.  ``timing``: a list that receives CUDA events
        (start, projected, rendered, packed) when given.  ``origin``: where the rays start in the scene (default: the target
        sensor's position, (0, 0, 0) unless it is mounted elsewhere); ``endpoints`` are in the target sensor's frame,
        ``endpoints_scene`` as rendered.  ``scan_index``: the output scan's index in its sequence, needed with a return
        model (``returns=``): the result is what the target sensor sees, with ``incidence`` and ``drop`` [n] beside it; and
        with a noise model (``noise=``): what it reports, with ``range_error`` and ``noise_state`` [n]."""
        if origin is None:
            origin = self.origin
        self.head.need_scan_index(scan_index, "DeviceDeform.mesh")
        if self.vol is None:
            raise RuntimeError("DeviceDeform.mesh: constructed without vol_bnds")
        torch, lib = self._torch, self._lib
        st = self._stream()
        n = len(clouds)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timing is not None else None
        if ev:
            ev[0].record(st)
        src = self.projector.project(clouds, self.fov_up, self.fov_down, self.H, self.W, new=True, remove=True,
                                     beam_angles=self.beam_angles, outputs=("range", "rem", "label_folded"), stream=st)
        if ev:
            ev[1].record(st)
        vp = C.c_void_p
        cp, dp, rp = (vp * max(n, 1))(), (vp * max(n, 1))(), (vp * max(n, 1))()
        for k, o in enumerate(src):
            cp[k], dp[k], rp[k] = o["label_folded"].data_ptr(), o["range"].data_ptr(), o["rem"].data_ptr()
        plan = self.head.plan(self.scene)   # (plan[2] is what the render writes: the sub-images, or ``rout``)
        with torch.cuda.device(self.device):
            _lib.check(lib.lt_fusion_scan_dev(self.vol._h, self.mesh_obj._h, self.scene._h, self.head.render_set._h,
                                              n, cp, dp, rp, self.H, self.W, 1.0, self._merge, _chain.origin3(origin),
                                              *_chain.out_ptrs(plan[2]), _chain.TRACE_FLAGS, vp(st.cuda_stream), 0),
                       "lt_fusion_scan_dev")
            res = self.head.finish(plan, scan_index, self.scene, self.mesh_obj, st, origin, source=src)
            if ev:
                ev[2].record(st)
            if pack:
                res["bin"], res["label_file"] = self.pack_result(res, st)
            if ev:
                ev[3].record(st)
                timing.append(ev)
        return res

    # ---- deform('mergemesh') + write ------------------------------------------------------------------------------------
    def _mm(self):
        if self._mm_state is None:
            self._mm_state = MergeMeshState(self.vol_bnds, self._voxel_size, self._idx)
            self.vol_bnds = self._mm_state.vol_bnds
        return self._mm_state

    def reset_bounds(self, vol_bnds=None):
        """A new sequence: ``vol_bnds`` (the configured bounds) replaces what the previous sequence's scans left in the array,
        as a fresh process of the reference would (experiments/run_lidar_deform.sh runs lidar_deform.py per sequence)."""
        if self.vol_bnds is None:
            raise RuntimeError("DeviceDeform.reset_bounds: constructed without vol_bnds")
        self._mm().reset(vol_bnds, self._stream())

    def mergemesh_bounds(self, clouds, seq=None):
        """The bounds bookkeeping of :meth:`mergemesh` WITHOUT the scan: projection of the merged cloud + the bounds statements
        on the device state, nothing read back.  For a rank of a multi-GPU job whose block starts inside a sequence
        (``lidar_transfer_amd.dist.mergemesh_plan``: the scans before the block are replayed through this)."""
        if self.vol_bnds is None:
            raise RuntimeError("DeviceDeform.mergemesh_bounds: constructed without vol_bnds")
        mm = self._mm()
        st = self._stream()
        src = self.projector.project([_chain.merged_cloud(clouds)], self.t_fov_up, self.t_fov_down, self.H, self.W, new=True,
                                     remove=True, beam_angles=self.beam_angles, outputs=("range", "bnds"), stream=st)[0]
        with mm._turn:
            mm.pred = None   # (the next scan waits for its own record: the replayed ones were not verified on the host)
        return mm.geometry(src["bnds"], st, seq)

    def _mergemesh_volume(self, given, dim):
        """The device volume of one geometry -- constructed from the bounds as laserscan.py:961-962 leave them, like the
        reference's TSDFVolume(vol_bnds, ...) (:968), which derives ``dim`` and the origin from them (fusion_lidar.py:33-37).
        Kept per geometry, most recently used last: the bounds only ever shrink and settle after a few scans of a sequence.
        At most three, and ONE when a volume exceeds 4 GiB (the default +-50 / +-50 / +-5 m at 5 cm is 12.8 GB): an evicted
        volume is closed -- a caller still holding it from an earlier result gets a RuntimeError, not freed memory."""
        import numpy as np

        from .fusion import TSDFVolume
        key = tuple(float(x) for x in given)
        vol = self._mm_vols.pop(key, None)
        if vol is None:
            nbytes = 16 * int(dim[0]) * int(dim[1]) * int(dim[2])
            keep = 0 if nbytes > (4 << 30) else 2
            while len(self._mm_vols) > keep:
                self._mm_vols.pop(next(iter(self._mm_vols))).close()
            vol = TSDFVolume(np.array(key).reshape(3, 2), self._voxel_size, self.t_fov_up, self.t_fov_down, device=self._idx,
                             merge=self._merge_flag, mode=self._fusion)   # (3) the TARGET field of view (:968-969)
            assert tuple(int(x) for x in vol._vol_dim) == tuple(int(x) for x in dim)
            vol.bnds_given = key   # (what the library keeps as the volume's ``bnds_given``: is this a scan's geometry?)
        self._mm_vols[key] = vol
        return vol

    def mergemesh(self, clouds, origin=None, pack=True, out=None, seq=None, source_images=False, scan_index=None):
        """``clouds``: the (points, remissions, label) CUDA triples of the source scans, already in the primary scan's frame
        (``apply_inv_pose``, laserscan.py:949: pose handling is out of scope).  Returns what :meth:`mesh` returns -- the
        target scan's ``range`` / ``rem`` / ``label`` images, ``endpoints``, ``tri``, the merged cloud's source image under
        ``source``, ``bin`` / ``label_file`` with ``pack`` -- plus ``vol_dim`` / ``vol_origin`` / ``vol_bnds_after`` of this
        scan's volume.  The kept points' bounds never visit the host before the fusion: the geometry statements run on the
        device (:class:`MergeMeshState`), the chain is launched on the previous scan's geometry and verified against the
        record afterwards (``mm_state.stats``: scans / waited = no prediction yet / rerun = the bounds moved).  ``seq``: this
        scan's number in its sequence when several chains share the state.  By default the whole scan is ONE native call
        (``lt_mergemesh_scan_dev``; the source image stays inside the projector); ``source_images=True`` composes it from
        the public steps instead and returns the merged cloud's images under ``source``.  ``origin`` / ``endpoints`` /
        ``endpoints_scene`` / ``scan_index``: as for :meth:`mesh`; a return model and a noise model are applied to the render
        that stands -- after a re-run, never to the speculative one."""
        if origin is None:
            origin = self.origin
        if self.vol_bnds is None:
            raise RuntimeError("DeviceDeform.mergemesh: constructed without vol_bnds")
        torch = self._torch
        mm = self._mm()
        try:   # (a scan that fails before its geometry call gives up its turn; a no-op once the call has been made)
            st = self._stream()
            cloud = _chain.merged_cloud(clouds)
            self.head.need_scan_index(scan_index, "DeviceDeform.mergemesh")
            plan = self.head.plan(self.scene, out)   # (plan[2] is what the render writes: the sub-images, or ``rout``)
            first, again, more = (self._mm_composed if source_images else self._mm_native)(
                mm, cloud, seq, _chain.origin3(origin), _chain.out_ptrs(plan[2]), st)
            pred, vol = mm.pred, None
            if pred is not None:
                vol = self._mm_vols.get(pred)
                if vol is None:       # (another chain of the sequence verified this geometry)
                    import numpy as np
                    b = np.array(pred).reshape(3, 2)
                    vol = self._mergemesh_volume(pred, np.ceil((b[:, 1] - b[:, 0]) / self._voxel_size).astype(int))
            with torch.cuda.device(self.device):
                geo, done = first(vol)
        except BaseException:
            if seq is not None:
                mm.skip(seq)
            raise
        with torch.cuda.device(self.device):
            mm.stats["scans"] += 1
            mm.settle(geo.ticket, geo)
            if geo.status == 1:
                raise ValueError("DeviceDeform.mergemesh: no point survives the projection (numpy: zero-size array to amin)")
            if geo.status == 2:
                raise RuntimeError(f"DeviceDeform.mergemesh: the clipped volume is empty (bounds {list(geo.bnds_given)})")
            if not done:   # nothing to assume (the first scan of a sequence), or the bounds moved: on its own geometry
                mm.stats["waited" if vol is None else "rerun"] += 1
                vol = self._mergemesh_volume(geo.bnds_given, geo.dim)
                again(vol)
            # (once, on the render that stands)
            res = self.head.finish(plan, scan_index, self.scene, self.mesh_obj, st, origin,
                                   vol_dim=tuple(int(x) for x in geo.dim), vol_origin=vol._vol_origin.copy(),
                                   vol_bnds_after=[float(x) for x in geo.bnds_after], volume=vol, **more)
            if pack:
                res["bin"], res["label_file"] = self.pack_result(res, st)
        return res

    # The two ways of issuing a mergemesh scan's device calls: ``first(vol or None) -> (geo, done)`` = projection + bounds
    # statements [+ the chain on ``vol``, the predicted geometry] + the record, ``done``: the chain ran on the scan's own
    # geometry; ``again(vol)`` = the chain once more on the projected images; and what the way adds to the result.
    def _mm_native(self, mm, cloud, seq, org, ptrs, st):
        """one native call per scan (+ ``lt_mergemesh_rerun_dev``): the source images stay inside the projector"""
        lib, vp = self._lib, C.c_void_p
        cl, keep, is_f64 = _chain.cloud_table([cloud])
        beams = _chain.beam_table(self.beam_angles)   # (pointer, n, the array: alive as long as the callables)
        p = self.projector._h
        rs = self.head.render_set

        def first(vol):
            tflags = vol._flags if vol is not None else (_lib.LT_TSDF_HOST_MODE if self._fusion == "numpy" else self._merge)
            geo, done = _lib.MMGeometry(), C.c_int(0)
            _lib.check(lib.lt_mergemesh_scan_dev(p, mm._h, -1 if seq is None else int(seq), vol._h if vol is not None else None,
                                                 self.mesh_obj._h, self.scene._h, rs._h, cl, is_f64, self.t_fov_up,
                                                 self.t_fov_down, self.H, self.W, beams[0], beams[1], 1.0, tflags, org, *ptrs,
                                                 _chain.TRACE_FLAGS, vp(st.cuda_stream), C.byref(geo), C.byref(done)),
                       "lt_mergemesh_scan_dev")
            return geo, bool(done.value)

        def again(vol):
            _lib.check(lib.lt_mergemesh_rerun_dev(p, vol._h, self.mesh_obj._h, self.scene._h, rs._h, self.H, self.W, 1.0,
                                                  vol._flags, org, *ptrs, _chain.TRACE_FLAGS, vp(st.cuda_stream)),
                       "lt_mergemesh_rerun_dev")
        return first, again, dict(_keep=tuple(keep))

    def _mm_composed(self, mm, cloud, seq, org, ptrs, st):
        """the public steps -- ``project``, ``lt_mm_geometry_dev``, ``lt_fusion_scan_dev`` -- with the merged cloud's images
        returned under ``source``"""
        vp = C.c_void_p
        src = {}
        rs = self.head.render_set

        def again(vol):
            cp, dp, rp = (vp * 1)(src["label_folded"].data_ptr()), (vp * 1)(src["range"].data_ptr()), (vp * 1)(src["rem"].data_ptr())
            _lib.check(self._lib.lt_fusion_scan_dev(vol._h, self.mesh_obj._h, self.scene._h, rs._h, 1, cp, dp, rp, self.H,
                                                    self.W, 1.0, vol._flags, org, *ptrs, _chain.TRACE_FLAGS, vp(st.cuda_stream), 0),
                       "lt_fusion_scan_dev")

        def first(vol):
            # (1) + (2): the SOURCE image size and beam angles, the TARGET field of view (laserscan.py:929-931, :952-954)
            src.update(self.projector.project([cloud], self.t_fov_up, self.t_fov_down, self.H, self.W, new=True, remove=True,
                                              beam_angles=self.beam_angles, outputs=("range", "rem", "label_folded", "bnds"),
                                              stream=st)[0])
            ticket = mm.geometry(src["bnds"], st, seq)
            if vol is not None:
                again(vol)            # (waits for the stream once, inside marching cubes: the record has arrived with it)
            geo = mm.get(ticket)
            return geo, vol is not None and geo.status == 0 and tuple(geo.bnds_given) == vol.bnds_given
        return first, again, dict(source=src)

    # ---- deform('cp') + write -----------------------------------------------------------------------------------------
    def cp(self, clouds, pack=True):
        """Closest point: the source scans merged into one cloud (laserscan.py:834-839), projected into the TARGET image
        (:841-843), re-projected to points (:844-845) and written (:1133-1160).  Returns ``range``, ``rem``, ``label``,
        ``index`` images, ``back_points`` [t_H*t_W,3] f64 and -- with ``pack`` -- ``bin`` / ``label_file``.
        The reference's ``cp`` path always holds float64 points (``apply_pose``, laserscan.py:98-104) and goldens F12 / F12b pin
        that; float32 clouds with ``preserve_float`` are re-projected in float64 here as well (numpy would stay in float32).
        ``cp`` renders no surface, so there is no incidence angle: with a return model it raises ``ValueError``; it renders
        no ray either, so there is no origin to jitter a range about: with a noise model it raises as well; and no beam to
        widen: with an echo model it raises too, and so with a dual return."""
        for name in ("dual", "echoes", "noise", "returns"):
            if getattr(self, name) is not None:
                key, a, what, why = _chain.CP_REFUSALS[name]
                raise ValueError(f"DeviceDeform.cp: the target sensor has {a} {key}, but cp renders no {what} ({why}): use mesh "
                                 "or mergemesh, or a target file without the key")
        torch = self._torch
        st = self._stream()
        pf = self.preserve_float
        outs = ("idx", "range", "rem", "label") + (("proj_xf", "proj_yf") if pf else ("proj_x", "proj_y"))
        m = self.t_model
        o = self.projector._project([_chain.merged_cloud(clouds)], self.t_fov_up, self.t_fov_down, self.t_H, self.t_W, m, new=True,
                                    remove=True, beam_angles=self.t_beam_angles if m.beam_table is None else None, outputs=outs,
                                    stream=st)[0]
        px, py = (o["proj_xf"], o["proj_yf"]) if pf else (o["proj_x"], o["proj_y"])
        if pf and px.dtype != torch.float64:
            px, py = px.double(), py.double()
        back = torch.empty((self.n_rays, 3), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._reverse_projection(o["range"], px, py, pf, back, st)
            res = dict(range=o["range"], rem=o["rem"], label=o["label"], index=o["idx"], back_points=back)
            if pack:
                res["bin"], res["label_file"] = self.pack_result(res, st)
        return res

    def _reverse_projection(self, rng, px, py, pf, back, st):
        """``do_reverse_projection_new`` by the target's model, through the one of the four entry points that knows it: along
        the winner's beam with the row's offset beside its column's nominal direction; along the ray of the winner's column
        of a sector; along the winner's beam of a table; the reference's (with ``pf`` along the winner's own yaw and pitch)"""
        m = self.t_model
        head, hw = (rng.data_ptr(), px.data_ptr(), py.data_ptr(), int(pf)), (self.t_H, self.t_W)
        fov, tail = (self.t_fov_up, self.t_fov_down), (back.data_ptr(), C.c_void_p(st.cuda_stream))
        brad = None if self._t_brad is None else self._t_brad.data_ptr()
        if m.beam_azimuth is not None:
            sec = None if m.sector is None else m.sector_rad.ctypes.data_as(C.POINTER(C.c_double))
            name, args = "lt_reverse_projection_beams_az_dev", head + (brad, self._t_az_dev.data_ptr(), sec) + hw + tail
        elif m.sector is not None:
            name, args = "lt_reverse_projection_sector_dev", \
                head + (int(brad is not None), brad) + fov + hw + tuple(m.sector_rad.tolist()) + tail
        elif m.beam_table is not None:
            name, args = "lt_reverse_projection_beams_dev", head + (brad,) + hw + tail
        else:
            name, args = "lt_reverse_projection_dev", head + fov + hw + tail
        _lib.check(getattr(self._lib, name)(*args), name)

    # ---- open_multiple_scans + deform(adaption, poses, idx) ----------------------------------------------------------------
    def deform(self, adaption, ingest, idx, back=None, **kw):
        """The reference's loop body from the sequence's files (lidar_deform.py:412-415): ``ingest`` (a
        :class:`lidar_transfer_amd.ingest.ScanIngest`) prepares the clouds of output scan ``idx`` on the caller's stream --
        poses applied, moving / ignore classes removed, back in the primary scan's frame -- and :meth:`cp` / :meth:`mesh` /
        :meth:`mergemesh` (``adaption``) takes them; ``kw`` goes to that method, ``back`` to ``ScanIngest.prepare``.  The clouds carry the raw scans' capacity
        (depth-0 points behind the kept ones, which the projection removes): the kept counts never visit the host."""
        if adaption not in ("cp", "mesh", "mergemesh"):
            raise ValueError(f"DeviceDeform.deform: adaption {adaption!r} (cp, mesh or mergemesh)")
        if ingest.device != self.device:
            raise ValueError("DeviceDeform.deform: the ingest stage lives on another device")
        st = self._stream()
        if back is None and adaption == "cp":    # a mounted target: the merged cloud straight into its frame
            back = self.cp_back(ingest.source.poses[int(idx)])
        clouds = ingest.prepare(idx, merged=adaption != "mesh", stream=st, back=back)
        return getattr(self, adaption)(clouds, **kw)

    @staticmethod
    def write(out, out_dir, idx):
        """``MultiSemLaserScan.write(out_dir, idx)`` (laserscan.py:1162-1178) for a result of :meth:`mesh` / :meth:`cp` that
        was packed: ``velodyne/NNNNNN.bin`` ([N,4] float32 x, y, z, remission) and ``labels/NNNNNN.label`` ([N] uint32) --
        the bytes the reference's per-point ``struct.pack`` loops write.  Returns the number of points."""
        import os
        if "bin" not in out or "label_file" not in out:
            raise ValueError("DeviceDeform.write: the result was produced with pack=False")
        os.makedirs(os.path.join(out_dir, "velodyne"), exist_ok=True)
        os.makedirs(os.path.join(out_dir, "labels"), exist_ok=True)
        b = out["bin"].cpu().numpy()
        b.tofile(os.path.join(out_dir, "velodyne", str(idx).zfill(6) + ".bin"))
        out["label_file"].cpu().numpy().view("uint32").tofile(os.path.join(out_dir, "labels", str(idx).zfill(6) + ".label"))
        return int(b.shape[0])

    def close(self):
        for v in getattr(self, "_mm_vols", {}).values():
            v.close()
        self._mm_vols = {}
        if getattr(self, "_mm_state", None) is not None and getattr(self, "_mm_own", False):
            self._mm_state.close()
        self._mm_state = None
        if getattr(self, "head", None) is not None:
            self.head.close()       # (the sub-ray set and the ray set, when they are this chain's own)
        self.rayset = None
        for name in ("scene", "mesh_obj", "vol", "projector"):
            obj = getattr(self, name, None)
            if obj is not None:
                obj.close()
                setattr(self, name, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
