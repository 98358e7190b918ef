"""A rig of target sensors around ONE chain: several heads on one vehicle look at the one scene that ingest,
projection, TSDF integration and marching cubes make of an output scan's source scans.

:class:`RigDeform` owns one :class:`~lidar_transfer_amd.deform.DeviceDeform` for head 0 -- projector, volume, mesh, scene,
head 0's ``_chain.TargetHead``, unchanged -- and one :class:`Head`, the same object, per further sensor: its rays, its
``RaySet`` and its own ``_chain.Sensing``.  ``mesh`` / ``mergemesh`` run head 0's call as it is, then ONE ``Scene.render_rig``
call on the same stream renders every further head from the mesh the scene now holds, then each head's ``finish`` and packing
follow.  A further head's scan is what a ``DeviceDeform`` of that sensor alone returns for ``mesh``; for ``mergemesh`` it is
its render of the volume that head 0's vertical field of view selected (see :class:`RigDeform`)."""
from __future__ import annotations

from . import _chain
from .deform import DeviceDeform


def head_keywords(sensor):
    """the ``DeviceDeform`` keywords that a ``config.SensorModel`` stands for as a TARGET: its shape tuple and its models; a
    plain ``(H, W, fov_up, fov_down)`` is its own shape and has no model"""
    if not hasattr(sensor, "fov_up"):
        return (int(sensor[0]), int(sensor[1]), float(sensor[2]), float(sensor[3])), dict(
            t_beam_table=None, t_sector=None, t_beam_azimuth=None, returns=None, noise=None, echoes=None, dual=None)
    m = sensor.target_model()
    return (sensor.H, sensor.W, float(sensor.fov_up), float(sensor.fov_down)), dict(
        t_beam_table=m.beam_table, t_sector=m.sector, t_beam_azimuth=m.beam_azimuth, returns=sensor.return_model(),
        noise=sensor.noise_model(), echoes=sensor.echo_model(), dual=sensor.dual_return())


class Head(_chain.TargetHead):
    """A further sensor of a rig: the ``_chain.TargetHead`` of a ``config.RigHead`` (``name``, ``sensor``).  ``share``: the
    same head of another :class:`RigDeform` of the same rig -- its ray set and bound echo sub-ray set are taken, not made
    again."""

    def __init__(self, head, device, share=None):
        self.name, self.sensor = head.name, head.sensor
        shape, kw = head_keywords(head.sensor)
        if share is not None and share.sensing.echoes:
            kw["echoes"] = share.sensing.echoes
        super().__init__(shape, head.mount, kw["returns"], kw["noise"], kw["echoes"], kw["dual"], f"rig head {head.name!r}", device,
                         kw["t_beam_table"], kw["t_sector"], kw["t_beam_azimuth"], rayset=None if share is None else share.rayset)


class RigResults(list):
    """the results of a rig's heads in rig order; ``bin`` / ``label_file``: the merged scan of the whole rig, or ``None``"""
    bin = label_file = None


class RigDeform:
    """``heads``: ``Approach.rig()`` -- 1 to 8 ``config.RigHead``; the other arguments are ``DeviceDeform``'s (``source``,
    ``vol_bnds``, ``voxel_size``, ``beam_angles``, ``preserve_float``, ``device``, ``merge``, ``fusion``, ``mesh_volume``,
    ``mm_state``).  ``share``: another ``RigDeform`` of the same rig (a second chain of a sequence): every ray set and bound
    echo sub-ray set is taken from it -- they are read-only.  ``merged``: ``Approach.rig_merged``.

    ``mesh`` and ``mergemesh`` return a LIST of results in rig order, each shaped like a ``DeviceDeform`` result.  With
    ``merged`` (and ``pack``) the list (a :class:`RigResults`) also carries ``bin`` / ``label_file`` of the whole rig: every
    head's packed rows, taken from ``endpoints_scene`` -- the primary scan's frame --, concatenated in rig order.

    The ``mergemesh`` limit: the volume holds what the source origin sees inside HEAD 0's vertical field of view.  A later
    head that looks higher or lower than head 0 would render a scene that was never fused there, so such a rig is refused
    for ``mergemesh``: order the rig widest first.  The test compares ``fov_up`` / ``fov_down`` of the sensor files and does
    NOT account for a head's pitch or height: a mounted head may still look at space the volume does not hold, and sees
    nothing there.  ``cp`` renders no ray and refuses a rig."""

    def __init__(self, source, heads, vol_bnds=None, voxel_size=0.1, share=None, merged=False, **kw):
        import torch
        heads = list(heads)
        if not 1 <= len(heads) <= 8:
            raise ValueError(f"RigDeform: a rig has 1 to 8 heads, not {len(heads)}")
        if share is not None and [h.name for h in share.rig] != [h.name for h in heads]:
            raise ValueError("RigDeform: share= is a RigDeform of another rig")
        self.rig, self.merged = heads, bool(merged)
        self.heads = []
        target, hkw = head_keywords(heads[0].sensor)
        if share is not None:
            kw = dict(kw, rayset=share.primary.rayset)
            if share.primary.bound_echoes:
                hkw["echoes"] = share.primary.bound_echoes
        self.primary = DeviceDeform(source, target, vol_bnds, voxel_size, transformation=heads[0].mount, **hkw, **kw)
        self.device = self.primary.device
        try:
            with torch.cuda.device(self.device):
                for k, h in enumerate(heads[1:]):
                    self.heads.append(Head(h, self.device.index, None if share is None else share.heads[k]))
        except BaseException:
            self.close()
            raise
        self.names = [h.name for h in heads]

    def check_mergemesh(self):
        """the ``mergemesh`` limit (the class's docstring): ``ValueError`` naming the first head that looks past head 0.  The
        fields of view are compared as the sensor files give them: a head's MOUNTING is not accounted for, so a head that is
        pitched against head 0 passes although part of what it looks at was never fused."""
        p = self.primary
        for h in self.heads:
            if h.t_fov_up > p.t_fov_up or h.t_fov_down < p.t_fov_down:
                raise ValueError(f"rig: mergemesh fuses what the source origin sees inside the FIRST head's vertical field of view "
                                 f"([{p.t_fov_down}, {p.t_fov_up}] degrees, head {self.names[0]!r}); head {h.name!r} looks past it "
                                 f"([{h.t_fov_down}, {h.t_fov_up}]) -- order the rig widest first")

    def cp(self, *a, **kw):
        raise ValueError("rig: adaption cp renders no ray -- a rig needs mesh or mergemesh")

    def _further(self, first, scan_index, pack, st):
        """steps 2 and 3: every further head rendered from the scene as head 0's call left it, in ONE call, then finished"""
        import torch
        p = self.primary
        results = RigResults([first])
        if self.heads:
            for h in self.heads:
                h.need_scan_index(scan_index)
            with torch.cuda.device(self.device), torch.cuda.stream(st):
                plans = [h.plan(p.scene) for h in self.heads]
                p.scene.render_rig([h.render_set for h in self.heads], [h.origin for h in self.heads],
                                   outs=[sub for _, _, sub in plans], stream=st, write_misses=True, label_image=True)
                for h, plan in zip(self.heads, plans):
                    res = h.finish(plan, scan_index, p.scene, p.mesh_obj, st)
                    if pack:
                        res["bin"], res["label_file"] = h.pack(res, st)
                    results.append(res)
        if pack and self.merged:
            results.bin, results.label_file = self.merged_rows(results, st)
        return results

    def pack_head(self, res, k, st=None, scene_frame=False):
        """``write``'s packing of head ``k``'s result ``res`` (``DeviceDeform.pack_result`` for any head of the rig) ->
        ``(bin, label_file)``; ``scene_frame``: the rows hold ``endpoints_scene``, the primary scan's frame"""
        st = st if st is not None else self.primary.last_stream
        return self.primary.pack_result(res, st, scene_frame) if k == 0 else self.heads[k - 1].pack(res, st, scene_frame)

    def merged_rows(self, results, st=None):
        """``(bin, label_file)`` of the whole rig: every head's packed rows from ``endpoints_scene`` -- one frame for all,
        the primary scan's -- concatenated in rig order"""
        import torch
        st = st if st is not None else self.primary.last_stream
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            parts = [self.pack_head(r, k, st, scene_frame=True) for k, r in enumerate(results)]
            return torch.cat([b for b, _ in parts]), torch.cat([lab for _, lab in parts])

    def mergemesh_bounds(self, clouds, seq=None):
        """``DeviceDeform.mergemesh_bounds`` of head 0's chain: the bounds statements of a scan that is not rendered"""
        return self.primary.mergemesh_bounds(clouds, seq=seq)

    def mesh(self, clouds, scan_index=None, pack=True):
        first = self.primary.mesh(clouds, pack=pack, scan_index=scan_index)
        return self._further(first, scan_index, pack, self.primary.last_stream)

    def mergemesh(self, clouds, seq=None, scan_index=None, pack=True):
        self.check_mergemesh()
        first = self.primary.mergemesh(clouds, pack=pack, seq=seq, scan_index=scan_index)   # (after settle / rerun)
        return self._further(first, scan_index, pack, self.primary.last_stream)

    def close(self):
        for h in self.heads:
            h.close()
        self.heads = []
        if getattr(self, "primary", None) is not None:
            self.primary.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
