"""A rig of target sensors around ONE chain: several heads on one vehicle look at the one scene that ingest,
projection, TSDF integration and marching cubes make of an output scan's source scans.

:class:`RigDeform` owns one :class:`~lidar_transfer_amd.deform.DeviceDeform` for head 0 -- projector, volume, mesh, scene,
head 0's ray set and ``Sensing``, unchanged -- and one light :class:`Head` per further sensor: its rays, its ``RaySet`` and
its own ``_chain.Sensing``.  ``mesh`` / ``mergemesh`` run head 0's call as it is, then ONE ``Scene.render_rig`` call on the
same stream renders every further head from the mesh the scene now holds, then each head's ``Sensing.finish`` and packing
follow.  A further head's scan is what a ``DeviceDeform`` of that sensor alone returns for ``mesh``; for ``mergemesh`` it is
its render of the volume that head 0's vertical field of view selected (see :class:`RigDeform`)."""
from __future__ import annotations

from . import _chain
from .deform import DeviceDeform
from .raytracer import RaySet


def head_keywords(sensor):
    """the ``DeviceDeform`` keywords that a ``config.SensorModel`` stands for as a TARGET: its shape tuple and its models"""
    m = sensor.target_model()
    return (sensor.H, sensor.W, float(sensor.fov_up), float(sensor.fov_down)), dict(
        t_beam_table=m.beam_table, t_sector=m.sector, t_beam_azimuth=m.beam_azimuth, returns=sensor.return_model(),
        noise=sensor.noise_model(), echoes=sensor.echo_model(), dual=sensor.dual_return())


class Head:
    """A further sensor of a rig: its rays (turned by its pose), its read-only ``RaySet`` and its own ``Sensing``, bound as
    ``DeviceDeform.__init__`` binds it.  ``share``: the same head of another :class:`RigDeform` of the same rig -- its ray set
    and bound echo sub-ray set are taken, not made again."""

    def __init__(self, head, device, share=None):
        from .laserscan import create_rays_device
        self.name, self.sensor = head.name, head.sensor
        (self.t_H, self.t_W, self.t_fov_up, self.t_fov_down), kw = head_keywords(head.sensor)
        self.n_rays = self.t_H * self.t_W
        who = f"rig head {head.name!r}"
        m = self.t_model = head.sensor.target_model().validate(self.t_H, (self.t_fov_up, self.t_fov_down), who)
        s = self.sensing = _chain.Sensing(head.mount, kw["returns"], kw["noise"],
                                          share.sensing.echoes if share is not None and share.sensing.echoes else kw["echoes"],
                                          who, kw["dual"])
        self.origin = s.origin
        self._own = share is None
        if share is None:
            keys = dict(beam_table=m.beam_table, sector=m.sector, beam_azimuth=m.beam_azimuth)
            rays = create_rays_device(self.t_fov_up, self.t_fov_down, self.t_H, self.t_W, device=device,
                                      rot=s.P[:3, :3] if s.P is not None else None, **keys)
            self.rayset = RaySet(rays, self.t_H, pose=s.P, grid=m.grid(self.t_W), **keys)
        else:
            self.rayset = share.rayset
        s.bind(self.rayset.rays, self.t_H, grid=self.rayset.grid, table=m.beam_table is not None)

    def close(self):
        self.sensing.close()
        if self._own and self.rayset is not None:
            self.rayset.close()
        self.rayset = None


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
                if h.sensing.needs_scan_index and scan_index is None:
                    raise ValueError(f"rig head {h.name!r}: a return or noise model needs scan_index, the output scan's index in its "
                                     "sequence")
            with torch.cuda.device(self.device), torch.cuda.stream(st):
                plans = []
                for h in self.heads:
                    out = p.scene.alloc_outputs(h.n_rays, label_image=True)
                    rout, sub = h.sensing.plan(out, h.n_rays, self.device)
                    plans.append((out, rout, sub))
                p.scene.render_rig([h.sensing.render_set(h.rayset) for h in self.heads], [h.origin for h in self.heads],
                                   outs=[sub for _, _, sub in plans], stream=st, write_misses=True, label_image=True)
                for h, (out, rout, sub) in zip(self.heads, plans):
                    seen = h.sensing.finish(out, rout, sub, scan_index, p.scene, h.rayset.rays, h.origin, st)
                    res = p.scan_result(out, rout, h.t_H, h.t_W, **seen)
                    if pack:
                        res["bin"], res["label_file"] = self.pack_head(res, len(results), st)
                    results.append(res)
        if pack and self.merged:
            results.bin, results.label_file = self.merged_rows(results, st)
        return results

    def n_rays_of(self, k):
        return self.primary.n_rays if k == 0 else self.heads[k - 1].n_rays

    def pack_head(self, res, k, st=None, scene_frame=False):
        """``write``'s packing of head ``k``'s result ``res`` (``DeviceDeform.pack_result`` for any head of the rig) ->
        ``(bin, label_file)``; ``scene_frame``: the rows hold ``endpoints_scene``, the primary scan's frame"""
        import torch
        p = self.primary
        st = st if st is not None else p.last_stream
        n = self.n_rays_of(k)
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            if res.get("second") is not None:   # a dual return: both planes in the one call
                planes = res["second"]["_planes"]
                pts = planes["endpoints"]
                if scene_frame:
                    pts = torch.cat([res["endpoints_scene"], res["second"]["endpoints_scene"]])
                return p.pack_rows(pts, planes["rem"], planes["label"], 2 * n, st)
            pts = res["endpoints_scene" if scene_frame else "endpoints"]
            return p.pack_rows(pts.contiguous(), res["rem"].reshape(-1), res["label"].reshape(-1), n, st)

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
