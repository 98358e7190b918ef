"""What the chain layer (``deform.py``, ``pipeline.py``, ``sequence.py``) hands the library's device entry points, in one
place: the merged cloud, the ``lt_cloud`` and beam tables, origin and output pointers, and -- :class:`Sensing` -- what
stands between a chain's render and its result: the target sensor's mounting, its echo, return and noise models and its
dual-return setting; the order of the models lives there and nowhere else.  :class:`TargetHead` is a target sensor on a
chain -- shape, model, ``Sensing``, ray set, origin -- and the steps of its scan: ``plan``, the chain's native call(s) with
``render_set`` and ``out_ptrs(sub)``, ``finish``; :func:`pack_result` packs any head's result for the files.
Private; imports without a GPU and without the library (torch and numpy on first use)."""
from __future__ import annotations

import ctypes as C

from . import _lib

TRACE_FLAGS = _lib.LT_TRACE_WRITE_MISSES | _lib.LT_TRACE_LABEL_IMAGE   # every cell written, ``endcolors`` = the label image
OUT_KEYS = ("endpoints", "endcolors", "range", "endrem", "tri")        # the render's outputs in the entry points' order
#: why ``cp`` cannot honour a model behind the render, by the chain layer's name of the model: (the sensor file's key, its
#: article, what ``cp`` does not render, what is missing).  Each site names its own order of precedence.
CP_REFUSALS = dict(returns=("return_model", "a", "surface", "no hit triangle, no incidence angle"),
                   noise=("noise_model", "a", "ray", "no origin to jitter a range about"),
                   echoes=("echo_model", "an", "ray", "no beam to widen"),
                   dual=("dual_return", "a", "ray", "no echo to choose a second from"))
#: what the return and noise models' seeds are xor-ed with (uint32) for a scan's SECOND return: a measurement of its own,
#: drawn for the same ``(scan, cell)``
SECOND_SEED_XOR = 0x9E3779B9


def merged_cloud(clouds):
    """``(points, rem, label)`` of the source scans as ONE cloud (laserscan.py:834-839, :939-949): the tensors themselves
    when there is one scan, else their concatenation in order"""
    if len(clouds) == 1:
        return clouds[0][0], clouds[0][1], clouds[0][2]
    import torch
    return tuple(torch.cat([c[k] for c in clouds]) for k in range(3))


def cloud_table(clouds):
    """``(lt_cloud array, tensors to keep alive, is_f64)`` of ``(points, rem, label)`` CUDA triples as the native scan calls
    read them: contiguous points of ONE dtype (float32 or float64, else ``TypeError``), ``rem`` float32, ``label`` int32.
    The array points into the kept tensors, which may be copies: keep them until the stream is done with them."""
    import torch
    cl = (_lib.Cloud * len(clouds))()
    keep = []
    dt = clouds[0][0].dtype
    for k, (pts, rem, lab) in enumerate(clouds):
        if pts.dtype != dt or dt not in (torch.float32, torch.float64):
            raise TypeError("clouds: float32 or float64 points, one dtype per output scan")
        pts = pts.contiguous()
        rem = rem.contiguous() if rem.dtype == torch.float32 else rem.to(torch.float32).contiguous()
        lab = lab.contiguous() if lab.dtype == torch.int32 else lab.to(torch.int32).contiguous()
        keep += [pts, rem, lab]
        cl[k].points, cl[k].rem, cl[k].label, cl[k].n = pts.data_ptr(), rem.data_ptr(), lab.data_ptr(), int(pts.shape[0])
    return cl, keep, int(dt == torch.float64)


def beam_table(beam_angles):
    """``(pointer or None, n, array to keep alive)`` of a sensor's beam angles (float64)"""
    if beam_angles is None or len(beam_angles) == 0:
        return None, 0, None
    import numpy as np
    beams = np.ascontiguousarray(beam_angles, dtype=np.float64)
    return beams.ctypes.data_as(C.c_void_p), len(beams), beams


def origin3(origin):
    return (C.c_float * 3)(*[float(x) for x in origin])


def out_ptrs(out):
    """the five output pointers ``endpoints, endcolors, range, endrem, tri``; ``None`` = not wanted"""
    return tuple(out[k].data_ptr() if out.get(k) is not None else None for k in OUT_KEYS)


def with_tri(rout, n_rays, device):
    """``rout`` itself when it holds a ``tri`` image already, else a copy with one (the models behind the render tell a return
    from a miss by it).  Allocates on the current stream."""
    if rout.get("tri") is not None:
        return rout
    import torch
    rout = dict(rout)
    rout["tri"] = torch.empty((n_rays,), dtype=torch.int32, device=device)
    return rout


def need_scan_index(scan_index, what, lead=None):
    """THE refusal of a missing ``scan_index``: ``ValueError`` when it is ``None``.  ``what``: the model(s) whose draws need it
    (``"return"``, ``"noise"``, ``"return or noise"``); ``lead``: the chain-layer caller the message is led by
    (:meth:`TargetHead.need_scan_index`), none for the models' own ``apply``"""
    if scan_index is None:
        raise ValueError(f"{lead}: a {what} model needs scan_index, the output scan's index in its sequence" if lead else
                         f"a {what} model needs the output scan's index in its sequence (scan_index=)")


class Returns:
    """The target sensor's return model on a chain (``config.ReturnModel`` or ``None``).  ``None``, or a model
    with every field at its default: nothing here allocates or launches.  Applied once per output scan, to the render that
    stands, behind it on the chain's stream and BEFORE the hits go into the target's frame, evaluation and packing."""

    KEYS = ("incidence", "drop")

    def __init__(self, model, who="return model"):
        from .config import ReturnModel
        if model is not None and not isinstance(model, ReturnModel):
            raise ValueError(f"{who}: returns= takes a lidar_transfer_amd.config.ReturnModel (SensorModel.return_model()) or None")
        self.model = None if model is None or model.is_default else model

    def __bool__(self):
        return self.model is not None

    def render_into(self, rout, n_rays, device):
        """What the render writes for this chain: ``rout`` itself without a model or when it holds ``tri`` already; else a
        copy with a ``tri`` image (the model reads the hit triangle).  Allocates on the current stream."""
        return rout if self.model is None else with_tri(rout, n_rays, device)

    def apply(self, rout, scan, scene, rays, stream, label_image=True, seed_xor=0):
        """the model on the rendered images ``rout`` of output scan ``scan`` (its index in its sequence), on ``stream``;
        returns ``dict(incidence=, drop=)``, or ``{}`` without a model.  ``seed_xor``: 0, or what the model's seed is xor-ed
        with for this call (a scan's second return)"""
        if self.model is None:
            return {}
        need_scan_index(scan, "return")
        from . import post
        more = dict(seed_xor=seed_xor) if seed_xor else {}   # (0: today's call, argument for argument)
        return post.return_model(scene, rays, self.model, scan, rout, label_image=label_image, stream=stream, **more)


class Noise:
    """The target sensor's noise model on a chain (``config.NoiseModel`` or ``None``), beside :class:`Returns`
    and shaped like it.  ``None``, or a model with every field at its default: nothing here allocates or launches.
    ``gate``: the chain's return model (``config.ReturnModel`` or ``None``), whose range gate a measured range must stay
    inside.  Applied once per output scan, to the render that stands, BEHIND the return model on the chain's stream and
    BEFORE the hits go into the target's frame, evaluation and packing: the kernel is read-modify-write, a second
    application would jitter the jittered scan."""

    KEYS = ("range_error", "noise_state")

    def __init__(self, model, gate=None, who="noise model"):
        from .config import NoiseModel
        if model is not None and not isinstance(model, NoiseModel):
            raise ValueError(f"{who}: noise= takes a lidar_transfer_amd.config.NoiseModel (SensorModel.noise_model()) or None")
        self.model = None if model is None or model.is_default else model
        self.gate = gate

    def __bool__(self):
        return self.model is not None

    def render_into(self, rout, n_rays, device):
        """as ``Returns.render_into``: the model reads ``tri`` to tell a return from a miss"""
        return rout if self.model is None else with_tri(rout, n_rays, device)

    def apply(self, rout, scan, origin, stream, label_image=True, seed_xor=0):
        """the model on the rendered images ``rout`` of output scan ``scan`` (its index in its sequence) whose rays start at
        ``origin``, on ``stream``; returns ``dict(range_error=, noise_state=)``, or ``{}`` without a model.  ``seed_xor``: as
        for :meth:`Returns.apply`"""
        if self.model is None:
            return {}
        need_scan_index(scan, "noise")
        from . import post
        more = dict(seed_xor=seed_xor) if seed_xor else {}
        return post.noise_model(origin, self.model, scan, rout, gate=self.gate, label_image=label_image, stream=stream, **more)


class Echoes:
    """The target sensor's echo model on a chain (``config.EchoModel`` or ``None``), beside :class:`Returns` and
    :class:`Noise`.  ``None``, or a model that is off (no divergence, one sub-ray): nothing here allocates or launches, and
    :meth:`render_set` / :meth:`render_into` hand back what they were given.  With a model the chain renders ``S`` sub-rays
    per cell -- :meth:`bind` makes them from the finished ray tensor and ONE read-only ``RaySet`` over them, shared by all
    chains of a pipeline as the plain ray set is -- into scratch images and :meth:`apply` resolves those into the chain's
    own images: behind the render that stands, AHEAD of the return model and the noise model, which see the resolved scan.
    ``model`` may be a bound :class:`Echoes`: its model and its ray set are shared, not owned."""

    KEYS = ("n_echoes", "echo_fraction")
    SUB_KEYS = ("endcolors", "range", "endrem", "tri")   # what a sub-render writes: no end points

    def __init__(self, model, who="echo model"):
        from .config import EchoModel
        self.rayset = self.subrays = None
        self._own = True
        if isinstance(model, Echoes):
            self.model, self.rayset, self.subrays, self._own = model.model, model.rayset, model.subrays, False
            return
        if model is not None and not isinstance(model, EchoModel):
            raise ValueError(f"{who}: echoes= takes a lidar_transfer_amd.config.EchoModel (SensorModel.echo_model()) or None")
        self.model = None if model is None or model.is_default else model

    def __bool__(self):
        return self.model is not None

    @staticmethod
    def grid_of(central, t_H, table=False):
        """The bin grid of the sub-ray set for a central set's ``grid`` (``None``: the image's rule): the central set's azimuth
        rule, and the central set's own ``t_H`` elevation rows -- not the ``S * t_H`` rows the image's rule would make of the
        taller set --, so that the ``S`` sub-rays of a cell share the bin their central ray sits in; with ``table`` (a target
        whose rows are not evenly spaced: a beam table) the image's rule, whose finer rows separate the beams that crowd near
        the horizon.  A speed choice only: every grid renders the same image.  Measured (profiles/echo_model/README.md): at
        64 x 2048 evenly spaced the central rows render in 0.34 of the time of the image's rule, with the VLP-32C table at
        32 x 1024 the image's rule in 0.64 of the time of the central rows; doubling the azimuth bins is slower in both."""
        az, el = (0, 0) if central is None else central
        return int(az), int(el) if el else (0 if table else int(t_H))

    def bind(self, rays, t_H, pose=None, grid=None, table=False, sub_grid=None):
        """the sub-rays of ``rays`` [n, 3] (the finished central rays of a target of ``t_H`` rows) and the ray set over them:
        ``S * t_H`` rows of the image's width, plane by plane, binned by ``sub_grid`` or, without one, by :meth:`grid_of` of the
        central set's ``grid`` and ``table``.  Once per pipeline; waits for the current stream.  Without a model, or when
        already bound (a shared one), nothing happens."""
        if self.model is None or self.rayset is not None:
            return self
        from . import post
        from .raytracer import RaySet
        n = (rays.shape[0] // int(t_H)) * int(t_H)   # (what the plain ray set keeps of them)
        self.subrays = post.create_subrays(rays if n == rays.shape[0] else rays[:n].contiguous(), self.model)
        self.rayset = RaySet(self.subrays, self.model.subrays * int(t_H), pose=pose,
                             grid=sub_grid if sub_grid is not None else self.grid_of(grid, t_H, table))
        return self

    def render_set(self, rayset):
        """the ray set the chain renders with: the sub-ray set, or ``rayset`` (the plain one) without a model"""
        if self.model is None:
            return rayset
        if self.rayset is None:
            raise RuntimeError("an echo model needs its sub-ray set: Echoes.bind(rays, t_H) first")
        return self.rayset

    def resolve_into(self, rout, n_rays, device):
        """What the resolve writes for this chain: ``rout`` itself without a model or when it holds ``tri`` already; else a
        copy with a ``tri`` image (the resolve always writes the representative's triangle)."""
        return rout if self.model is None else with_tri(rout, n_rays, device)

    def render_into(self, rout, n_rays, device):
        """What the render writes for this chain: ``rout`` itself without a model; else scratch images of the ``S * n_rays``
        sub-rays -- the label image, range, remission and triangle, no end points.  Allocates on the current stream."""
        if self.model is None:
            return rout
        import torch
        m = self.model.subrays * int(n_rays)
        sub = dict(endpoints=None, endcolors=torch.empty((m,), dtype=torch.int32, device=device),
                   range=torch.empty((m,), dtype=torch.float32, device=device),
                   endrem=torch.empty((m,), dtype=torch.float32, device=device),
                   tri=torch.empty((m,), dtype=torch.int32, device=device))
        return sub

    def apply(self, sub, rout, rays, origin, stream):
        """the sub-render ``sub`` resolved into the chain's images ``rout`` (which hold a ``tri`` image: :func:`with_tri`) on
        ``stream``; ``rays``: the CENTRAL rays, ``origin``: where they start.  Returns ``dict(n_echoes=, echo_fraction=)``, or
        ``{}`` without a model."""
        if self.model is None:
            return {}
        from . import post
        return post.echo_resolve(rays, origin, self.model, sub, rout, stream=stream)

    def close(self):
        if self._own and self.rayset is not None:
            self.rayset.close()
        self.rayset = self.subrays = None


class Dual:
    """The target sensor's dual-return setting on a chain (``config.DualReturn`` or ``None``), beside
    :class:`Echoes`, whose resolve it widens: ``None`` or ``second: none`` is off, and then nothing anywhere changes.  On, a
    scan's images are PLANE 0 of allocations of ``2 n`` cells whose plane 1 holds the second return (:meth:`planes`), so that
    one frame change and one packing serve both."""

    KEYS = ("second",)

    def __init__(self, setting, who="dual return"):
        from .config import DualReturn
        if setting is not None and not isinstance(setting, DualReturn):
            raise ValueError(f"{who}: dual= takes a lidar_transfer_amd.config.DualReturn (SensorModel.dual_return()) or None")
        self.setting = None if setting is None or setting.is_default else setting

    def __bool__(self):
        return self.setting is not None

    @staticmethod
    def planes(n_rays, device):
        """the render's five images for ``2 * n_rays`` cells, plane by plane.  Allocates on the current stream."""
        import torch
        m = 2 * int(n_rays)
        return dict(endpoints=torch.empty((m, 3), dtype=torch.float32, device=device),
                    endcolors=torch.empty((m,), dtype=torch.int32, device=device),
                    range=torch.empty((m,), dtype=torch.float32, device=device),
                    endrem=torch.empty((m,), dtype=torch.float32, device=device),
                    tri=torch.empty((m,), dtype=torch.int32, device=device))


class Mount:
    """The target sensor's mounting from the approach file's ``transformation`` (``config.mount_of``).  ``pair``: ``(T, P)``,
    or ``None`` for no mounting (``None``, empty, the identity) -- then nothing here allocates or launches.  ``T``
    (``x_target = T . x_source``, float64, contiguous) takes the hits into the target's frame; ``P = inv(T)`` is the pose the
    target's ray set is built with; ``origin``: where its rays start in the scene, ``float32(P[:3, 3])``."""

    def __init__(self, transformation):
        from .config import mount_of
        self.pair = mount_of(transformation)
        self.T = self.P = None
        self.origin = (0.0, 0.0, 0.0)
        if self.pair is not None:
            import numpy as np
            self.T = np.ascontiguousarray(self.pair[0], dtype=np.float64)
            self.P = self.pair[1]
            self.origin = tuple(float(np.float32(x)) for x in self.P[:3, 3])

    def render_into(self, out, n_rays, device):
        """What the render writes: ``out`` itself without a mounting or without ``endpoints``; else the scene-frame end
        points go to a buffer of their own (the caller's ``endpoints`` receive the target frame) and the hit triangle is
        always wanted (misses stay (0, 0, 0)).  Allocates on the current stream."""
        if self.pair is None or out.get("endpoints") is None:
            return out
        import torch
        rout = dict(out)
        rout["endpoints"] = torch.empty_like(out["endpoints"])
        if rout.get("tri") is None:
            rout["tri"] = torch.empty((n_rays,), dtype=torch.int32, device=device)
        return rout

    def to_target(self, rout, out, stream):
        """the hits of ``rout["endpoints"]`` (as rendered) into the target's frame in ``out["endpoints"]``, on ``stream``;
        nothing when the render wrote the caller's end points themselves (no mounting, or no end points wanted)"""
        if rout.get("endpoints") is out.get("endpoints"):
            return
        from . import post
        post.points_to_frame(rout["endpoints"], self.T, tri=rout["tri"], out=out["endpoints"], stream=stream)


class Sensing:
    """What stands between a chain's render and its result, one object per chain: the target sensor's :class:`Mount`,
    :class:`Echoes`, :class:`Returns`, :class:`Noise` and :class:`Dual` (``mounting``, ``echoes``, ``returns``, ``noise``,
    ``dual``; each may be off), made from the chain's ``transformation=``, ``returns=``, ``noise=``, ``echoes=`` and ``dual=``
    with the constructors' messages, led by ``who``.  THE ORDER LIVES HERE: :meth:`finish` resolves the echoes, then runs
    the return model, then the noise model (gated by the return model's range gate), then takes the hits into the target's
    frame -- each once, on the render that stands.  With a dual return the resolve writes two returns, each model runs on the
    primary and then on the second (seeds xor-ed with :data:`SECOND_SEED_XOR`), and ONE frame change covers both planes.  A
    site that did this in another order would still run and write other bytes; no site does it itself.  ``mount``,
    ``origin``, ``P``: the mounting's pair, ray origin and pose.  With nothing on, nothing here allocates or launches."""

    def __init__(self, transformation, returns, noise, echoes, who, dual=None):
        self.mounting = Mount(transformation)
        self.returns = Returns(returns, who)
        self.noise = Noise(noise, self.returns.model, who)
        self.echoes = Echoes(echoes, who)
        self.dual = Dual(dual, who)
        if self.dual and not self.echoes:
            raise ValueError(f"{who}: dual= needs echoes=, an echo model with a divergence and at least two sub-rays (a second "
                             "return is another echo of the same beam)")
        self.mount, self.origin, self.P = self.mounting.pair, self.mounting.origin, self.mounting.P
        self._t_H = None

    @property
    def keys(self):
        """the result keys of the models that are on"""
        return tuple(k for m in (self.returns, self.noise, self.echoes, self.dual) if m for k in m.KEYS)

    @property
    def needs_scan_index(self):
        """a return or a noise model is on: their draws are a function of the output scan's index in its sequence"""
        return bool(self.returns or self.noise)

    def bind(self, rays, t_H, grid=None, table=False, sub_grid=None):
        """:meth:`Echoes.bind` with the mounting's pose"""
        self._t_H = int(t_H)
        self.echoes.bind(rays, t_H, pose=self.P, grid=grid, table=table, sub_grid=sub_grid)
        return self

    def render_set(self, rayset):
        """the ray set the chain renders with: :meth:`Echoes.render_set`"""
        return self.echoes.render_set(rayset)

    def plan(self, out, n_rays, device):
        """``(rout, sub)`` for a scan whose result goes to ``out``: ``sub`` is what the native call renders into
        (``out_ptrs(sub)``), ``rout`` the scan's images as rendered, which :meth:`finish` works on; both are ``out`` itself
        with nothing on.  With a dual return the five images of ``out`` are REPLACED, in place, by the plane-0 views of fresh
        allocations of ``2 * n_rays`` cells, and ``rout`` carries the planes to :meth:`finish`.  Allocates on the current
        stream."""
        if self.dual:
            return self._plan_dual(out, n_rays, device)
        rout = self.returns.render_into(self.mounting.render_into(out, n_rays, device), n_rays, device)
        rout = self.echoes.resolve_into(self.noise.render_into(rout, n_rays, device), n_rays, device)
        return rout, self.echoes.render_into(rout, n_rays, device)

    def _plan_dual(self, out, n_rays, device):
        import torch
        n = int(n_rays)
        store = Dual.planes(n, device)                      # what the result holds: end points in the target's frame
        rstore = store if self.mount is None else dict(store, endpoints=torch.empty_like(store["endpoints"]))   # as rendered
        for k in OUT_KEYS:
            out[k] = store[k][:n]
        rout = dict(out)
        if rstore is not store:
            rout["endpoints"] = rstore["endpoints"][:n]
        rout["_dual"] = (rstore, store)
        return rout, self.echoes.render_into(rout, n, device)

    def finish(self, out, rout, sub, scan_index, scene, rays, origin, stream, label_image=True):
        """Behind the render that stands, on ``stream``: ``sub`` resolved into ``rout``, the return model, the noise model,
        the hits into the target's frame in ``out`` (``post.echo_resolve``, ``post.return_model``, ``post.noise_model``,
        ``post.points_to_frame``, each only when it is on).  ``rays``: the CENTRAL rays, ``origin``: where they start,
        ``scene``: what rendered.  Returns what the models add to the result (:attr:`keys`)."""
        if self.dual:
            return self._finish_dual(rout, sub, scan_index, scene, rays, origin, stream, label_image)
        seen = self.echoes.apply(sub, rout, rays, origin, stream)
        seen.update(self.returns.apply(rout, scan_index, scene, rays, stream, label_image))
        seen.update(self.noise.apply(rout, scan_index, origin, stream, label_image))
        self.mounting.to_target(rout, out, stream)
        return seen

    def _finish_dual(self, rout, sub, scan_index, scene, rays, origin, stream, label_image):
        """:meth:`finish` with a dual return: ONE resolve into both planes, each model on plane 0 exactly as without the
        setting and then on plane 1 with the xor-ed seed, ONE frame change over both planes.  The result's ``second``: the
        second return's images, and under ``_planes`` the whole allocations that the packing reads."""
        from . import post
        rstore, store = rout["_dual"]
        n = rout["tri"].numel()
        second = {k: rstore[k][n:] for k in OUT_KEYS}       # plane 1, as rendered
        seen = post.echo_resolve_dual(rays, origin, self.echoes.model, self.dual.setting, sub, rout, second, stream=stream)
        more = dict(echo_fraction=seen.pop("echo_fraction2"))
        seen.update(self.returns.apply(rout, scan_index, scene, rays, stream, label_image))
        more.update(self.returns.apply(second, scan_index, scene, rays, stream, label_image, seed_xor=SECOND_SEED_XOR))
        seen.update(self.noise.apply(rout, scan_index, origin, stream, label_image))
        more.update(self.noise.apply(second, scan_index, origin, stream, label_image, seed_xor=SECOND_SEED_XOR))
        if rstore is not store:
            post.points_to_frame(rstore["endpoints"], self.mounting.T, tri=rstore["tri"], out=store["endpoints"], stream=stream)
        H = self._t_H or 1
        image = (H, n // H)
        seen["second"] = dict(range=store["range"][n:].view(image), rem=store["endrem"][n:].view(image),
                              label=store["endcolors"][n:].view(image), endpoints=store["endpoints"][n:],
                              endpoints_scene=second["endpoints"], tri=second["tri"],
                              _planes=dict(endpoints=store["endpoints"], rem=store["endrem"], label=store["endcolors"]), **more)
        return seen

    def close(self):
        """closes the sub-ray set when this object owns it (a bound :class:`Echoes` handed in is shared)"""
        self.echoes.close()


class TargetHead:
    """A target sensor on a chain, ONE object for the target of a ``DeviceDeform`` and for a further head of a rig
    (``rig.Head``): its shape (``t_H``, ``t_W``, ``t_fov_up``, ``t_fov_down``, ``n_rays``), its validated ``t_model``
    (``config.TargetModel`` of ``beam_table``, ``sector``, ``beam_azimuth``), its :class:`Sensing` (``sensing``, of
    ``transformation`` and the four models), its posed rays in a read-only ``RaySet`` (``rayset``) and where they start in the
    scene (``origin``); ``who`` leads every message.  ``rayset``: a shared ray set of the same sensor at the same pose --
    checked, taken and not closed here; ``echoes`` may likewise be a bound :class:`Echoes`.  ``cast=False``: a chain that
    renders no ray (``cp`` without a scene) -- no ray set is made and nothing is bound.
    A scan is :meth:`need_scan_index`, :meth:`plan`, the chain's native render(s) with ``render_set`` and
    ``out_ptrs(plan[2])``, then :meth:`finish`."""

    def __init__(self, shape, transformation, returns, noise, echoes, dual, who, device, beam_table=None, sector=None,
                 beam_azimuth=None, rayset=None, cast=True):
        import torch

        from .config import TargetModel
        self.who = who
        self.t_H, self.t_W, self.t_fov_up, self.t_fov_down = int(shape[0]), int(shape[1]), float(shape[2]), float(shape[3])
        self.n_rays = self.t_H * self.t_W
        self.device = torch.device("cuda", int(device))
        # what stands between the render and the result (and the only place that knows its order)
        s = self.sensing = Sensing(transformation, returns, noise, echoes, who, dual)
        m = self.t_model = TargetModel(beam_table, sector, beam_azimuth, who).validate(self.t_H, (self.t_fov_up, self.t_fov_down), who)
        self.origin = s.origin       # the target sensor in the scene, where its rays are cast from by default
        self.rayset, self._own = None, rayset is None
        if not cast:
            return
        pose = s.P
        if rayset is None:
            from .laserscan import create_rays_device
            from .raytracer import RaySet
            keys = dict(beam_table=m.beam_table, sector=m.sector, beam_azimuth=m.beam_azimuth)
            rays = create_rays_device(self.t_fov_up, self.t_fov_down, self.t_H, self.t_W, device=int(device),
                                      rot=pose[:3, :3] if pose is not None else None, **keys)
            rayset = RaySet(rays, self.t_H, pose=pose, grid=m.grid(self.t_W), **keys)
        else:
            import numpy as np
            theirs = getattr(rayset, "pose", None)
            if (theirs is None) != (pose is None) or (pose is not None and not np.array_equal(theirs, pose)):
                raise ValueError(f"{who}: the shared rayset was built for another sensor pose than `transformation`")
            differs = m.difference(rayset.model)
            if differs is not None:
                what = dict(beam_table="another beam table", sector="another sector",
                            beam_azimuth="other beam azimuth offsets")[differs]
                raise ValueError(f"{who}: the shared rayset was built for {what} than `t_{differs}`")
        self.rayset = rayset
        # (the central rays stay in ``rayset.rays``: the return model reads its directions from them)
        s.bind(rayset.rays, self.t_H, grid=rayset.grid, table=m.beam_table is not None)

    @property
    def render_set(self):
        """the ray set the chain renders this head with (``Sensing.render_set``: the sub-ray set of an echo model)"""
        return self.sensing.render_set(self.rayset)

    def need_scan_index(self, scan_index, where=None):
        """``ValueError`` when a return or a noise model is on and ``scan_index`` is missing; ``where``: the method that
        leads the message and is told which model (``DeviceDeform.mesh``), default: ``who``, told both"""
        if self.sensing.needs_scan_index:
            need_scan_index(scan_index, "return or noise" if where is None else "return" if self.sensing.returns else "noise",
                            where or self.who)

    def plan(self, scene, out=None):
        """``(out, rout, sub)`` of a scan on ``scene``: its outputs (``Scene.alloc_outputs`` unless the caller brings ``out``)
        and their :meth:`Sensing.plan`.  Allocates on the current stream."""
        if out is None:
            out = scene.alloc_outputs(self.n_rays, label_image=True)
        return (out,) + self.sensing.plan(out, self.n_rays, self.device)

    def finish(self, plan, scan_index, scene, mesh, stream, origin=None, **more):
        """:meth:`Sensing.finish` behind the render of ``plan`` with this head's rays, cast from ``origin`` (default: its
        own), and what ``mesh`` / ``mergemesh`` return of the scan: the images, ``endpoints`` in the target's frame,
        ``endpoints_scene`` and ``tri`` as rendered, the sizes of ``mesh`` (the ``DeviceMesh`` that was rendered), ``more``
        and what the models add"""
        out, rout, sub = plan
        seen = self.sensing.finish(out, rout, sub, scan_index, scene, self.rayset.rays, self.origin if origin is None else origin,
                                   stream)
        H, W = self.t_H, self.t_W
        return dict(range=out["range"].view(H, W), rem=out["endrem"].view(H, W), label=out["endcolors"].view(H, W),
                    endpoints=out["endpoints"], endpoints_scene=rout["endpoints"], tri=rout["tri"],
                    n_verts=mesh.n_verts, n_faces=mesh.n_faces, **more, **seen)

    def pack(self, res, stream, scene_frame=False, rows=None):
        """:func:`pack_result` of this head's result ``res``"""
        return pack_result(res, self.n_rays, self.device, stream, scene_frame, rows)

    def close(self):
        """closes the sub-ray set and the ray set when this head owns them"""
        self.sensing.close()
        if self._own and self.rayset is not None:
            self.rayset.close()
        self.rayset = None


def pack_rows(points, is_f64, rem, label, index, n, stream, device):
    """``lt_pack_scan_dev`` (the one place it is called from on a chain; ``DeviceDeform._pack`` is this on the chain's
    device): ``n`` cells of ``points`` [n, 3] (float64 with
    ``is_f64``), ``rem``, ``label`` and ``index`` (or ``None``: no index filter) -> ``(bin [N, 4] f32, label_file [N] i32)``.
    Allocates on the current stream; reads the number of kept points back."""
    import torch
    out_bin = torch.empty((n, 4), dtype=torch.float32, device=device)
    out_lab = torch.empty((n,), dtype=torch.int32, device=device)
    kept = C.c_int(0)
    _lib.check(_lib.load().lt_pack_scan_dev(points.data_ptr(), int(is_f64), rem.data_ptr(), label.data_ptr(),
                                            index.data_ptr() if index is not None else None, n, out_bin.data_ptr(),
                                            out_lab.data_ptr(), C.byref(kept), C.c_void_p(stream.cuda_stream)), "lt_pack_scan_dev")
    return out_bin[:kept.value], out_lab[:kept.value]


def pack_result(res, n_rays, device, stream, scene_frame=False, rows=None):
    """``write``'s filter + packing (laserscan.py:1133-1178) of a scan's result ``res`` of ``n_rays`` cells, on ``stream`` ->
    ``(bin [N, 4] f32, label_file [N] i32)``, for any head.  ``cp`` packs its float64 ``back_points`` where ``index > 0``
    (:1133-1144); the mesh adaptions their float32 ``endpoints``, no index filter (:1145-1148) -- with ``scene_frame`` their
    ``endpoints_scene``, the primary scan's frame.  A dual-return result packs both of its planes in the ONE call: the
    primary's rows in cell order, then the second returns'.  ``rows``: what packs the rows, called as :func:`pack_rows`
    without the device (a ``DeviceDeform`` hands in its ``_pack``); default: :func:`pack_rows` on ``device``."""
    import torch
    n = int(n_rays)
    if rows is None:
        rows = lambda *a: pack_rows(*a, device)   # noqa: E731
    with torch.cuda.device(device), torch.cuda.stream(stream):
        if res.get("second") is not None:
            planes = res["second"]["_planes"]
            points = planes["endpoints"]
            if scene_frame:
                points = torch.cat([res["endpoints_scene"], res["second"]["endpoints_scene"]])
            return rows(points, False, planes["rem"], planes["label"], None, 2 * n, stream)
        rem, label = res["rem"].reshape(-1), res["label"].reshape(-1)
        if "back_points" in res:
            return rows(res["back_points"], True, rem, label, res["index"].reshape(-1), n, stream)
        points = res["endpoints_scene" if scene_frame else "endpoints"].contiguous()
        return rows(points, False, rem, label, None, n, stream)
