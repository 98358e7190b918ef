"""Sensor-model and approach YAML files, consumed unchanged.

The reference reads two kinds of YAML (``lidar_deform.py``):

* the *sensor model* -- ``config.yaml`` inside a dataset directory for the source sensor, ``--target`` for the
  target sensor (``lidar_deform.py:231-235, :289-295``): keys ``name, fov_up, fov_down, beams, angle_res_hor,
  fov_hor`` and optionally ``beam_angles``; the image width is ``W = int(fov_hor / angle_res_hor)``
  (``:264-277`` source, ``:302-315`` target);
* the *approach* file ``config/lidar_transfer.yaml`` (``:318-351``): adaption, number_of_scans, voxel_size,
  voxel_bounds, batch_interval, ignore / moving classes, labels and ``color_map``.

Host logic only: what the files say is turned into the arguments of the device path (``create_rays``,
``RaySet``, ``TSDFVolume``, the scan index list).  ``beam_angles`` is sorted in place like the reference does and
is ``None`` when absent; ``create_rays`` ignores it (``laserscan.py:1092-1119``), the projection uses it
(``laserscan.py:233-238``).

Three optional keys are this project's own, for a TARGET sensor; :class:`TargetModel` carries what they say to the device path
(``SensorModel.target_model()``), and without them nothing changes:

* ``beam_model: table`` (default ``linear``): ``beam_angles`` are the real elevation of every beam in degrees -- its rays leave
  at these angles and a point's image row is its nearest beam (:meth:`SensorModel.beam_table`);
* ``azimuth_model: sector`` (default ``full``) and ``azimuth_center`` (degrees, default 0): ``fov_hor`` is the width of the
  sensor's horizontal field of view around the direction ``azimuth_center`` and the ``W`` columns span that sector alone, not
  the whole circle (:meth:`SensorModel.sector`);
* ``beam_azimuth_offsets``, with ``beam_model: table``: one number per beam in degrees, in the order in which the file lists
  ``beam_angles`` (the loader pairs the two before it sorts the angles) -- the lasers of one firing do not share an azimuth,
  beam ``h`` of a column looks ``offset[h]`` to the LEFT of the column's nominal direction, measured like ``azimuth_center``
  (:meth:`SensorModel.beam_azimuth`); offsets that are all zero are none.

A fourth is what the target MEASURES along those rays, :class:`ReturnModel` (``SensorModel.return_model()``):

* ``return_model``: a block of ``min_range``, ``max_range`` (metres), ``max_incidence`` (degrees), ``remission`` (``none`` |
  ``lambert``), ``drop_rate`` and ``seed`` -- returns outside the range gate, seen too close to edge-on or dropped at random
  become misses of the rendered scan; a block with every field at its default is none.

A fifth is the ERROR of what it measures, :class:`NoiseModel` (``SensorModel.noise_model()``), beside the fourth,
not inside it:

* ``noise_model``: a block of ``range_sigma`` (metres), ``range_sigma_rel`` (metres per metre), ``range_resolution`` (metres),
  ``remission_sigma``, ``remission_levels`` and ``seed`` -- the range of a return is jittered along its ray and reported on a
  grid, its remission is jittered, clamped to [0, 1] and reported on ``remission_levels`` levels; a block with every field at
  its default is none.

A sixth is the WIDTH of its beams, :class:`EchoModel` (``SensorModel.echo_model()``), beside the two:

* ``echo_model``: a block of ``divergence`` (degrees, the full cone angle), ``subrays`` (1..8: the centre ray and ``subrays -
  1`` on a ring), ``ring`` (the ring's radius as a fraction of the half angle), ``separation`` (metres), ``min_subrays`` and
  ``mode`` (``first`` | ``strongest`` | ``last``) -- every cell is rendered with ``subrays`` rays, their hits are grouped into
  echoes along the range and one echo is reported, with the blended range of what the spot covers; ``divergence`` 0 or
  ``subrays`` 1 is none.
* ``dual_return``: a block of ``second`` (``none`` | ``first`` | ``strongest`` | ``last``), :class:`DualReturn`
  (``SensorModel.dual_return()``) -- a SECOND echo of every cell, chosen by ``second`` among the detected echoes other than
  the reported one, goes through the return and noise models and into the files behind the primary's points; ``none`` is
  off; it needs an ``echo_model`` that is on.

The approach file has two keys of this project's own for SEVERAL target sensors on one vehicle (:meth:`Approach.rig`, DESIGN
7i); a file without them behaves as before:

* ``rig``: a list of 1 to 8 heads ``{name, sensor, transformation}`` -- ``name`` unique and ``[A-Za-z0-9_-]+`` (a folder of the
  output), ``sensor`` the path of a sensor file relative to the approach file (or a mapping), ``transformation`` with the
  meaning of the top-level key, absent or empty for a head at the source pose; the top-level ``transformation`` must then be
  empty or the identity;
* ``rig_merged`` (default ``false``): the whole rig's points are also written as one scan, in the primary scan's frame.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field
from functools import cached_property
from typing import Dict, List, Optional

import numpy as np


@dataclass
class SensorModel:
    """One scanner description (``lidar_deform.py:264-277``)."""
    name: str
    fov_up: float
    fov_down: float
    beams: int
    angle_res_hor: float
    fov_hor: float
    beam_angles: Optional[List[float]] = None
    raw: dict = field(default_factory=dict, repr=False)
    beam_model: str = "linear"
    azimuth_model: str = "full"
    azimuth_center: float = 0.0
    #: per-beam azimuth offsets in degrees, paired with ``beam_angles`` index by index (the loader sorts the two together)
    beam_azimuth_offsets: Optional[List[float]] = None
    #: the file's ``return_model`` block as read (a mapping), ``None`` without the key: :meth:`return_model`
    return_block: Optional[dict] = None
    #: the file's ``noise_model`` block as read (a mapping), ``None`` without the key: :meth:`noise_model`
    noise_block: Optional[dict] = None
    #: the file's ``echo_model`` block as read (a mapping), ``None`` without the key: :meth:`echo_model`
    echo_block: Optional[dict] = None
    #: the file's ``dual_return`` block as read (a mapping), ``None`` without the key: :meth:`dual_return`
    dual_block: Optional[dict] = None

    @property
    def H(self) -> int:
        return int(self.beams)

    @property
    def W(self) -> int:
        # W = int(fov_hor / angle_res_hor)  (lidar_deform.py:277, :309) -- float division, truncation
        return int(self.fov_hor / self.angle_res_hor)

    def as_tuple(self):
        """``(name, fov_up, fov_down, H, W, beam_angles)``"""
        return self.name, self.fov_up, self.fov_down, self.H, self.W, self.beam_angles

    def create_rays(self):
        """Host mirror of ``MultiSemLaserScan.create_rays(fov_up, fov_down, H, W)`` for this model:
        ``[H*W, 3]`` float32 (beam_angles are ignored there, as in the reference)."""
        from .laserscan import create_rays
        m = self.target_model()
        return create_rays(self.fov_up, self.fov_down, self.H, self.W, m.beam_table, m.sector, m.beam_azimuth)

    def target_model(self):
        """What this sensor has beyond the reference's evenly spaced full circle as ONE :class:`TargetModel`, validated against
        the sensor: what the device path is handed for a TARGET.  Its fields: :meth:`beam_table`, :meth:`sector`, :meth:`beam_azimuth`."""
        who = f"sensor {self.name!r}"
        if self.beam_model not in ("linear", "table"):
            raise ValueError(f"{who}: beam_model {self.beam_model!r} (linear or table)")
        if self.azimuth_model not in ("full", "sector"):
            raise ValueError(f"{who}: azimuth_model {self.azimuth_model!r} (full or sector)")

        def numbers(values, else_say):
            try:
                return np.array([float(v) for v in values], dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: {else_say}") from None
        table = az = None
        if self.beam_model == "table":
            angles = numbers(self.beam_angles or (), "beam_model table needs beam_angles, a list of numbers")
            order = np.argsort(-angles, kind="stable")   # (a table's angles are distinct: one order)
            table = angles[order]
        if self.beam_azimuth_offsets is not None:
            az = numbers(self.beam_azimuth_offsets, "beam_azimuth_offsets must be a list of numbers")
            if table is not None and len(az) == len(table):   # (another count: refused below)
                az = az[order]
        sector = (self.azimuth_center, self.fov_hor) if self.azimuth_model == "sector" else None
        return TargetModel(table, sector, az, who).validate(self.H, (self.fov_up, self.fov_down), who)

    def return_model(self):
        """The sensor's :class:`ReturnModel` -- what a TARGET measures along its rays: range gate, incidence, dropout (DESIGN
        7e) -- or ``None`` without the ``return_model`` key or with every field at its default.  ``ValueError`` led by the
        sensor's name for a block that cannot be used.  :class:`TargetModel` stays rows and columns."""
        return ReturnModel.of(self.return_block, f"sensor {self.name!r}")

    def noise_model(self):
        """The sensor's :class:`NoiseModel` -- the error of what a TARGET measures: range jitter and grid, remission jitter
        and levels -- or ``None`` without the ``noise_model`` key or with every field at its default.
        ``ValueError`` led by the sensor's name for a block that cannot be used."""
        return NoiseModel.of(self.noise_block, f"sensor {self.name!r}")

    def echo_model(self):
        """The sensor's :class:`EchoModel` -- the width of a TARGET's beams: sub-rays, echoes, mixed cells -- or
        ``None`` without the ``echo_model`` key, with ``divergence`` 0 or with ``subrays`` 1.  ``ValueError`` led by the
        sensor's name for a block that cannot be used."""
        return EchoModel.of(self.echo_block, f"sensor {self.name!r}")

    def dual_return(self):
        """The sensor's :class:`DualReturn` -- a SECOND echo per cell -- or ``None`` without the ``dual_return``
        key or with ``second: none``.  ``ValueError`` led by the sensor's name for a block that cannot be used, and for one
        that is on while the sensor's echo model is off or absent: there is no second echo of a line."""
        who = f"sensor {self.name!r}"
        dual = DualReturn.of(self.dual_block, who)
        if dual is not None and self.echo_model() is None:
            raise ValueError(f"{who}: dual_return second: {dual.second} -- a second return needs an echo_model with a "
                             "divergence and at least two sub-rays")
        return dual

    def sector(self):
        """``None`` for ``azimuth_model: full``; for ``sector`` ``(center_deg, span_deg)`` as floats: the ``W`` columns span
        ``span_deg = fov_hor`` degrees around the direction ``center_deg = azimuth_center`` (``atan2(y, x)`` in the sensor's
        frame: 0 is straight ahead, positive to the left), column 0 at the left edge, clockwise seen from above.  A centre
        beyond +-180 comes back reduced by a full turn.  ``ValueError`` for another model, a ``fov_hor`` outside (0, 360),
        or a centre that is not finite or beyond +-360."""
        return self.target_model().sector

    def beam_table(self):
        """``None`` for ``beam_model: linear``; for ``table`` the beams' elevations in degrees, float64 [H], sorted
        descending -- row 0 is the highest beam, as ``create_rays``' row 0 is ``fov_up``.  ``ValueError`` unless there is
        one angle per beam, all are finite with |angle| < 90, neighbours differ by at least 1e-6 degrees and every angle
        lies in ``[fov_down, fov_up]`` (``mergemesh`` fuses only what the target's field of view holds, laserscan.py:952,
        :968: a beam outside it would look at nothing)."""
        return self.target_model().beam_table

    def beam_azimuth(self):
        """``None`` without ``beam_azimuth_offsets`` or when all of them are zero; else the beams' azimuth offsets in degrees,
        float64 [H], in the row order of :meth:`beam_table` (descending elevation) -- ``beam_azimuth_offsets[k]`` belongs to
        ``beam_angles[k]`` and travels with it.  Beam ``h`` of a column looks ``offset[h]`` to the left of the column's nominal
        direction.  ``ValueError`` unless the sensor has ``beam_model: table`` and there is one finite number per beam with
        ``|offset| <= 90``."""
        return self.target_model().beam_azimuth


def check_beam_azimuth(a, H, who="beam azimuth offsets"):
    """the conditions of :meth:`SensorModel.beam_azimuth` on a float64 array of offsets in degrees; returns it"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 1 or len(a) != int(H):
        raise ValueError(f"{who}: {a.size} beam_azimuth_offsets for {int(H)} beams")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{who}: beam_azimuth_offsets must be finite")
    if not np.all(np.abs(a) <= 90.0):
        raise ValueError(f"{who}: beam_azimuth_offsets must lie within +-90 degrees")
    return a


def beam_azimuth_radians(az):
    """What the column rule of the offsets reads (``LT_PROJ_BEAM_AZIMUTH``, ``lt_reverse_projection_beams_az_dev``), float64
    [H]: ``az / 180 * pi``."""
    return np.ascontiguousarray(np.asarray(az, dtype=np.float64) / 180. * np.pi)


def check_beam_table(b, H, fov_up, fov_down, who="beam table"):
    """the conditions of :meth:`SensorModel.beam_table` on a descending float64 table; returns it"""
    if b.ndim != 1 or len(b) != int(H):
        raise ValueError(f"{who}: {b.size} beam_angles for {int(H)} beams")
    if not np.all(np.isfinite(b)) or not np.all(np.abs(b) < 90.0):
        raise ValueError(f"{who}: beam_angles must be finite and within (-90, 90) degrees")
    if len(b) > 1 and not np.all(b[:-1] - b[1:] >= 1e-6):
        raise ValueError(f"{who}: neighbouring beam_angles must differ by at least 1e-6 degrees")
    if not np.all((b >= float(fov_down)) & (b <= float(fov_up))):
        raise ValueError(f"{who}: every beam angle must lie in [fov_down, fov_up] = [{fov_down}, {fov_up}]")
    return b


def check_sector(sector, who="sector"):
    """the conditions of :meth:`SensorModel.sector` on ``(center_deg, span_deg)``; returns the pair as floats, the centre
    within [-180, 180]"""
    try:
        c, s = (float(v) for v in sector)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: azimuth_center and fov_hor must be numbers") from None
    if not (0.0 < s < 360.0):
        raise ValueError(f"{who}: azimuth_model sector needs 0 < fov_hor < 360 (fov_hor = {s})")
    if not (np.isfinite(c) and abs(c) <= 360.0):
        raise ValueError(f"{who}: azimuth_center must be finite and within +-360 degrees (azimuth_center = {c})")
    if c > 180.0:
        c -= 360.0
    elif c < -180.0:
        c += 360.0
    return c, s


def sector_radians(sector):
    """What the column rule of a sector reads (``LT_PROJ_SECTOR``, ``lt_reverse_projection_sector_dev``), float64: the yaw of
    its middle ``yc = -center / 180 * pi`` and its width ``span / 180 * pi``."""
    c, s = sector
    return -c / 180. * np.pi, s / 180. * np.pi


def beam_rows(table):
    """What the row rule of a beam table reads (``LT_PROJ_BEAM_ROWS``), float64, derived once: ``Brad = B / 180 * pi`` and
    ``halfw[k]``, half the smaller of the gaps to the two neighbours in radians (the one existing gap for the first and the
    last row; 0 and unused for H = 1)."""
    B = np.asarray(table, dtype=np.float64)
    Brad = B / 180.0 * np.pi
    halfw = np.zeros_like(Brad)
    if len(Brad) > 1:
        gap = Brad[:-1] - Brad[1:]
        halfw[0], halfw[-1] = gap[0] / 2, gap[-1] / 2
        halfw[1:-1] = np.minimum(gap[:-1], gap[1:]) / 2
    return Brad, halfw


def _same(a, b):
    return (a is None) == (b is None) and (a is None or np.array_equal(a, b))


class TargetModel:
    """What distinguishes a TARGET sensor's rows and columns from the reference's evenly spaced full circle, as one immutable
    value -- the ONE thing the device path passes around (``create_rays``, ``RaySet``, ``Projector``, ``DeviceDeform``).  Its
    fields ``beam_table``, ``sector`` and ``beam_azimuth`` are what :meth:`SensorModel.beam_table`, :meth:`SensorModel.sector` and
    :meth:`SensorModel.beam_azimuth` return, each ``None`` where the sensor is the reference's.  The
    constructor normalises and nothing else does: dtype, the centre reduced by a full turn (:func:`check_sector`, whose
    conditions no sensor enters), offsets that are all zero become ``None``; offsets without a table are a ``ValueError``.
    :meth:`validate` holds the model against a sensor; ``who`` leads the messages of both.  What the library reads --
    :attr:`rows`, :attr:`sector_rad`, :attr:`azimuth_rad`, :attr:`proj_flags`, :meth:`grid` -- is derived from the fields on
    first use and kept.  Two models are equal when their fields are, arrays by value."""

    def __init__(self, beam_table=None, sector=None, beam_azimuth=None, who="target model"):
        def frozen(v):
            a = np.array(v, dtype=np.float64)
            a.setflags(write=False)
            return a
        if beam_table is not None:
            beam_table = frozen(beam_table)
        if sector is not None:
            sector = check_sector(sector, who)   # (no sensor enters its conditions, and the reduction needs them)
        if beam_azimuth is not None:
            if beam_table is None:
                raise ValueError(f"{who}: beam_azimuth_offsets needs beam_model: table (the offsets belong to the beams of a "
                                 "beam table)")
            beam_azimuth = frozen(beam_azimuth)
            if not np.any(beam_azimuth != 0.0):   # (all zero: the table alone)
                beam_azimuth = None
        self.__dict__.update(beam_table=beam_table, sector=sector, beam_azimuth=beam_azimuth)

    def __setattr__(self, name, value):
        raise AttributeError("a TargetModel does not change: make another")

    def validate(self, H, fov=None, who="target model"):
        """``ValueError``, its message led by ``who``, unless the model fits a sensor of ``H`` beams: one table entry and one
        offset per beam, the conditions of :func:`check_beam_azimuth`, and -- given the sensor's ``fov = (fov_up, fov_down)``
        -- those of :func:`check_beam_table`.  Returns the model."""
        if self.beam_table is not None:
            if fov is not None:
                check_beam_table(self.beam_table, H, fov[0], fov[1], who)
            elif self.beam_table.shape != (int(H),):
                raise ValueError(f"{who}: {self.beam_table.size} beam_angles for {int(H)} beams")
        if self.beam_azimuth is not None:
            check_beam_azimuth(self.beam_azimuth, H, who)
        return self

    def difference(self, other):
        """the first field in which two models differ -- ``"beam_table"``, ``"sector"``, ``"beam_azimuth"`` -- or ``None``"""
        if not _same(self.beam_table, other.beam_table):
            return "beam_table"
        if self.sector != other.sector:
            return "sector"
        return None if _same(self.beam_azimuth, other.beam_azimuth) else "beam_azimuth"

    def __eq__(self, other):
        return isinstance(other, TargetModel) and self.difference(other) is None

    @cached_property
    def rows(self):
        """the table as ``LT_PROJ_BEAM_ROWS`` reads it, float64 [2 H]: ``Brad`` followed by ``halfw`` (:func:`beam_rows`)"""
        return None if self.beam_table is None else np.ascontiguousarray(np.concatenate(beam_rows(self.beam_table)))

    @property
    def rows_ptr(self):
        """``void *`` to :attr:`rows` (which the model keeps alive), ``None`` without a table"""
        import ctypes as C
        return None if self.rows is None else self.rows.ctypes.data_as(C.c_void_p)

    @cached_property
    def sector_rad(self):
        """the sector as ``LT_PROJ_SECTOR`` reads it, float64 [2]: :func:`sector_radians`"""
        return None if self.sector is None else np.array(sector_radians(self.sector), dtype=np.float64)

    @cached_property
    def azimuth_rad(self):
        """the offsets as ``LT_PROJ_BEAM_AZIMUTH`` reads them, float64 [H]: :func:`beam_azimuth_radians`"""
        return None if self.beam_azimuth is None else beam_azimuth_radians(self.beam_azimuth)

    @property
    def proj_flags(self):
        """the ``LT_PROJ_*`` bits of the three fields"""
        from . import _lib
        return (_lib.LT_PROJ_BEAM_ROWS if self.beam_table is not None else 0) | \
            (_lib.LT_PROJ_SECTOR if self.sector is not None else 0) | \
            (_lib.LT_PROJ_BEAM_AZIMUTH if self.beam_azimuth is not None else 0)

    def grid(self, W):
        """the bin grid of this sensor's ray set at image width ``W`` (``RaySet(..., grid=...)``): ``raytracer.sector_grid``
        for a sector, ``None`` (the image's own rule) without one"""
        from .raytracer import sector_grid
        return None if self.sector is None else sector_grid(W, self.sector)


def return_hash_mix(x):
    """``mix`` of the return model's hash (include/lidarhip.h), uint32 with wrapping products, on a Python int"""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def return_hash(seed, scan, i):
    """``hash(seed, scan, i) = mix(mix(mix(seed) + scan) + i)`` (uint32 sums wrap): the random rule of :class:`ReturnModel`, a
    pure function of the three -- a scan's pattern is the same whichever chain, rank or order renders it"""
    return return_hash_mix(return_hash_mix(return_hash_mix(int(seed)) + int(scan)) + int(i))


class _ModelBlock:
    """What :class:`ReturnModel`, :class:`NoiseModel` and :class:`EchoModel` share: one immutable value per block of a
    TARGET sensor's file.  A class names its block's key (``KEY``) and its fields with their defaults (``DEFAULTS``), and its
    constructor validates with :meth:`_number` / :meth:`_integer`, whose messages are led by ``who`` and the key.  Equality
    is per block: a model never equals one of another block with the same field values."""

    KEY = None
    DEFAULTS = {}

    @classmethod
    def _number(cls, who, name, v, ok, say):
        """``v`` as a float: a number (no bool, no string) for which ``ok(v)`` holds, else ``ValueError``: must be ``say``"""
        try:
            if isinstance(v, (bool, str)):
                raise TypeError
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: {cls.KEY} {name} must be a number, not {v!r}") from None
        if not ok(v):
            raise ValueError(f"{who}: {cls.KEY} {name} must be {say}, not {v}")
        return v

    @classmethod
    def _integer(cls, who, name, v, lo=0, hi=0xFFFFFFFF, say="[0, 2^32)"):
        """``v`` as an int: an integer (no bool) in ``lo .. hi``, else ``ValueError``: must be an integer in ``say``"""
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"{who}: {cls.KEY} {name} must be an integer in {say}, not {v!r}")
        return int(v)

    def __setattr__(self, name, value):
        kind = type(self).__name__
        raise AttributeError(f"{'an' if kind[0] in 'AEIOU' else 'a'} {kind} does not change: make another")

    @classmethod
    def of(cls, block, who=None):
        """The model of a sensor file's block (a mapping, or ``None``: no key), or ``None`` when it is at its default (for an
        :class:`EchoModel`: off); an unknown key and a block that is no mapping are ``ValueError``, led by ``who`` (default:
        the key in words).  A model of this class passes through (``None`` if at its default)."""
        if who is None:
            who = cls.KEY.replace("_", " ")
        if block is None:
            return None
        if isinstance(block, cls):
            return None if block.is_default else block
        if not isinstance(block, dict):
            raise ValueError(f"{who}: {cls.KEY} must be a mapping of {', '.join(cls.DEFAULTS)}")
        unknown = sorted(set(map(str, block)) - set(cls.DEFAULTS))
        if unknown:
            raise ValueError(f"{who}: {cls.KEY} has unknown key(s) {', '.join(unknown)} (known: {', '.join(cls.DEFAULTS)})")
        m = cls(who=who, **block)
        return None if m.is_default else m

    def fields(self):
        return {k: getattr(self, k) for k in self.DEFAULTS}

    @property
    def is_default(self):
        return self.fields() == self.DEFAULTS

    def __eq__(self, other):
        return isinstance(other, _ModelBlock) and other.KEY == self.KEY and self.fields() == other.fields()

    def __hash__(self):
        return hash(tuple(self.fields().values()))

    def __repr__(self):
        return type(self).__name__ + "(" + ", ".join(f"{k}={v!r}" for k, v in self.fields().items()) + ")"


class ReturnModel(_ModelBlock):
    """What a TARGET sensor measures along its rays beyond the reference's "every hit returns" (the sensor file's
    ``return_model`` block), as one immutable value like :class:`TargetModel`: a range gate ``min_range`` /
    ``max_range`` (metres), ``max_incidence`` (degrees between ray and surface normal; 90 never drops), ``remission``
    (``"none"`` or ``"lambert"``: the remission times the cosine of the incidence angle), ``drop_rate`` (probability of a
    random drop) and its ``seed``.  The constructor is the only place that normalises and validates -- finite numbers,
    ``0 <= min_range <= max_range`` (``max_range`` may be ``inf``), ``0 < max_incidence <= 90``, ``0 <= drop_rate < 1``,
    ``seed`` in uint32, else ``ValueError`` led by ``who`` -- and :meth:`of` returns ``None`` for a model in which every field
    is at its default, as all-zero azimuth offsets are none.  What the library reads is derived here in float64 / Python
    ints: :attr:`min_cos` ``= cos(max_incidence * pi / 180)`` (exactly 0 for 90), :attr:`drop_threshold`
    ``= floor(drop_rate * 2^32)``."""

    KEY = "return_model"
    DEFAULTS = dict(min_range=0.0, max_range=float("inf"), max_incidence=90.0, remission="none", drop_rate=0.0, seed=0)

    def __init__(self, min_range=0.0, max_range=float("inf"), max_incidence=90.0, remission="none", drop_rate=0.0, seed=0,
                 who="return model"):
        import math

        def number(name, v):
            return self._number(who, name, v, lambda v: math.isfinite(v) or (name == "max_range" and v == math.inf),
                                "finite (max_range may be +inf)")
        lo, hi = number("min_range", min_range), number("max_range", max_range)
        inc, rate = number("max_incidence", max_incidence), number("drop_rate", drop_rate)
        if not 0.0 <= lo <= hi:
            raise ValueError(f"{who}: return_model needs 0 <= min_range <= max_range (min_range = {lo}, max_range = {hi})")
        if not 0.0 < inc <= 90.0:
            raise ValueError(f"{who}: return_model needs 0 < max_incidence <= 90 degrees (max_incidence = {inc})")
        if not 0.0 <= rate < 1.0:
            raise ValueError(f"{who}: return_model needs 0 <= drop_rate < 1 (drop_rate = {rate})")
        seed = self._integer(who, "seed", seed)
        if remission not in ("none", "lambert"):
            raise ValueError(f"{who}: return_model remission {remission!r} (none or lambert)")
        self.__dict__.update(min_range=lo, max_range=hi, max_incidence=inc, remission=str(remission), drop_rate=rate,
                             seed=seed)

    @cached_property
    def min_cos(self):
        """``cos(max_incidence * pi / 180)`` in float64; exactly 0 for 90 degrees (where the float64 cosine is 6e-17)"""
        import math
        return 0.0 if self.max_incidence == 90.0 else math.cos(self.max_incidence * math.pi / 180.0)

    @property
    def drop_threshold(self):
        """``floor(drop_rate * 2^32)`` as a Python int (below 2^32: ``drop_rate < 1``)"""
        return min(int(self.drop_rate * 4294967296.0), 0xFFFFFFFF)

    @property
    def lambert(self):
        return self.remission == "lambert"

    def args(self):
        """the model as ``lt_return_model_dev`` reads it (``_lib.ReturnModelArgs``)"""
        from . import _lib
        return _lib.ReturnModelArgs(self.min_range, self.max_range, self.min_cos, self.drop_threshold, self.seed,
                                    _lib.LT_RETURN_LAMBERT if self.lambert else 0)


class NoiseModel(_ModelBlock):
    """The error of what a TARGET sensor measures (the sensor file's ``noise_model`` block), one immutable value
    like :class:`ReturnModel` and beside it: the standard deviation of the range jitter ``range_sigma + range_sigma_rel *
    range`` (metres; metres per metre), the grid ``range_resolution`` ranges are reported on (metres, 0: none), the standard
    deviation ``remission_sigma`` of the remission jitter, the number ``remission_levels`` of levels remission is reported on
    (0: off, else at least 2) and the ``seed`` of the draws.  The constructor is the only place that normalises and
    validates -- finite numbers that are not negative, ``remission_levels`` 0 or an integer in [2, 2^32), ``seed`` in uint32,
    else ``ValueError`` led by ``who`` -- and :meth:`of` returns ``None`` for a model in which every field is at its
    default.  The draws are a pure function of ``(seed, scan, cell)``: :func:`return_hash_mix` in a stream of its own."""

    KEY = "noise_model"
    DEFAULTS = dict(range_sigma=0.0, range_sigma_rel=0.0, range_resolution=0.0, remission_sigma=0.0, remission_levels=0, seed=0)

    def __init__(self, range_sigma=0.0, range_sigma_rel=0.0, range_resolution=0.0, remission_sigma=0.0, remission_levels=0,
                 seed=0, who="noise model"):
        import math

        def number(name, v):
            return self._number(who, name, v, lambda v: math.isfinite(v) and v >= 0.0, "finite and not negative")

        def integer(name, v):
            return self._integer(who, name, v)
        fields = dict(range_sigma=number("range_sigma", range_sigma), range_sigma_rel=number("range_sigma_rel", range_sigma_rel),
                      range_resolution=number("range_resolution", range_resolution),
                      remission_sigma=number("remission_sigma", remission_sigma),
                      remission_levels=integer("remission_levels", remission_levels), seed=integer("seed", seed))
        if fields["remission_levels"] == 1:
            raise ValueError(f"{who}: noise_model remission_levels must be 0 (off) or at least 2, not 1")
        self.__dict__.update(fields)

    def args(self, gate=None):
        """the model as ``lt_noise_model_dev`` reads it (``_lib.NoiseModelArgs``); ``gate``: the sensor's :class:`ReturnModel`
        -- a measured range outside its ``min_range`` .. ``max_range`` is not reported -- or ``None``: 0 and +inf"""
        from . import _lib
        lo, hi = (0.0, float("inf")) if gate is None else (gate.min_range, gate.max_range)
        return _lib.NoiseModelArgs(self.range_sigma, self.range_sigma_rel, self.range_resolution, self.remission_sigma, lo, hi,
                                   self.remission_levels, self.seed)


class EchoModel(_ModelBlock):
    """The width of a TARGET sensor's beams (the sensor file's ``echo_model`` block), one immutable value like
    :class:`ReturnModel` and :class:`NoiseModel` and beside them: the full cone angle ``divergence`` of a beam (degrees, 0:
    a line), the number ``subrays`` of rays a cell is rendered with (1..8, 1: a line) -- the centre ray and ``subrays - 1``
    evenly on a ring of radius ``ring`` times the half angle --, the distance ``separation`` (metres) behind an echo's first
    sub-hit beyond which a sub-hit starts a new echo, the number ``min_subrays`` of sub-hits an echo needs to be detected and
    the ``mode`` that picks the reported echo.  The constructor is the only place that normalises and validates, else
    ``ValueError`` led by ``who``; :meth:`of` returns ``None`` for a model that is off (``divergence`` 0 or ``subrays`` 1)."""

    KEY = "echo_model"
    DEFAULTS = dict(divergence=0.0, subrays=1, ring=0.7071, separation=0.5, min_subrays=1, mode="strongest")
    MODES = ("first", "strongest", "last")   # in the order of LT_ECHO_FIRST, LT_ECHO_STRONGEST, LT_ECHO_LAST
    MAX_SUBRAYS = 8                          # LT_ECHO_MAX_SUBRAYS

    def __init__(self, divergence=0.0, subrays=1, ring=0.7071, separation=0.5, min_subrays=1, mode="strongest",
                 who="echo model"):
        import math

        def number(name, v, ok, say):
            return self._number(who, name, v, lambda v: math.isfinite(v) and ok(v), say)

        def integer(name, v, lo, hi):
            return self._integer(who, name, v, lo, hi, f"[{lo}, {hi}]")
        fields = dict(divergence=number("divergence", divergence, lambda v: 0.0 <= v < 180.0, "in [0, 180) degrees"),
                      subrays=integer("subrays", subrays, 1, self.MAX_SUBRAYS),
                      ring=number("ring", ring, lambda v: 0.0 < v <= 1.0, "in (0, 1]"),
                      separation=number("separation", separation, lambda v: v > 0.0, "finite and positive"))
        fields["min_subrays"] = integer("min_subrays", min_subrays, 1, fields["subrays"])
        if not isinstance(mode, str) or mode not in self.MODES:
            raise ValueError(f"{who}: echo_model mode must be one of {', '.join(self.MODES)}, not {mode!r}")
        fields["mode"] = mode
        self.__dict__.update(fields)

    @property
    def is_default(self):
        """off: a beam without a width, or one ray per cell -- the absence of the key"""
        return self.divergence == 0.0 or self.subrays == 1

    def offsets(self):
        """The sub-rays' offsets, float64 ``[subrays, 2]``: row 0 is (0, 0), the centre ray; row ``k >= 1`` is ``tan(rho) *
        (cos phi_k, sin phi_k)`` with ``rho = radians(divergence / 2 * ring)`` and ``phi_k = 2 pi (k - 1) / (S - 1) + pi / (S -
        1)``: ``a`` to the left, ``b`` upwards, in units of the central ray's length.  Made here, on the host: the device
        evaluates no transcendental."""
        S = self.subrays
        off = np.zeros((S, 2), dtype=np.float64)
        if S > 1:
            rho = np.radians(self.divergence / 2.0 * self.ring)
            phi = 2.0 * np.pi * np.arange(S - 1, dtype=np.float64) / (S - 1) + np.pi / (S - 1)
            off[1:, 0] = np.tan(rho) * np.cos(phi)
            off[1:, 1] = np.tan(rho) * np.sin(phi)
        return off

    def args(self):
        """the model as ``lt_create_subrays_dev`` and ``lt_echo_resolve_dev`` read it (``_lib.EchoModelArgs``)"""
        from . import _lib
        a = _lib.EchoModelArgs()
        for k, v in enumerate(self.offsets().ravel()):
            a.off[k] = float(v)
        a.separation, a.n_subrays, a.min_subrays = self.separation, self.subrays, self.min_subrays
        a.mode, a.reserved = self.MODES.index(self.mode), 0
        return a


class DualReturn(_ModelBlock):
    """A TARGET sensor's dual-return mode (the sensor file's ``dual_return`` block), beside :class:`EchoModel`:
    ``second`` names the rule that picks a SECOND echo among a cell's detected echoes other than the reported one -- ``first``
    the earliest of the rest, ``last`` the latest, ``strongest`` the one with the largest remission sum -- or ``none``, which
    is off and the absence of the key.  Validated by the constructor alone, else ``ValueError`` led by ``who``."""

    KEY = "dual_return"
    DEFAULTS = dict(second="none")
    SECONDS = ("none",) + EchoModel.MODES

    def __init__(self, second="none", who="dual return"):
        if not isinstance(second, str) or second not in self.SECONDS:
            raise ValueError(f"{who}: dual_return second must be one of {', '.join(self.SECONDS)}, not {second!r}")
        self.__dict__.update(second=second)

    @property
    def mode(self):
        """``second`` as ``lt_echo_resolve_dual_dev``'s ``second_mode`` (LT_ECHO_FIRST, LT_ECHO_STRONGEST, LT_ECHO_LAST)"""
        if self.is_default:
            raise ValueError("dual_return second: none has no second_mode")
        return EchoModel.MODES.index(self.second)


def _load_yaml(path_or_dict):
    if isinstance(path_or_dict, dict):
        return path_or_dict
    import yaml
    with open(path_or_dict, "r") as f:
        return yaml.safe_load(f)


def load_sensor(path_or_dict) -> SensorModel:
    """Read a sensor YAML exactly as ``lidar_deform.py:264-277`` / ``:302-315`` do.

    Missing mandatory keys raise ``KeyError`` (the reference indexes the dict directly); a missing
    ``beam_angles`` means "equidistant angles" (``None``); present ones are sorted ascending."""
    cfg = _load_yaml(path_or_dict)
    name = cfg["name"]
    fov_up = cfg["fov_up"]
    fov_down = cfg["fov_down"]
    beams = cfg["beams"]
    angle_res_hor = cfg["angle_res_hor"]
    fov_hor = cfg["fov_hor"]
    try:
        beam_angles = list(cfg["beam_angles"])
        beam_angles.sort()
    except Exception:
        beam_angles = None
    offsets = cfg.get("beam_azimuth_offsets")
    if offsets is not None:
        try:   # pair with the angles in the FILE's order, then carry along into the sorted one
            offsets, listed = list(offsets), list(cfg["beam_angles"])
            if len(offsets) == len(listed):
                offsets = [offsets[k] for k in sorted(range(len(listed)), key=lambda k: listed[k])]
        except Exception:
            raise ValueError(f"sensor {name!r}: beam_azimuth_offsets needs beam_model: table and its beam_angles, "
                             "one number per beam") from None
    model = SensorModel(name, fov_up, fov_down, beams, angle_res_hor, fov_hor, beam_angles, raw=cfg,
                        beam_model=str(cfg.get("beam_model", "linear")),
                        azimuth_model=str(cfg.get("azimuth_model", "full")), azimuth_center=cfg.get("azimuth_center", 0.0),
                        beam_azimuth_offsets=offsets, return_block=cfg.get("return_model"),
                        noise_block=cfg.get("noise_model"), echo_block=cfg.get("echo_model"),
                        dual_block=cfg.get("dual_return"))
    model.target_model()   # (a table, a sector or offsets that cannot be used: said at load time)
    model.return_model()   # (and a return model that cannot be)
    model.noise_model()    # (nor a noise model)
    model.echo_model()     # (nor an echo model)
    model.dual_return()    # (nor a second return, or one without an echo model)
    return model


def refuse_source_table(source):
    """A table is a property of the TARGET: the TSDF kernel's pixel model of the source scan is the reference's linear one."""
    if getattr(source, "beam_model", "linear") != "linear":
        raise ValueError(f"source sensor {getattr(source, 'name', '')!r}: beam_model {source.beam_model!r} is for target sensors "
                         "only (the source scan is fused by the reference's evenly spaced pixel model)")


def refuse_source_sector(source):
    """A sector is a property of the TARGET as well: the source scan is fused by the reference's full-circle pixel model."""
    if getattr(source, "azimuth_model", "full") != "full":
        raise ValueError(f"source sensor {getattr(source, 'name', '')!r}: azimuth_model {source.azimuth_model!r} is for target "
                         "sensors only (the source scan is fused by the reference's full-circle pixel model)")


def refuse_source_beam_azimuth(source):
    """Azimuth offsets are a property of the TARGET's table as well: the source scan is fused by the reference's pixel model,
    whose rows share one azimuth per column."""
    if getattr(source, "beam_azimuth_offsets", None) is not None:
        raise ValueError(f"source sensor {getattr(source, 'name', '')!r}: beam_azimuth_offsets is for target sensors only (the "
                         "source scan is fused by the reference's pixel model: one azimuth per column)")


def refuse_source_return_model(source):
    """A return model is a property of the TARGET as well: the source scan is what its sensor recorded."""
    if getattr(source, "return_block", None) is not None:
        raise ValueError(f"source sensor {getattr(source, 'name', '')!r}: return_model is for target sensors only (the source "
                         "scan holds the returns its sensor recorded)")


def refuse_source_noise_model(source):
    """So is its noise model: the source scan holds the error its sensor made."""
    if getattr(source, "noise_block", None) is not None:
        raise ValueError(f"source sensor {getattr(source, 'name', '')!r}: noise_model is for target sensors only (the source "
                         "scan holds the measurement error of its own sensor)")


def refuse_source_echo_model(source):
    """And its echo model: the source scan holds the echoes its own beams produced."""
    if getattr(source, "echo_block", None) is not None:
        raise ValueError(f"source sensor {getattr(source, 'name', '')!r}: echo_model is for target sensors only (the source "
                         "scan holds the echoes of its own sensor's beams)")


def refuse_source_dual_return(source):
    """And a second return: the source scan holds the returns its own sensor wrote."""
    if getattr(source, "dual_block", None) is not None:
        raise ValueError(f"source sensor {getattr(source, 'name', '')!r}: dual_return is for target sensors only (the source "
                         "scan holds the returns its own sensor wrote)")


def refuse_source_models(source):
    """everything a :class:`TargetModel`, a :class:`ReturnModel`, a :class:`NoiseModel` or an :class:`EchoModel` holds is a
    property of the TARGET, and so is a :class:`DualReturn`: the seven refusals, the table's first"""
    refuse_source_table(source)
    refuse_source_sector(source)
    refuse_source_beam_azimuth(source)
    refuse_source_return_model(source)
    refuse_source_noise_model(source)
    refuse_source_echo_model(source)
    refuse_source_dual_return(source)


RIG_MAX_HEADS = 8   # sensors of one lt_scene_render_rig_dev call


@dataclass
class RigHead:
    """One sensor of a rig (:meth:`Approach.rig`): its name (a folder of the output), its model, its mounting."""
    name: str
    sensor: SensorModel
    mount: Optional[tuple]


@dataclass
class Approach:
    """``config/lidar_transfer.yaml`` (``lidar_deform.py:318-351``)."""
    adaption: str
    preserve_float: bool
    voxel_size: float
    voxel_bounds: np.ndarray          # [3, 2] (xmin xmax / ymin ymax / zmin zmax), lidar_deform.py:347-350
    number_of_scans: int
    ignore: List[int]
    moving: List[int]
    transformation: List[float]
    batch_interval: int               # default 1 when absent (lidar_deform.py:352-355)
    color_map: Dict[int, List[int]]   # bgr
    labels: Dict[int, str]
    rig_block: Optional[list] = None  # the `rig` key as read: 1 to 8 entries {name, sensor, transformation}; None: no rig
    rig_merged: bool = False          # with a rig: also write the whole rig's points as one scan
    base_dir: Optional[str] = None    # directory of the approach file: a head's `sensor` path is relative to it

    def rig(self):
        """The heads of the approach's sensor rig, validated, in the file's order: a list of :class:`RigHead` (``name``,
        ``sensor``: its :class:`SensorModel`, ``mount``: :func:`mount_of` its ``transformation`` -- ``None`` at the source
        pose); ``None`` for an approach without the key.  ``ValueError``: not 1 to 8 entries, an entry that is no mapping of
        ``name, sensor, transformation``, a name that is not unique or does not match ``[A-Za-z0-9_-]+``, a top-level
        ``transformation`` other than the identity next to a ``rig`` (each head has its own), ``rig_merged`` without a rig."""
        if self.rig_block is None:
            if self.rig_merged:
                raise ValueError("rig_merged: true needs a rig")
            return None
        block = self.rig_block
        if not isinstance(block, (list, tuple)) or not 1 <= len(block) <= RIG_MAX_HEADS:
            n = len(block) if isinstance(block, (list, tuple)) else type(block).__name__
            raise ValueError(f"rig: a list of 1 to {RIG_MAX_HEADS} heads {{name, sensor, transformation}}, not {n}")
        if mount_of(self.transformation) is not None:
            raise ValueError("rig: the top-level transformation must be empty or the identity next to a rig (every head of the "
                             "rig has its own transformation)")
        heads, seen = [], set()
        for k, entry in enumerate(block):
            if not isinstance(entry, dict) or "name" not in entry or "sensor" not in entry:
                raise ValueError(f"rig: head {k} must be a mapping of name, sensor and (optionally) transformation")
            unknown = sorted(set(entry) - {"name", "sensor", "transformation"})
            if unknown:
                raise ValueError(f"rig: head {k} has unknown key(s) {', '.join(map(str, unknown))} (known: name, sensor, "
                                 "transformation)")
            name = entry["name"]
            if not isinstance(name, str) or not re.fullmatch(r"[A-Za-z0-9_-]+", name):
                raise ValueError(f"rig: head {k}: name {name!r} must match [A-Za-z0-9_-]+")
            if name in seen:
                raise ValueError(f"rig: head {k}: the name {name!r} is used twice")
            seen.add(name)
            sensor = entry["sensor"]
            if isinstance(sensor, str):
                sensor = sensor if os.path.isabs(sensor) or self.base_dir is None else os.path.join(self.base_dir, sensor)
            elif not isinstance(sensor, dict):
                raise ValueError(f"rig: head {name!r}: sensor must be the path of a sensor file or a mapping")
            try:
                mount = mount_of(entry.get("transformation"))
            except ValueError as e:
                raise ValueError(f"rig: head {name!r}: {e}") from None
            heads.append(RigHead(name, load_sensor(sensor), mount))
        return heads

    def color_lut(self) -> np.ndarray:
        """``SemLaserScan.__init__``'s look-up table (``laserscan.py:547-555``): ``[max(key) + 1 + 100, 3]`` float32,
        ``color_map`` values / 255."""
        max_key = 0
        for key in self.color_map:
            if key + 1 > max_key:
                max_key = key + 1
        lut = np.zeros((max_key + 100, 3), dtype=np.float32)
        for key, value in self.color_map.items():
            lut[key] = np.array(value, np.float32) / 255.0
        return lut

    def mount(self):
        """The target sensor's mounting: ``None`` when ``transformation`` is empty, ``None`` or the exact identity, else the
        validated ``(T, P)`` float64 pair (see :func:`mount_of`)."""
        return mount_of(self.transformation)

    def scan_indices(self, n_scan_files: int, offset: int = 0):
        """Scan list of the batch loop (``lidar_deform.py:385-390, :457-459``)."""
        from .dist import scan_indices
        return scan_indices(n_scan_files, self.number_of_scans, offset, self.batch_interval)


def mount_of(transformation):
    """``transformation`` of the approach file as the target sensor's mounting.  ``T`` (16 numbers, row-major 4x4) maps
    coordinates in the source sensor's frame of the primary scan to the target sensor's frame, ``x_target = T . x_source``;
    the target sensor stands at ``P = inv(T) = [Rp | tp]`` in the scene.  Returns ``None`` for an empty list, ``None`` or the
    exact identity (nothing downstream changes then), else ``(T, P)`` as float64 [4, 4] arrays; a ``(T, P)`` pair returned
    earlier is accepted as well.  ``ValueError`` unless ``T`` is rigid: 16 numbers, last row ``0 0 0 1``,
    ``max |R . R^T - I| <= 1e-6``, ``det R > 0``."""
    if transformation is None:
        return None
    if isinstance(transformation, tuple) and len(transformation) == 2 and np.shape(transformation[0]) == (4, 4):
        transformation = transformation[0]
    t = np.asarray(transformation, dtype=np.float64)
    if t.size == 0:
        return None
    if t.size != 16:
        raise ValueError(f"transformation: 16 numbers (a row-major 4x4 matrix), not {t.size}")
    T = np.ascontiguousarray(t.reshape(4, 4))
    if not np.all(np.isfinite(T)):
        raise ValueError("transformation: not finite")
    if np.array_equal(T, np.eye(4)):
        return None
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f"transformation: the last row is 0 0 0 1, not {T[3].tolist()}")
    R = T[:3, :3]
    err = float(np.abs(R @ R.T - np.eye(3)).max())
    if not err <= 1e-6:
        raise ValueError(f"transformation: the upper-left 3x3 is not a rotation (|R R^T - I| = {err:.3g} > 1e-6)")
    if not np.linalg.det(R) > 0:
        raise ValueError("transformation: the upper-left 3x3 is a reflection (det < 0)")
    return T, np.ascontiguousarray(np.linalg.inv(T))


def _rig_merged(cfg):
    """the approach file's ``rig_merged``: a real boolean (``"false"`` is a string, and true), and only next to a ``rig``"""
    v = cfg.get("rig_merged", False)
    if not isinstance(v, bool):
        raise ValueError(f"rig_merged: true or false, not {v!r}")
    if v and cfg.get("rig") is None:
        raise ValueError("rig_merged: true needs a rig")
    return v


def load_approach(path_or_dict) -> Approach:
    cfg = _load_yaml(path_or_dict)
    vb = np.array(cfg["voxel_bounds"])
    try:
        vb = vb.reshape(3, 2)
    except Exception:
        pass
    return Approach(adaption=cfg["adaption"], preserve_float=cfg["preserve_float"], voxel_size=cfg["voxel_size"],
                    voxel_bounds=vb, number_of_scans=cfg["number_of_scans"], ignore=list(cfg["ignore"]),
                    moving=list(cfg["moving"]), transformation=list(cfg["transformation"]),
                    batch_interval=cfg.get("batch_interval", 1), color_map=dict(cfg["color_map"]),
                    labels=dict(cfg.get("labels", {})), rig_block=cfg.get("rig"), rig_merged=_rig_merged(cfg),
                    base_dir=None if isinstance(path_or_dict, dict) else os.path.dirname(os.path.abspath(path_or_dict)))
