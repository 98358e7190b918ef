"""``lidar_transfer_amd._chain``: what the chain layer hands the library's device entry points -- the merged cloud, the
``lt_cloud`` and beam tables, the output pointers and the target sensor's mounting -- on CPU tensors, without the library;
and ``_chain.Sensing``, the one object that knows what follows a render and in which order, with recording fakes in place of
``post``'s wrappers and a stand-in ray set."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from lidar_transfer_amd import _chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]


def _cloud(n, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n, 3), generator=g).to(dtype), torch.rand((n,), generator=g), torch.arange(n, dtype=torch.int32) + 7 * seed)


def test_merged_cloud_is_the_cloud_itself_or_the_concatenation_in_order():
    one = _cloud(5)
    got = _chain.merged_cloud([one])
    assert len(got) == 3 and all(a is b for a, b in zip(got, one))
    clouds = [_cloud(5, seed=1), _cloud(0, seed=2), _cloud(3, seed=3)]
    got = _chain.merged_cloud(clouds)
    assert len(got) == 3
    for k in range(3):
        assert got[k].shape[0] == 8 and got[k].dtype == clouds[0][k].dtype
        assert torch.equal(got[k][:5], clouds[0][k]) and torch.equal(got[k][5:], clouds[2][k])


def test_cloud_table_coerces_keeps_and_counts():
    pts, rem, lab = _cloud(6, torch.float64)
    wide = torch.rand((6, 6), dtype=torch.float64)[:, ::2]                   # [6, 3], not contiguous
    assert not wide.is_contiguous()
    clouds = [(pts, rem.double(), lab.long()), (wide, rem[::2][:3].repeat(2), lab)]
    cl, keep, is_f64 = _chain.cloud_table(clouds)
    assert is_f64 == 1 and len(cl) == 2 and len(keep) == 6
    assert [cl[k].n for k in range(2)] == [6, 6]
    for k in range(2):
        p, r, l = keep[3 * k:3 * k + 3]
        assert p.is_contiguous() and p.dtype == torch.float64 and r.dtype == torch.float32 and l.dtype == torch.int32
        assert r.is_contiguous() and l.is_contiguous()
        assert (cl[k].points, cl[k].rem, cl[k].label) == (p.data_ptr(), r.data_ptr(), l.data_ptr())
        assert torch.equal(p, clouds[k][0]) and torch.equal(r, clouds[k][1].float()) and torch.equal(l, clouds[k][2].int())
    assert keep[0] is pts                                                    # (what needs no coercion is not copied)
    assert keep[3].data_ptr() != wide.data_ptr()                             # the contiguous copy is what the table points to
    cl, keep, is_f64 = _chain.cloud_table([_cloud(4)])
    assert is_f64 == 0 and cl[0].n == 4 and keep[1].dtype == torch.float32
    with pytest.raises(TypeError):
        _chain.cloud_table([_cloud(4, torch.float16)])
    with pytest.raises(TypeError):
        _chain.cloud_table([_cloud(4, torch.float32), _cloud(4, torch.float64)])


def test_beam_table_origin_and_output_pointers():
    for none in (None, []):
        ptr, n, _ = _chain.beam_table(none)
        assert ptr is None and n == 0
    ptr, n, arr = _chain.beam_table([-3, 1.5, 2])
    assert n == 3 and arr.dtype == np.float64 and arr.flags["C_CONTIGUOUS"] and ptr.value == arr.ctypes.data
    assert arr.tolist() == [-3.0, 1.5, 2.0]
    org = _chain.origin3((1, 2.5, np.float32(0.1)))
    assert isinstance(org, C.c_float * 3) and list(org) == [1.0, 2.5, float(np.float32(0.1))]
    out = dict(endpoints=torch.zeros((4, 3)), range=torch.zeros(4), endrem=None, tri=torch.zeros(4, dtype=torch.int32))
    got = _chain.out_ptrs(out)
    assert got == (out["endpoints"].data_ptr(), None, out["range"].data_ptr(), None, out["tri"].data_ptr())
    assert _chain.OUT_KEYS == ("endpoints", "endcolors", "range", "endrem", "tri")
    assert _chain.out_ptrs({}) == (None,) * 5
    from lidar_transfer_amd import _lib
    assert _chain.TRACE_FLAGS == _lib.LT_TRACE_WRITE_MISSES | _lib.LT_TRACE_LABEL_IMAGE


def test_mount_of_nothing_is_no_mounting():
    out = dict(endpoints=torch.zeros((4, 3)), tri=None)
    for t in (None, [], IDENTITY, np.eye(4)):
        m = _chain.Mount(t)
        assert m.pair is None and m.T is None and m.P is None and m.origin == (0.0, 0.0, 0.0)
        assert m.render_into(out, 4, "cpu") is out
        m.to_target(out, out, None)                                          # (nothing to launch: touches no library)


def test_mount_of_the_example_approach():
    from lidar_transfer_amd.config import load_approach
    t = load_approach(os.path.join(ROOT, "config", "approach_mount_example.yaml")).transformation
    m = _chain.Mount(t)
    T = np.array(t, dtype=np.float64).reshape(4, 4)
    assert np.array_equal(m.T, T) and m.T.dtype == np.float64 and m.T.flags["C_CONTIGUOUS"]
    assert np.array_equal(m.P, np.linalg.inv(T)) and m.pair[0] is not None
    want = np.linalg.inv(T)[:3, 3].astype(np.float32)
    assert np.array_equal(np.array(m.origin, dtype=np.float32), want) and all(isinstance(x, float) for x in m.origin)
    assert np.array_equal(_chain.Mount(m.pair).T, T)                         # (a pair handed on, as the pipeline does)
    none = dict(range=torch.zeros(4), endpoints=None)
    assert m.render_into(none, 4, "cpu") is none                             # no end points wanted: nothing to transform
    out = dict(endpoints=torch.zeros((4, 3)), range=torch.zeros(4))
    rout = m.render_into(out, 4, "cpu")
    assert rout is not out and rout["range"] is out["range"] and "tri" not in out
    assert rout["endpoints"].shape == (4, 3) and rout["endpoints"].data_ptr() != out["endpoints"].data_ptr()
    assert rout["tri"].dtype == torch.int32 and rout["tri"].shape == (4,)    # the hit triangle is forced
    tri = torch.zeros(4, dtype=torch.int32)
    assert m.render_into(dict(out, tri=tri), 4, "cpu")["tri"] is tri


# ---- _chain.Sensing: who is called, once, in which order, with what -------------------------------------------------------
N, S, T_H = 6, 3, 2
MOUNT = [1, 0, 0, 1, 0, 1, 0, 2, 0, 0, 1, 3, 0, 0, 0, 1]                     # a translation: rigid, not the identity


class _RaySet:
    """stands in for ``raytracer.RaySet``: keeps what it was made with, counts ``close``"""

    def __init__(self, rays, H, pose=None, grid=None):
        self.rays, self.H, self.pose, self.grid, self.closed = rays, H, pose, grid, 0

    def close(self):
        self.closed += 1


@pytest.fixture
def fakes(monkeypatch):
    """``post``'s four wrappers replaced by fakes that record ``(name, args, kwargs)`` and return their result keys; the
    sub-rays and the ray set over them replaced by stand-ins; every ``torch.empty`` / ``empty_like`` recorded"""
    from lidar_transfer_amd import post, raytracer
    calls, allocs = [], []

    def fake(name, keys):
        def f(*args, **kw):
            calls.append((name, args, kw))
            return {k: object() for k in keys}
        return f
    monkeypatch.setattr(post, "echo_resolve", fake("resolve", _chain.Echoes.KEYS))
    monkeypatch.setattr(post, "return_model", fake("return", _chain.Returns.KEYS))
    monkeypatch.setattr(post, "noise_model", fake("noise", _chain.Noise.KEYS))
    monkeypatch.setattr(post, "points_to_frame", fake("frame", ()))
    monkeypatch.setattr(post, "create_subrays", lambda rays, model: rays.repeat(model.subrays, 1))
    monkeypatch.setattr(raytracer, "RaySet", _RaySet)
    empty, empty_like = torch.empty, torch.empty_like

    def recording(make):
        def f(*a, **kw):
            t = make(*a, **kw)
            allocs.append((tuple(t.shape), t.dtype))
            return t
        return f
    monkeypatch.setattr(torch, "empty", recording(empty))
    monkeypatch.setattr(torch, "empty_like", recording(empty_like))
    return calls, allocs


def _models():
    from lidar_transfer_amd.config import EchoModel, NoiseModel, ReturnModel
    return ReturnModel(max_range=50.0), NoiseModel(range_sigma=0.01), EchoModel(divergence=0.2, subrays=S)


def _out(tri=False):
    out = dict(endpoints=torch.zeros((N, 3)), endcolors=torch.zeros(N, dtype=torch.int32), range=torch.zeros(N),
               endrem=torch.zeros(N))
    if tri:
        out["tri"] = torch.zeros(N, dtype=torch.int32)
    return out


def _tri_images(allocs):
    return [a for a in allocs if a == ((N,), torch.int32)]


def test_sensing_with_nothing_on_hands_back_what_it_is_given(fakes):
    calls, allocs = fakes
    from lidar_transfer_amd.config import EchoModel, NoiseModel, ReturnModel
    for models in ((None, None, None), (ReturnModel(), NoiseModel(), EchoModel(subrays=4))):   # (all-default, off: none)
        s = _chain.Sensing(IDENTITY, *models, "test").bind(torch.ones((N, 3)), T_H)
        assert not s.returns and not s.noise and not s.echoes and s.mount is None and s.P is None
        assert s.origin == (0.0, 0.0, 0.0) and s.keys == () and not s.needs_scan_index
        out, plain = _out(), object()
        rout, sub = s.plan(out, N, "cpu")
        assert rout is out and sub is out
        assert s.render_set(plain) is plain
        assert s.finish(out, rout, sub, None, object(), torch.ones((N, 3)), s.origin, None) == {}
        s.close()
    assert calls == [] and allocs == []


def test_sensing_with_everything_on_calls_each_once_in_order(fakes):
    calls, allocs = fakes
    returns, noise, echoes = _models()
    rays = torch.arange(3 * N, dtype=torch.float32).reshape(N, 3)
    s = _chain.Sensing(MOUNT, returns, noise, echoes, "test").bind(rays, T_H, grid=(8, 4))
    assert (s.returns.model, s.noise.model, s.echoes.model) == (returns, noise, echoes) and s.noise.gate is returns
    assert s.mount is s.mounting.pair and s.P is s.mounting.P and s.origin == (-1.0, -2.0, -3.0)
    assert s.keys == ("incidence", "drop", "range_error", "noise_state", "n_echoes", "echo_fraction") and s.needs_scan_index
    subset = s.render_set(object())
    assert isinstance(subset, _RaySet) and subset.H == S * T_H and subset.rays.shape == (S * N, 3) and subset.pose is s.P
    assert subset.grid == _chain.Echoes.grid_of((8, 4), T_H)
    del allocs[:]
    out = _out()
    rout, sub = s.plan(out, N, "cpu")
    assert "tri" not in out and rout["tri"].dtype == torch.int32 and rout["tri"].shape == (N,)
    assert rout["endpoints"] is not out["endpoints"] and rout["endpoints"].shape == (N, 3)
    assert all(rout[k] is out[k] for k in ("endcolors", "range", "endrem"))
    assert sub["endpoints"] is None and set(sub) == set(_chain.OUT_KEYS)
    assert {k: (sub[k].numel(), sub[k].dtype) for k in _chain.Echoes.SUB_KEYS} == dict(
        endcolors=(S * N, torch.int32), range=(S * N, torch.float32), endrem=(S * N, torch.float32), tri=(S * N, torch.int32))
    assert len(_tri_images(allocs)) == 1 and len(allocs) == 6                # end points, ONE tri, four sub-images
    scene, stream, origin = object(), object(), (0.5, 0.25, -1.0)
    seen = s.finish(out, rout, sub, 7, scene, rays, origin, stream, label_image=False)
    assert tuple(seen) == ("n_echoes", "echo_fraction", "incidence", "drop", "range_error", "noise_state")
    assert [c[0] for c in calls] == ["resolve", "return", "noise", "frame"]
    (_, a, kw), = [c for c in calls if c[0] == "resolve"]
    assert a[0] is rays and a[1] == origin and a[2] is echoes and a[3] is sub and a[4] is rout and kw == dict(stream=stream)
    (_, a, kw), = [c for c in calls if c[0] == "return"]
    assert a[0] is scene and a[1] is rays and a[2] is returns and a[3] == 7 and a[4] is rout
    assert kw == dict(label_image=False, stream=stream)
    (_, a, kw), = [c for c in calls if c[0] == "noise"]
    assert a[0] == origin and a[1] is noise and a[2] == 7 and a[3] is rout
    assert kw["gate"] is returns and kw["label_image"] is False and kw["stream"] is stream and len(kw) == 3
    (_, a, kw), = [c for c in calls if c[0] == "frame"]
    assert a[0] is rout["endpoints"] and a[1] is s.mounting.T
    assert kw["tri"] is rout["tri"] and kw["out"] is out["endpoints"] and kw["stream"] is stream and len(kw) == 3
    with pytest.raises(ValueError, match="a return model needs the output scan's index"):
        s.finish(out, rout, sub, None, scene, rays, origin, stream)


@pytest.mark.parametrize("which", ["mount", "returns", "noise", "echoes"])
def test_sensing_with_one_model_calls_only_its_own(fakes, which):
    calls, allocs = fakes
    returns, noise, echoes = _models()
    args = dict(mount=(MOUNT, None, None, None), returns=(None, returns, None, None), noise=(None, None, noise, None),
                echoes=(None, None, None, echoes))[which]
    rays = torch.ones((N, 3))
    s = _chain.Sensing(*args, "test").bind(rays, T_H)
    assert s.keys == dict(mount=(), returns=_chain.Returns.KEYS, noise=_chain.Noise.KEYS, echoes=_chain.Echoes.KEYS)[which]
    assert s.needs_scan_index == (which in ("returns", "noise"))
    for tri in (False, True):                                                # the caller's images without and with ``tri``
        del calls[:], allocs[:]
        out = _out(tri)
        rout, sub = s.plan(out, N, "cpu")
        assert len(_tri_images(allocs)) == (0 if tri else 1)
        assert (rout is out) == tri or which == "mount"
        assert (sub is rout) == (which != "echoes")
        seen = s.finish(out, rout, sub, 3, object(), rays, s.origin, None)
        assert [c[0] for c in calls] == [dict(mount="frame", returns="return", noise="noise", echoes="resolve")[which]]
        assert tuple(seen) == s.keys
    s.close()


def test_sensing_made_from_a_bound_echoes_shares_the_set_and_does_not_close_it(fakes):
    _, _, echoes = _models()
    owner = _chain.Sensing(None, None, None, echoes, "test").bind(torch.ones((N, 3)), T_H)
    subset = owner.echoes.rayset
    shared = _chain.Sensing(None, None, None, owner.echoes, "test").bind(torch.ones((N, 3)), T_H)   # (bound already: no-op)
    assert shared.echoes.model is echoes and shared.render_set(object()) is subset and shared.echoes.subrays is owner.echoes.subrays
    shared.close()
    assert subset.closed == 0 and owner.render_set(object()) is subset
    owner.close()
    assert subset.closed == 1 and owner.echoes.rayset is None
    with pytest.raises(RuntimeError, match="an echo model needs its sub-ray set"):
        owner.render_set(object())


def test_sensing_validates_as_the_four_constructors_do():
    returns, noise, echoes = _models()
    for args, text in (((None, noise, None, None), "DeviceDeform: returns= takes a lidar_transfer_amd.config.ReturnModel"),
                       ((None, None, returns, None), "DeviceDeform: noise= takes a lidar_transfer_amd.config.NoiseModel"),
                       ((None, None, None, noise), "DeviceDeform: echoes= takes a lidar_transfer_amd.config.EchoModel")):
        with pytest.raises(ValueError, match=text):
            _chain.Sensing(*args, "DeviceDeform")
    with pytest.raises(ValueError):
        _chain.Sensing([2, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1], None, None, None, "DeviceDeform")   # not rigid
