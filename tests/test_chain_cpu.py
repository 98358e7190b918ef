"""``lidar_transfer_amd._chain``: what the chain layer hands the library's device entry points -- the merged cloud, the
``lt_cloud`` and beam tables, the output pointers and the target sensor's mounting -- on CPU tensors, without the library."""
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
