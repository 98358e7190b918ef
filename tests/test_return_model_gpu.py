"""The target sensor's return model on the GPU.  `lt_return_model_dev` through the C ABI into sentinel-filled
buffers with guards, bit for bit against the numpy restatement of tests/return_cases.py (pinned without a GPU by
tests/test_return_model_cpu.py); then the chains -- `DeviceDeform`, `FusionScanPipeline`, `SequenceTransfer`, the CLI -- against
the same call without a model followed by the restatement on its outputs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import beam_cases as bc  # noqa: E402
import mount_common as mc  # noqa: E402
import return_cases as rc  # noqa: E402
import test_evaluate_cpu as ev  # noqa: E402
import test_ingest_cpu as cpu  # noqa: E402
import test_mount_gpu as tm  # noqa: E402
import test_sequence_cpu as sq  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, FILL = 1024, 0xA5
LT_OK, LT_ERR_INVALID_ARG, LT_ERR_BAD_INDEX = 0, -1, -4
SHIPPED = os.path.join(ROOT, "config", "vlp32c_table_returns_1024.yaml")
IMAGES = ("endpoints", "endcolors", "range", "endrem", "tri")
H0, W0 = rc.SHAPES[-1]                     # the rendered scan every kernel case takes its cells from: 16 x 130
POSE = mc.POSE_GENERAL


def _L():
    from lidar_transfer_amd import _lib
    return _lib


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class Buf:
    """the bytes of a host array on the device between two guards of 1024 bytes, everything else 0xA5"""

    def __init__(self, a=None, nbytes=0):
        import torch
        self.n = a.nbytes if a is not None else nbytes
        h = np.full(self.n + 2 * GUARD, FILL, np.uint8)
        if a is not None:
            h[GUARD:GUARD + self.n] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.t = torch.from_numpy(h).cuda()
        self.ptr = self.t.data_ptr() + GUARD

    def host(self, dtype, shape=(-1,)):
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == FILL).all() and (h[GUARD + self.n:] == FILL).all(), "a guard was overwritten"
        return h[GUARD:GUARD + self.n].view(dtype).reshape(shape).copy()


# ---- the scene and its rendered scans (made once) -------------------------------------------------------------------------------
_S = {}


def _scene():
    """a street scene of ~3 000 triangles plus ONE degenerate face (its last: two equal corners, nn == 0) which no ray hits"""
    if "scene" not in _S:
        import torch
        from lidar_transfer_amd.raytracer import Scene
        from lidar_transfer_amd.synth import synth_scene
        v, f, c, r = synth_scene(3, 3000)
        f = np.ascontiguousarray(np.concatenate([f, np.array([[f[0, 0], f[0, 0], f[0, 1]]], np.int32)]))
        assert f.shape[0] <= 6000
        sc = Scene(0)
        dev = [torch.from_numpy(x).cuda() for x in (v, f, c, r)]
        sc.set_mesh(*dev)
        _S.update(scene=sc, mesh=(v, f, c, r), dev=dev)
    return _S["scene"], _S["mesh"]


def _rendered(label=True, posed=False):
    """the 16 x 130 scan of the scene (fov 30 .. -25: hits on ground and walls from 3 m on, misses above the roofs), all on
    the host: rays, the five images, and what the restatement says about every cell's cosine"""
    key = ("scan", label, posed)
    if key not in _S:
        import torch
        from lidar_transfer_amd.laserscan import create_rays_device
        from lidar_transfer_amd.raytracer import RaySet
        sc, (v, f, _, _) = _scene()
        P = POSE if posed else None
        d_rays = create_rays_device(30.0, -25.0, H0, W0, rot=P[:3, :3] if posed else None)
        rs = RaySet(d_rays, H0, pose=P)
        out = sc.render(rs, mc.origin_of(P) if posed else (0.0, 0.0, 0.0), label_image=label)
        torch.cuda.synchronize()
        sc.status()
        case = {k: out[k].cpu().numpy() for k in IMAGES}
        case["rays"] = d_rays.cpu().numpy()
        rs.close()
        hit = case["tri"] >= 0
        assert 0.5 * hit.size < hit.sum() < hit.size - 100, "the scan needs many hits and a hundred misses"
        assert (case["tri"] != f.shape[0] - 1).all()
        case["cos"] = rc.restate(rc.params(), 0, case["rays"], v, f, case["tri"], case["range"])["cos"]
        _S[key] = case
    return _S[key]


def _cells(case, sel):
    return {k: np.ascontiguousarray(a[sel]) for k, a in case.items()}


def _subset(case, n, seed=0):
    """``n`` cells of the scan in a fixed shuffled order: hits and misses side by side in every wave"""
    return _cells(case, np.random.default_rng(seed).permutation(H0 * W0)[:n])


def call_model(case, p, scan, nulls=(), label=True, stream=None, model_args=None, scene=None, n=None):
    """one lt_return_model_dev call on copies of the case's images; returns (rc, dict of the buffers afterwards, the Bufs)"""
    import torch
    L = _L()
    sc = scene if scene is not None else _scene()[0]
    n = len(case["tri"]) if n is None else n
    bufs = {k: Buf(case[k]) for k in IMAGES if k not in nulls}
    bufs["rays"] = Buf(case["rays"])
    if "incidence" not in nulls:
        bufs["incidence"] = Buf(nbytes=4 * len(case["tri"]))
    if "drop" not in nulls:
        bufs["drop"] = Buf(nbytes=len(case["tri"]))
    a = model_args if model_args is not None else L.ReturnModelArgs(p["min_range"], p["max_range"], p["min_cos"], p["drop_threshold"],
                                                                     p["seed"], L.LT_RETURN_LAMBERT if p["lambert"] else 0)
    torch.cuda.current_stream().synchronize()           # the buffers are in place before a side stream reads them
    st = stream if stream is not None else torch.cuda.current_stream()
    ptr = lambda k: bufs[k].ptr if k in bufs else None   # noqa: E731
    ret = L.load().lt_return_model_dev(sc._h, ptr("rays"), n, C.byref(a), scan, ptr("endpoints"), ptr("endcolors"), ptr("range"),
                                       ptr("endrem"), ptr("tri"), ptr("incidence"), ptr("drop"),
                                       L.LT_TRACE_LABEL_IMAGE if label else 0, C.c_void_p(st.cuda_stream))
    st.synchronize()
    types = dict(endpoints=np.float32, endcolors=np.int32, range=np.float32, endrem=np.float32, tri=np.int32, rays=np.float32,
                 incidence=np.float32, drop=np.uint8)
    got = {k: b.host(types[k]) for k, b in bufs.items()}
    return ret, got


def check(case, p, scan, tag, nulls=(), label=True, stream=None):
    """the call equals the restatement bit for bit in every image it was given; returns the restatement"""
    _, (v, f, _, _) = _scene()
    ret, got = call_model(case, p, scan, nulls, label, stream)
    assert ret == LT_OK, (tag, _L().load().lt_last_error())
    opt = {k: (case[k] if k not in nulls else None) for k in ("endrem", "endpoints", "endcolors")}
    want = rc.restate(p, scan, case["rays"], v, f, case["tri"], case["range"], **opt)
    assert np.array_equal(got["rays"], case["rays"].reshape(-1)), (tag, "the rays were written")
    for k in ("drop", "incidence") + IMAGES:
        if k in nulls:
            continue
        bad = np.nonzero(_bits(got[k]).reshape(-1) != _bits(want[k]).reshape(-1))[0]
        assert bad.size == 0, f"{tag}: {k} differs in {bad.size} elements, first at {bad[0]}: {got[k].reshape(-1)[bad[0]]!r} " \
                              f"against {want[k].reshape(-1)[bad[0]]!r}"
    return want


def _tight(case, **kw):
    """thresholds from the scan itself: each rule takes about a fifth of what reaches it"""
    hit = case["tri"] >= 0
    r, c = case["range"][hit].astype(np.float64), case["cos"][hit]
    p = dict(min_range=np.quantile(r, 0.2), max_range=np.quantile(r, 0.8), min_cos=np.quantile(c, 0.3), drop_threshold=int(0.25 * 2 ** 32),
             seed=11, lambert=True)
    p.update(kw)
    return rc.params(**p)


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rc.SHAPES)
def test_every_ray_count_equals_the_restatement(shape):
    n = shape[0] * shape[1]
    base = _rendered()
    case = _subset(base, n) if n < H0 * W0 else base
    want = check(case, _tight(base), 3, f"n={n}")
    if n == H0 * W0:
        assert set(rc.totals(want["drop"])[k] > 0 for k in range(6)) == {True}, rc.totals(want["drop"])
    check(case, rc.params_of(_shipped()), 3, f"n={n}, the shipped model")


def _shipped():
    from lidar_transfer_amd.config import load_sensor
    return load_sensor(SHIPPED).return_model()


def test_all_cells_miss_and_all_cells_hit():
    base = _rendered()
    rs = np.random.default_rng(5)
    miss = _cells(base, rs.choice(np.nonzero(base["tri"] < 0)[0], 300))
    want = check(miss, _tight(base), 0, "all miss")
    assert rc.totals(want["drop"]) == [0, 300, 0, 0, 0, 0] and (want["incidence"] == -1).all()
    hit = _cells(base, rs.choice(np.nonzero(base["tri"] >= 0)[0], 700))
    want = check(hit, _tight(base), 0, "all hit")
    assert rc.totals(want["drop"])[1] == 0 and min(rc.totals(want["drop"])[2:]) > 0
    want = check(hit, rc.params(), 0, "all hit, a model that drops nothing")
    assert rc.totals(want["drop"]) == [700, 0, 0, 0, 0, 0]
    for k in ("range", "endrem", "tri"):
        assert np.array_equal(_bits(want[k]), _bits(hit[k]))


@pytest.mark.parametrize("rule", ["min_range", "max_range", "min_cos", "drop_threshold"])
def test_each_rule_alone(rule):
    base = _rendered()
    t = _tight(base)
    want = check(base, rc.params(**{rule: t[rule]}, seed=5), 2, rule)
    code = dict(min_range=2, max_range=3, min_cos=4, drop_threshold=5)[rule]
    tot = rc.totals(want["drop"])
    assert tot[code] > 100 and tot[0] > 100 and sum(tot) == tot[0] + tot[1] + tot[code], tot


def test_all_rules_together_keep_the_priority_of_the_codes():
    base = _rendered()
    hit = base["tri"] >= 0
    r, c = base["range"].astype(np.float64), base["cos"]
    # thresholds under which MANY cells break several rules at once: near AND grazing, far AND grazing, and every fourth
    p = rc.params(min_range=np.quantile(r[hit], 0.4), max_range=np.quantile(r[hit], 0.6), min_cos=np.quantile(c[hit], 0.7),
                  drop_threshold=int(0.5 * 2 ** 32), seed=3, lambert=True)
    want = check(base, p, 9, "all rules")
    h = rc.hash32(3, 9, np.arange(hit.size)) < np.uint64(p["drop_threshold"])
    near, far, graze = hit & (r < p["min_range"]), hit & (r > p["max_range"]), hit & (c < p["min_cos"])
    assert (near & graze & h).sum() > 20 and (far & graze & h).sum() > 20 and (graze & h & ~near & ~far).sum() > 5
    d = want["drop"]
    assert (d[near] == 2).all() and (d[far] == 3).all() and (d[graze & ~near & ~far] == 4).all()
    assert (d[hit & h & ~near & ~far & ~graze] == 5).all() and (d[~hit] == 1).all() and (d == 0).sum() > 20


def test_a_cell_exactly_at_a_threshold_is_kept():
    base = _rendered()
    hit = np.nonzero(base["tri"] >= 0)[0]
    r, c = base["range"].astype(np.float64), base["cos"]
    steep = hit[c[hit] >= np.median(c[hit])]              # the three cells come from the steeper half, so that each is kept
    order = steep[np.argsort(r[steep])]
    k_lo, k_hi = order[len(order) // 3], order[2 * len(order) // 3]
    inside = steep[(r[steep] >= r[k_lo]) & (r[steep] <= r[k_hi])]
    k_c = inside[np.argmin(c[inside])]
    p = rc.params(min_range=r[k_lo], max_range=r[k_hi], min_cos=c[k_c])
    want = check(base, p, 0, "at the thresholds")
    assert want["drop"][k_lo] == 0 and want["drop"][k_hi] == 0 and want["drop"][k_c] == 0
    tot = rc.totals(want["drop"])
    assert tot[2] > 100 and tot[3] > 100 and tot[4] > 50, tot
    # one float64 step inside each threshold and the three cells go
    p2 = rc.params(min_range=np.nextafter(r[k_lo], np.inf), max_range=np.nextafter(r[k_hi], -np.inf), min_cos=np.nextafter(c[k_c], np.inf))
    w2 = check(base, p2, 0, "a step inside the thresholds")
    assert (w2["drop"][k_lo], w2["drop"][k_hi], w2["drop"][k_c]) == (2, 3, 4)


@pytest.mark.parametrize("lambert", [False, True])
def test_lambert_on_and_off(lambert):
    base = _rendered()
    want = check(base, _tight(base, lambert=lambert), 1, f"lambert={lambert}")
    kept = want["drop"] == 0
    if lambert:
        assert (want["endrem"][kept] <= base["endrem"][kept]).all() and (want["endrem"][kept] != base["endrem"][kept]).sum() > 100
    else:
        assert np.array_equal(_bits(want["endrem"][kept]), _bits(base["endrem"][kept]))


def test_both_colour_layouts():
    rgb = _rendered(label=False)
    assert rgb["endcolors"].shape == (H0 * W0, 3)
    want = check(rgb, _tight(rgb), 4, "endcolors [n, 3]", label=False)
    gone = want["drop"] >= 2
    assert not want["endcolors"][gone].any() and want["endcolors"][want["drop"] == 0].any()
    assert np.array_equal(rgb["endcolors"][:, 2], _rendered()["endcolors"])
    check(_subset(rgb, 185), _tight(rgb), 4, "endcolors [185, 3]", label=False)


@pytest.mark.parametrize("null", ["endpoints", "endcolors", "endrem", "incidence", "drop", "all five"])
def test_every_optional_image_may_be_null(null):
    base = _rendered()
    nulls = ("endpoints", "endcolors", "endrem", "incidence", "drop") if null == "all five" else (null,)
    check(base, _tight(base), 6, f"NULL {null}", nulls=nulls)
    check(_subset(base, 65), _tight(base), 6, f"NULL {null}, 65 cells", nulls=nulls)


def test_a_degenerate_face_has_cosine_zero():
    base = _rendered()
    _, (v, f, _, _) = _scene()
    case = _subset(base, 185, seed=2)
    hit = np.nonzero(case["tri"] >= 0)[0]
    assert len(hit) > 40
    case["tri"][hit[::2]] = f.shape[0] - 1               # a hand-made tri: every other hit lies on the degenerate face
    want = check(case, rc.params(lambert=True), 0, "degenerate, min_cos 0")
    on = np.zeros(185, bool)
    on[hit[::2]] = True
    assert (want["drop"][on] == 0).all() and (want["incidence"][on] == 0).all() and (want["endrem"][on] == 0).all()
    want = check(case, rc.params(min_cos=1e-300), 0, "degenerate, min_cos above 0")
    assert (want["drop"][on] == 4).all() and (want["drop"][hit[1::2]] == 0).all()


def test_posed_rays():
    posed = _rendered(posed=True)
    plain = _rendered()
    assert not np.array_equal(posed["rays"], plain["rays"]) and not np.array_equal(posed["tri"], plain["tri"])
    want = check(posed, _tight(posed), 8, "posed rays")
    assert min(rc.totals(want["drop"])) > 0


def test_a_side_stream():
    import torch
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    base = _rendered()
    check(base, _tight(base), 12, "side stream", stream=s)


def test_a_tri_beside_the_mesh_is_the_deferred_error_and_reads_nothing():
    sc, (v, f, _, _) = _scene()
    sc.status()
    base = _rendered()
    case = _subset(base, 185, seed=4)
    bad = np.array([f.shape[0], f.shape[0] + 5, 2 ** 31 - 1, -2, -2 ** 31, 10 ** 9], np.int32)
    at = np.arange(3, 3 + 7 * len(bad), 7)
    case["tri"][at] = bad
    want = check(case, _tight(base), 0, "tri beside the mesh")
    assert (want["drop"][at] == 1).all() and np.array_equal(want["tri"][at], bad)
    with pytest.raises(RuntimeError, match=f"status {LT_ERR_BAD_INDEX}"):
        sc.status()
    sc.status()                                           # (the flag is read once)
    check(case, _tight(base), 0, "once more: the scene still works")
    with pytest.raises(RuntimeError):
        sc.status()


def test_a_face_whose_vertices_lie_beside_the_mesh_is_the_deferred_error_too():
    """a scene of its own whose mesh was never rendered: face 1 names vertex 4 of 4, face 2 vertex -1"""
    import torch
    from lidar_transfer_amd.raytracer import Scene
    v = np.array([[5, -1, -1], [5, 1, -1], [5, 0, 1], [6, 0, 1]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 4], [-1, 1, 2], [1, 2, 3]], np.int32)
    dev = [torch.from_numpy(x).cuda() for x in (v, f, np.zeros((4, 3), np.int32), np.zeros(4, np.float32))]
    sc = Scene(0)
    sc.set_mesh(*dev)
    n = 70
    case = dict(rays=np.tile(np.array([[1, 0, 0]], np.float32), (n, 1)), tri=(np.arange(n) % 4).astype(np.int32),
                range=np.full(n, 5, np.float32), endrem=np.full(n, 0.5, np.float32), endpoints=np.ones((n, 3), np.float32),
                endcolors=np.full(n, 7, np.int32))
    p = rc.params(min_cos=0.9, lambert=True)
    ret, got = call_model(case, p, 0, scene=sc)
    assert ret == LT_OK
    want = rc.restate(p, 0, case["rays"], v, f, case["tri"], case["range"], case["endrem"], case["endpoints"], case["endcolors"])
    assert want["drop"][:4].tolist() == [0, 1, 1, 4]
    for k in ("drop", "incidence") + IMAGES:
        assert np.array_equal(_bits(got[k]).reshape(-1), _bits(want[k]).reshape(-1)), k
    with pytest.raises(RuntimeError, match=f"status {LT_ERR_BAD_INDEX}"):
        sc.status()
    sc.close()


def test_bad_arguments_are_refused_with_a_message():
    L = _L()
    lib = L.load()
    base = _subset(_rendered(), 64)
    ok = rc.params()
    for tag, kw in (("tri", dict(nulls=("tri",))), ("range", dict(nulls=("range",))), ("n", dict(n=-1))):
        ret, _ = call_model(base, ok, 0, **kw)
        assert ret == LT_ERR_INVALID_ARG and b"lt_return_model_dev" in lib.lt_last_error(), tag
    for tag, a in (("min > max", (5.0, 4.0, 0.0, 0, 0, 0)), ("min < 0", (-1.0, 4.0, 0.0, 0, 0, 0)), ("nan", (float("nan"), 4.0, 0.0, 0, 0, 0)),
                   ("max nan", (0.0, float("nan"), 0.0, 0, 0, 0)), ("cos > 1", (0.0, 4.0, 1.5, 0, 0, 0)), ("cos < 0", (0.0, 4.0, -0.1, 0, 0, 0)),
                   ("cos nan", (0.0, 4.0, float("nan"), 0, 0, 0)), ("flags", (0.0, 4.0, 0.0, 0, 0, 2))):
        ret, got = call_model(base, ok, 0, model_args=L.ReturnModelArgs(*a))
        assert ret == LT_ERR_INVALID_ARG and b"lt_return_model_dev" in lib.lt_last_error(), tag
        assert (got["drop"] == FILL).all() and np.array_equal(got["tri"], base["tri"]), tag
    sc = _scene()[0]
    b = Buf(base["tri"])
    a = L.ReturnModelArgs(0.0, 1.0, 0.0, 0, 0, 0)
    assert lib.lt_return_model_dev(None, b.ptr, 64, C.byref(a), 0, None, None, b.ptr, None, b.ptr, None, None, 0, None) == LT_ERR_INVALID_ARG
    assert lib.lt_return_model_dev(sc._h, b.ptr, 64, None, 0, None, None, b.ptr, None, b.ptr, None, None, 0, None) == LT_ERR_INVALID_ARG
    assert lib.lt_return_model_dev(sc._h, None, 64, C.byref(a), 0, None, None, b.ptr, None, b.ptr, None, None, 0, None) == LT_ERR_INVALID_ARG
    assert lib.lt_return_model_dev(sc._h, None, 0, C.byref(a), 0, None, None, None, None, None, None, None, 0, None) == LT_OK   # no cells


def test_the_wrapper_is_the_entry_point():
    import torch
    from lidar_transfer_amd import post
    from lidar_transfer_amd.config import ReturnModel
    sc, (v, f, _, _) = _scene()
    base = _rendered()
    m = ReturnModel(4.0, 30.0, 75.0, "lambert", 0.1, 9)
    out = {k: torch.from_numpy(base[k]).cuda() for k in IMAGES}
    more = post.return_model(sc, torch.from_numpy(base["rays"]).cuda(), m, 17, out)
    torch.cuda.synchronize()
    want = rc.restate(rc.params_of(m), 17, base["rays"], v, f, base["tri"], base["range"], base["endrem"], base["endpoints"], base["endcolors"])
    for k in IMAGES:
        assert np.array_equal(_bits(out[k].cpu().numpy()), _bits(want[k])), k
    assert np.array_equal(more["drop"].cpu().numpy(), want["drop"]) and more["drop"].dtype == torch.uint8
    assert np.array_equal(_bits(more["incidence"].cpu().numpy()), _bits(want["incidence"]))
    assert min(rc.totals(want["drop"])) > 0
    only = post.return_model(sc, torch.from_numpy(base["rays"]).cuda(), m, 17, dict(tri=torch.from_numpy(base["tri"]).cuda(),
                                                                                     range=torch.from_numpy(base["range"]).cuda()),
                             incidence=None, drop=True)
    assert only["incidence"] is None and np.array_equal(only["drop"].cpu().numpy(), want["drop"])
    with pytest.raises(ValueError):
        post.return_model(sc, torch.from_numpy(base["rays"]).cuda(), m, 17, dict(range=out["range"]))
    with pytest.raises(ValueError):
        post.return_model(sc, torch.from_numpy(base["rays"]).cuda(), None, 17, out)


# ---- the chains -----------------------------------------------------------------------------------------------------------------
SEQ_TARGET = (32, 171, bc.VLP32C_FOV[0], bc.VLP32C_FOV[1])
TIGHT_BLOCK = dict(min_range=4.6, max_range=8.0, max_incidence=60.0, remission="lambert", drop_rate=0.25, seed=7)
T_EXAMPLE = tm.T_EXAMPLE


def _models():
    """the shipped file's model, and one whose rules bite on the F17 sequence's few metres (its scans' ranges: 1 .. 18 m, the
    middle half between 4.5 and 8 m)"""
    from lidar_transfer_amd.config import ReturnModel
    return dict(shipped=_shipped(), tight=ReturnModel(**TIGHT_BLOCK))


def _bites(tot):
    """kept cells, a range rule, the incidence rule and the random rule all took part"""
    return tot[0] > 0 and tot[2] + tot[3] > 0 and tot[4] > 0 and tot[5] > 0


def _host(out, mesh=None):
    """what the restatement needs of a chain's result, on the host (copies: the chain reuses its buffers)"""
    import torch
    torch.cuda.synchronize()
    h = {k: out[k].cpu().numpy().copy() for k in ("range", "rem", "label", "endpoints", "endpoints_scene", "tri", "bin", "label_file",
                                                 "incidence", "drop") if k in out}
    if mesh is not None:
        h["mesh"] = [t.cpu().numpy().copy() for t in mesh.tensors()]
    return h


def _expect(base, model, scan, rays):
    """the model restated on a result ``base`` made WITHOUT it: images, incidence, drop and the bytes write() packs.  The end
    points: a dropped cell is (0, 0, 0) in the scene's frame and in the target's (a miss is not transformed), a kept one is
    the base run's."""
    import oracle_chain as oc
    v, f = base["mesh"][0], base["mesh"][1]
    n = base["tri"].shape[0]
    w = rc.restate(rc.params_of(model), scan, rays, v, f, base["tri"], base["range"].reshape(-1), base["rem"].reshape(-1),
                   base["endpoints_scene"], base["label"].reshape(-1))
    gone = w["drop"] >= 2
    w["endpoints_target"] = np.where(gone[:, None], np.float32(0), base["endpoints"].reshape(n, 3)).astype(np.float32)
    w["bin"], w["label_file"] = oc.pack_write(w["endpoints_target"], w["endcolors"], w["endrem"])
    return w


def _check_result(got, w, tag):
    pairs = (("range", "range"), ("rem", "endrem"), ("label", "endcolors"), ("tri", "tri"), ("endpoints_scene", "endpoints"),
             ("endpoints", "endpoints_target"), ("incidence", "incidence"), ("drop", "drop"))
    for gk, wk in pairs:
        assert np.array_equal(_bits(got[gk]).reshape(-1), _bits(w[wk]).reshape(-1)), (tag, gk)
    if "bin" in got:
        assert got["bin"].tobytes() == w["bin"].tobytes(), (tag, "velodyne bytes")
        assert got["label_file"].view(np.uint32).tobytes() == w["label_file"].astype(np.uint32).tobytes(), (tag, "label bytes")


@pytest.mark.parametrize("mounted", [False, True])
@pytest.mark.parametrize("adaption", ["mesh", "mergemesh"])
def test_device_deform_with_a_model_is_the_plain_call_followed_by_the_restatement(adaption, mounted):
    """with the shipped model and with one whose rules all bite; ``mounted``: the example mounting and the VLP-32C table
    combined -- dropped cells are (0, 0, 0) in the target's frame"""
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    g17, g18, a, target = tm._seq_setup(adaption, [])
    kw = dict(transformation=T_EXAMPLE, t_beam_table=bc.VLP32C) if mounted else {}
    if mounted:
        target = SEQ_TARGET
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    indices = [int(x) for x in a.scan_indices(8)[:2]]
    mk = lambda **more: DeviceDeform(ev.SOURCE, target, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=adaption == "mesh",   # noqa: E731
                                     **kw, **more)
    with mk() as plain:
        rays = plain.rayset.rays.cpu().numpy()
        base = []
        for idx in indices:
            out = plain.deform(adaption, ing, idx)
            assert "incidence" not in out and "drop" not in out
            base.append(_host(out, plain.mesh_obj))
    for name, model in _models().items():
        with mk(returns=model) as dd:
            assert dd.returns == model
            for idx, b in zip(indices, base):
                got = _host(dd.deform(adaption, ing, idx, scan_index=idx))
                w = _expect(b, model, idx, rays)
                tag = f"{adaption}/{name}/mounted={mounted}/scan {idx}"
                _check_result(got, w, tag)
                tot = rc.totals(w["drop"])
                print(f"\n{tag}: cells per code {tot}, {w['bin'].shape[0]} points written ({b['bin'].shape[0]} without the model)")
                assert w["bin"].shape[0] > 50
                if name == "tight":
                    assert _bites(tot), tot
                    assert w["bin"].shape[0] < b["bin"].shape[0]
                    assert not got["endpoints"][w["drop"] >= 2].any()
            with pytest.raises(ValueError, match="scan_index"):
                dd.deform(adaption, ing, indices[0])
    src.close()


def test_fusion_pipeline_with_three_chains_equals_the_serial_runs_per_scan_index():
    """six output scans (the sequence's, twice over) with scan_index 40 .. 45 on three chains: ``submit_mergemesh`` -- its first
    scan has no geometry to assume and waits -- and ``submit_clouds``, against one DeviceDeform scan after scan"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.pipeline import FusionScanPipeline
    model = _models()["tight"]
    g17, g18, a, target = tm._seq_setup("mergemesh", [])
    am = sq.approach_for(g18, "mesh")
    src = tm._source(g17)
    rays = create_rays_device(target[2], target[3], target[0], target[1], device=0)
    order = [int(x) for x in a.scan_indices(8)]
    order = (order * 6)[:6]
    keys = ("range", "endrem", "endcolors", "endpoints", "tri", "incidence", "drop")
    host = lambda r: {k: r[k].cpu().numpy().copy() for k in keys}   # noqa: E731
    # mergemesh
    ing = ScanIngest(src, a)
    with FusionScanPipeline(a.voxel_bounds.copy(), a.voxel_size, target[2], target[3], rays, target[0], chains=3, device=0,
                            label_image=True, source_hw=ev.SOURCE[:2], fixed_volume=False, returns=model) as pipe:
        tickets = []
        for k, idx in enumerate(order):
            clouds = ing.prepare(idx, merged=True)
            torch.cuda.synchronize()
            tickets.append(pipe.submit_mergemesh(clouds, inputs_ready=True, scan_index=40 + k))
        got = [host(pipe.wait(t)) for t in tickets]
        stats = dict(pipe._mm_state.stats)
        with pytest.raises(ValueError, match="scan_index"):
            pipe.submit_mergemesh(ing.prepare(order[0], merged=True), inputs_ready=True)
    assert stats["scans"] == 6 and stats["waited"] >= 1, stats
    with DeviceDeform(ev.SOURCE, target, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=False, returns=model) as dd:
        for k, idx in enumerate(order):
            s = dd.mergemesh(ing.prepare(idx, merged=True), pack=False, scan_index=40 + k)
            torch.cuda.synchronize()
            want = dict(range=s["range"], endrem=s["rem"], endcolors=s["label"], endpoints=s["endpoints"], tri=s["tri"],
                        incidence=s["incidence"], drop=s["drop"])
            for key in keys:
                assert np.array_equal(_bits(got[k][key]).reshape(-1), _bits(want[key].cpu().numpy()).reshape(-1)), ("mergemesh", k, key)
            assert _bites(rc.totals(got[k]["drop"])), rc.totals(got[k]["drop"])
    if len(set(order)) < 6:
        assert not np.array_equal(got[0]["drop"], got[len(set(order))]["drop"]), "the same clouds under another scan_index: another pattern"
    # mesh, from clouds
    ingm = ScanIngest(src, am)
    with FusionScanPipeline(am.voxel_bounds.copy(), am.voxel_size, ev.SOURCE[2], ev.SOURCE[3], rays, target[0], chains=3, device=0,
                            label_image=True, source_hw=ev.SOURCE[:2], returns=model) as pipe:
        tickets = []
        for k, idx in enumerate(order):
            clouds = ingm.prepare(idx, merged=False)
            torch.cuda.synchronize()
            tickets.append(pipe.submit_clouds(clouds, inputs_ready=True, scan_index=40 + k))
        got = [host(pipe.wait(t)) for t in tickets]
    with DeviceDeform(ev.SOURCE, target, am.voxel_bounds.copy(), am.voxel_size, returns=model) as dd:
        for k, idx in enumerate(order):
            s = dd.mesh(ingm.prepare(idx, merged=False), pack=False, scan_index=40 + k)
            torch.cuda.synchronize()
            want = dict(range=s["range"], endrem=s["rem"], endcolors=s["label"], endpoints=s["endpoints"], tri=s["tri"],
                        incidence=s["incidence"], drop=s["drop"])
            for key in keys:
                assert np.array_equal(_bits(got[k][key]).reshape(-1), _bits(want[key].cpu().numpy()).reshape(-1)), ("mesh", k, key)
    src.close()


def _target_sensor(block, **kw):
    from lidar_transfer_amd.config import load_sensor
    tH, tW, tfu, tfd = SEQ_TARGET
    cfg = dict(name="VLP-32C table with a return model", fov_up=tfu, fov_down=tfd, beams=tH, angle_res_hor=360.0 / tW, fov_hor=360.0,
               beam_model="table", beam_angles=[float(x) for x in bc.VLP32C])
    if block is not None:
        cfg["return_model"] = block
    cfg.update(kw)
    return load_sensor(cfg)


def _run_sequence(a, target, out_dir, chains):
    from lidar_transfer_amd.sequence import SequenceTransfer
    g17, g18 = cpu.gold(), sq.gold18()
    src = tm._source(g17)
    with SequenceTransfer(src, a, ev.SOURCE, target, out_dir=str(out_dir), chains=chains, nclasses=int(g18["nclasses"])) as tr:
        recs = list(tr.run())
        summary, returns = tr.summary, tr.returns
    src.close()
    return recs, summary, returns


def test_a_sequence_writes_the_restated_files_with_one_chain_and_with_three(tmp_path):
    """the mergemesh sequence with a table target and a return model: every file is write() of the restatement on the plain
    chain's scan of that FILE index; the totals are the restatement's bincount"""
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.sequence import format_return_totals
    g17, g18, a, _ = tm._seq_setup("mergemesh", [])
    sensor = _target_sensor(TIGHT_BLOCK)
    model = sensor.return_model()
    r1, s1, ret1 = _run_sequence(a, sensor, tmp_path / "c1", 1)
    r3, s3, _ = _run_sequence(a, sensor, tmp_path / "c3", 3)
    r0, s0, ret0 = _run_sequence(a, _target_sensor(None), tmp_path / "plain", 1)
    assert ret1 == model and ret0 is None and s0["return_totals"] is None and s3["chains"] == 3
    indices = [r["idx"] for r in r1]
    assert indices == [r["idx"] for r in r3] == [int(x) for x in a.scan_indices(8)] and len(indices) >= 3
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    total = np.zeros(6, np.int64)
    with DeviceDeform(ev.SOURCE, SEQ_TARGET, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=False, t_beam_table=bc.VLP32C) as plain:
        rays = plain.rayset.rays.cpu().numpy()
        for rec in r1:
            idx = rec["idx"]
            w = _expect(_host(plain.deform("mergemesh", ing, idx), plain.mesh_obj), model, idx, rays)
            total += np.array(rc.totals(w["drop"]))
            b1, l1 = tm._read(tmp_path / "c1", idx)
            assert b1 == w["bin"].tobytes(), f"scan {idx}: velodyne file"
            assert l1 == w["label_file"].astype(np.uint32).tobytes(), f"scan {idx}: label file"
            assert rec["n_points"] == w["bin"].shape[0]
            assert (b1, l1) == tm._read(tmp_path / "c3", idx), f"scan {idx}: one chain vs three"
            assert len(tm._read(tmp_path / "plain", idx)[0]) > len(b1), f"scan {idx}: the model dropped nothing"
    src.close()
    assert s1["return_totals"] == s3["return_totals"] == total.tolist() and _bites(total.tolist())
    assert int(total.sum()) == len(indices) * SEQ_TARGET[0] * SEQ_TARGET[1]
    print("\n" + format_return_totals(s1["return_totals"]))


def _write_dataset(tmp_path, adaption="mergemesh"):
    g17, g18, a, _ = tm._seq_setup(adaption, [])
    data = tmp_path / "data"
    seq = data / "sequences" / "00"
    (seq / "velodyne").mkdir(parents=True)
    (seq / "labels").mkdir()
    for k, (xyzr, lab) in enumerate(cpu.raw_scans(g17)):
        xyzr.tofile(seq / "velodyne" / f"{k:06d}.bin")
        lab.tofile(seq / "labels" / f"{k:06d}.label")
    g17["calib_txt"].tofile(seq / "calib.txt")
    g17["poses_txt"].tofile(seq / "poses.txt")
    H, W, fu, fd = ev.SOURCE
    (data / "config.yaml").write_text(f"name: src\nfov_up: {fu}\nfov_down: {fd}\nbeams: {H}\nangle_res_hor: {360.0 / W!r}\nfov_hor: 360.0\n")
    cm = "\n".join(f"  {k}: {list(v)}" for k, v in ev.COLOR_DICT.items())
    cfgs = {}
    for ad in ("mergemesh", "cp"):
        cfgs[ad] = tmp_path / f"approach_{ad}.yaml"
        cfgs[ad].write_text(f"adaption: {ad}\npreserve_float: false\nnumber_of_scans: {a.number_of_scans}\n"
                            f"batch_interval: {a.batch_interval}\nvoxel_size: {a.voxel_size!r}\n"
                            f"voxel_bounds: {[float(x) for x in np.asarray(a.voxel_bounds).reshape(-1)]}\n"
                            f"transformation: []\nignore: {a.ignore}\nmoving: {a.moving}\ncolor_map:\n{cm}\n")
    return data, cfgs, a


def test_the_cli_prints_the_totals_of_the_six_codes(tmp_path):
    """the shipped file through ``python -m lidar_transfer_amd`` in a child process: the closing line's numbers are the bincount of
    the restatement over the run's scans (the plain chain at the shipped file's 32 x 1024, restated); ``cp`` and a source sensor
    with the key end with a message and status 1"""
    import json
    import subprocess
    from lidar_transfer_amd.config import load_sensor
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.sequence import format_return_totals
    data, cfgs, a = _write_dataset(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    log = tmp_path / "log.jsonl"
    base = [sys.executable, "-m", "lidar_transfer_amd", "-d", str(data), "-s", "00"]
    res = subprocess.run(base + ["-c", str(cfgs["mergemesh"]), "-t", SHIPPED, "-w", "-p", str(out), "--log", str(log)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    rows = [json.loads(x) for x in log.read_text().splitlines()]
    sensor = load_sensor(SHIPPED)
    model = sensor.return_model()
    g17 = cpu.gold()
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    total = np.zeros(6, np.int64)
    tgt = (sensor.H, sensor.W, sensor.fov_up, sensor.fov_down)
    with DeviceDeform(ev.SOURCE, tgt, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=False, t_beam_table=sensor.beam_table()) as plain:
        rays = plain.rayset.rays.cpu().numpy()
        for row in rows[:-1]:
            w = _expect(_host(plain.deform("mergemesh", ing, row["idx"]), plain.mesh_obj), model, row["idx"], rays)
            total += np.array(rc.totals(w["drop"]))
            assert tm._read(out, row["idx"])[0] == w["bin"].tobytes(), row["idx"]
    src.close()
    lines = [x for x in res.stdout.splitlines() if x.startswith("Returns:")]
    assert lines == [format_return_totals(total.tolist())], (lines, total)
    assert rows[-1]["summary"]["return_totals"] == total.tolist() and len(rows) >= 4
    # cp renders no surface; a source sensor with the key
    res = subprocess.run(base + ["-c", str(cfgs["cp"]), "-t", SHIPPED], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 1 and "cp renders no surface" in res.stdout
    (data / "config.yaml").write_text((data / "config.yaml").read_text() + "return_model:\n  drop_rate: 0.5\n")
    res = subprocess.run(base + ["-c", str(cfgs["mergemesh"])], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 1 and "return_model is for target sensors only" in res.stdout


@pytest.mark.parametrize("adaption", ["cp", "mesh", "mergemesh"])
def test_without_the_key_and_with_an_all_default_block_nothing_changes(adaption, monkeypatch):
    """no new keys, the bytes of the path without ``returns=``, and the wrapper is never called"""
    import torch
    from lidar_transfer_amd import post
    from lidar_transfer_amd.config import ReturnModel
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    calls = []
    real = post.return_model
    monkeypatch.setattr(post, "return_model", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    g17, g18, a, target = tm._seq_setup(adaption, [])
    sensors = [_target_sensor(None), _target_sensor({}), _target_sensor(dict(ReturnModel.DEFAULTS)),
               _target_sensor(dict(min_range=0.0, max_incidence=90, drop_rate=0, remission="none"))]
    assert all(s.return_model() is None for s in sensors)
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    res = []
    for kw in ({}, dict(returns=None), dict(returns=sensors[1].return_model()), dict(returns=ReturnModel())):
        bnds = None if adaption == "cp" else a.voxel_bounds.copy()
        with DeviceDeform(ev.SOURCE, target, bnds, a.voxel_size, mesh_volume=adaption == "mesh", **kw) as dd:
            assert dd.returns is None and not dd._returns
            outs = []
            for idx in a.scan_indices(8)[:2]:
                out = dd.deform(adaption, ing, idx)
                torch.cuda.synchronize()
                assert "incidence" not in out and "drop" not in out
                outs.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
            res.append(outs)
    for other in res[1:]:
        for x, y in zip(res[0], other):
            tm._same(x, y, adaption)
    assert res[0][0]["bin"].shape[0] > 100
    src.close()
    assert calls == []
    if adaption != "cp":      # (and the wrapper IS what a model goes through)
        src = tm._source(g17)
        with DeviceDeform(ev.SOURCE, target, a.voxel_bounds.copy(), a.voxel_size, mesh_volume=adaption == "mesh",
                          returns=ReturnModel(seed=1)) as dd:
            out = dd.deform(adaption, ScanIngest(src, a), int(a.scan_indices(8)[0]), scan_index=0)
            torch.cuda.synchronize()
            assert rc.totals(out["drop"].cpu().numpy())[2:] == [0, 0, 0, 0]     # (a seed alone drops nothing)
            tm._same({k: v for k, v in out.items() if k not in ("incidence", "drop")}, res[0][0], adaption)
        src.close()
        assert calls == [1]


def test_sequences_without_the_key_write_the_bytes_they_wrote(tmp_path, monkeypatch):
    from lidar_transfer_amd import post
    calls = []
    monkeypatch.setattr(post, "return_model", lambda *a, **k: calls.append(1))
    g17, g18, a, _ = tm._seq_setup("mergemesh", [])
    r0, s0, _ = _run_sequence(a, _target_sensor(None), tmp_path / "none", 1)
    r1, s1, ret = _run_sequence(a, _target_sensor({}), tmp_path / "default", 3)
    r2, s2, _ = _run_sequence(a, SEQ_TARGET, tmp_path / "tuple", 1)      # (a plain tuple has no model; nor the table: other bytes)
    assert ret is None and calls == [] and s0["return_totals"] is None and s1["return_totals"] is None and s2["return_totals"] is None
    for rec in r0:
        assert tm._read(tmp_path / "none", rec["idx"]) == tm._read(tmp_path / "default", rec["idx"])
        assert "incidence" not in rec and "drop" not in rec


def test_cp_with_a_model_raises():
    from lidar_transfer_amd.deform import DeviceDeform
    from lidar_transfer_amd.ingest import ScanIngest
    from lidar_transfer_amd.sequence import SequenceTransfer
    model = _models()["tight"]
    g17, g18, a, target = tm._seq_setup("cp", [])
    src = tm._source(g17)
    ing = ScanIngest(src, a)
    with DeviceDeform(ev.SOURCE, target, None, returns=model) as dd:
        with pytest.raises(ValueError, match="cp renders no surface"):
            dd.deform("cp", ing, int(a.scan_indices(8)[0]))
        with pytest.raises(ValueError, match="cp renders no surface"):
            dd.cp(ing.prepare(int(a.scan_indices(8)[0]), merged=True))
    with pytest.raises(ValueError, match="cp renders no surface"):
        SequenceTransfer(src, a, ev.SOURCE, _target_sensor(TIGHT_BLOCK))
    with pytest.raises(ValueError, match="target sensors only"):
        SequenceTransfer(src, sq.approach_for(g18, "mesh"), _target_sensor(TIGHT_BLOCK, beam_model="linear"), SEQ_TARGET)
    with pytest.raises(ValueError, match="ReturnModel"):
        DeviceDeform(ev.SOURCE, target, None, returns=TIGHT_BLOCK)
    src.close()
