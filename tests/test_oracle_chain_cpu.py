"""The host steps of tests/oracle_chain.py that restate reference code in numpy, against what the reference's own code produced:
``create_rays`` (goldens F1 / F16), ``do_reverse_projection_new`` + ``write()``'s filter and pack (golden F7) and the mergemesh
bounds bookkeeping + volume geometry (the fusion-independent fields of goldens F14 / F14b / F14c: ``vol_dim``, ``vol_origin``,
``bnds_after``).  The GPU tests of the default chain compare the product's bytes with these restatements."""
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import oracle_chain as oc  # noqa: E402


def _gold(name):
    return np.load(os.path.join(GOLD, name))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_oracle_chain_imports_nothing_of_the_product():
    import ast
    tree = ast.parse(open(os.path.join(HERE, "oracle_chain.py")).read())
    names = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names] + \
        [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert not [m for m in names if m.startswith("lidar_transfer_amd")], names


def test_create_rays_restatement_vs_the_reference():
    import pin_cases as pc
    g = _gold("f1_create_rays.npz")
    for case in ("a", "b"):
        fu, fd, H, W = [float(x) for x in g[f"{case}_args"]]
        assert np.array_equal(oc.create_rays(fu, fd, int(H), int(W)).view(np.int32), g[f"{case}_rays"].view(np.int32)), case
    g16 = _gold("f16_live_fuzz.npz")
    for k, (fu, fd, H, W) in enumerate(pc.create_rays_fuzz_cases()):
        assert np.array_equal(pc.array_digest(oc.create_rays(fu, fd, H, W)), g16["rays_sha256"][k]), (fu, fd, H, W)


@pytest.mark.parametrize("pf", [False, True])
def test_reverse_projection_restatement_vs_f7(pf):
    g = _gold("f7_post.npz")
    px = g["proj_x_float"] if pf else g["proj_x"]
    py = g["proj_y_float"] if pf else g["proj_y"]
    got = oc.reverse_projection(g["range_image"], px, py, float(g["fov_up"]), float(g["fov_down"]))
    want = g[f"back_points_{'float' if pf else 'int'}"]
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(got.view(np.int64), want.view(np.int64))     # the same numpy expressions: the same doubles


def test_write_filter_and_pack_restatement_vs_f7():
    g = _gold("f7_post.npz")
    # cp adaption: the reference wrote the files from the preserve_float back-points, index > 0 filter
    b, l = oc.pack_write(g["back_points_float"], g["label_image"], g["proj_remissions"], index=g["index"])
    assert np.array_equal(b.view(np.uint8).reshape(-1), g["cp_bin_bytes"])
    assert np.array_equal(l.view(np.uint8).reshape(-1), g["cp_label_bytes"])
    back = oc.reverse_projection(g["range_image"], g["proj_x_float"], g["proj_y_float"], float(g["fov_up"]), float(g["fov_down"]))
    b2, _ = oc.pack_write(back, g["label_image"], g["proj_remissions"], index=g["index"])
    assert np.array_equal(b2.view(np.uint8).reshape(-1), g["cp_bin_bytes"])
    # mesh adaptions: the images of a raytraced scan (golden F4), no index filter
    g4 = _gold("f4_50k_64x256.npz")
    b, l = oc.pack_write(g4["endpoints"], g4["label"], g4["endrem"])
    assert b.shape[0] == int(g4["n_hits"])
    assert np.array_equal(b.view(np.uint8).reshape(-1), g["mesh_bin_bytes"])
    assert np.array_equal(l.view(np.uint8).reshape(-1), g["mesh_label_bytes"])
    # the filter's corners: (0, 0, 0) and a zero coordinate sum dropped, a negative label dropped
    pts = np.array([[1, 2, 3], [0, 0, 0], [1, -1, 0], [4, 5, 6], [7, 8, 9]], np.float32)
    b, l = oc.pack_write(pts, np.array([10, 40, 40, -1, 50], np.int32), np.arange(5, dtype=np.float32))
    assert np.array_equal(b, np.array([[1, 2, 3, 0], [7, 8, 9, 4]], np.float32)) and l.tolist() == [10, 50]


def _host_render(v, f, c, r, H, W, fu, fd):
    """the reference raytracer's search restated (MODE_REF_BVH, its tie rule; the RSQRTSS seed the goldens were made with)"""
    from oracle import binding as ob
    o = ob.oracle_trace(oc.create_rays(fu, fd, H, W), np.zeros(3, np.float32), v, f, c, r, H, mode=ob.MODE_REF_BVH,
                        norm=ob.NORM_SSE_TABLE, nthreads=oc.THREADS)
    return o["endpoints"], o["endcolors"][:, 2], o["endrem"], o["range"]


def _check_step(bnds, clouds, source, target, voxel, g, tag):
    pts = np.concatenate([c[0] for c in clouds])
    rem = np.concatenate([c[1] for c in clouds])
    lab = np.concatenate([c[2] for c in clouds])
    _, _, _, kept = oc.project(pts, rem, lab, source[0], source[1], target[2], target[3])
    dim, origin, _ = oc.mergemesh_bounds(bnds, kept, voxel)
    assert tuple(dim) == tuple(int(x) for x in g[f"{tag}_vol_dim"]), tag
    assert np.array_equal(bnds, g[f"{tag}_bnds_after"]) and bnds.dtype == g[f"{tag}_bnds_after"].dtype, tag
    if f"{tag}_vol_origin" in g.files:
        assert np.array_equal(origin.view(np.int32), g[f"{tag}_vol_origin"].view(np.int32)), tag


def test_mergemesh_bounds_restatement_vs_f14():
    g = _gold("f14_deform_mergemesh.npz")
    for case in [str(c) for c in g["cases"]]:
        src, tgt = tuple(g[f"{case}_source"]), tuple(g[f"{case}_target"])
        src, tgt = (int(src[0]), int(src[1]), src[2], src[3]), (int(tgt[0]), int(tgt[1]), tgt[2], tgt[3])
        bnds = g[f"{case}_bnds"].copy()
        for step in range(2):
            tag = f"{case}{step}"
            clouds = [(g[f"{tag}_points{k}"], g[f"{tag}_rem{k}"], g[f"{tag}_label{k}"]) for k in range(int(g[f"{case}_n_scans"]))]
            _check_step(bnds, clouds, src, tgt, float(g[f"{case}_voxel"]), g, tag)


def test_mergemesh_bounds_and_mesh_geometry_restatement_vs_f13b_f14b():
    import pin_cases
    g = _gold("f13b_deform_mesh_fuzz.npz")
    n_mm = 0
    for k in range(int(g["n_cases"])):
        adaption, src, tgt, n_scans, bnds, voxel, seeds = pin_cases.deform_mesh_case(k)
        bnds = bnds.copy()
        for step in range(2 if adaption == "mergemesh" else 1):
            tag = f"c{k}s{step}"
            clouds = pin_cases.deform_mesh_clouds(seeds[step], n_scans, src, _host_render)
            assert _sha(np.concatenate([c[0].reshape(-1) for c in clouds])) == str(g[f"{tag}_cloud_sha"]), tag + ": source clouds"
            if adaption == "mesh":
                dim, _ = oc.volume_geometry(bnds.copy(), voxel)
                assert tuple(dim) == tuple(int(x) for x in g[f"{tag}_vol_dim"]), tag
            else:
                _check_step(bnds, clouds, src, tgt, voxel, g, tag)
                n_mm += 1
    assert n_mm >= 8


def test_mergemesh_bounds_restatement_vs_f14c_sequences():
    import pin_cases
    g = _gold("f14c_mergemesh_seq.npz")
    for k in range(int(g["n_cases"])):
        src, tgt, bnds, voxel, seed, limits = pin_cases.mergemesh_seq_case(k)
        bnds = bnds.copy()
        for step, lim in enumerate(limits):
            tag = f"q{k}s{step}"
            clouds = pin_cases.mergemesh_seq_clouds(seed, src, _host_render, lim)
            assert _sha(np.concatenate([c[0].reshape(-1) for c in clouds])) == str(g[f"{tag}_cloud_sha"]), tag
            _check_step(bnds, clouds, src, tgt, voxel, g, tag)


def test_mergemesh_bounds_refuse_an_empty_cloud_and_an_empty_volume():
    b = np.array([[-7, 7], [-7, 7], [-2, 3]])
    with pytest.raises(ValueError):
        oc.mergemesh_bounds(b, np.zeros((0, 3)), 0.1)
    with pytest.raises(ValueError):
        oc.mergemesh_bounds(b, np.array([[0.0, 0.0, 40.0], [1.0, 1.0, 41.0]]), 0.1)
