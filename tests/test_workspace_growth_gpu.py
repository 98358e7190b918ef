"""A reused object whose device workspaces GROW equals a fresh one (csrc/lt_devmem.h: every growth site of the library's
host code goes through one group replacement).  Per object the sequence is small, then large, then small again on ONE
object, every result compared bit for bit with the same call on an object created for it.  The shapes are the smallest that
cross each site's capacity rule; where a rule's headroom swallows the step the issue names, a larger step follows it.

What grows where:
  Scene                 lt_scene_reserve (headroom, 12 -> 3000 faces), lt_scene_reserve_rays, sc_reserve (cells exact, queues)
  Projector             pj_reserve (points: headroom; cells + 1024), bacc (blocks + blocks / 4 + 64: regrown by 20 000 points),
                        dmin (float64 clouds of the old variant), img of lt_deform_scan_dev (exact)
  TSDFVolume            dct, rowtab, the wedge table (class-aware: the pixel pass); colmax, dct (plain average: the column walk);
                        obs4 of lt_tsdf_integrate_multi_dev (8 images of the shape: regrown by the larger image)
  DeviceMesh            words, blocks, records, vertex and face arrays, the renumbering's arrays
  Evaluator             key (exact), partial (exact)
  post.pack_scan        the process-wide block counts (2 * blocks + 1024: 1026 after 100 points, regrown by 300 000)
  lt_hostpipe, lt_ctrace  the slot's mesh block, the owned mesh of the scene, io, rays_cached
"""
import ctypes as C
import threading

import numpy as np
import pytest

import post_cases
import writeback_cases as wc
from lidar_transfer_amd.laserscan import create_rays
from lidar_transfer_amd.synth import synth_cloud

pytestmark = pytest.mark.gpu

KEYS = wc.KEYS
ORIGIN = wc.ORIGIN
SMALL, LARGE = (4, 16), (16, 128)          # rays
FOV = (3.0, -25.0)


def soup(n_faces, seed):
    """n_faces triangles facing ORIGIN, 3-8 m away, inside the rays' field of view; the fewer, the larger"""
    rng = np.random.default_rng(seed)
    yaw, pitch = rng.uniform(-np.pi, np.pi, n_faces), np.deg2rad(rng.uniform(-9.0, 9.0, n_faces))
    d = np.stack([np.cos(pitch) * np.cos(yaw), np.cos(pitch) * np.sin(yaw), np.sin(pitch)], 1)
    dist = rng.uniform(3.0, 8.0, n_faces)
    u = np.cross(d, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    radius = (0.25 if n_faces < 100 else 0.03) * dist
    tri = wc._facing(np.asarray(ORIGIN, np.float64) + d * dist[:, None], u, np.cross(d, u), radius, rng)
    return wc.soup_of(tri, wc.attrs(3 * n_faces, seed + 1))


MESH_SMALL, MESH_LARGE = soup(12, 1), soup(3000, 2)       # 3000 > 12 + 12 / 4 + 1024


def rays_of(shape):
    return create_rays(10.0, -10.0, *shape)


def bits(t):
    """a device tensor (or array) as host bytes"""
    a = t.detach().cpu().contiguous().numpy() if hasattr(t, "detach") else np.ascontiguousarray(t)
    return a.reshape(-1).view(np.uint8).copy()


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: output {k} differs from a fresh object's"


def grown_equals_fresh(make, run, steps, what):
    """run(obj, step) for every step on ONE object from make() and on a fresh one per step; results are lists of bytes"""
    reused = make()
    try:
        for i, step in enumerate(steps):
            got = run(reused, step)
            fresh = make()
            try:
                want = run(fresh, step)
            finally:
                fresh.close()
            same(got, want, f"{what}, step {i}")
    finally:
        reused.close()


# ---- Scene: render and the LBVH path -------------------------------------------------------------------------------------
def test_scene_render_and_trace_after_growth_equal_a_fresh_scene():
    import torch
    from lidar_transfer_amd.raytracer import RaySet, Scene
    dev = torch.device("cuda", 0)
    hits = []

    def run(sc, step):
        mesh, shape = step
        keep = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in mesh]
        rays = torch.from_numpy(rays_of(shape)).to(dev)
        sc.set_mesh(*keep)
        rs = RaySet(rays, shape[0])
        a = sc.render(rs, ORIGIN)
        sc.build()
        b = sc.trace(rays, ORIGIN, shape[0])
        torch.cuda.synchronize()
        sc.status()
        rs.close()
        hits.append(int((a["tri"] >= 0).sum()))
        return [bits(o[k]) for o in (a, b) for k in KEYS]

    steps = [(MESH_SMALL, SMALL), (MESH_LARGE, LARGE), (MESH_SMALL, SMALL)]
    grown_equals_fresh(lambda: Scene(0), run, steps, "Scene")
    assert min(hits) > 0, hits


# ---- Projector ---------------------------------------------------------------------------------------------------------------
def _cloud(seed, n, dtype, dev):
    import torch
    p, rm, lb = synth_cloud(seed, n, dtype=dtype, rmin=2.0, rmax=6.0)
    return torch.from_numpy(p).to(dev), torch.from_numpy(rm).to(dev), torch.from_numpy(lb.astype(np.int32)).to(dev)


@pytest.mark.parametrize("new", [True, False])   # False with float64 clouds: the old variant's dmin keys as well
def test_projector_after_growth_equals_a_fresh_projector(new):
    import torch
    from lidar_transfer_amd.laserscan import Projector
    dev = torch.device("cuda", 0)
    outputs = ("idx", "range", "rem", "label", "n_kept", "bnds")

    def run(pj, step):
        n, (H, W) = step
        got = pj.project([_cloud(40 + n % 7, n, np.float64, dev)], *FOV, H, W, new=new, remove=new, outputs=outputs)
        torch.cuda.synchronize()
        return [bits(got[0][k]) for k in outputs]

    # 100 -> 5000 points, 4 x 16 -> 16 x 512 cells; 20 000 points: more than the 66 blocks of partial bounds the first call left
    steps = [(100, (4, 16)), (5000, (16, 512)), (20000, (16, 512)), (100, (4, 16))]
    grown_equals_fresh(lambda: Projector(0), run, steps, f"Projector(new={new})")


class _DeformChain:
    """the objects lt_deform_scan_dev works on, and one call of it"""

    def __init__(self):
        import torch
        from lidar_transfer_amd.fusion import DeviceMesh, TSDFVolume
        from lidar_transfer_amd.laserscan import Projector
        from lidar_transfer_amd.raytracer import RaySet, Scene
        self.dev = torch.device("cuda", 0)
        self.pj, self.mesh, self.scene = Projector(0), DeviceMesh(0), Scene(0)
        self.vol = TSDFVolume(np.array([[-6.4, 6.4], [-6.4, 6.4], [-3.2, 3.2]]), 0.1, *FOV, device=0)
        self.rays = torch.from_numpy(create_rays(*FOV, *LARGE)).to(self.dev)
        self.rs = RaySet(self.rays, LARGE[0])

    def run(self, n_clouds):
        import torch
        from lidar_transfer_amd import _chain, _lib
        H, W = LARGE
        cl, keep, is_f64 = _chain.cloud_table([_cloud(60 + k, 3000, np.float32, self.dev) for k in range(n_clouds)])
        out = self.scene.alloc_outputs(H * W, label_image=True)
        st = torch.cuda.current_stream(self.dev)
        _lib.check(self.pj._lib.lt_deform_scan_dev(self.pj._h, self.vol._h, self.mesh._h, self.scene._h, self.rs._h, n_clouds, cl,
                                                   is_f64, FOV[0], FOV[1], H, W, None, 0, 1.0, self.vol._flags,
                                                   _chain.origin3((0.0, 0.0, 0.0)), *_chain.out_ptrs(out), _chain.TRACE_FLAGS,
                                                   C.c_void_p(st.cuda_stream), 1), "lt_deform_scan_dev")
        torch.cuda.synchronize()
        self.n_faces = self.mesh.n_faces
        return [bits(out[k]) for k in KEYS] + [np.array([self.mesh.n_verts, self.mesh.n_faces])]

    def close(self):
        for o in (self.rs, self.scene, self.mesh, self.vol, self.pj):
            o.close()


def test_deform_scan_of_one_cloud_then_three_equals_a_fresh_chain():
    faces = []

    def run(ch, n_clouds):
        r = ch.run(n_clouds)
        faces.append(ch.n_faces)
        return r

    grown_equals_fresh(_DeformChain, run, [1, 3, 1], "lt_deform_scan_dev")
    assert min(faces) > 0, faces


# ---- TSDFVolume ----------------------------------------------------------------------------------------------------------------
VOL_BNDS = np.array([[2.0, 4.0], [-1.0, 1.0], [-0.5, 0.5]])    # 16 x 16 x 8 voxels of 0.125 m, ahead of the sensor
VOXEL = 0.125


def _observation(shape, seed):
    """(label image [H, W, 3], depth, remission) whose surface crosses VOL_BNDS"""
    H, W = shape
    rng = np.random.default_rng([seed, H, W])
    color = np.zeros((H, W, 3), np.float32)
    color[:, :, 2] = rng.choice(np.array([10, 40, 48, 50], np.float32), (H, W))
    return color, rng.uniform(2.3, 3.7, (H, W)).astype(np.float32), rng.uniform(0, 1, (H, W)).astype(np.float32)


def _fields(vol):
    import torch
    torch.cuda.synchronize()
    return [bits(t) for t in vol.get_volume_tensors()]


def _volume(merge):
    from lidar_transfer_amd.fusion import TSDFVolume
    return TSDFVolume(VOL_BNDS, VOXEL, *FOV, device=0, merge=merge)


@pytest.mark.parametrize("merge", [True, False])   # the class-aware pixel pass; the plain average's column walk
def test_volume_integrate_after_growth_equals_a_fresh_volume(merge):
    written = []

    def run(vol, shape):
        vol.reset()
        vol.integrate(*_observation(shape, 5))
        f = _fields(vol)
        written.append(int((f[0].view(np.float32) != 1.0).sum()))   # (tsdf starts at 1)
        return f

    grown_equals_fresh(lambda: _volume(merge), run, [SMALL, LARGE, SMALL], f"TSDFVolume(merge={merge}).integrate")
    assert min(written) > 0, written


def test_volume_integrate_multi_after_growth_equals_a_fresh_volume():
    def run(vol, step):
        n_obs, shape = step
        vol.reset()
        vol.integrate_multi([_observation(shape, 20 + k) for k in range(n_obs)])
        return _fields(vol)

    # one observation (not fused), three (obs4 appears), three of the larger image (obs4 grows), one again
    steps = [(1, SMALL), (3, SMALL), (3, LARGE), (1, SMALL)]
    grown_equals_fresh(lambda: _volume(True), run, steps, "TSDFVolume.integrate_multi")


# ---- DeviceMesh ----------------------------------------------------------------------------------------------------------------
def test_mesh_extraction_and_renumbering_after_growth_equal_a_fresh_mesh():
    import torch
    from lidar_transfer_amd.fusion import DeviceMesh
    dev = torch.device("cuda", 0)
    vol = _volume(True)
    vol.integrate(*_observation(LARGE, 5))
    torch.cuda.synchronize()
    t, _, c, r = [x.contiguous() for x in vol.get_volume_tensors()]
    small = (t, c, r, VOXEL, VOL_BNDS[:, 0])
    g = np.stack(np.meshgrid(np.arange(48), np.arange(48), np.arange(16), indexing="ij"), -1).astype(np.float32)
    sphere = np.clip((np.linalg.norm(g - np.array([23.5, 23.5, 7.5], np.float32), axis=-1) - 20.0) / 5.0, -1.0, 1.0).astype(np.float32)
    rng = np.random.default_rng(9)
    big = (torch.from_numpy(sphere).to(dev), torch.from_numpy(rng.choice(np.array([10, 40], np.float32), sphere.shape)).to(dev),
           torch.from_numpy(rng.uniform(0, 1, sphere.shape).astype(np.float32)).to(dev), 0.1, (0.0, 0.0, 0.0))
    sizes = []

    def run(mesh, fields):
        mesh.extract(*fields)
        mesh.renumber()
        torch.cuda.synchronize()
        sizes.append(mesh.n_faces)
        return [bits(x) for x in mesh.tensors()]

    grown_equals_fresh(lambda: DeviceMesh(0), run, [small, big, small], "DeviceMesh")
    vol.close()
    assert min(sizes) > 0 and sizes[2] > sizes[0] + sizes[0] // 4 + 1024, sizes   # (the sphere's faces pass the first capacity)


# ---- Evaluator -----------------------------------------------------------------------------------------------------------------
def test_evaluator_after_growth_equals_a_fresh_evaluator():
    import torch
    from lidar_transfer_amd.evaluate import Evaluator
    dev = torch.device("cuda", 0)
    lut = np.random.default_rng(3).uniform(0.1, 1.0, (360, 3)).astype(np.float32)
    lut[[0, 48]] = 0

    def run(e, shape):
        e.H, e.W = shape                                   # (the native evaluator takes the shape per call)
        p, rm, lb = synth_cloud(70, 4000, rmin=2.0, rmax=30.0)
        xyzr = torch.from_numpy(np.ascontiguousarray(np.concatenate([p, rm[:, None]], 1), np.float32)).to(dev)
        src = e.source_scan(xyzr, torch.from_numpy(lb.astype(np.int32)).to(dev))
        rng = np.random.default_rng([8, *shape])
        tl = torch.from_numpy(rng.choice(np.array([0, 10, 40, 48, 50], np.int32), shape)).to(dev)
        tr = torch.from_numpy(rng.uniform(0.0, 30.0, shape).astype(np.float32)).to(dev)
        status, present, counts, sq_sum, n_cells, bad = e.compare(src, tl, tr).counts()   # (the record's defined part)
        torch.cuda.synchronize()
        assert status == 0 and n_cells == shape[0] * shape[1]
        return [bits(src[k]) for k in ("range", "rem", "label", "black", "bad_labels")] + \
               [bits(present), bits(counts), bits(np.array([sq_sum, bad], np.float64))]

    grown_equals_fresh(lambda: Evaluator((*SMALL, *FOV), [40], lut, device=0), run, [(4, 16), (16, 512), (4, 16)], "Evaluator")


# ---- post.pack_scan ------------------------------------------------------------------------------------------------------------
def test_pack_scan_across_a_regrown_block_count_buffer():
    """The block counts are process-wide: there is no fresh object, the numpy restatement stands in for it."""
    from lidar_transfer_amd.post import pack_scan
    for n in (100, 300_000, 100):      # 300 000 points: 1172 workgroups, more than the 1026 counts the first call may have left
        c = post_cases.pack_case(n, np.float32, keep=post_cases.keep_pattern("random50", n))
        b, l = pack_scan(c["points"], c["label"], c["rem"])
        wb, wl = post_cases.restate_pack(c["points"], c["label"], c["rem"])
        assert np.array_equal(b.view(np.uint32), wb.view(np.uint32)) and np.array_equal(l, wl), n


# ---- lt_hostpipe, lt_ctrace ------------------------------------------------------------------------------------------------------
def _ctrace(mesh, shape):
    from lidar_transfer_amd.raytracer import C_Trace
    v, f, c, r = mesh
    n = shape[0] * shape[1]
    out = dict(endpoints=np.zeros(3 * n, np.float32), endcolors=np.zeros(3 * n, np.int32), range=np.zeros(n, np.float32),
               endrem=np.zeros(n, np.float32), tri=np.full(n, -1, np.int32))
    C_Trace(np.ascontiguousarray(rays_of(shape)).reshape(-1), np.asarray(ORIGIN, np.float32), v.reshape(-1), f.reshape(-1),
            np.ascontiguousarray(c, np.int32).reshape(-1), r.reshape(-1), out["endpoints"], out["endcolors"], out["range"],
            out["endrem"], shape[0], shape[1], tri_image=out["tri"])
    return [bits(out[k]) for k in KEYS]


def _in_thread(fn):
    """fn() on a thread of its own: lt_ctrace's context (scene, io, cached rays) is per calling thread"""
    box = {}

    def body():
        try:
            box["value"] = fn()
        except BaseException as e:   # noqa: B902 -- handed to the caller
            box["error"] = e

    t = threading.Thread(target=body)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def test_ctrace_on_one_thread_after_growth_equals_a_fresh_thread():
    # the meshes grow the scene's owned mesh; the rays grow io and replace the cached rays of the thread's ray set
    steps = [(MESH_SMALL, SMALL), (MESH_LARGE, SMALL), (MESH_SMALL, SMALL), (MESH_SMALL, LARGE), (MESH_SMALL, SMALL)]
    got = _in_thread(lambda: [_ctrace(*s) for s in steps])
    for i, s in enumerate(steps):
        same(got[i], _in_thread(lambda: _ctrace(*s)), f"lt_ctrace, step {i}")
    assert (got[0][4].view(np.int32) >= 0).any()


def test_hostpipe_slot_after_growth_equals_a_fresh_pipe():
    from lidar_transfer_amd.pipeline import HostScanPipeline

    def run(pipe, mesh):
        o = pipe.wait(pipe.submit(*mesh, ORIGIN))
        return [bits(o[k]) for k in KEYS]

    # depth 1: every scan goes through the one slot, whose mesh block grows with the second
    grown_equals_fresh(lambda: HostScanPipeline(rays_of(SMALL), SMALL[0], depth=1), run, [MESH_SMALL, MESH_LARGE, MESH_SMALL],
                       "lt_hostpipe")
