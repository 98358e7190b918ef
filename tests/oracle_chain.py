"""An independent chain for one output scan of the reference's ``deform('mesh')`` / ``deform('mergemesh')`` + ``write()`` with
the CUDA fusion mode (TEST INFRASTRUCTURE).  No step imports ``lidar_transfer_amd``:

  projection     oracle/projection.py (``method="new"``, ``remove=True``; goldens F6 / F9 / F16)
  mergemesh      the clipping of ``vol_bnds`` by the kept points' rounded bounds and the volume geometry the reference derives
  bounds         from them (laserscan.py:957-962, fusion_lidar.py:33-37), restated below (CPU-checked against F14 / F14b / F14c)
  integrate      the reference's own class-aware ``integrate`` kernel source compiled for gfx950 (``ob.ref_tsdf_lib(True)``)
  mesh           ``ob.marching_cubes`` (= scikit-image 0.18's arrays: golden F10)
  render         the reference raytracer (``ob.ref_trace(kind="strict")``) with the rays of ``create_rays`` restated below, and
                 ``ob.oracle_trace(mode=MODE_BRUTE)`` for the hit triangle and the (t, face) minimum at exact-t ties
  write          ``do_reverse_projection_new`` and ``write()``'s filter + pack (laserscan.py:475-501, :1133-1160), restated below
                 (CPU-checked against F7)

The volumes live on the device (the reference kernel runs there); everything else runs on the host with at most 16 threads.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import binding as ob
from oracle import projection as op

THREADS = 16


# ---- sensor rays (laserscan.py:1092-1119) --------------------------------------------------------------------------------
def create_rays(fov_up, fov_down, H, W):
    """[H*W, 3] float32 unit directions, row by row; yaw starts at 180 degrees and wraps; float64 until the final cast."""
    yaw = np.linspace(0, 360, W) + 180
    yaw[yaw > 360] -= 360
    yaw = yaw / 180.0 * np.pi
    rows = []
    for pitch in np.pi / 2 - np.linspace(fov_up, fov_down, H) / 180.0 * np.pi:
        rows.append(np.stack([np.sin(pitch) * np.cos(-yaw), np.sin(pitch) * np.sin(-yaw), np.cos(pitch) * np.ones(W)], 1))
    return np.ascontiguousarray(np.concatenate(rows).astype(np.float32))


# ---- volume geometry (fusion_lidar.py:33-37) and the mergemesh bounds (laserscan.py:957-962) -------------------------------
def volume_geometry(vol_bnds, voxel):
    """What ``TSDFVolume.__init__`` derives from the bounds it is given: ``dim = ceil(extent / voxel)``, the upper bounds
    rewritten IN PLACE to ``lower + dim * voxel`` (stored in the array's own dtype: an integer array truncates), the origin
    = the lower bounds in float32.  Returns (dim int64 [3], origin float32 [3])."""
    dim = np.ceil((vol_bnds[:, 1] - vol_bnds[:, 0]) / voxel).astype(np.int64)
    vol_bnds[:, 1] = vol_bnds[:, 0] + dim * voxel
    return dim, vol_bnds[:, 0].astype(np.float32)


def mergemesh_bounds(vol_bnds, kept_points, voxel):
    """One mergemesh output scan's bookkeeping on the sequence's ONE bounds array (modified in place): the bounds of the
    points that survived the projection, rounded half to even to integers, narrow the array (never widen it); then the
    volume geometry of the narrowed array.  Returns (dim, origin, bounds given to the volume [3, 2] float64)."""
    pts = np.asarray(kept_points)
    if pts.shape[0] == 0:
        raise ValueError("no point survives the projection")
    lo, hi = np.rint(pts.min(axis=0)).astype(np.int64), np.rint(pts.max(axis=0)).astype(np.int64)
    vol_bnds[:, 0] = np.maximum(vol_bnds[:, 0], lo)
    vol_bnds[:, 1] = np.minimum(vol_bnds[:, 1], hi)
    given = vol_bnds.astype(np.float64)
    dim, origin = volume_geometry(vol_bnds, voxel)
    if np.any(dim <= 0):
        raise ValueError(f"the clipped volume is empty (bounds {given.tolist()})")
    return dim, origin, given


# ---- write() (laserscan.py:475-501, :1133-1160) -----------------------------------------------------------------------------
def reverse_projection(range_image, proj_x, proj_y, fov_up, fov_down):
    """``do_reverse_projection_new``: pixel coordinates (int or float) and depth back to points, float64 [H*W, 3]."""
    H, W = np.asarray(range_image).shape
    fu, fd = fov_up / 180.0 * np.pi, fov_down / 180.0 * np.pi
    fov = abs(fd) + abs(fu)
    depth = np.asarray(range_image)
    yaw = (np.asarray(proj_x) / W * 2 - 1.0) * np.pi
    pitch = np.pi / 2 - (1.0 * fov - np.asarray(proj_y) / H * fov - abs(fd))
    x = depth * np.sin(pitch) * np.cos(-yaw)
    y = depth * np.sin(pitch) * np.sin(-yaw)
    z = depth * np.cos(pitch)
    return np.stack([x, y, z], 2).reshape(-1, 3)


def pack_write(back_points, label_image, remissions, index=None):
    """``write()``'s filter and pack: with ``index`` (the ``cp`` adaption) only cells whose index is > 0; then labels >= 0;
    then points whose coordinate SUM is not 0.  Returns (bin [N, 4] float32 = x, y, z, remission; label [N] uint32) -- the
    bytes of ``velodyne/N.bin`` / ``labels/N.label``."""
    pts = np.asarray(back_points).reshape(-1, 3)
    lab = np.asarray(label_image).reshape(-1)
    rem = np.asarray(remissions).reshape(-1)
    if index is not None:
        keep = np.asarray(index).reshape(-1) > 0
        pts, rem, lab = pts[keep], rem[keep], lab[keep].astype(np.int32)
    keep = lab >= 0
    pts, rem, lab = pts[keep], rem[keep], lab[keep].astype(np.int32)
    keep = pts.sum(axis=1) != 0
    pts, rem, lab = pts[keep], rem[keep], lab[keep]
    out = np.empty((pts.shape[0], 4), np.float32)
    out[:, :3] = pts
    out[:, 3] = rem
    return out, lab.astype(np.uint32)


# ---- the chain ---------------------------------------------------------------------------------------------------------------
class RefVolume:
    """The four fields of one volume, integrated by the reference's own kernel on the device.  64 spare floats stay behind
    each field: the kernel's thread N (one past the end, fusion_lidar.py:92-93) may write element N."""

    def __init__(self, dim, origin, voxel, fov_up, fov_down, device=0):
        import torch
        self.dim, self.origin, self.voxel = tuple(int(x) for x in dim), np.asarray(origin, np.float32), float(voxel)
        self.fov_up, self.fov_down = float(fov_up), float(fov_down)
        n = int(np.prod(self.dim))
        dev = torch.device("cuda", device)
        self._dev = dev
        flat = [torch.ones(n + 64, device=dev)] + [torch.zeros(n + 64, device=dev) for _ in range(3)]
        self.fields = [t[:n].view(self.dim) for t in flat]      # tsdf, weight, color, rem

    def integrate(self, label_image, depth, rem):
        """``integrate(proj_label3, proj_range, proj_remissions, obs_weight=1)`` with the label in channel 0 (laserscan.py:893-895,
        :970-972); the RGB fold of fusion_lidar.py:260-264 in float32."""
        import torch
        H, W = depth.shape
        c = np.zeros((H, W, 3), np.float64)
        c[:, :, 0] = label_image
        c = c.astype(np.float32)
        folded = np.floor(c[:, :, 0] * 256 * 256 + c[:, :, 1] * 256 + c[:, :, 2]).astype(np.float32)
        ims = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self._dev) for a in (folded, depth, rem)]
        vp = C.c_void_p
        st = torch.cuda.current_stream(self._dev)
        rc = ob.ref_tsdf_lib(True).ref_tsdf_integrate(
            *[vp(t.data_ptr()) for t in self.fields], (C.c_int * 3)(*self.dim), (C.c_float * 3)(*[float(x) for x in self.origin]),
            C.c_float(np.float32(self.voxel)), C.c_float(np.float32(self.voxel * 5)), C.c_float(self.fov_up),
            C.c_float(self.fov_down), vp(ims[0].data_ptr()), vp(ims[1].data_ptr()), vp(ims[2].data_ptr()), H, W, C.c_float(1.0),
            vp(st.cuda_stream))
        assert rc == 0, f"reference integrate kernel launch failed ({rc})"
        st.synchronize()

    def mesh(self):
        tsdf, _, color, rem = [t.cpu().numpy() for t in self.fields]
        return ob.marching_cubes(tsdf, color, rem, np.float32(self.voxel), self.origin)


def project(points, rem, labels, H, W, fov_up, fov_down):
    """``do_range_projection_new(fov, remove=True)`` + ``do_label_projection_new``: (range, rem, label images, kept points)"""
    p = op.range_projection(points, rem, H, W, fov_up, fov_down, remove=True, method="new")
    lab = op.label_projection(p["index"], np.asarray(labels)[p["kept"]].astype(np.int64)).astype(np.int32)
    return p["range"], p["remission"], lab, np.asarray(points)[p["kept"]]


_HOST_IS_TABLE = None


def host_rsqrt_is_the_table():
    """does this CPU's RSQRTSS return the seed table the product replays by default (an Intel CPU)?"""
    global _HOST_IS_TABLE
    if _HOST_IS_TABLE is None:
        rng = np.random.default_rng(1)
        r = (rng.normal(size=(1 << 16, 3)) * 10.0 ** rng.uniform(-6, 6, (1 << 16, 1))).astype(np.float32)
        _HOST_IS_TABLE = bool(np.array_equal(ob.normalize_rays(r, ob.NORM_SSE).view(np.int32),
                                             ob.normalize_rays(r, ob.NORM_SSE_TABLE).view(np.int32)))
    return _HOST_IS_TABLE


def render(mesh, target):
    """``throw_rays_at_mesh``'s ray cast and the images ``deform`` unpacks (laserscan.py:899-914, :995-1006): the reference
    raytracer's output, plus MODE_BRUTE's for the hit triangle and the tie rule"""
    tH, tW, tfu, tfd = target
    verts, faces, colors, vrem = mesh
    rays = create_rays(tfu, tfd, tH, tW)
    org = np.zeros(3, np.float32)
    ref = ob.ref_trace(rays, org, verts, faces, colors, vrem, tH, kind="strict")
    if not host_rsqrt_is_the_table():
        # The compiled reference normalises its rays with THIS CPU's RSQRTSS seed, vendor specific in the last bits; the
        # product (and every golden) replays the seed of the Intel CPU the goldens were made on.  Here: the restatement of
        # the reference's BVH and tie rule, first held to the compiled reference with this host's own seed (bit for bit),
        # then run with the Intel seed -- the reference as run on that CPU.
        mine = ob.oracle_trace(rays, org, verts, faces, colors, vrem, tH, mode=ob.MODE_REF_BVH, norm=ob.NORM_SSE,
                               nthreads=THREADS)
        for k in ("range", "endrem", "endpoints", "endcolors"):
            assert np.array_equal(np.asarray(mine[k]).view(np.int32), np.asarray(ref[k]).view(np.int32)), \
                f"the restated reference raytracer differs from the compiled one in {k}"
        ref = ob.oracle_trace(rays, org, verts, faces, colors, vrem, tH, mode=ob.MODE_REF_BVH, norm=ob.NORM_SSE_TABLE,
                              nthreads=THREADS)
    brute = ob.oracle_trace(rays, org, verts, faces, colors, vrem, tH, mode=ob.MODE_BRUTE, norm=ob.NORM_SSE_TABLE,
                            nthreads=THREADS)
    ref["rays"] = brute["rays"] = rays
    return ref, brute


def finish(vol, target):
    mesh = vol.mesh()
    ref, brute = render(mesh, target)
    tH, tW = target[0], target[1]
    label = ref["endcolors"][:, 2].reshape(tH, tW)
    b, l = pack_write(ref["endpoints"], label, ref["endrem"])
    return dict(volume=vol, mesh=mesh, ref=ref, brute=brute, bin=b, label_file=l)


def deform_mesh(clouds, source, target, vol_bnds, voxel, device=0):
    """``deform('mesh')`` + ``write()``: every source scan projected at the source field of view into one fresh volume of the
    configured bounds (a copy: this adaption leaves the caller's array as it is between output scans here)."""
    H, W, fu, fd = source
    b = np.array(vol_bnds, copy=True)
    dim, origin = volume_geometry(b, voxel)
    vol = RefVolume(dim, origin, voxel, fu, fd, device)
    for pts, rem, lab in clouds:
        rng, remi, labi, _ = project(pts, rem, lab, H, W, fu, fd)
        vol.integrate(labi, rng, remi)
    out = finish(vol, target)
    out.update(vol_dim=tuple(int(x) for x in dim), vol_origin=origin)
    return out


def deform_mergemesh(clouds, source, target, vol_bnds, voxel, device=0):
    """``deform('mergemesh')`` + ``write()`` of one output scan on the sequence's bounds array ``vol_bnds`` (clipped in place):
    the merged cloud at the TARGET field of view onto the SOURCE H x W, a volume of the target field of view."""
    H, W = source[0], source[1]
    tfu, tfd = target[2], target[3]
    pts = np.concatenate([c[0] for c in clouds])
    rem = np.concatenate([c[1] for c in clouds])
    lab = np.concatenate([c[2] for c in clouds])
    rng, remi, labi, kept = project(pts, rem, lab, H, W, tfu, tfd)
    dim, origin, given = mergemesh_bounds(vol_bnds, kept, voxel)
    vol = RefVolume(dim, origin, voxel, tfu, tfd, device)
    vol.integrate(labi, rng, remi)
    out = finish(vol, target)
    out.update(vol_dim=tuple(int(x) for x in dim), vol_origin=origin, bnds_after=vol_bnds.copy(),
               source=dict(range=rng, rem=remi, label=labi))
    return out


# ---- the equality rule ---------------------------------------------------------------------------------------------------------
def check_images(got, want, tag):
    """``got``: the product's range [R], label [R] (int), rem [R], endpoints [R, 3], tri [R] (numpy).  Every pixel equals the
    reference raytracer bit for bit, but
      * where the reference and MODE_BRUTE report the same t with different attributes (two faces hit at exactly the same t:
        an exact-t tie), and
      * on rays that run inside a lattice plane through the sensor (a direction component below 1e-7: marching-cubes vertices
        lie IN that plane, the ray meets triangle edges, and the reference's unpadded SSE slab test can reject the box of the
        closest triangle -- DESIGN.md section 3, golden F15's seam pixels), where the reference and MODE_BRUTE differ;
    there it equals MODE_BRUTE's (t, face) minimum, bit for bit.  ``tri`` equals MODE_BRUTE's everywhere.  Returns
    (exact-t tie pixels off those planes, in-plane pixels at which the reference differs from MODE_BRUTE)."""
    ref, brute = want["ref"], want["brute"]
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)   # noqa: E731
    same = lambda a, b: (a == b).reshape(len(a), -1).all(1)               # noqa: E731
    r_rng, r_lab, r_rem, r_end = bits(ref["range"]), ref["endcolors"][:, 2], bits(ref["endrem"]), bits(ref["endpoints"])
    b_rng, b_lab, b_rem, b_end = bits(brute["range"]), brute["endcolors"][:, 2], bits(brute["endrem"]), bits(brute["endpoints"])
    g_rng, g_lab, g_rem, g_end = bits(got["range"]).reshape(-1), np.asarray(got["label"]).reshape(-1), \
        bits(got["rem"]).reshape(-1), bits(got["endpoints"]).reshape(-1, 3)
    ref_is_brute = same(r_rng, b_rng) & same(r_lab, b_lab) & same(r_rem, b_rem) & same(r_end, b_end)
    in_plane = (np.abs(np.asarray(ref["rays"], np.float32).reshape(-1, 3)) < 1e-7).any(1)
    tie = ~ref_is_brute & same(r_rng, b_rng) & ~in_plane
    plane = ~ref_is_brute & in_plane
    use_brute = tie | plane
    want_rng, want_lab = np.where(use_brute, b_rng, r_rng), np.where(use_brute, b_lab, r_lab)
    want_rem, want_end = np.where(use_brute, b_rem, r_rem), np.where(use_brute[:, None], b_end, r_end)
    for name, g, w in (("range", g_rng, want_rng), ("label", g_lab, want_lab), ("remission", g_rem, want_rem),
                       ("endpoints", g_end, want_end)):
        bad = np.nonzero(~same(g, w))[0]
        assert len(bad) == 0, f"{tag}: {name} differs from the reference raytracer at {len(bad)} of {len(g_rng)} pixels " \
                              f"(first {bad[:8].tolist()}; {int(tie.sum())} exact-t tie pixels, {int(plane.sum())} in-plane)"
    # what write() packs from the images this rule selects (the reference's own where ref_is_brute / off the exceptions)
    want["bin_rule"], want["label_file_rule"] = pack_write(want_end.view(np.float32), want_lab, want_rem.view(np.float32))
    bad = np.nonzero(np.asarray(got["tri"]).reshape(-1) != brute["tri"])[0]
    assert len(bad) == 0, f"{tag}: hit triangle differs from MODE_BRUTE's at {len(bad)} pixels (first {bad[:8].tolist()})"
    return int(tie.sum()), int(plane.sum())
