"""A miss is the same bytes whoever writes it.

Six producers turn a cell into a miss: the scatter render and the LBVH trace with write_misses over rays that hit nothing,
lt_return_model_dev with a max_range below every hit, lt_noise_model_dev with a gate that every noised range leaves,
lt_echo_resolve_dev with min_subrays above every cell's sub-hits, and the second set of lt_echo_resolve_dual_dev on cells
with one detected echo.  Each is made to write its misses into sentinel-filled buffers with guard words on both sides of
every view, and the WHOLE buffers are compared as int32 bits: every miss cell holds

    end point 0, 0, 0 | label 0 or colour 0, 0, 0 | range 0.0f | remission 0.0f | tri -1

and the guards, and every buffer whose pointer was not passed, keep the sentinel.  Both colour layouts where the entry has
both; two pointer sets, all five and range + tri only; H = 1 and W in {1, 63, 65, 257}: the wave and block seams of a
256-thread kernel with one cell per thread.  The mesh is the one-triangle wall of writeback_cases.wall, which every ray
hits at 4.06 .. 5.73 m, or its mirror image behind the sensor, which none does."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import writeback_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = (1, 63, 65, 257)
LAYOUTS = (True, False)                        # label_image
POINTER_SETS = (wc.KEYS, ("range", "tri"))
GUARD = 64                                     # sentinel elements in front of every view; wc.tail_of behind it
NEAR_GATE = 1.0                                # metres: below every hit of the wall


def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(x):
    import torch
    return torch.from_numpy(np.array(x)).to(_dev())


class Guarded:
    """the five sentinel-filled device buffers of a scan of n cells, and the views of `ptrs` into them"""

    def __init__(self, n, label_image, ptrs):
        import torch
        self.n, self.label_image, self.ptrs = n, label_image, ptrs
        self.buf, self.out = {}, {}
        for k in wc.KEYS:
            w = wc.width_of(k, label_image)
            self.buf[k] = torch.full((GUARD + n * w + wc.tail_of(n),), wc.SENTINEL, dtype=torch.int32, device=_dev())
            if k in ptrs:
                v = self.buf[k][GUARD:GUARD + n * w]
                self.out[k] = (v if k in ("endcolors", "tri") else v.view(torch.float32)).view((n, 3) if w == 3 else (n,))

    def check_all_misses(self, what):
        """every cell of every view a miss, every other element the sentinel"""
        import torch
        torch.cuda.synchronize()
        bad = []
        for k in wc.KEYS:
            want = np.full(self.buf[k].numel(), wc.SENTINEL, np.int32)
            if k in self.ptrs:
                want[GUARD:GUARD + self.n * wc.width_of(k, self.label_image)] = wc.MISS[k]
            got = self.buf[k].cpu().numpy()
            i = np.flatnonzero(got != want)
            if i.size:
                bad.append(f"{what} {k}: {i.size} elements differ, first at buffer element {i[0]} (view starts at {GUARD}): "
                           f"got {got[i[0]]:#x} expected {want[i[0]]:#x}")
        assert not bad, "\n".join(bad)


def _variants():
    for label_image in LAYOUTS:
        for ptrs in POINTER_SETS:
            yield label_image, ptrs, f"label_image={label_image} ptrs={','.join(ptrs)}"


class Rig:
    """a scene with the wall (or its mirror image behind the sensor), LBVH built, and the wall's rays"""

    def __init__(self, W, behind=False):
        from lidar_transfer_amd.raytracer import RaySet, Scene
        mesh, rays = wc.wall(1, W)
        v = np.array(mesh[0])
        if behind:
            v[:, 0] = 2 * np.float32(wc.ORIGIN[0]) - v[:, 0]
        self.n = W
        self.sc = Scene(0)
        self.mesh_t = [_up(x) for x in (v,) + mesh[1:]]
        self.sc.set_mesh(*self.mesh_t)
        self.rays_t = _up(rays)
        self.rs = RaySet(self.rays_t, 1)
        assert self.rs.n_rays == W
        self.sc.build()

    def render(self, g, strategy="scatter"):
        kw = dict(out=g.out, write_misses=True, label_image=g.label_image)
        if strategy == "scatter":
            self.sc.render(self.rs, wc.ORIGIN, **kw)
        else:
            self.sc.trace(self.rays_t, wc.ORIGIN, 1, **kw)

    def render_hits(self, g):
        """the wall rendered into g's views: every cell a hit beyond NEAR_GATE"""
        self.render(g)
        tri, rng = g.out["tri"].cpu().numpy(), g.out["range"].cpu().numpy()
        assert (tri == 0).all() and (rng > NEAR_GATE).all()

    def close(self):
        self.rs.close()
        self.sc.close()


@pytest.mark.parametrize("strategy", ["scatter", "lbvh"])
@pytest.mark.parametrize("W", WIDTHS)
def test_render_over_rays_that_hit_nothing(W, strategy):
    rig = Rig(W, behind=True)
    try:
        for label_image, ptrs, what in _variants():
            g = Guarded(W, label_image, ptrs)
            rig.render(g, strategy)
            g.check_all_misses(f"{strategy} W={W} {what}")
        rig.sc.status()
    finally:
        rig.close()


@pytest.mark.parametrize("W", WIDTHS)
def test_return_model_with_every_hit_beyond_its_gate(W):
    from lidar_transfer_amd import post
    from lidar_transfer_amd.config import ReturnModel
    rig = Rig(W)
    try:
        for label_image, ptrs, what in _variants():
            g = Guarded(W, label_image, ptrs)
            rig.render_hits(g)
            more = post.return_model(rig.sc, rig.rays_t, ReturnModel(max_range=NEAR_GATE), 3, g.out, label_image=label_image)
            g.check_all_misses(f"return model W={W} {what}")
            assert (more["drop"].cpu().numpy() == 3).all()   # every cell: too far
        rig.sc.status()
    finally:
        rig.close()


@pytest.mark.parametrize("W", WIDTHS)
def test_noise_model_with_every_range_outside_its_gate(W):
    from lidar_transfer_amd import post
    from lidar_transfer_amd.config import NoiseModel, ReturnModel
    rig = Rig(W)
    try:
        for label_image, ptrs, what in _variants():
            g = Guarded(W, label_image, ptrs)
            rig.render_hits(g)
            # sigma 1 cm, |z| <= 6: a range of 4 m and more stays far beyond the gate's 1 m
            more = post.noise_model(wc.ORIGIN, NoiseModel(0.01), 3, g.out, gate=ReturnModel(max_range=NEAR_GATE),
                                    label_image=label_image)
            g.check_all_misses(f"noise model W={W} {what}")
            assert (more["noise_state"].cpu().numpy() == 2).all()   # every cell: lost
    finally:
        rig.close()


def _one_subhit(n, S=2):
    """sub-images of S planes over n cells: plane 0 a hit of face 0 at 4.5 m, the other planes misses"""
    rng = np.zeros(S * n, np.float32)
    tri = np.full(S * n, -1, np.int32)
    lab = np.zeros(S * n, np.int32)
    rem = np.zeros(S * n, np.float32)
    rng[:n], tri[:n], lab[:n], rem[:n] = 4.5, 0, 40, 0.5
    return dict(range=_up(rng), tri=_up(tri), endcolors=_up(lab), endrem=_up(rem))


@pytest.mark.parametrize("W", WIDTHS)
def test_echo_resolve_with_too_few_subhits(W):
    from lidar_transfer_amd import post
    from lidar_transfer_amd.config import EchoModel
    rays = _up(wc.wall(1, W)[1])
    sub = _one_subhit(W)
    for ptrs in POINTER_SETS:   # (the resolve writes the label image only)
        g = Guarded(W, True, ptrs)
        more = post.echo_resolve(rays, wc.ORIGIN, EchoModel(0.2, 2, min_subrays=2), sub, g.out)
        g.check_all_misses(f"echo resolve W={W} ptrs={','.join(ptrs)}")
        assert (more["n_echoes"].cpu().numpy() == 0).all() and (more["echo_fraction"].cpu().numpy() == 0).all()


@pytest.mark.parametrize("W", WIDTHS)
def test_dual_resolve_second_set_with_one_echo(W):
    from lidar_transfer_amd import post
    from lidar_transfer_amd.config import DualReturn, EchoModel
    rays = _up(wc.wall(1, W)[1])
    sub = _one_subhit(W)
    for ptrs in POINTER_SETS:
        first, second = Guarded(W, True, wc.KEYS), Guarded(W, True, ptrs)
        more = post.echo_resolve_dual(rays, wc.ORIGIN, EchoModel(0.2, 2, min_subrays=1), DualReturn("last"), sub, first.out,
                                      second.out)
        second.check_all_misses(f"dual resolve, second set W={W} ptrs={','.join(ptrs)}")
        assert (more["n_echoes"].cpu().numpy() == 1).all() and (first.out["tri"].cpu().numpy() == 0).all()
        assert (more["echo_fraction2"].cpu().numpy() == 0).all()
