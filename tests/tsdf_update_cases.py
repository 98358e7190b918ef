"""Constructed inputs for the per-voxel TSDF update (lidar_transfer_amd/csrc/lt_tsdf.hip) off the `obs_weight = 1` path, and
two numpy restatements.  numpy only, imports without a GPU: tests/test_tsdf_update_cases_cpu.py proves that the cases reach
the arms they are named for (a census with the C oracle, oracle/lt_tsdf_oracle.c) and pins the restatements;
tests/test_tsdf_update_gpu.py holds the product to the oracles on these inputs.

Why these values.  With `obs_weight = 1` every weight in the volume is a small integer, every `old * w_old` is exact, a fused
and an unfused multiply-add agree and the class-aware comparison `dist < dist_old` -- which the reference makes against the
WEIGHT volume -- only tells a voxel without a weight from one with a weight (dist <= 1 <= w).  Labels in one channel with even
sums never meet a rounding tie, never reach the clamp at 255 and never average the g and r channels.

Geometry (every case): voxel 0.25 m, 65 x 63 x 24 voxels -- 4095 columns = 63 * 64 + 63, the last chunk of 64 columns is
partial; the voxel (32, 32, 12) lies at the sensor itself -- field of view (10, -25) degrees, images 16 x 96.  The pixel-driven
integrate applies here (tsdf_pix_applies: the class-aware flag, a field of view below +-80 degrees, and 30 - ceil(log2(96)) =
23 >= 12 bits left for the rho quantum), so no wider image is needed.
"""
import functools

import numpy as np

f32, f64 = np.float32, np.float64

VOXEL = 0.25
BNDS = np.array([[-8.0, 8.25], [-8.0, 7.75], [-3.0, 3.0]])
DIMS = (65, 63, 24)
ORIGIN = BNDS[:, 0].astype(f32)
FOV_UP, FOV_DOWN = 10.0, -25.0
H, W = 16, 96
TRUNC = VOXEL * 5

# (b, g, r) before folding
CLASSES = np.array([(0, 0, 0),
                    (40, 0, 0), (41, 0, 0),     # 40 + 41: a tie at equal weights
                    (41, 3, 200),
                    (0, 1, 0), (0, 0, 1),
                    (255, 255, 255),
                    (259, 0, 7),                # b needs the clamp
                    (259, 3, 201)],             # folds to 16 974 793 > 2^24: not a float32 (-> ...792, the even neighbour)
                   dtype=f32)

# class 0 -- the fresh volume's own colour, the only one a FRESH voxel integrates as "same class" -- on 3 pixels in 10: a voxel
# reaches weight 3 w (the first weight whose product with tsdf is inexact at w = 2^24) only through three such updates
CLASS_P = np.array([0.3] + [0.7 / 8] * 8)

W24 = 16777216.0   # 2^24: `tsdf * w_old + dist` loses dist below half an ulp of the product
WEIGHTS = (1.0, 0.25, 0.7, 2.5, W24)


def _wname(w):
    return "2p24" if w == W24 else str(w)


def _case(name, merge=True, weight=1.0, n_obs=4, broken=False, mode="cuda"):
    return dict(name=name, merge=merge, weight=weight, n_obs=n_obs, broken=broken, mode=mode)


CASES = {}
for _w in WEIGHTS:
    CASES[f"A-{_wname(_w)}"] = _case(f"A-{_wname(_w)}", True, _w)            # class-aware
for _w in WEIGHTS:
    CASES[f"B-{_wname(_w)}"] = _case(f"B-{_wname(_w)}", False, _w)           # plain average
CASES["C-merge"] = _case("C-merge", True, 0.7, broken=True)                   # NaN / infinite depth pixels
CASES["C-plain"] = _case("C-plain", False, 0.7, broken=True)
CASES["D-nine"] = _case("D-nine", True, 0.7, n_obs=9)                         # one fused pass of eight, then the single path
for _w in (1.0, 0.25, 2.5):
    CASES[f"E-{_wname(_w)}"] = _case(f"E-{_wname(_w)}", False, _w, n_obs=2, mode="numpy")   # host mode

DEVICE_CASES = [k for k, c in CASES.items() if c["mode"] == "cuda"]
HOST_CASES = [k for k, c in CASES.items() if c["mode"] == "numpy"]


def fold(label3):
    """The three label channels in one float32 per pixel, operation by operation as `integrate` folds them
    (floor(c0 * 256 * 256 + c1 * 256 + c2) in float32).  (259, 3, 201) comes out as 16 974 792: every implementation is
    handed this rounded value."""
    c = np.asarray(label3, f32)
    return np.floor(c[:, :, 0] * f32(256) * f32(256) + c[:, :, 1] * f32(256) + c[:, :, 2]).astype(f32)


@functools.lru_cache(maxsize=None)
def _observations(n_obs, broken):
    rng = np.random.default_rng(20)
    rng_broken = np.random.default_rng(21)     # its own stream: the broken pixels change nothing else
    yaw = np.linspace(-np.pi, np.pi, W)
    obs, idx = [], None
    for k in range(n_obs):
        # surfaces 4 .. 7 m away that step by about a metre from one observation to the next; the truncation band is
        # 1.25 m deep, so consecutive bands overlap partly
        shift = (0.0, 1.0, 0.0, -1.0)[k % 4]
        depth = (5.5 + 0.5 * np.sin(2 * yaw + 0.3 * k)[None, :] + shift + 0.2 * (rng.random((H, W)) - 0.5)).astype(f32)
        depth[rng.random((H, W)) < 0.05] = 0.0
        if broken:
            depth[rng_broken.random((H, W)) < 0.005] = np.nan
            depth[rng_broken.random((H, W)) < 0.005] = np.inf
        depth[:, 36:40] = -1.0                 # "no data": with a 1.25 m margin the voxels next to the sensor are written
        new = rng.choice(len(CLASSES), (H, W), p=CLASS_P)
        idx = new if idx is None else np.where(rng.random((H, W)) < 0.5, idx, new)   # half keep their class
        label3 = CLASSES[idx]
        rem = rng.uniform(0.0, 255.0, (H, W)).astype(f32)
        u = rng.random((H, W))
        rem[u < 0.1] = 0.0
        rem[(u >= 0.1) & (u < 0.2)] = -1.0     # the reference's "no data" value
        rem[(u >= 0.2) & (u < 0.22)] = 255.0
        for a in (label3, depth, rem):
            a.setflags(write=False)
        obs.append((label3, depth, rem))
    return tuple(obs)


def observations(case):
    """The case's observations [(label3 [H,W,3], depth [H,W], rem [H,W]) float32, ...] -- shared and read-only."""
    c = CASES[case] if isinstance(case, str) else case
    return _observations(c["n_obs"], c["broken"])


def fresh_volumes(dims=DIMS):
    return [np.ones(dims, f32), np.zeros(dims, f32), np.zeros(dims, f32), np.zeros(dims, f32)]


# ---- restatement 1: the update alone ------------------------------------------------------------------------------------

ARM_NONE, ARM_PLAIN, ARM_SAME, ARM_WINS, ARM_REJECTED = 0, 1, 2, 3, 4


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays.  The product of two float32 is exact in float64; the sum is rounded to float64 and
    then to float32.  The two roundings disagree with the single one only where the float64 sum lands exactly on the midpoint
    of two float32 while the exact sum does not: the sum's rounding error (TwoSum) says on which side the exact value lies."""
    p = np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)
    c = np.asarray(c, f32).astype(f64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
    bits = np.ascontiguousarray(s).view(np.int64)
    mid = ((bits & 0x1FFFFFFF) == 0x10000000) & np.isfinite(s) & (e != 0)
    s = np.where(mid, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    with np.errstate(over="ignore"):
        return s.astype(f32)


def round_half_away(x):
    """roundf."""
    x = np.asarray(x, f32).astype(f64)
    t = np.trunc(x)
    return (t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0.0)).astype(f32)


def unfold(color):
    """(b, g, r) of a folded colour, as every update body takes it apart (float32; b is not bounded by 255)."""
    color = np.asarray(color, f32)
    b = np.floor(color / f32(65536))
    g = np.floor((color - b * f32(65536)) / f32(256))
    r = color - b * f32(65536) - g * f32(256)
    return b, g, r


def update(old, hit, dist, new_color, new_rem, obs_weight, merge):
    """One observation's update of every voxel, given what the projection found: `old` = (tsdf, weight, colour, remission),
    `hit` the voxels that pass the depth tests, and per voxel the truncated distance, the folded colour and the remission of
    its pixel.  Both branches of the update, operation by operation in float32 with the multiply-adds fused.  Returns the
    new four arrays and a dict: `arm` (ARM_*) and, for the plain branch, `avg` -- the three channel averages before rounding."""
    t0, w0, c0, r0 = [np.asarray(a, f32) for a in old]
    dist, new_color, new_rem = np.asarray(dist, f32), np.asarray(new_color, f32), np.asarray(new_rem, f32)
    ow = f32(obs_weight)
    arm = np.zeros(t0.shape, np.int8)
    with np.errstate(all="ignore"):
        w_new = w0 + ow
        t_avg = fma32(t0, w0, dist) / w_new
        r_avg = fma32(r0, w0, new_rem) / w_new
        nb, ng, nr = unfold(new_color)
        if not merge:
            ob, og, orr = unfold(c0)
            avg = [fma32(o, w0, n) / w_new for o, n in ((ob, nb), (og, ng), (orr, nr))]
            b, g, r = [np.fmin(round_half_away(a), f32(255)) for a in avg]
            c_new = b * f32(65536) + g * f32(256) + r
            arm[hit] = ARM_PLAIN
            out = [np.where(hit, n, o) for n, o in ((t_avg, t0), (w_new, w0), (c_new, c0), (r_avg, r0))]
            return out, dict(arm=arm, avg=np.stack(avg))
        same = hit & (c0 == new_color)
        wins = hit & ~same & (dist < w0)          # sic: the distance against the WEIGHT volume
        arm[same] = ARM_SAME
        arm[wins] = ARM_WINS
        arm[hit & ~same & ~wins] = ARM_REJECTED
        c_new = nb * f32(65536) + ng * f32(256) + nr
        out = [np.where(same, t_avg, np.where(wins, dist, t0)), np.where(same, w_new, w0),
               np.where(wins, c_new, c0), np.where(same, r_avg, np.where(wins, new_rem, r0))]
        return out, dict(arm=arm)


# ---- restatement 2: the host-mode contract (LT_TSDF_HOST_MODE, include/lidarhip.h; k_tsdf_integrate_host_mode) ------------

def host_mode_integrate(vols, origin, voxel_size, fov_up_deg, fov_down_deg, color_im, depth_im, obs_weight=1.0):
    """One observation into `vols` = [tsdf, weight, colour, remission] (float32 [dx, dy, dz], updated in place) by the
    contract of LT_TSDF_HOST_MODE: the voxel is projected in float64 (float32 origin + index * float64 voxel size) and the
    field of view is tested on the float64 pitch, both limits exclusive; a pixel counts with `depth_val > 0` and a distance
    of at least minus the truncation margin of five voxels; tsdf is the plain running average with the float32 product
    `tsdf * w_old`, the sum and the quotient in float64, stored as float32; the colour is averaged per channel in float32
    (product, sum, quotient: three roundings), rounded half to even and clamped at 255; remissions stay as they are.
    `color_im` is folded.  Returns dict(hit, avg [3, ...]: the channel averages before rounding)."""
    tsdf, weight, color, _ = vols
    dx, dy, dz = tsdf.shape
    org = np.asarray(origin, f32).astype(f64)
    vs = float(voxel_size)
    im_h, im_w = depth_im.shape
    x = (org[0] + np.arange(dx) * vs)[:, None, None]
    y = (org[1] + np.arange(dy) * vs)[None, :, None]
    z = (org[2] + np.arange(dz) * vs)[None, None, :]
    fu, fd = fov_up_deg / 180.0 * np.pi, fov_down_deg / 180.0 * np.pi
    with np.errstate(all="ignore"):
        depth = np.sqrt(x * x + y * y + z * z)
        yaw = -np.arctan2(y, x) + 0.0 * depth
        pitch = np.arcsin(z / depth)
        proj_x = 0.5 * (yaw / np.pi + 1.0) * im_w
        proj_y = (1.0 - (pitch + abs(fd)) / (abs(fd) + abs(fu))) * im_h
        ok = ~(np.isnan(proj_x) | np.isnan(proj_y)) & (pitch < fu) & (pitch > fd)
        px = np.clip(np.floor(np.where(ok, proj_x, 0.0)), 0, im_w - 1).astype(np.int64)
        py = np.clip(np.floor(np.where(ok, proj_y, 0.0)), 0, im_h - 1).astype(np.int64)
        depth_val = np.asarray(depth_im, f32).astype(f64)[py, px]
        trunc = vs * 5
        diff = depth_val - depth
        hit = ok & (depth_val > 0.0) & (diff >= -trunc)
        dist = np.minimum(1.0, diff / trunc)
        ow = f32(obs_weight)
        w_new = weight + ow
        tw = tsdf * weight                                               # float32
        t_new = ((tw.astype(f64) + dist) / w_new.astype(f64)).astype(f32)
        ob, og, orr = unfold(color)
        nb, ng, nr = unfold(np.asarray(color_im, f32)[py, px])
        avg = [(o * weight + n) / w_new for o, n in ((ob, nb), (og, ng), (orr, nr))]   # float32, nothing fused
        b, g, r = [np.fmin(np.rint(a), f32(255)) for a in avg]                         # np.rint: half to even
        c_new = b * f32(65536) + g * f32(256) + r
    tsdf[hit], weight[hit], color[hit] = t_new[hit], w_new[hit], c_new[hit]
    return dict(hit=hit, avg=np.stack(avg))


@functools.lru_cache(maxsize=None)
def host_case(case):
    """The E case on the host-mode restatement: (volumes, number of channel averages on a tie that half-to-even and
    half-away-from-zero round differently, number of averages on x.5)."""
    c = CASES[case]
    vols = fresh_volumes()
    ties = on_half = 0
    for label3, depth, rem in observations(case):
        info = host_mode_integrate(vols, ORIGIN, VOXEL, FOV_UP, FOV_DOWN, fold(label3), depth, c["weight"])
        avg = info["avg"][:, info["hit"]]
        ties += int((np.rint(avg) != round_half_away(avg)).sum())
        on_half += int((avg - np.floor(avg) == 0.5).sum())
    return vols, ties, on_half
