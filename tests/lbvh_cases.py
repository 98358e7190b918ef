"""Inputs that drive the least-travelled code of the LBVH traversal (lidar_transfer_amd/csrc/lt_trace.hip), and a
replay of its walk.  Imports without a GPU: tests/test_lbvh_cases_cpu.py pins the generators against the oracle's LBVH
model, tests/test_lbvh_paths_gpu.py runs them on the device.

* deep_staircase(n_cluster): a 30-level Karras chain that ends in a balanced cluster, every box on the way around one
  point c*; a ray through c* defers a child at every level, so its stack passes LT_STACK_LDS / LT_STACK4_LDS.
  With tilted=True the cluster's triangles do not tie, so that the image depends on the whole walk.
* identical(n), cluster_stairs(rng), adversarial_soup(rng, n): the scenes of tests/test_trace_gpu.py.
* same_box(n, rng), same_box_pinned(n, rng): n different triangles in the one box of identical(n), the second with
  identical(n)'s balanced tree: the nearest face of a ray is any of the n, not the one met first.
* replay_identical(nodes4, cap): on identical(n) the walk of a ray that meets the one box is a function of the node
  array alone; the replay restates k_trace4's first `cap` steps and k_trace4_tail's rounds over it.  replay(nodes4, cap,
  order) is the same walk for any ray that no hit can shorten, slab_order(nodes4, origin, d) the kernels' choice among
  the children of every node for one ray.
"""
import collections
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    """A constant of lt_internal.h, from the source."""
    with open(os.path.join(ROOT, "lidar_transfer_amd", "csrc", "lt_internal.h")) as f:
        m = re.search(r"^#define %s\s+(\d+)\b" % name, f.read(), re.M)
    return int(m.group(1))


LT_STACK_LDS = _define("LT_STACK_LDS")
LT_STACK_MAX = _define("LT_STACK_MAX")
LT_STACK4_LDS = _define("LT_STACK4_LDS")
LT_STACK4_MAX = _define("LT_STACK4_MAX")
LT_TAIL_STACK = _define("LT_TAIL_STACK")
LT_TAIL_DFS = _define("LT_TAIL_DFS")
LT_TRACE4_STEP_CAP = _define("LT_TRACE4_STEP_CAP")
LT_TRACE_DEBUG_STEPS = 0x4000   # internal trace flag (lt_internal.h): `tri` receives the steps of each ray, cap off
UNUSED = 0x7FFFFFFF             # reference of a child slot that does not exist

# image shapes (H, W, extra rays) for the hand-over; the last has n_rays % H != 0: W = n_rays / H truncates and the
# trailing rays stay untouched
IMAGE_SHAPES = ((1, 1, 0), (3, 5, 0), (4, 4, 0), (5, 8, 0), (8, 33, 0), (5, 8, 3))


# ---- meshes -----------------------------------------------------------------------------------------------------------
def mesh_of(tri, rng):
    """triangle soup [n, 3, 3] -> (verts f32, faces i32, colors i32, rem f32) with seeded attributes"""
    n = len(tri)
    v = np.ascontiguousarray(np.asarray(tri).reshape(-1, 3).astype(np.float32))
    f = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
    c = rng.integers(0, 256, (3 * n, 3)).astype(np.int32)
    r = rng.uniform(0, 1, 3 * n).astype(np.float32)
    return v, f, c, r


def adversarial_soup(rng, n):
    cen = rng.normal(size=(n, 3)) * rng.choice([0.05, 0.5, 5.0, 40.0], size=(n, 1))
    size = rng.choice([0.01, 0.1, 1.0, 20.0], size=(n, 1, 1))
    tri = cen[:, None, :] + rng.normal(size=(n, 3, 3)) * size
    k = n // 15
    tri[:k, :, 1] = 0.0                          # edge-on: in the plane y = 0 through the sensor
    tri[k:2 * k, :, 2] = tri[k:2 * k, :1, 2]     # horizontal triangles (many contain the vertical axis)
    tri[2 * k:3 * k, 1, :2] = tri[2 * k:3 * k, 0, :2]   # vertical walls: two vertices above each other
    tri[3 * k:4 * k, :, 0] = -np.abs(tri[3 * k:4 * k, :, 0])  # behind the sensor: straddle azimuth +-pi
    tri[3 * k:4 * k, 0, 1] = -np.abs(tri[3 * k:4 * k, 0, 1]) - 1e-3
    tri[3 * k:4 * k, 1, 1] = np.abs(tri[3 * k:4 * k, 1, 1]) + 1e-3
    # beyond the reference's initial t = 999999999.f (BVH.cpp:20): must stay misses
    nf = min(8, n - 4 * k)
    far = rng.normal(size=(nf, 1, 3)); far /= np.linalg.norm(far, axis=2, keepdims=True)
    tri[4 * k:4 * k + nf] = far * 3e9 + rng.normal(size=(nf, 3, 3)) * 1e9
    v = np.ascontiguousarray(tri.reshape(-1, 3).astype(np.float32))
    f = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
    c = rng.integers(0, 256, (3 * n, 3)).astype(np.int32)
    r = rng.uniform(0, 1, 3 * n).astype(np.float32)
    return v, f, c, r


ONE = np.array([[4.0, -1.0, -1.0], [4.0, 1.0, -1.0], [4.0, 0.0, 1.5]])   # seen from the origin along +x


def identical(n):
    """n copies of one triangle [n, 3, 3]: one Morton key, the tree is decided by the index tie-break alone, every
    existing child of every node has the same box"""
    return np.repeat(ONE[None], n, axis=0)


SAME_BOX_DX = 5e-4


def plane_offsets(rng, n):
    """[n, 3] offsets in [0, 1] for the three vertices of n triangles: one vertex at 0, one at 1, one anywhere -- n different
    planes through one box"""
    abc = np.stack([np.zeros(n), np.ones(n), rng.uniform(0.0, 1.0, n)], 1)
    return rng.permuted(abc, axis=1)


def same_box(n, rng):
    """n different triangles with the box of identical(n)'s one: a corner of the box, a point on the opposite side edge
    and a point on the top edge, mirrored in y for every second one, vertex k moved by offset * SAME_BOX_DX along x.
    Every node of the tree has the same box again, so the walk is replay_identical's (over the tree of THESE keys), but
    the triangles cover different parts of the box at different depths: the nearest one of a ray may be any of the n and
    a stack entry lost anywhere on the walk changes the image (on identical(n) face 0, met first, wins every tie)."""
    tri = identical(n)
    tri[:, :, 0] += plane_offsets(rng, n) * SAME_BOX_DX
    tri[:, 1, 2] = rng.uniform(-1.0, 1.5, n)      # vertex 1 anywhere on the edge y = 1
    tri[:, 2, 1] = rng.uniform(-1.0, 1.0, n)      # vertex 2 anywhere on the edge z = 1.5
    tri[rng.random(n) < 0.5, :, 1] *= -1.0
    return tri


PIN_LO, PIN_HI = -1000.0, 5000.0   # Morton cells of 6000 / 1024 = 5.86: the cell walls nearest the box are at -3.9 and 1.95


def same_box_pinned(n, rng):
    """same_box(n) between two tiny triangles at (-1000, -1000, -1000) and (5000, 5000, 5000), which make the Morton cells
    so large that the n centroids share one: the n triangles get one key, and below the two nodes that split the pins off
    the tree is identical(n)'s -- decided by the index alone, balanced, every box the same -- while the nearest triangle of
    a ray may be any of the n.  The boxes that hold a pin hold the origin too; replay() with slab_order() walks them."""
    eps = 0.5
    lo = PIN_LO + np.array([[0, 0, 0], [eps, 0, 0], [0, eps, 0]], np.float64)
    hi = PIN_HI - np.array([[0, 0, 0], [eps, 0, 0], [0, eps, 0]], np.float64)
    return np.concatenate([lo[None], same_box(n, rng), hi[None]])


def cluster_stairs(rng, levels=14, copies=600):
    """a staircase of clusters at x = 30 * 2^-k, `copies` jittered copies each: a chain of wide nodes, one per key bit"""
    stairs = []
    for k in range(levels):
        base = ONE * [1.0, 0.2, 0.2] + [30.0 * 2.0 ** -k, 0.0, 0.0]
        stairs.append(np.repeat(base[None], copies, axis=0) + rng.normal(size=(copies, 1, 3)) * 1e-4)
    return stairs


def rays_along_x(rng, n_rays):
    """rays for identical / cluster_stairs, from the origin: around +x, every second one inside the +-0.05 rad the
    stairs subtend; ray 0 is the axis itself"""
    spread = np.where(np.arange(n_rays)[:, None] % 2 == 0, 0.25, 0.03)
    rays = (np.array([1.0, 0.0, 0.0]) + rng.normal(size=(n_rays, 3)) * spread * [0.0, 1.0, 1.0]).astype(np.float32)
    rays[0] = [1.0, 0.0, 0.0]
    return rays


# ---- the deep staircase -------------------------------------------------------------------------------------------------
CUBE = 64.0
CELL = CUBE / 1024.0
C_STAR = np.full(3, 1023.5 * CELL)          # centre of cell (1023, 1023, 1023): exact in float32
STAIR_ORIGIN = (3.0, 5.0, 1.0)
N_CHAIN = 30
STAIR_FIRST_SPLIT = 2                       # faces: 0, 1 the pins, 2 .. 31 the split-offs, 32 .. the cluster


def split_cell(m):
    """cell of split-off m: bit 9 - m // 3 of coordinate m % 3 cleared, so that its 30-bit Morton key (x, y, z bits
    interleaved from the top) shares exactly m leading bits with the cluster's key of thirty ones"""
    cell = [1023, 1023, 1023]
    cell[m % 3] &= ~(1 << (9 - m // 3))
    return cell


def deep_staircase(n_cluster, tilted=False):
    """-> (verts, faces, colors, rem) of 2 pins + 30 split-offs + n_cluster identical (or `tilted`) triangles inside [0, 64]^3.

    Sorted by key the split-offs come first, in order, then the cluster: node m of the Karras tree splits the leaf
    "split-off m" from everything behind it.  Split-off m is a sliver along axis m % 3 from deep inside the cube to
    0.2 cell past c*, 0.2 cell thin on the other two axes: its centroid lies in split_cell(m), its box holds c*.  The
    box of "everything behind it" is long on all three axes while the sliver's is thin on two, so a ray through c*
    enters the rest first and defers the sliver: one entry per chain level, then one per level of the balanced cluster.
    No vertex leaves the cube (the pins at its corners fix the Morton scale at 16 cells per unit)."""
    rng = np.random.default_rng(4242)
    eps = 0.25 * CELL
    tri = [np.array([[0, 0, 0], [eps, 0, 0], [0, eps, 0]], np.float64),
           CUBE - np.array([[0, 0, 0], [eps, 0, 0], [0, eps, 0]], np.float64)]
    hi = 1023.7
    for m in range(N_CHAIN):
        a = m % 3
        k = split_cell(m)[a]
        lo = (3.0 * (k + 0.5) - hi) / 2.0                    # two vertices at lo, one at hi: centroid at k + 0.5
        t = np.empty((3, 3))
        t[:, a] = [lo, lo, hi]
        t[:, (a + 1) % 3] = [1023.4, 1023.6, 1023.6]
        t[:, (a + 2) % 3] = [1023.4, 1023.6, 1023.4]
        tri.append(t * CELL)
    d = C_STAR - np.asarray(STAIR_ORIGIN)
    d /= np.linalg.norm(d)
    u = np.cross(d, [0.0, 0.0, 1.0]); u /= np.linalg.norm(u)
    w = np.cross(d, u)
    ang = np.arange(3) * (2 * np.pi / 3)
    one = C_STAR + 0.45 * CELL * (np.cos(ang)[:, None] * u + np.sin(ang)[:, None] * w)   # faces the rays, inside the cell
    cluster = np.repeat(one[None], n_cluster, axis=0)
    if tilted:
        # each cluster triangle tilted its own way, vertices up to 0.02 cell before or behind c* along the ray: the nearest
        # one of a ray may be any of them, so a stack entry lost anywhere in the cluster changes the image (with identical
        # triangles the first face of the cluster wins every tie)
        cluster += (plane_offsets(rng, n_cluster) - 0.5)[:, :, None] * (0.04 * CELL) * d
    tri = np.concatenate([np.stack(tri), cluster])
    assert tri.min() >= 0.0 and tri.max() <= CUBE
    return mesh_of(tri, rng)


def staircase_rays(n_rays):
    """every fourth ray runs exactly from STAIR_ORIGIN through c*, the others get normal jitter of 0.02 on the
    (unnormalised) direction: a third of a cell at c*"""
    rng = np.random.default_rng(99)
    d = (C_STAR - np.asarray(STAIR_ORIGIN)).astype(np.float32)
    rays = (d + rng.normal(size=(n_rays, 3)) * 0.02).astype(np.float32)
    rays[::4] = d
    return rays


def morton_keys(v, f):
    """the 30-bit Morton code of every face, as the build computes it (float32; oracle/lt_lbvh_model.h: scene bounds over
    all vertices, centroid ((v0 + v1) + v2) / 3, 10 bits per axis, x bit first)"""
    v = np.asarray(v, np.float32)
    lo, hi = v.min(0), v.max(0)
    ext = np.float32((hi - lo).max())
    scale = np.float32(1024.0) / ext if ext > 0 else np.float32(0.0)
    t = v[np.asarray(f)]
    cen = ((t[:, 0] + t[:, 1]) + t[:, 2]) / np.float32(3.0)
    q = np.clip((cen - lo) * scale, np.float32(0.0), np.float32(1023.0)).astype(np.uint32)
    key = np.zeros(len(q), np.uint32)
    for b in range(10):
        for a in range(3):
            key |= ((q[:, a] >> b) & 1) << np.uint32(3 * b + (2 - a))
    return key


# ---- the scenes of the suite, by name -----------------------------------------------------------------------------------
SCENES = ("deep_staircase", "deep_staircase_tilted", "identical", "same_box", "soup", "stairs")
N_STAIR_CLUSTER = 16384
N_IDENTICAL = 20000


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> ((verts, faces, colors, rem), origin)"""
    if name == "deep_staircase":
        return deep_staircase(N_STAIR_CLUSTER), STAIR_ORIGIN
    if name == "deep_staircase_tilted":
        return deep_staircase(N_STAIR_CLUSTER, tilted=True), STAIR_ORIGIN
    if name == "identical":
        return mesh_of(identical(N_IDENTICAL), np.random.default_rng(5)), (0.0, 0.0, 0.0)
    if name == "same_box":
        rng = np.random.default_rng(6)
        return mesh_of(same_box(N_IDENTICAL, rng), rng), (0.0, 0.0, 0.0)
    if name == "soup":
        return adversarial_soup(np.random.default_rng(7), 3000), (0.3, -0.2, 0.1)
    if name == "stairs":
        rng = np.random.default_rng(77)
        return mesh_of(np.concatenate(cluster_stairs(rng)), rng), (0.0, 0.0, 0.0)
    raise KeyError(name)


def scene_rays(name, n_rays):
    """the rays a scene is looked at with; the first rays of a longer set are the shorter set"""
    if name.startswith("deep_staircase"):
        return staircase_rays(n_rays)
    if name == "soup":
        return np.random.default_rng(8).normal(size=(n_rays, 3)).astype(np.float32)
    return rays_along_x(np.random.default_rng(9), n_rays)


# ---- the walk over a 4-wide node array----------------------------------------------------------------------------------
def node_children(nodes4, node):
    """references of the existing children of a node of lt_debug_nodes4_get's array ([n, 32] uint32; child j: its box in
    words 8j .. 8j+5, its reference in word 8j+6), in lane order.  >= 0: a node, < 0: a leaf."""
    refs = [int(r) & 0xFFFFFFFF for r in nodes4[node, 6::8]]
    return [r - (1 << 32) if r >> 31 else r for r in refs if r != UNUSED]


def tree_depth(nodes4):
    """node levels on the longest path from the root (the root alone: 1)"""
    depth, level = 0, [0]
    while level:
        depth += 1
        level = [c for n in level for c in node_children(nodes4, n) if c >= 0]
    return depth


def slab_order(nodes4, origin, d):
    """-> order(node): the references of the children of `node` that ONE ray (origin, normalised direction d, float32)
    meets, nearest first -- the kernels' slab test and (entry distance, lane) rank, operation by operation in float32, for
    all nodes at once.  No hit is taken into account: replay() with this order is the walk of a ray that no hit can
    shorten.  On deep_staircase every box of the tree holds c*, so a ray through c* meets each of them no farther away
    than any of its hits; on same_box_pinned every box a ray meets begins in front of every triangle."""
    boxes = nodes4.view(np.float32).reshape(-1, 4, 8)
    refs = nodes4.reshape(-1, 4, 8)[:, :, 6].astype(np.int64)
    refs = np.where(refs >> 31 != 0, refs - (1 << 32), refs)
    o = np.asarray(origin, np.float32)
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / np.asarray(d, np.float32)
        l1 = (boxes[:, :, 0:3] - o) * inv
        l2 = (boxes[:, :, 3:6] - o) * inv
        lo, hi = np.fmin(l1, l2), np.fmax(l1, l2)
        tn = np.fmax(np.fmax(lo[..., 0], lo[..., 1]), np.fmax(lo[..., 2], np.float32(0.0)))
        tf = np.fmin(np.fmin(hi[..., 0], hi[..., 1]), np.fmin(hi[..., 2], np.float32(999999999.0)))
        hit = (tn <= tf) & (refs != UNUSED)
    key = np.where(hit, (tn.view(np.uint32).astype(np.int64) & ~3) | np.arange(4), 1 << 40)
    rank = np.argsort(key, axis=1, kind="stable")
    ranked = np.take_along_axis(refs, rank, axis=1)
    count = hit.sum(1)
    return lambda node: [int(r) for r in ranked[node, :count[node]]]


Replay = collections.namedtuple("Replay", "high_water rounds saved_sp quad_sp steps")


def replay(nodes4, cap, order, tail_dfs=LT_TAIL_DFS):
    """The walk of k_trace4 and k_trace4_tail over a node array when `order(node)` gives the children a node step goes on
    with, nearest first, and nothing is ever culled.

    First `cap` steps as k_trace4 takes them (cap <= 0: no cap): a node step goes on with the nearest child and pushes
    the others so that rank 1 ends on top, a leaf step pops.  If the walk is not over, its stack plus the reference it
    was about to visit go to k_trace4_tail: a round takes min(sp, 16) entries -- one above `tail_dfs` --, quad q reads
    stk[sp - 1 - q], and the children of quad q land at sp + above + (nh - 1 - rank), `above` counting the children of
    the quads q + 1 .. 15.

    -> Replay(high-water mark of the tail's stack (0: not handed over), rounds of the tail, entries saved at the
       hand-over, high-water mark of the quad's own stack, steps taken by k_trace4)"""
    done = None
    cur, stack, steps, quad_sp = 0, [], 0, 0
    while cur is not done and (cap <= 0 or steps < cap):
        steps += 1
        ch = order(cur) if cur >= 0 else []
        if ch:
            stack.extend(reversed(ch[1:]))      # slot sp + (nh - 1 - rank): rank nh - 1 lowest, rank 1 on top
            quad_sp = max(quad_sp, len(stack))
            cur = ch[0]
        else:
            cur = stack.pop() if stack else done
    if cur is done:
        return Replay(0, 0, 0, quad_sp, steps)
    stk = stack + [cur]
    sp = saved = high = len(stk)
    rounds = 0
    while sp > 0:
        take = 1 if sp > tail_dfs else min(sp, 16)
        kids = [order(r) if r >= 0 else [] for r in (stk[sp - 1 - q] for q in range(take))]
        sp -= take
        del stk[sp:]
        total = sum(len(k) for k in kids)
        new = [done] * total
        for q, ch in enumerate(kids):
            above = sum(len(k) for k in kids[q + 1:])
            for rank, ref in enumerate(ch):
                new[above + (len(ch) - 1 - rank)] = ref
        stk.extend(new)
        sp += total
        high = max(high, sp)
        rounds += 1
    return Replay(high, rounds, saved, quad_sp, steps)


def replay_identical(nodes4, cap, tail_dfs=LT_TAIL_DFS):
    """The walk of a ray that meets the box of identical(n), from the node array alone: every existing child of every
    node has that box and is met at the same distance, so the rank of a child is its lane."""
    return replay(nodes4, cap, lambda node: node_children(nodes4, node), tail_dfs)
