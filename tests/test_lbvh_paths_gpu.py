"""Every path of the LBVH traversal (lidar_transfer_amd/csrc/lt_trace.hip), driven on purpose and shown to have run.

k_trace4 keeps LT_STACK4_LDS stack entries of a ray in LDS and spills the rest to HBM; a ray that is not done after the
step cap parks its stack -- LDS part and spilled part -- for k_trace4_tail, which walks it with a whole wave, 16 entries at
a time or one above LT_TAIL_DFS; two hand-over counters alternate between launches, each re-armed by the tail kernel of
the launch before.  The inputs of tests/lbvh_cases.py reach each of these: every case compares all five images bit for
bit with the brute-force oracle and asserts from the kernels' own numbers -- stack_overflows of a count=True trace, the
per-ray step image (internal flag 0x4000), the parked rays and the largest saved stack from lt_debug_trace_tail -- that
its path was taken: a case whose condition does not hold is a wrong input, not a pass.  The step cap and the binary twin
k_trace are chosen once per process (LIDARHIP_STEP_CAP, LIDARHIP_TRACE), so those cases run this file as a child
process, one after the other.  Counters observed: profiles/lbvh_paths/README.md."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import lbvh_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("tri", "range", "endpoints", "endcolors", "endrem")
SENTINEL = -7   # what the output images hold before a trace: rays beyond W * H must keep it


def _step_cap():
    """the cap of this process, as lt_trace_launch reads it (0: off)"""
    e = os.environ.get("LIDARHIP_STEP_CAP")
    return max(int(e), 0) if e else lc.LT_TRACE4_STEP_CAP


CAP = _step_cap()
BINARY = os.environ.get("LIDARHIP_TRACE") == "binary"


# ---- device side --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lib():
    from lidar_transfer_amd import _lib as L
    lib = L.load()
    lib.lt_debug_trace_tail.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.lt_debug_trace_tail.restype = C.c_int
    lib.lt_debug_nodes4_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.lt_debug_nodes4_get.restype = C.c_int
    return lib


def _built(mesh, sc=None):
    import torch
    from lidar_transfer_amd.raytracer import Scene
    sc = sc or Scene(0)
    sc.set_mesh(*[torch.from_numpy(np.ascontiguousarray(x)).to(sc.device) for x in mesh])
    sc.build()
    return sc


def _nodes4(sc, n_faces):
    a = np.empty((n_faces, 32), np.uint32)
    assert _lib().lt_debug_nodes4_get(sc._h, a.ctypes.data_as(C.c_void_p), n_faces) == 0
    return a


def _tail(sc):
    """(rays the last plain launch parked for k_trace4_tail, largest number of stack entries one of them saved)"""
    n, m = C.c_int(-1), C.c_int(-1)
    assert _lib().lt_debug_trace_tail(sc._h, C.byref(n), C.byref(m)) == 0
    return n.value, m.value


def _trace(sc, rays, origin, H, **kw):
    """Scene.trace into images that hold SENTINEL -> (numpy images, stats or None)"""
    import torch
    rays_t = torch.from_numpy(np.ascontiguousarray(rays)).to(sc.device)
    out = sc.alloc_outputs(rays.shape[0])
    for t in out.values():
        t.fill_(SENTINEL)
    o = sc.trace(rays_t, origin, H, out=out, **kw)
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in KEYS}, o.get("stats")


def _steps(sc, rays, origin, H):
    """steps of each ray's undisturbed walk (no cap, no hand-over); SENTINEL beyond W * H"""
    return _trace(sc, rays, origin, H, _extra_flags=lc.LT_TRACE_DEBUG_STEPS)[0]["tri"]


def _oracle(mesh, rays, origin, H):
    from oracle import binding as ob
    n = rays.shape[0] // H * H
    return ob.oracle_trace(rays[:n], np.asarray(origin, np.float32), *mesh, H, mode=ob.MODE_BRUTE, norm=ob.NORM_SSE_TABLE)


@functools.lru_cache(maxsize=None)
def _ref(name, n_rays, H):
    return _oracle(lc.scene(name)[0], lc.scene_rays(name, n_rays), lc.scene(name)[1], H)


def _assert_images(got, ref, what, keys=KEYS):
    n = ref["tri"].shape[0]
    for k in keys:
        a, b = got[k][:n], ref[k]
        assert a.shape == b.shape, f"{what} {k}"
        bad = np.nonzero(a.view(np.int32).reshape(-1) != b.view(np.int32).reshape(-1))[0]
        assert bad.size == 0, f"{what} {k}: {bad.size} of {a.size} elements differ, first at {bad[:5]}"
        assert np.all(got[k][n:] == SENTINEL), f"{what} {k}: rays beyond W * H were written"


def _parked_expected(steps, n_used):
    """a ray is parked if and only if its uncapped walk has more than CAP steps"""
    return int((steps[:n_used] > CAP).sum()) if CAP > 0 and not BINARY else 0


def run_case(name, H, W, extra=0):
    """One scene at one image shape in THIS process (its cap, its kernel): step image, count=True trace, plain trace, all
    against the oracle; the parked rays against the step image.  -> record of what ran"""
    t0 = time.time()
    mesh, origin = lc.scene(name)
    n_rays, n_used = H * W + extra, H * W
    rays = lc.scene_rays(name, n_rays)
    ref = _ref(name, n_rays, H)
    what = f"{name} {H}x{W}+{extra} cap {CAP}{' binary' if BINARY else ''}"
    rec = dict(case=name, H=H, W=W, extra=extra, cap=CAP, binary=BINARY)
    sc = _built(mesh)
    try:
        walk_steps = None
        if name in ("identical", "same_box") and not BINARY:
            # the tail's stack is written without a bound check: the replay on the device's own tree says how high this
            # walk gets BEFORE anything is launched on it
            nodes = _nodes4(sc, mesh[1].shape[0])
            rp, depth = lc.replay_identical(nodes, CAP), lc.tree_depth(nodes)
            assert rp.high_water <= 304 + 3 * depth < lc.LT_TAIL_STACK, (what, rp, depth)
            assert rp.quad_sp < lc.LT_STACK4_MAX
            walk_steps = lc.replay_identical(nodes, 0).steps
            rec.update(replay_high_water=rp.high_water, replay_rounds=rp.rounds, replay_saved=rp.saved_sp, depth4=depth)
        steps = None
        if not BINARY:
            steps = _steps(sc, rays, origin, H)
            assert np.all(steps[n_used:] == SENTINEL) and np.all(steps[:n_used] >= 0)
            rec.update(max_steps=int(steps[:n_used].max()))
            if walk_steps is not None:   # a ray meets the one box of the scene, or nothing: the replay IS the device's walk
                assert set(np.unique(steps[:n_used])) <= {1, walk_steps}, (what, np.unique(steps[:n_used]), walk_steps)
                assert steps[0] == walk_steps
        got, st = _trace(sc, rays, origin, H, count=True)
        _assert_images(got, ref, what + " count=True")
        assert st["n_hits"] == int((ref["tri"] >= 0).sum())
        got, _ = _trace(sc, rays, origin, H)
        _assert_images(got, ref, what)
        parked, saved = _tail(sc)
        assert parked == _parked_expected(steps, n_used), (what, parked)
        assert saved <= lc.LT_STACK4_MAX + 1
        if walk_steps is not None and parked:
            assert saved == rec["replay_saved"]
        if name == "identical":   # the lowest face index among the ties
            assert np.all(got["tri"][:n_used][ref["tri"] >= 0] == 0)
        rec.update(stack_overflows=int(st["stack_overflows"]), parked=parked, max_saved_sp=saved, n_used=n_used,
                   hits=int((ref["tri"] >= 0).sum()), seconds=round(time.time() - t0, 2))
    finally:
        sc.close()
    return rec


WRITEBACK_CASE = ("stairs", 5, 8, 3)   # 16 hits, 24 misses, 3 trailing rays; two ragged tiles of either kernel


def run_writeback_variants(name, H, W, extra):
    """What the write-back does besides the five full images, in THIS process (its kernel): the label image, hits only,
    two of the five images.  -> record of what ran"""
    import torch
    t0 = time.time()
    mesh, origin = lc.scene(name)
    n_rays, n = H * W + extra, H * W
    ref = _ref(name, n_rays, H)
    hit = ref["tri"] >= 0
    assert 0 < int(hit.sum()) < n, "the case needs hits and misses"
    what = f"{name} {H}x{W}+{extra}{' binary' if BINARY else ''}"
    sc = _built(mesh)
    try:
        rays_t = torch.from_numpy(np.ascontiguousarray(lc.scene_rays(name, n_rays))).to(sc.device)

        def cast(out, **kw):
            for t in out.values():
                t.fill_(SENTINEL)
            sc.trace(rays_t, origin, H, out=out, **kw)
            torch.cuda.synchronize()
            return {k: t.cpu().numpy() for k, t in out.items()}

        # label_image: endcolors is [R], channel 2 of the colours
        got = cast(sc.alloc_outputs(n_rays, label_image=True), label_image=True)
        assert got["endcolors"].shape == (n_rays,)
        _assert_images(got, dict(ref, endcolors=ref["endcolors"][:, 2]), what + " label_image")
        # write_misses=False: nothing is written where nothing was hit
        got = cast(sc.alloc_outputs(n_rays), write_misses=False)
        for k in KEYS:
            assert np.array_equal(got[k][:n][hit].view(np.int32), ref[k][hit].view(np.int32)), f"{what} hits only {k}"
            assert np.all(got[k][:n][~hit] == SENTINEL), f"{what} hits only {k}: a missed cell was written"
            assert np.all(got[k][n:] == SENTINEL), f"{what} hits only {k}: rays beyond W * H were written"
        # two images wanted, null pointers for the other three
        full = sc.alloc_outputs(n_rays)
        got = cast({k: full[k] for k in ("range", "tri")})
        _assert_images(got, ref, what + " range and tri only", keys=("range", "tri"))
    finally:
        sc.close()
    return dict(case="writeback " + name, H=H, W=W, extra=extra, binary=BINARY, hits=int(hit.sum()), n_used=n,
                seconds=round(time.time() - t0, 2))


def _run(case):
    return run_writeback_variants(*case[1:]) if case[0] == "writeback" else run_case(*case)


def _children(env, cases):
    """run_case (a case that begins with "writeback": run_writeback_variants) for every case in a child process with
    `env` set -> records"""
    e = dict(os.environ)
    for k in ("LIDARHIP_STEP_CAP", "LIDARHIP_TRACE"):
        e.pop(k, None)
    e.update(env)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(cases)], capture_output=True, text=True,
                         env=e, timeout=300)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("LBVH_CASES ")]
    assert res.returncode == 0 and len(lines) == 1, res.stdout[-3000:] + res.stderr[-3000:]
    recs = json.loads(lines[0][len("LBVH_CASES "):])
    assert len(recs) == len(cases)
    for r in recs:
        print(json.dumps(r))
    return recs


ALL_CASES = [(name, H, W, extra) for name in lc.SCENES for H, W, extra in lc.IMAGE_SHAPES]


# ---- the default process: cap LT_TRACE4_STEP_CAP, the quad kernels -----------------------------------------------------------
STAIRCASES = ("deep_staircase", "deep_staircase_tilted")


@pytest.mark.parametrize("name", STAIRCASES)
def test_spill_to_hbm_and_its_hand_over(name):
    """deep_staircase(16384): the four-wide walk of a ray through c* stacks more than LT_STACK4_LDS entries (the walk
    over the device's node array says how many, and its length is the device's own step count of that ray), so a
    count=True trace reports stack_overflows > 0; the plain trace -- spill stores, spill reads in pop, parked rays --
    equals the oracle.  With the cluster's triangles tilted the nearest one of a ray is any of them (the identical ones
    all tie and the first wins), so the image also tells of an entry lost on the way."""
    rec = run_case(name, 8, 32)
    mesh, origin = lc.scene(name)
    rays = lc.scene_rays(name, 8 * 32)
    from oracle import binding as ob
    d = ob.normalize_rays(rays[:1], ob.NORM_SSE_TABLE)[0]
    sc = _built(mesh)
    try:
        nodes = _nodes4(sc, mesh[1].shape[0])
        steps = _steps(sc, rays, origin, 8)
    finally:
        sc.close()
    order = lc.slab_order(nodes, origin, d)
    walk, parked = lc.replay(nodes, 0, order), lc.replay(nodes, CAP, order)
    rec.update(walk_steps=walk.steps, walk_max_sp=walk.quad_sp, walk_saved_sp=parked.saved_sp,
               walk_tail_high_water=parked.high_water, depth4=lc.tree_depth(nodes))
    print(json.dumps(rec))
    assert np.all(steps[::4] == walk.steps), (np.unique(steps[::4]), walk.steps)   # the rays through c*
    assert parked.high_water <= 304 + 3 * rec["depth4"] < lc.LT_TAIL_STACK
    assert rec["max_saved_sp"] >= parked.saved_sp > lc.LT_STACK4_LDS   # (parked with spilled entries at the default cap already)
    assert lc.LT_STACK4_LDS < walk.quad_sp < lc.LT_STACK4_MAX
    assert rec["stack_overflows"] > 0
    assert rec["parked"] >= 64 and rec["hits"] >= 100
    winners = np.unique(_ref(name, 8 * 32, 8)["tri"])
    assert (winners.size > 20) if name.endswith("tilted") else (list(winners) == [-1, lc.STAIR_FIRST_SPLIT + lc.N_CHAIN])


@pytest.mark.parametrize("name", lc.SCENES)
def test_parked_rays_are_exactly_those_with_more_steps_than_the_cap(name):
    rec = run_case(name, 8, 33)
    print(json.dumps(rec))
    assert rec["parked"] > 0 and rec["max_steps"] > CAP


# identical(n) up to 65 536 stays in the 16-at-a-time mode (high-water mark 182 at 20 000, 228 at 65 536: a round takes 16
# entries and the tree, 7 node levels there, runs out of nodes with four children before the stack has grown by 240)
DFS_CANDIDATES = (20000, 65536, 98304, 131072, 163840, 196608, 229376, 262144)


@pytest.mark.parametrize("kind", ["identical", "same_box_pinned"])
def test_tail_takes_one_entry_at_a_time_above_lt_tail_dfs(kind):
    """identical(n) -- and same_box_pinned(n): the same balanced tree of equal boxes, but the nearest face of a ray sits
    anywhere in it, not in the leaf met first, so the image depends on every entry of the walk -- at the default cap, for
    the smallest n of DFS_CANDIDATES at which the replay on the device's own node array puts the tail's stack above
    LT_TAIL_DFS: the bound 304 + 3 * depth that keeps the unchecked 512-entry LDS stack in bounds holds, the images equal
    the oracle, on identical(n) every ray returns the lowest face index among the ties."""
    from oracle import binding as ob
    t0 = time.time()
    rng = np.random.default_rng(5)
    H, W = 8, 16
    origin = (0.0, 0.0, 0.0)
    rays = lc.rays_along_x(np.random.default_rng(9), H * W)
    d0 = ob.normalize_rays(rays[:1], ob.NORM_SSE_TABLE)[0]   # ray 0, the axis: it meets the box
    found = None
    for n in DFS_CANDIDATES:
        mesh = lc.mesh_of(lc.identical(n) if kind == "identical" else lc.same_box_pinned(n, rng), rng)
        sc = _built(mesh)
        nodes = _nodes4(sc, mesh[1].shape[0])
        order = (lambda node: lc.node_children(nodes, node)) if kind == "identical" else lc.slab_order(nodes, origin, d0)
        rp, depth = lc.replay(nodes, CAP, order), lc.tree_depth(nodes)
        # (a prediction of LT_TAIL_STACK or more is a finding about the kernel: nothing is launched on such a tree)
        assert rp.high_water <= 304 + 3 * depth < lc.LT_TAIL_STACK, (n, rp, depth)
        assert rp.quad_sp < lc.LT_STACK4_MAX
        print(json.dumps(dict(case=kind, n=n, cap=CAP, depth4=depth, **rp._asdict())))
        if rp.high_water > lc.LT_TAIL_DFS:
            found = n
            break
        sc.close()
    assert found is not None, "no candidate reaches the one-at-a-time mode"
    try:
        ref = _oracle(mesh, rays, origin, H)
        steps = _steps(sc, rays, origin, H)
        full = lc.replay(nodes, 0, order).steps   # a ray meets the one box of the n triangles -- then this is its walk -- or not
        assert steps[0] == steps.max() == full and np.all((steps == full) | (steps <= 4))
        got, _ = _trace(sc, rays, origin, H)
        _assert_images(got, ref, f"{kind}({found})")
        parked, saved = _tail(sc)
        assert parked == int((steps > CAP).sum()) == int((steps == full).sum()) > H * W // 2
        assert saved == rp.saved_sp
        assert np.all(got["tri"][steps < full] == -1) and int((ref["tri"] >= 0).sum()) > H * W // 2
        if kind == "identical":
            assert np.all(got["tri"][ref["tri"] >= 0] == 0)
        else:
            assert np.unique(ref["tri"]).size > 50
    finally:
        sc.close()
    print(json.dumps(dict(case=kind + " one-at-a-time", n=found, parked=parked, max_saved_sp=saved, depth4=depth,
                          replay_high_water=rp.high_water, replay_rounds=rp.rounds, seconds=round(time.time() - t0, 2))))


def test_hand_over_counters_across_a_sequence_of_launches():
    """One scene through: heavy, light, count=True, heavy, a call with n_rays < height (no launch), heavy, a larger ray
    count (the ray reservation regrows), a new mesh with build, heavy.  Every image equals the one a fresh scene gives and
    the oracle's; every plain launch parked exactly its own rays with more than CAP steps -- a counter that was not
    re-armed, or the wrong one of the two, shows in the count."""
    H = 8
    mesh, origin = lc.scene("deep_staircase_tilted")
    heavy = lc.scene_rays("deep_staircase_tilted", H * 32)
    light = np.concatenate([heavy[:1], -heavy[1:H * 2]])       # one ray through c*, the others turned away
    big = lc.scene_rays("deep_staircase_tilted", H * 64)
    mesh2, origin2 = lc.scene("stairs")
    heavy2 = lc.scene_rays("stairs", H * 32)

    def fresh(m, rays, o):
        sc = _built(m)
        try:
            img, _ = _trace(sc, rays, o, H)
            return img, _oracle(m, rays, o, H), int((_steps(sc, rays, o, H)[:rays.shape[0] // H * H] > CAP).sum())
        finally:
            sc.close()

    want = {"heavy": fresh(mesh, heavy, origin), "light": fresh(mesh, light, origin), "big": fresh(mesh, big, origin),
            "heavy2": fresh(mesh2, heavy2, origin2)}
    assert want["heavy"][2] >= 64 and want["big"][2] > want["heavy"][2] > want["light"][2] >= 1 and want["heavy2"][2] > 0
    inputs = {"heavy": (heavy, origin), "light": (light, origin), "big": (big, origin), "heavy2": (heavy2, origin2)}
    sc = _built(mesh)
    log = []
    try:
        for step in ("heavy", "light", "count", "heavy", "empty", "heavy", "big", "rebuild", "heavy2"):
            if step == "rebuild":
                _built(mesh2, sc)
                continue
            if step == "empty":      # n_rays < height: W = 0, nothing is launched, nothing is written
                before = _tail(sc)
                got, _ = _trace(sc, heavy[:H - 1], origin, H)
                assert all(np.all(got[k] == SENTINEL) for k in KEYS)
                assert _tail(sc) == before
                continue
            key = "heavy" if step == "count" else step
            rays, o = inputs[key]
            img, ref, n_parked = want[key]
            before = _tail(sc)
            got, st = _trace(sc, rays, o, H, count=(step == "count"))
            _assert_images(got, ref, f"launch {len(log)} ({step})")
            for k in KEYS:
                assert np.array_equal(got[k].view(np.int32), img[k].view(np.int32)), f"launch {len(log)} ({step}) {k} vs fresh"
            if step == "count":      # a counting launch hands nothing over and leaves both counters alone
                assert _tail(sc) == before and st["stack_overflows"] > 0
            else:
                assert _tail(sc)[0] == n_parked, f"launch {len(log)} ({step}): parked {_tail(sc)[0]}, its step image says {n_parked}"
            log.append((step, _tail(sc)))
    finally:
        sc.close()
    print(json.dumps(dict(case="sequence", launches=log)))


# ---- child processes: another cap, the binary twin --------------------------------------------------------------------------
def test_hand_over_of_a_spilled_stack_in_subprocess():
    """LIDARHIP_STEP_CAP=24 on deep_staircase: a ray through c* is parked while it still walks down the chain, with more
    than LT_STACK4_LDS entries saved -- the copy at the hand-over takes its upper part from the spill area."""
    for rec in _children({"LIDARHIP_STEP_CAP": "24"}, [(name, 8, 32, 0) for name in STAIRCASES]):
        assert rec["cap"] == 24 and rec["parked"] >= 64
        assert rec["max_saved_sp"] > lc.LT_STACK4_LDS


def test_tail_alone_in_subprocess():
    """LIDARHIP_STEP_CAP=1: every ray that needs more than one step goes to k_trace4_tail with the root's other
    children as its stack; all scenes, all image shapes."""
    recs = _children({"LIDARHIP_STEP_CAP": "1"}, ALL_CASES)
    for r in recs:
        assert r["cap"] == 1 and r["max_saved_sp"] <= 4
    assert all(r["parked"] > 0 for r in recs if (r["H"], r["W"]) != (1, 1) or r["case"] != "soup")
    assert sum(r["parked"] == r["n_used"] for r in recs) > 0


def test_no_tail_in_subprocess():
    """LIDARHIP_STEP_CAP=0 turns the cap off: k_trace4 walks every ray to its end, k_trace4_tail finds an empty queue."""
    recs = _children({"LIDARHIP_STEP_CAP": "0"}, ALL_CASES)
    assert all(r["cap"] == 0 and r["parked"] == 0 and r["max_saved_sp"] == 0 for r in recs)
    assert max(r["max_steps"] for r in recs) > 1000
    assert all(r["stack_overflows"] > 0 for r in recs if r["case"] in STAIRCASES)


def test_binary_twin_spills_in_subprocess():
    """LIDARHIP_TRACE=binary on deep_staircase: k_trace stacks 42 entries (the oracle's model of the binary tree) against
    LT_STACK_LDS = 32."""
    for rec in _children({"LIDARHIP_TRACE": "binary"}, [(name, 8, 32, 0) for name in STAIRCASES]):
        assert rec["binary"] and rec["stack_overflows"] > 0 and rec["parked"] == 0 and rec["hits"] >= 100


# k_trace shares its tile mapping and its write-back with the quad kernels: every image shape, ragged against its 4 x 16 tile
BINARY_EDGE_CASES = [(name, H, W, extra) for name in ("soup", "stairs") for H, W, extra in lc.IMAGE_SHAPES]


@functools.lru_cache(maxsize=None)
def _binary_edge_child():
    """ONE LIDARHIP_TRACE=binary child for the two tests that follow: the edge shapes, then the write-back variants"""
    return _children({"LIDARHIP_TRACE": "binary"}, BINARY_EDGE_CASES + [("writeback",) + WRITEBACK_CASE])


def test_binary_twin_at_the_edge_shapes_in_subprocess():
    """LIDARHIP_TRACE=binary on soup and stairs at every entry of lc.IMAGE_SHAPES: all five images of the count=True and
    of the plain trace equal the oracle, the trailing rays of 5 x 8 + 3 stay untouched (run_case)."""
    recs = _binary_edge_child()[:len(BINARY_EDGE_CASES)]
    assert [(r["H"], r["W"], r["extra"]) for r in recs] == 2 * [tuple(s) for s in lc.IMAGE_SHAPES]
    assert all(r["binary"] and r["parked"] == 0 and r["n_used"] == r["H"] * r["W"] for r in recs)
    assert any(r["hits"] > 0 for r in recs) and any(r["hits"] < r["n_used"] for r in recs)


def test_write_back_variants_of_the_quad_kernels_and_of_the_binary_twin():
    """run_writeback_variants on WRITEBACK_CASE here (k_trace4, and k_trace4_tail for the rays with more than CAP steps)
    and in the LIDARHIP_TRACE=binary child (k_trace)."""
    here = run_writeback_variants(*WRITEBACK_CASE)
    print(json.dumps(here))
    twin = _binary_edge_child()[-1]
    assert twin["case"] == here["case"] and twin["binary"] and not here["binary"]
    assert twin["hits"] == here["hits"] == 16


if __name__ == "__main__":
    print("LBVH_CASES " + json.dumps([_run(case) for case in json.loads(sys.argv[1])]))
