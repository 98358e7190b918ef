"""The LBVH build and its radix sort (lidar_transfer_amd/csrc/lt_build.hip) held to the numpy restatement of
tests/lbvh_build_cases.py, bit for bit.

The sort -- lt_sort_pairs through lt_debug_sort_pairs, its own workspace -- against the stable argsort of the masked keys at
the tile, quarter-tile and k_scan-round seams and on key patterns where one digit, or stability alone, decides.  The build
-- every case of lbvh_build_cases.CASES -- in all its products: sorted keys, triangle records, params, the 4-wide node array
including the nodes that must stay unwritten, and the number of nodes k_hierarchy4 queued for k_hierarchy4_big, which says
that the hand-over ran (or did not).  The binary node array of LIDARHIP_TRACE=binary is compared in a child process: the
kernel is chosen once per process.  Which seam every case crosses is asserted without a GPU in
tests/test_lbvh_build_cpu.py; what was observed on the MI355X: profiles/lbvh_build/README.md."""
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
import lbvh_build_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu
LT_ERR_INVALID_ARG, LT_ERR_BAD_INDEX = -1, -4     # include/lidarhip.h
BINARY = os.environ.get("LIDARHIP_TRACE") == "binary"


@functools.lru_cache(maxsize=None)
def _lib():
    from lidar_transfer_amd import _lib as L
    lib = L.load()
    vp, u32p = C.c_void_p, C.POINTER(C.c_uint32)
    lib.lt_debug_sort_pairs.argtypes = [u32p, u32p, C.c_int, C.c_int, u32p, u32p]
    lib.lt_debug_sort_pairs.restype = C.c_int
    lib.lt_debug_build_get.argtypes = [vp, C.c_int, vp, C.c_int]
    lib.lt_debug_build_get.restype = C.c_int
    lib.lt_debug_nodes4_fill.argtypes = [vp, C.c_int]
    lib.lt_debug_nodes4_fill.restype = C.c_int
    lib.lt_debug_nodes4_get.argtypes = [vp, vp, C.c_int]
    lib.lt_debug_nodes4_get.restype = C.c_int
    return lib


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


# ---- the sort -----------------------------------------------------------------------------------------------------------
def _sort(keys, vals, key_bits):
    n = len(keys)
    ko, vo = np.full(n, 0xDEADBEEF, np.uint32), np.full(n, 0xDEADBEEF, np.uint32)
    rc = _lib().lt_debug_sort_pairs(_u32p(keys), _u32p(vals), n, key_bits, _u32p(ko), _u32p(vo))
    assert rc == 0, rc
    return ko, vo


def _check_sort(pattern, n, key_bits=None):
    keys, vals, bits = bc.sort_input(pattern, n)
    bits = key_bits or bits
    t0 = time.time()
    ko, vo = _sort(keys, vals, bits)
    tiles, rounds = bc.sort_tiles_rounds(n)
    print(json.dumps(dict(sort=pattern, n=n, key_bits=bits, tiles=tiles, scan_rounds=rounds,
                          seconds=round(time.time() - t0, 3))))
    found = bc.compare_sort(keys, vals, bits, ko, vo)
    assert not found, (pattern, n, bits, found[:4])


@pytest.mark.parametrize("n", bc.SORT_SIZES)
def test_sort_sizes(n):
    _check_sort("random30", n)
    _check_sort("ties17", n)


@pytest.mark.parametrize("pattern", bc.SORT_PATTERNS)
@pytest.mark.parametrize("n", bc.SORT_PATTERN_SIZES)
def test_sort_key_patterns(n, pattern):
    _check_sort(pattern, n)


@pytest.mark.parametrize("pattern", bc.SORT_BIG_PATTERNS)
@pytest.mark.parametrize("n", bc.SORT_BIG_SIZES)
def test_sort_beyond_one_round_of_k_scan(n, pattern):
    """256 tiles are the most one round of k_scan covers: 256 * 4096 + 1 keys are the first with a carry into a second
    round, 2 * 256 * 4096 + 4097 make three."""
    assert bc.sort_tiles_rounds(n)[1] == {bc.SCAN_TILES - 1: 1, bc.SCAN_TILES: 1, bc.SCAN_TILES + 1: 2}.get(n, 3)
    _check_sort(pattern, n)


@pytest.mark.parametrize("key_bits", [10, 20, 32])
def test_sort_key_bits(key_bits):
    """one, two and four passes: only the low key_bits bits order, all 32 are carried"""
    _check_sort("random32", 12289, key_bits)


def test_sort_twice_in_a_row_leaves_nothing_behind():
    for pattern, n in (("random30", 12289), ("ties17", 1025), ("random30", 8193), ("equal", 2)):
        _check_sort(pattern, n)


def test_sort_arguments():
    lib = _lib()
    k = np.arange(4, dtype=np.uint32)
    out = np.full(4, 7, np.uint32)
    assert lib.lt_debug_sort_pairs(None, None, 0, 30, None, None) == 0           # n == 0: nothing to do
    assert lib.lt_debug_sort_pairs(_u32p(k), _u32p(k), -1, 30, _u32p(out), _u32p(out)) == LT_ERR_INVALID_ARG
    for bits in (0, 33, -5):
        assert lib.lt_debug_sort_pairs(_u32p(k), _u32p(k), 4, bits, _u32p(out), _u32p(out)) == LT_ERR_INVALID_ARG
    assert lib.lt_debug_sort_pairs(None, _u32p(k), 4, 30, _u32p(out), _u32p(out)) == LT_ERR_INVALID_ARG
    assert lib.lt_debug_sort_pairs(_u32p(k), _u32p(k), 4, 30, _u32p(out), None) == LT_ERR_INVALID_ARG
    assert np.all(out == 7)


# ---- the build ----------------------------------------------------------------------------------------------------------
def _set_and_build(sc, mesh):
    import torch
    sc.set_mesh(*[torch.from_numpy(x).to(sc.device) for x in mesh])
    sc.build()


def _get(sc, what, n, shape, dtype=np.uint32):
    a = np.full(shape, 0xDEADBEEF, np.uint32).view(dtype)
    assert _lib().lt_debug_build_get(sc._h, what, a.ctypes.data_as(C.c_void_p), n) == 0
    return a


def _check_build(sc, case):
    """build, fill the node array, build again, fetch every product, compare -> record"""
    lib = _lib()
    t0 = time.time()
    mesh = case.mesh()
    want = case.build()
    n = want.n
    _set_and_build(sc, mesh)
    status = lib.lt_scene_status(sc._h)
    if not BINARY:
        assert lib.lt_debug_nodes4_fill(sc._h, bc.FILL) == 0
    sc.build()
    keys = _get(sc, bc.GET_KEYS, n, n)
    tris = _get(sc, bc.GET_TRIS, n, (n, 12))
    params = _get(sc, bc.GET_PARAMS, n, 5, np.float32)
    found = []
    rec = dict(case=case.name, n=n, live=int(want.live.sum()), binary=BINARY)
    if BINARY:
        nodes2 = _get(sc, bc.GET_NODES2, n, (n, 16))
        found += bc.compare_nodes2(nodes2[:max(n - 1, 1)], want.nodes2[:max(n - 1, 1)])
        queued = bc.queued_expected(want)     # (no queue on this path)
    else:
        queued = int(_get(sc, bc.GET_QUEUED, 0, 1)[0])
        nodes4 = np.full((n, 32), 0xDEADBEEF, np.uint32)
        assert lib.lt_debug_nodes4_get(sc._h, nodes4.ctypes.data_as(C.c_void_p), n) == 0
        found += bc.compare_nodes(nodes4, want.nodes4)
        rec.update(queued=queued)
    found += bc.compare_build(want, keys, tris, params, queued)
    assert not found, (case.name, len(found), found[:6])
    assert status == lib.lt_scene_status(sc._h) == (LT_ERR_BAD_INDEX if case.bad_index else 0), status
    rec.update(seconds=round(time.time() - t0, 3))
    return rec


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_build_equals_the_restatement(name):
    from lidar_transfer_amd.raytracer import Scene
    sc = Scene(0)
    try:
        print(json.dumps(_check_build(sc, bc.BY_NAME[name])))
    finally:
        sc.close()


def test_one_scene_through_every_case_and_back():
    """Capacity reuse: the workspace of the largest case serves all the smaller ones, whose keys, records and segment-tree
    leaves beyond n are those of earlier builds; then up again through the regrowth of nothing."""
    from lidar_transfer_amd.raytracer import Scene
    down = sorted(bc.CASES, key=lambda c: -c.n)
    sc = Scene(0)
    try:
        recs = [_check_build(sc, case) for case in down + down[::-1]]
    finally:
        sc.close()
    assert recs[0]["n"] == max(c.n for c in bc.CASES) and recs[len(down) - 1]["n"] == 1
    print(json.dumps(dict(case="reuse", builds=2 * len(recs), seconds=round(sum(r["seconds"] for r in recs), 2))))


def test_build_get_arguments():
    from lidar_transfer_amd.raytracer import Scene
    lib = _lib()
    buf = np.zeros(64, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    sc = Scene(0)
    try:
        assert lib.lt_debug_build_get(sc._h, bc.GET_PARAMS, p, 0) == LT_ERR_INVALID_ARG      # not built
        _set_and_build(sc, bc.BY_NAME["synth_9"].mesh())
        assert lib.lt_debug_build_get(sc._h, bc.GET_PARAMS, p, 0) == 0
        assert lib.lt_debug_build_get(sc._h, 5, p, 1) == LT_ERR_INVALID_ARG
        assert lib.lt_debug_build_get(sc._h, -1, p, 1) == LT_ERR_INVALID_ARG
        assert lib.lt_debug_build_get(sc._h, bc.GET_KEYS, p, -1) == LT_ERR_INVALID_ARG
        assert lib.lt_debug_build_get(sc._h, bc.GET_KEYS, p, 1 << 24) == LT_ERR_INVALID_ARG  # beyond cap_faces
        assert lib.lt_debug_build_get(sc._h, bc.GET_KEYS, None, 1) == LT_ERR_INVALID_ARG
        assert lib.lt_debug_build_get(None, bc.GET_KEYS, p, 1) == LT_ERR_INVALID_ARG
    finally:
        sc.close()


def test_binary_node_array_in_subprocess():
    """LIDARHIP_TRACE=binary: k_hierarchy writes the 64-byte nodes; six cases against the restatement's binary nodes (a dead
    node: both references 0x7FFFFFFF, boxes unspecified), with keys, records and params."""
    e = dict(os.environ)
    e.pop("LIDARHIP_STEP_CAP", None)
    e["LIDARHIP_TRACE"] = "binary"
    res = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(list(bc.BINARY_CASES))],
                         capture_output=True, text=True, env=e, timeout=300)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("LBVH_BUILD ")]
    assert res.returncode == 0 and len(lines) == 1, res.stdout[-3000:] + res.stderr[-3000:]
    recs = json.loads(lines[0][len("LBVH_BUILD "):])
    for r in recs:
        print(json.dumps(r))
    assert [r["case"] for r in recs] == list(bc.BINARY_CASES) and all(r["binary"] for r in recs)


def _main(names):
    from lidar_transfer_amd.raytracer import Scene
    recs = []
    for name in names:
        sc = Scene(0)
        try:
            recs.append(_check_build(sc, bc.BY_NAME[name]))
        finally:
            sc.close()
    print("LBVH_BUILD " + json.dumps(recs))


if __name__ == "__main__":
    _main(json.loads(sys.argv[1]))
