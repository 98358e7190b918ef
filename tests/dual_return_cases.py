"""The dual-return resolve (include/lidarhip.h: ``lt_echo_resolve_dual_dev``) restated in numpy on
``echo_cases.walk`` and ``echo_cases.frame``, and the hand-written cells the CPU and GPU tests share."""
import numpy as np

import echo_cases as ec

SECONDS = ec.MODES                      # first, strongest, last: LT_ECHO_FIRST, LT_ECHO_STRONGEST, LT_ECHO_LAST
PAIRS = [(m, s) for m in ec.MODES for s in SECONDS]
SECOND_SEED_XOR = 0x9E3779B9            # what the chain xors into the models' seeds for the second return
KEYS = ("endpoints", "endcolors", "range", "endrem", "tri", "fraction")


def second_of(det, j, second):
    """the index in ``det`` (the detected echoes in walk order) of the SECOND echo for the primary ``j`` under the rule
    ``second`` (0 first, 1 strongest, 2 last), or ``None``: chosen among the echoes other than ``j``"""
    rest = [q for q in range(len(det)) if q != j]
    if j is None or not rest:
        return None
    if second == 0:
        return rest[0]
    if second == 2:
        return rest[-1]
    best = rest[0]
    for q in rest[1:]:
        if det[q]["sr"] > det[best]["sr"] or (det[q]["sr"] == det[best]["sr"] and det[q]["c"] > det[best]["c"]):
            best = q
    return best


def restate_resolve_dual(p, second, rays, origin, sub_range, sub_tri, sub_label=None, sub_rem=None):
    """``k_echo_resolve_dual``: ``(first, second)``, two dicts of NEW arrays under ``echo_cases.restate_resolve``'s keys (the
    second without ``n_echoes``).  ``p``: ``echo_cases.params``; ``second``: a name of ``SECONDS`` or its index."""
    sec = SECONDS.index(second) if isinstance(second, str) else int(second)
    S = p["S"]
    rays = np.asarray(rays, np.float32).reshape(-1, 3)
    n = rays.shape[0]
    t = np.asarray(sub_range, np.float32).reshape(S, n)
    tri = np.asarray(sub_tri, np.int32).reshape(S, n)
    rem = np.zeros((S, n), np.float32) if sub_rem is None else np.asarray(sub_rem, np.float32).reshape(S, n)
    lab = np.zeros((S, n), np.int32) if sub_label is None else np.asarray(sub_label, np.int32).reshape(S, n)
    o = np.asarray(origin, np.float32).astype(np.float64)
    h, _, _, dd, _ = ec.frame(rays)

    def blank():
        return dict(endpoints=np.zeros((n, 3), np.float32), endcolors=np.zeros(n, np.int32), range=np.zeros(n, np.float32),
                    endrem=np.zeros(n, np.float32), tri=np.full(n, -1, np.int32), fraction=np.zeros(n, np.float32))
    one, two = blank(), blank()
    one["n_echoes"] = np.zeros(n, np.uint8)
    for i in range(n):
        det, j = ec.walk(p, t[:, i], tri[:, i], rem[:, i])
        one["n_echoes"][i] = len(det)
        if j is None or not dd[i] > 0:
            continue
        for out, q in ((one, j), (two, second_of(det, j, sec))):
            if q is None:
                continue
            e = det[q]
            with np.errstate(all="ignore"):
                r = np.float32(e["st"] / np.float64(e["c"]))
                out["range"][i] = r
                out["endrem"][i] = np.float32(e["sr"] / np.float64(S))
                out["fraction"][i] = np.float32(np.float64(e["c"]) / np.float64(S))
                out["endpoints"][i] = (o + h[i] * np.float64(r)).astype(np.float32)
            out["endcolors"][i] = lab[e["rep"], i]
            out["tri"][i] = tri[e["rep"], i]
    return one, two


def census(p, case):
    """``(echoes per cell [n], cells whose chosen echo lies strictly between two others)`` of a case under ``p``"""
    S = p["S"]
    n = case["rays"].shape[0]
    t, tri, rem = (case[k].reshape(S, n) for k in ("range", "tri", "rem"))
    m = np.zeros(n, np.int64)
    between = 0
    for i in range(n):
        det, j = ec.walk(p, t[:, i], tri[:, i], rem[:, i])
        m[i] = len(det)
        between += j is not None and 0 < j < len(det) - 1
    return m, between


def crafted_cells(S=5, origin=(0.0, 0.0, 0.0)):
    """hand-written cells for ``S = 5`` sub-rays and ``separation = 0.5``, one column each, in ``echo_cases.crafted_cells``'
    form; ``names`` says what each is for"""
    f = np.float32
    cells = [
        ("three echoes, the strongest in the middle", [(4.0, 0.25), (7.0, 0.5), (7.1, 0.5), (11.0, 0.5), None]),
        ("three echoes, the strongest is the last", [(4.0, 0.25), (7.0, 0.5), (11.0, 0.5), (11.1, 0.5), None]),
        ("two echoes, min_subrays = 2 removes one", [(4.0, 0.75), None, (9.0, 0.25), (9.1, 0.25), None]),
        ("all sub-hits in one echo", [(6.0, 0.5), (6.1, 0.25), (6.2, 0.5), (6.3, 0.25), (6.4, 0.5)]),
        ("all misses", [None] * 5),
        ("the rest ties on Srem, the count decides", [(3.0, 0.75), (3.1, 0.75), (6.0, 0.5), (9.0, 0.25), (9.1, 0.25)]),
        ("the rest ties on Srem and the count, the earlier decides", [(3.0, 0.75), (3.1, 0.75), (6.0, 0.5), (9.0, 0.5), None]),
        ("a zero central ray with two echoes", [(5.0, 0.5), (5.1, 0.5), (8.0, 0.25), None, None]),
        ("the second's representative is the centre, the primary's is not", [(10.0, 0.25), (5.0, 0.5), (5.02, 0.5), None,
                                                                            (10.04, 0.25)]),
    ]
    n = len(cells)
    t = np.zeros((S, n), f)
    rem = np.zeros((S, n), f)
    tri = np.full((S, n), -1, np.int32)
    lab = np.zeros((S, n), np.int32)
    for i, (_, subs) in enumerate(cells):
        for k, s in enumerate(subs):
            if s is not None:
                t[k, i], rem[k, i], tri[k, i], lab[k, i] = s[0], s[1], 1000 * i + k, 100 + 10 * i + k
    rays = np.tile(np.array([[0.6, 0.0, 0.8]], f), (n, 1))
    rays[[c[0] for c in cells].index("a zero central ray with two echoes")] = 0
    return dict(names=[c[0] for c in cells], rays=rays, origin=np.asarray(origin, f), range=t.reshape(-1), tri=tri.reshape(-1),
                label=lab.reshape(-1), rem=rem.reshape(-1))
