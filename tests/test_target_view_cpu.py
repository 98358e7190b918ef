"""The contract of `lt_target_view_dev` (include/lidarhip.h) without a GPU: its numpy restatement (tests/target_view_cases.py)
against the route it is defined by -- ignore filter, optional transform, the existing restatements of the models' projections
with their sequential loops --, the header as C with the new struct against its ctypes mirror, the argument checks that come
before any device work, and the command line's new flag.  tests/test_target_view_gpu.py compares the kernel with the merged
entry points bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import target_view_cases as tv  # noqa: E402

ROOT = tv.ROOT


@pytest.mark.parametrize("name", ("linear", "table", "sector", "table_az", "sector_table_az", "one_row"))
@pytest.mark.parametrize("mounted", (False, True))
def test_restatement_equals_filter_transform_and_the_existing_projection(name, mounted):
    """rules 1-6 cell for cell: the same winner (by raw index), range bits, remission, label; a cell is empty in one iff it
    is in the other; on seeded clouds with ties, one-ulp neighbours, depth-0 points and NaNs, both class-list forms"""
    T = tv.mounting() if mounted else None
    for (H, W), n, seed in (((4, 8), 257, 1), ((32, 171), 5000, 2)):
        m = tv.models(H, W)[name]
        xyzr, label = tv.cloud(n, seed + 10 * mounted, m["sector"])
        for ignore in (tv.IGNORE_SHORT, tv.IGNORE_LONG):
            got = tv.restate_view(xyzr, label, ignore, T, m, tv.LUT)
            want = tv.composed_view(xyzr, label, ignore, T, m)
            tag = (name, mounted, H, W, len(ignore))
            has = got["index"] >= 0
            assert np.array_equal(has, want["has"]), tag
            assert np.array_equal(got["index"], want["index"]), tag
            for k in ("range", "rem"):
                assert np.array_equal(got[k][has].view(np.int32), want[k][has].view(np.int32)), (tag, k)
                assert (got[k][~has] == -1).all(), (tag, k)
            assert np.array_equal(got["label"][has], want["label"][has]) and (got["label"][~has] == 0).all(), tag
            l = label & 0xFFFF
            assert got["bad_labels"] == int((l >= len(tv.LUT)).sum()) > 0, tag
            assert not np.isin(got["label"][has], ignore).any(), tag
            lab = got["label"]
            colour = np.where((lab < len(tv.LUT))[..., None], tv.LUT[np.minimum(lab, len(tv.LUT) - 1)], 0).astype(np.float64)
            assert np.array_equal(got["black"] != 0, ~has | (colour.sum(2) == 0)), tag
            if n >= 5000 and name != "one_row":
                assert has.sum() > H * W // 8 and got["black"][has].any() and not got["black"][has].all(), tag


def test_restatement_edge_inputs():
    m = tv.models(4, 8)["linear"]
    empty = tv.restate_view(np.zeros((0, 4), np.float32), np.zeros(0, np.uint32), tv.IGNORE_SHORT, None, m, tv.LUT)
    assert (empty["range"] == -1).all() and (empty["rem"] == -1).all() and (empty["label"] == 0).all() and empty["black"].all()
    one = tv.restate_view(np.array([[5, 0, -0.5, 0.25]], np.float32), np.array([(7 << 16) | 40], np.uint32), tv.IGNORE_SHORT,
                          None, m, tv.LUT)
    assert (one["index"] >= 0).sum() == 1 and one["label"].max() == 40 and one["black"].sum() == 4 * 8 - 1
    # equal float64 depths: the lower raw index; one float32 bucket, the later point BELOW the float32 value: the later one
    two = tv.restate_view(np.array([[5, 0, -0.5, 0.25], [5, 0, -0.5, 0.75]], np.float32), np.array([40, 50], np.uint32),
                          tv.IGNORE_SHORT, None, m, tv.LUT)
    assert two["label"].max() == 40 and two["rem"].max() == 0.25
    # -0.0 keeps its sign without T: atan2(-0.0, -5) = -pi, the last column; a product with the identity would give +0.0
    seam = tv.restate_view(np.array([[-5, -0.0, -0.5, 0.5]], np.float32), np.array([40], np.uint32), [], None, m, tv.LUT)
    assert np.flatnonzero(seam["index"].reshape(-1) >= 0)[0] % 8 == 7
    ident = tv.restate_view(np.array([[-5, -0.0, -0.5, 0.5]], np.float32), np.array([40], np.uint32), [], np.eye(4), m, tv.LUT)
    assert np.flatnonzero(ident["index"].reshape(-1) >= 0)[0] % 8 == 0


def test_header_compiles_as_c_and_lt_view_model_matches_its_mirror(tmp_path):
    from lidar_transfer_amd import _lib
    fields = [f for f, _ in _lib.ViewModel._fields_]
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lidarhip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(lt_view_model));\n'
                   + "".join(f'  printf(" %zu", offsetof(lt_view_model, {f}));\n' for f in fields)
                   + '  printf(" %d\\n", LT_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    V = _lib.ViewModel
    assert got == [ctypes.sizeof(V)] + [getattr(V, f).offset for f in fields] + [_lib.LT_ABI_VERSION]
    assert "lt_target_view_dev" in _lib.SYMBOLS


def test_target_view_rejects_bad_arguments_before_any_device_work():
    import ctypes as C
    from lidar_transfer_amd import _lib
    lib = _lib.load()
    dummy = C.c_void_p(256)   # (never dereferenced: every call below is refused before the evaluator is touched)
    im = _lib.SourceImages()
    rows = (C.c_double * 8)(0.1, 0.0, -0.1, -0.2, 0.05, 0.05, 0.05, 0.05)
    az = (C.c_double * 4)(0.01, 0.0, -0.01, 0.0)
    R, S, A = _lib.LT_PROJ_BEAM_ROWS, _lib.LT_PROJ_SECTOR, _lib.LT_PROJ_BEAM_AZIMUTH

    def vm(H=4, W=8, flags=0, rows=None, az=None, yc=0.0, span=0.0):
        return _lib.ViewModel(15.0, -25.0, H, W, flags, C.cast(rows, C.c_void_p) if rows is not None else None,
                              C.cast(az, C.c_void_p) if az is not None else None, yc, span)

    def call(ev=dummy, rs=None, ignore=None, n_ignore=0, model=None, no_scan=False, no_model=False):
        rs = _lib.RawScan(None, None, 0) if rs is None else rs
        model = vm() if model is None else model
        return lib.lt_target_view_dev(ev, None if no_scan else C.byref(rs), ignore, n_ignore, None,
                                      None if no_model else C.byref(model), None, 0, C.byref(im), None)

    assert call(ev=None) == -1
    assert call(no_scan=True) == -1
    assert call(no_model=True) == -1
    assert call(rs=_lib.RawScan(None, None, 10)) == -1                                  # n > 0 without buffers
    assert call(rs=_lib.RawScan(264, 256, 10)) == -1 and b"aligned" in lib.lt_last_error()
    assert call(ignore=(C.c_int * 1)(70000), n_ignore=1) == -1 and b"65535" in lib.lt_last_error()
    assert call(model=vm(H=0)) == -1
    assert call(model=vm(H=65536, W=65536)) == -1                                       # beyond the key range
    assert call(model=vm(flags=A, az=az)) == -1 and b"LT_PROJ_BEAM_ROWS" in lib.lt_last_error()
    assert call(model=vm(flags=R | A, rows=rows)) == -1                                 # offsets wanted, none given
    assert call(model=vm(flags=R)) == -1                                                # a table wanted, none given
    assert call(model=vm(flags=S, yc=0.0, span=0.0)) == -1 and b"width" in lib.lt_last_error()
    assert call(model=vm(flags=S, yc=4.0, span=1.0)) == -1
    assert call(model=vm(flags=_lib.LT_PROJ_NEW)) == -1                                 # only the three model bits
    assert call(model=vm(H=600, flags=R, rows=rows)) == -1                              # at most 511 rows


def test_parser_accepts_evaluate_and_defaults_to_auto():
    from lidar_transfer_amd.__main__ import build_parser
    p = build_parser()
    assert p.parse_args(["-d", "x"]).evaluate == "auto"
    for v in ("auto", "target", "off"):
        assert p.parse_args(["-d", "x", "--evaluate", v]).evaluate == v
    with pytest.raises(SystemExit):
        p.parse_args(["-d", "x", "--evaluate", "source"])
