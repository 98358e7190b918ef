"""The two stateful places that carry a ``config.TargetModel`` on the device.  ONE ``Projector`` sees a model with offsets, one
with other offsets and a sector, no model and the first again: what it tells ``lt_projector_set_sector`` /
``lt_projector_set_beam_azimuth`` follows the model, so every result is bit for bit a fresh projector's and equals the
restatement.  ``DeviceDeform.cp`` re-projects through the one of the four ``lt_reverse_projection*_dev`` entry points its model
names: every branch, with and without ``preserve_float``, bit for bit against that entry point called here.  8 x 33 cells and
2000 points (tests/target_model_cases.py; the condition on the cloud: tests/test_target_model_cpu.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import beam_az_cases as ac  # noqa: E402
import beam_cases as bc  # noqa: E402
import target_model_cases as tc  # noqa: E402
import test_beam_table_gpu as btg  # noqa: E402
import test_sector_gpu as tsg  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("range", "idx", "proj_x", "proj_y")
OUTS = tsg.PROJ_KEYS + ("proj_xf", "proj_yf", "n_kept")
H, W, FOV = tc.H, tc.W, tc.FOV
dp = C.POINTER(C.c_double)


def _keywords(name):
    table, sector, az = tc.MODELS[name]
    return dict(beam_table=table, sector=sector, beam_azimuth=az)


def _project(pj, cloud, name):
    import torch
    got = pj.project([cloud], FOV[0], FOV[1], H, W, new=True, remove=True, outputs=OUTS, **_keywords(name))[0]
    torch.cuda.synchronize()
    return got


@pytest.fixture(scope="module")
def alone():
    """every model on a projector that never saw another: name -> images (device tensors), computed once"""
    from lidar_transfer_amd.laserscan import Projector
    cloud = btg._up(tc.cloud())
    out = {}
    for name in tc.MODELS:
        pj = Projector()
        out[name] = _project(pj, cloud, name)
        pj.close()
    return out


def test_one_projector_follows_the_models_it_is_handed(alone):
    from lidar_transfer_amd.config import TargetModel
    from lidar_transfer_amd.laserscan import Projector
    from oracle import projection as op
    pts, rem, lab = tc.cloud()
    cloud = btg._up((pts, rem, lab))
    pj = Projector()
    for step, name in enumerate(tc.SEQUENCE):
        got = _project(pj, cloud, name)
        for k in OUTS:
            assert np.array_equal(got[k].cpu().numpy(), alone[name][k].cpu().numpy(), equal_nan=True), (step, name, k)
        table, sector, az = tc.MODELS[name]
        if table is not None:
            tsg._check_projection(got, ac.project(pts, rem, lab, table, FOV, az, W, sector), W, len(pts), f"step {step}: {name}")
        else:                                                      # no model: the reference's projection (float64: exact)
            w = op.range_projection(pts, rem, H, W, FOV[0], FOV[1], remove=True, method="new")
            assert np.array_equal(got["idx"].cpu().numpy(), w["index"]), step
            assert np.array_equal(btg._bits(got["range"].cpu().numpy()), btg._bits(w["range"])), step
            assert np.array_equal(got["label"].cpu().numpy(), op.label_projection(w["index"], lab[w["kept"]])), step
    a, b, p = (alone[k]["range"].cpu().numpy() for k in ("A", "B", "plain"))
    assert not np.array_equal(a, b) and not np.array_equal(a, p) and not np.array_equal(b, p)    # three different images
    assert pj._applied == (TargetModel(**_keywords("A")), H)      # what the projector holds is the last model it was handed
    pj.close()


def _entry_point(lib, name, pf, rng, px, py, back):
    """the reverse projection of model ``name`` by the entry point that knows it, called directly"""
    import torch
    from lidar_transfer_amd.config import beam_azimuth_radians, sector_radians
    table, sector, az = tc.MODELS[name]
    head, tail = (rng.data_ptr(), px.data_ptr(), py.data_ptr(), int(pf)), (H, W, back.data_ptr(), None)
    brad = None if table is None else torch.from_numpy(bc.rows_of(table)[0]).cuda()
    sec = None if sector is None else np.array(sector_radians(sector), np.float64)
    if az is not None:
        azd = torch.from_numpy(beam_azimuth_radians(az)).cuda()
        rc = lib.lt_reverse_projection_beams_az_dev(*head, brad.data_ptr(), azd.data_ptr(),
                                                    None if sec is None else sec.ctypes.data_as(dp), *tail)
    elif sector is not None:
        rc = lib.lt_reverse_projection_sector_dev(*head, int(table is not None), None if brad is None else brad.data_ptr(),
                                                  FOV[0], FOV[1], H, W, float(sec[0]), float(sec[1]), back.data_ptr(), None)
    elif table is not None:
        rc = lib.lt_reverse_projection_beams_dev(*head, brad.data_ptr(), *tail)
    else:
        rc = lib.lt_reverse_projection_dev(*head, FOV[0], FOV[1], *tail)
    assert rc == 0, lib.lt_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("preserve_float", [False, True])
def test_cp_reprojects_through_the_entry_point_of_its_model(alone, preserve_float):
    """the four steps of the projector test as chains of their own, then the two models that reach the remaining branches:
    ``cp``'s images are the fresh projector's, its ``back_points`` the named entry point's on those images, bit for bit; for
    the models with offsets also the restatement's to tests/test_beam_az_gpu.py's rtol = atol = 1e-13"""
    import torch
    from lidar_transfer_amd import _lib
    from lidar_transfer_amd.deform import DeviceDeform
    lib = _lib.load()
    cloud = btg._up(tc.cloud())
    src, tgt = (H, W, FOV[0], FOV[1]), (H, W, FOV[0], FOV[1])
    seen = {}
    for name in tc.SEQUENCE + ("sector", "table"):
        table, sector, az = tc.MODELS[name]
        with DeviceDeform(src, tgt, None, preserve_float=preserve_float, t_beam_table=table, t_sector=sector, t_beam_azimuth=az) as dd:
            assert dd.t_model.proj_flags == (_lib.LT_PROJ_BEAM_ROWS if table is not None else 0) | \
                (_lib.LT_PROJ_SECTOR if sector is not None else 0) | (_lib.LT_PROJ_BEAM_AZIMUTH if az is not None else 0)
            out = dd.cp([cloud], pack=False)
            torch.cuda.synchronize()
            want = alone[name]
            assert np.array_equal(btg._bits(out["range"].cpu().numpy()), btg._bits(want["range"].cpu().numpy())), name
            assert np.array_equal(out["index"].cpu().numpy(), want["idx"].cpu().numpy()), name
            px, py = (want["proj_xf"], want["proj_yf"]) if preserve_float else (want["proj_x"], want["proj_y"])
            back = torch.full((H * W, 3), -7.0, dtype=torch.float64, device="cuda")
            _entry_point(lib, name, preserve_float, want["range"], px, py, back)
            got = out["back_points"].cpu().numpy()
            assert got.shape == (H * W, 3) and np.array_equal(got, back.cpu().numpy(), equal_nan=True), name
            if az is not None:
                r = ac.reverse_projection(want["range"].cpu().numpy(), px.cpu().numpy(), py.cpu().numpy(), table, az, preserve_float, sector)
                assert np.allclose(got, r, rtol=1e-13, atol=1e-13), name
            if name in seen:                                       # the first model again
                assert np.array_equal(got, seen[name], equal_nan=True), name
            seen[name] = got
    filled = {k: v[np.abs(v).sum(1) > 0] for k, v in seen.items()}
    assert all(len(v) > 0.1 * H * W for v in filled.values()), {k: len(v) for k, v in filled.items()}
    assert len({v.tobytes() for v in seen.values()}) == len(seen)  # five models, five clouds
