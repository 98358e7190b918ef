"""Every path of marching cubes' counting sweep (lt_mc.hip: k_mc_words, k_mc_amb, k_mc_compact) driven on purpose: rows of
more than four words, words counted by the wave and words counted by their lane although heavy, the ambiguous cells'
buffer at its brim and beyond, heavy words owned by the first and the last lane, clean blocks next to written ones, and one
mesh object taking all of it in turn.  Which path a volume takes is ASSERTED on the input, by the numpy restatement of the
sweep's dispatch rule (tests/mc_sweep_cases.py), before the device is asked; every mesh is compared with the CPU oracle's
(tests/mesh_canon.py: the same vertices, the same face stream)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_sweep_cases as mc  # noqa: E402
from mesh_canon import assert_same_mesh  # noqa: E402

pytestmark = pytest.mark.gpu

VOXEL, ORIGIN = 0.05, np.array([-1.25, 2.5, 0.75], np.float32)
LONG_ROWS = [(3, 4, 257), (3, 4, 320), (3, 4, 321), (2, 3, 1344)]
CASES = {"noise_%dx%dx%d" % s: (lambda s=s: mc.white_noise(s)) for s in LONG_ROWS}
CASES.update({"wave_300": lambda: mc.wave_counted(300), "wave_200": lambda: mc.wave_counted(200), "walls": mc.walls,
              "owner_lanes": mc.owner_lanes, "seam_0": lambda: mc.seam(0), "seam_96": lambda: mc.seam(96),
              "seam_97": lambda: mc.seam(97), "small": lambda: mc.white_noise((9, 8, 7))})
_CACHE = {}


def case(oracle, name):
    """(tsdf, colour, remission, the restatement's view of tsdf, the oracle's mesh) of a named volume, computed once"""
    if name not in _CACHE:
        t = CASES[name]()
        col, rem = mc.attributes(t.shape)
        _CACHE[name] = (t, col, rem, mc.Sweep(t), oracle.marching_cubes(t, col, rem, VOXEL, ORIGIN))
    return _CACHE[name]


def extract(mesh, t, col, rem):
    import torch
    dev = torch.device("cuda", 0)
    mesh.extract(*[torch.from_numpy(a).to(dev) for a in (t, col, rem)], VOXEL, ORIGIN)
    return [a.cpu().numpy() for a in mesh.tensors()]


def check(oracle, name, mesh=None):
    from lidar_transfer_amd.fusion import DeviceMesh
    t, col, rem, S, want = case(oracle, name)
    m = mesh or DeviceMesh(0)
    assert_same_mesh(extract(m, t, col, rem), want, name + ": ")
    if mesh is None:
        m.close()
    return want


@pytest.mark.parametrize("shape", LONG_ROWS, ids=lambda s: "x".join(map(str, s)))
def test_rows_of_more_than_four_words(oracle, shape):
    """wz = 5, 5, 6 and 21 (the limit): k_mc_words' loader of one word at a time and k_mc_compact's loop over the counts."""
    S = case(oracle, "noise_%dx%dx%d" % shape)[3]
    assert S.wz == (shape[2] + 63) // 64 > 4 and S.amb.sum() > 100
    want = check(oracle, "noise_%dx%dx%d" % shape)
    assert want[1].shape[0] > 1000


def test_one_word_too_many_is_refused_and_the_mesh_object_lives_on(oracle):
    import torch
    from lidar_transfer_amd.fusion import DeviceMesh
    dev = torch.device("cuda", 0)
    m = DeviceMesh(0)
    big = torch.ones((2, 3, mc.NZ_MAX + 1), device=dev)
    with pytest.raises(RuntimeError) as err:
        m.extract(big, big.clone(), big.clone(), VOXEL, ORIGIN)
    assert "(status -6)" in str(err.value) and "exceeds 1344" in str(err.value)
    check(oracle, "small", m)
    m.close()


@pytest.mark.parametrize("nz", [300, 200])
def test_words_counted_by_the_wave_with_more_ambiguous_cells_than_the_buffer_holds(oracle, nz):
    """Block 1 has five heavy rows in every word: the wave counts them, queues their ambiguous cells under the OWNER's
    (x, y) and overflows its buffer of 96.  nz = 300: five words a row, 200: four -- the two loaders."""
    S = case(oracle, "wave_%d" % nz)[3]
    n_words = 5 if nz == 300 else 3                      # (the last word of nz = 200 has seven cells a row)
    assert S.wz == (5 if nz == 300 else 4)
    assert ((S.heavy_lanes[1][:n_words] >= 1) & (S.heavy_lanes[1][:n_words] <= mc.HEAVY_LANES)).all()
    assert np.array_equal(S.by_wave, S.heavy)
    assert (S.block(S.amb, 1) * S.block(S.by_wave, 1)).sum() > mc.QW
    check(oracle, "wave_%d" % nz)


def test_heavy_words_walked_by_the_lanes_next_to_a_block_counted_by_the_wave(oracle):
    S = case(oracle, "walls")[3]
    assert (S.heavy_lanes[1] > mc.HEAVY_LANES).sum() == 2 and not S.block(S.by_wave, 1).any()
    assert S.heavy_lanes[0].max() == 2 and S.block(S.by_wave, 0).sum() == 8
    check(oracle, "walls")


def test_heavy_words_owned_by_the_first_and_the_last_lane(oracle):
    S = case(oracle, "owner_lanes")[3]
    amb_by_wave = (S.amb * S.by_wave).sum(axis=1)
    assert amb_by_wave[64 + 0] > 10 and amb_by_wave[64 + 63] > 10 and S.heavy_lanes[1].max() == mc.HEAVY_LANES
    assert S.by_wave[63].any() and S.by_wave[128].any()
    check(oracle, "owner_lanes")


@pytest.mark.parametrize("n_amb", [0, 96, 97])
def test_the_buffers_seam(oracle, n_amb):
    """No ambiguous cell, exactly as many as a wave's buffer holds, and one more (the direct route), all in block 0."""
    S = case(oracle, "seam_%d" % n_amb)[3]
    assert S.block(S.amb, 0).sum() == n_amb == S.amb.sum() and not S.heavy.any() and mc.QW == 96
    want = check(oracle, "seam_%d" % n_amb)
    assert want[1].shape[0] >= 48 * 4      # (a voxel on the volume's face x = 0 alone: four cells, a triangle each)


def test_clean_blocks_around_two_written_rows_at_a_block_seam(oracle):
    """A TSDF volume supplies its own sign bits, column stamps and chunk stamps.  Five blocks of 64 rows; one observation
    writes row 127 (the last of block 1) and row 128 (the first of block 2): the four flags of mc_block_live and the
    neighbours of mc_rows_dirty at a block seam, clean blocks before and behind."""
    import torch
    from lidar_transfer_amd.fusion import TSDFVolume
    vol = TSDFVolume(mc.CLEAN_BOUNDS, 0.1, *mc.CLEAN_FOV)
    assert tuple(vol.get_volume_tensors()[0].shape) == mc.CLEAN_SHAPE
    assert vol.extract_mesh().n_faces == 0                                  # (nothing written: every block clean)
    vol.integrate(*[torch.from_numpy(a) for a in mc.clean_blocks_images()])
    tsdf, weight, color, rem = [a.cpu().numpy() for a in vol.get_volume_tensors()]
    assert list(mc.written_rows(tsdf, weight)) == list(mc.CLEAN_ROWS) == [64 + 63, 128]
    S = mc.Sweep(tsdf)
    per_block = S.cells.reshape(S.n_blocks, -1).sum(axis=1)
    assert S.n_blocks == 5 and per_block[1] > 0 and per_block[2] > 0 and per_block[[0, 3, 4]].sum() == 0
    want = oracle.marching_cubes(tsdf, color, rem, np.float32(0.1), vol._vol_origin)
    assert want[1].shape[0] > 20
    assert_same_mesh([a.cpu().numpy() for a in vol.extract_mesh().tensors()], want)
    vol.close()


def test_one_mesh_object_takes_every_case_from_the_largest_to_the_smallest_and_back(oracle):
    """k_mc_clear between extractions, workspaces that shrink and grow, the ambiguous cells' table emptied every time."""
    from lidar_transfer_amd.fusion import DeviceMesh
    names = sorted(CASES, key=lambda n: -case(oracle, n)[0].size)
    assert case(oracle, names[0])[0].size > 50 * case(oracle, names[-1])[0].size
    m = DeviceMesh(0)
    for name in names + names[-2::-1]:
        check(oracle, name, m)
    m.close()
