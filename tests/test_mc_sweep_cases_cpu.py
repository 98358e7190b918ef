"""The volumes of tests/mc_sweep_cases.py have the properties that tests/test_mc_sweep_gpu.py relies on -- held here without a
GPU, by the numpy restatement of the sweep's dispatch rule in the same module (and, for the clean-block volume, by the CPU
oracle's restatement of the integration)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_sweep_cases as mc  # noqa: E402


def test_the_ambiguous_marks_are_lewiners_seven_cases():
    """128 of the 256 case indices belong to the cases 3, 4, 6, 7, 10, 12, 13, complements included; the two corners of a
    face diagonal (device corners 0 and 3: (0, 0, 0) and (1, 1, 0)) are case 3, one corner alone is not ambiguous."""
    amb = mc.ambiguous_cases()
    assert amb.sum() == 128 and not amb[0] and not amb[255]
    assert amb[0b1001] and amb[255 ^ 0b1001] and not amb[1] and not amb[0b11]


def test_restatement_on_a_volume_small_enough_to_count_by_hand():
    """One negative voxel at (1, 1, 70) of a (3, 3, 130) volume: its eight cells -- rows (0, 0), (0, 1), (1, 0), (1, 1), z = 69
    and 70, word 1 -- are active; rows at x = 2 or y = 2 have no cells."""
    t = np.ones((3, 3, 130), np.float32)
    t[1, 1, 70] = -1.0
    S = mc.Sweep(t)
    assert (S.wz, S.n_rows, S.n_blocks) == (3, 9, 1)
    want = np.zeros((64, 3), int)
    want[[0, 1, 3, 4], 1] = 2
    assert np.array_equal(S.cells, want) and not S.amb.any() and not S.heavy.any()
    t[1, 1, 70] = 0.0                                  # the bit is !(t > 0): an exact zero counts as below
    assert np.array_equal(mc.Sweep(t).cells, want)


@pytest.mark.parametrize("shape, wz", [((3, 4, 257), 5), ((3, 4, 320), 5), ((3, 4, 321), 6), ((2, 3, 1344), 21)])
def test_long_rows_take_the_general_loader(shape, wz):
    S = mc.Sweep(mc.white_noise(shape))
    assert S.wz == wz > 4 and shape[2] <= mc.NZ_MAX
    assert S.amb.sum() > 100 and S.cells.sum() > 1000


@pytest.mark.parametrize("nz, wz", [(300, 5), (200, 4)])
def test_wave_counted_volume(nz, wz):
    S = mc.Sweep(mc.wave_counted(nz))
    assert S.wz == wz
    words = S.heavy_lanes[1][:5 if nz == 300 else 3]               # (the last word of nz = 200 has 7 cells a row: light)
    assert ((words >= 1) & (words <= mc.HEAVY_LANES)).all(), S.heavy_lanes[1]
    assert np.array_equal(S.by_wave, S.heavy)                       # no heavy word is left to its lane
    in_heavy = int((S.block(S.amb, 1) * S.block(S.by_wave, 1)).sum())
    assert in_heavy > mc.QW, in_heavy                               # the wave's turns overflow the buffer of 96


def test_walls_volume():
    S = mc.Sweep(mc.walls())
    assert S.wz == 5
    assert (S.heavy_lanes[1] > mc.HEAVY_LANES).sum() == 2 and S.heavy_lanes[1].max() == 20
    assert not S.block(S.by_wave, 1).any() and S.block(S.heavy, 1).sum() == 40      # heavy, and walked by the lanes
    assert S.heavy_lanes[0].max() == 2 and S.block(S.by_wave, 0).sum() == 8         # ... and the wave's, in one launch


def test_owner_lanes_volume():
    S = mc.Sweep(mc.owner_lanes())
    assert S.n_blocks == 3 and S.wz == 3
    lanes = np.flatnonzero(S.block(S.by_wave, 1).any(axis=1))
    assert list(lanes) == [0, 1, 24, 25, 38, 39, 62, 63] and S.heavy_lanes[1].max() == mc.HEAVY_LANES
    amb_by_wave = (S.amb * S.by_wave).sum(axis=1)
    assert amb_by_wave[64] > 10 and amb_by_wave[127] > 10            # lanes 0 and 63 of block 1
    assert S.by_wave[63].any() and S.by_wave[128].any()             # lane 63 of block 0, lane 0 of block 2
    assert np.array_equal(S.by_wave, S.heavy)


@pytest.mark.parametrize("n_amb", [0, 96, 97])
def test_seam_volumes(n_amb):
    S = mc.Sweep(mc.seam(n_amb))
    assert S.block(S.amb, 0).sum() == n_amb == S.amb.sum()
    assert not S.heavy.any() and S.cells.sum() > 100
    assert mc.QW == 96                                              # 96 fills the buffer, 97 is one too many


def test_clean_blocks_observation_writes_the_two_rows_at_a_block_seam(oracle):
    """The CPU restatement of the integration writes rows 127 and 128 of the (6, 48, 65) volume and nothing else: five blocks
    of 64 rows, the written rows the last of block 1 and the first of block 2; the surface crosses both columns."""
    lab, depth, rem = mc.clean_blocks_images()
    shape = mc.CLEAN_SHAPE
    assert tuple(np.ceil((mc.CLEAN_BOUNDS[:, 1] - mc.CLEAN_BOUNDS[:, 0]) / 0.1).astype(int)) == shape
    vols = [np.ones(shape, np.float32)] + [np.zeros(shape, np.float32) for _ in range(3)]
    folded = np.floor(lab[:, :, 0] * 65536 + lab[:, :, 1] * 256 + lab[:, :, 2]).astype(np.float32)
    oracle.tsdf_integrate(vols, shape, mc.CLEAN_BOUNDS[:, 0].astype(np.float32), 0.1, *mc.CLEAN_FOV, folded, depth, rem)
    assert list(mc.written_rows(vols[0], vols[1])) == list(mc.CLEAN_ROWS) == [64 * 1 + 63, 64 * 2]
    S = mc.Sweep(vols[0])
    assert S.n_blocks == 5 and S.cells.sum() > 20
    per_block = S.cells.reshape(S.n_blocks, -1).sum(axis=1)
    assert per_block[1] > 0 and per_block[2] > 0 and per_block[0] == per_block[3] == per_block[4] == 0
