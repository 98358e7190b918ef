"""Volumes that drive every path of marching cubes' counting sweep (lt_mc.hip: k_mc_words, k_mc_compact) on purpose, and a
numpy restatement of the sweep's dispatch rule that says which path a volume takes.

The rule (lt_mc.hip):
  * a voxel's sign bit is `!(t > 0)`;
  * the cell at (x, y, z), x < nx - 1, y < ny - 1, z < nz - 1, is ACTIVE when its eight bits are not all equal; its case index
    has bit i = the bit of voxel (x + (i & 1), y + ((i >> 1) & 1), z + ((i >> 2) & 1));
  * row = x * ny + y, block = row // 64 (one wave walks a block, a lane per row), word k of a row = its voxels 64 k .. 64 k + 63;
  * a word is HEAVY with more than LT_MC_HEAVY = 16 active cells; a heavy word is counted by the whole wave unless more than
    LT_MC_HEAVY_LANES = 8 rows of its block hold a heavy word k -- then, like every light word, by its own lane;
  * a cell is AMBIGUOUS when its case is marked 0xFFFFFFFF in LT_LWC_FIXED (lt_mc_lewiner_table.h, the table
    tests/test_mc_cpu.py regenerates); a wave buffers LT_MC_QW = 96 ambiguous cells per block, the rest goes straight to
    the queue;
  * rows hold at most 21 words: nz <= 1344.
Used by tests/test_mc_sweep_cases_cpu.py (the generators have the properties they claim) and tests/test_mc_sweep_gpu.py."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAVY, HEAVY_LANES, QW, NZ_MAX = 16, 8, 96, 1344


def ambiguous_cases():
    """bool [256]: the device's case indices that LT_LWC_FIXED marks as ambiguous, read from the committed header."""
    text = open(os.path.join(ROOT, "lidar_transfer_amd", "csrc", "lt_mc_lewiner_table.h")).read()
    body = re.search(r"LT_LWC_FIXED\[256\] = \{(.*?)\};", text, re.S).group(1)
    fixed = np.array([int(v.strip().rstrip("u"), 16) for v in body.split(",") if v.strip()], np.uint64)
    assert fixed.shape == (256,)
    return fixed == 0xFFFFFFFF


class Sweep:
    """What the sweep does with the field `t` [nx, ny, nz], per (row, word): `cells` active cells, `amb` ambiguous ones,
    `heavy`, `by_wave` (counted by the wave); per (block, word): `heavy_lanes`."""

    def __init__(self, t):
        nx, ny, nz = t.shape
        s = ~(t > 0)
        cs = np.zeros((nx, ny, nz), np.int64)          # (cells that do not exist keep case 0)
        for i in range(8):
            dx, dy, dz = i & 1, (i >> 1) & 1, (i >> 2) & 1
            cs[:nx - 1, :ny - 1, :nz - 1] |= s[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << i
        active = (cs != 0) & (cs != 255)
        amb = active & ambiguous_cases()[cs]
        self.wz = (nz + 63) // 64
        self.n_rows = nx * ny
        self.n_blocks = (self.n_rows + 63) // 64

        def per_word(a):
            a = np.pad(a, ((0, 0), (0, 0), (0, self.wz * 64 - nz))).reshape(self.n_rows, self.wz, 64).sum(axis=2)
            return np.pad(a, ((0, self.n_blocks * 64 - self.n_rows), (0, 0)))      # rows beyond the volume: nothing

        self.cells, self.amb = per_word(active), per_word(amb)
        self.heavy = self.cells > HEAVY
        self.heavy_lanes = self.heavy.reshape(self.n_blocks, 64, self.wz).sum(axis=1)
        self.by_wave = self.heavy & (np.repeat(self.heavy_lanes, 64, axis=0) <= HEAVY_LANES)

    def block(self, a, b):
        """rows of block b of a per-(row, word) array"""
        return a[64 * b:64 * b + 64]


def attributes(shape, seed=0):
    """colour (label 0 .. 259 folded like the reference folds it) and remission fields"""
    rng = np.random.default_rng(1000 + seed)
    col = (rng.integers(0, 260, shape) * 65536 + rng.integers(0, 256, shape) * 256 + rng.integers(0, 256, shape))
    return col.astype(np.float32), rng.random(shape).astype(np.float32)


def white_noise(shape, seed=0):
    rng = np.random.default_rng(seed + sum(shape))
    t = rng.normal(size=shape).astype(np.float32)
    t[rng.random(shape) < 0.05] = 0.0
    return t


def noise_columns(shape, columns, seed=7):
    """+1 everywhere, white noise along z in the given (x, y) columns: the four rows around a column hold heavy words
    full of ambiguous cells, every other word is empty"""
    rng = np.random.default_rng(seed)
    t = np.ones(shape, np.float32)
    for x, y in columns:
        t[x, y, :] = rng.normal(size=shape[2]).astype(np.float32)
    return t


def wave_counted(nz):
    """(6, 32, nz): block 1 (x = 2, 3) holds the five rows around the columns (2, 10) and (3, 11)"""
    return noise_columns((6, 32, nz), [(2, 10), (3, 11)])


def walls():
    """(6, 32, 300): five walls along z across block 1 (20 heavy rows in words 1 and 2: walked by the lanes although
    heavy) and one in block 0 (2 heavy rows: counted by the wave) -- both routes in one launch"""
    t = np.ones((6, 32, 300), np.float32)
    for y in (3, 8, 13, 18, 23):
        t[3, y, 70:200] = -0.5
    t[0, 5, 10:250] = -0.5
    return t


def owner_lanes():
    """(8, 24, 130): two diagonal pairs of noise columns, (2, 16) + (3, 17) and (5, 7) + (6, 8).  The cells of a row (x, y)
    see both columns of a pair only at (2, 16) = row 64 and (5, 7) = row 127: lanes 0 and 63 of block 1 own heavy words
    WITH ambiguous cells; the other rows around the columns (lanes 1, 24, 25, 38, 39, 62 of block 1, lane 63 of block 0,
    lane 0 of block 2, ...) own heavy words without.  Block 1 has exactly LT_MC_HEAVY_LANES = 8 heavy lanes: still the
    wave's.  With ny = 24 no such row lies at y = ny - 1, where a row has no cells."""
    return noise_columns((8, 24, 130), [(2, 16), (3, 17), (5, 7), (6, 8)], seed=11)


def seam(n_amb):
    """(4, 32, 130), +1 everywhere, with isolated face-diagonal pairs t[0, y, z] = t[1, y + 1, z] = -0.5: a pair makes the two
    cells that share its face ambiguous (case 3), so 48 pairs (y = 1, 4, 7; z = 8, 16, .. 128) fill a wave's buffer of 96 to
    the brim, and one more pair at z = 0 -- it has no cell below it -- gives 97: one entry takes the direct route.
    n_amb = 0: the first voxel of every pair alone (case 1, not ambiguous)."""
    assert n_amb in (0, 96, 97)
    t = np.ones((4, 32, 130), np.float32)
    for y in (1, 4, 7):
        for z in range(8, 129, 8):
            t[0, y, z] = -0.5
            if n_amb:
                t[1, y + 1, z] = -0.5
    if n_amb == 97:
        t[0, 10, 0] = t[1, 11, 0] = -0.5
    return t


# ---- clean blocks: a volume that knows which of its columns were written ---------------------------------------------------
# 6 x 48 x 65 voxels of 0.1 m high above the sensor (z = 20 .. 26.5 m), so that every (x, y) column has an azimuth of its own.
# The depth image is 23 m in the two pixel columns that the voxel columns (2, 31) and (2, 32) project to and 0 elsewhere:
# integrating it writes rows 127 and 128 -- the last row of block 1 and the first of block 2 -- and nothing else.
CLEAN_BOUNDS = np.array([[-0.33, 0.26], [-2.36, 2.43], [20.0, 26.45]])   # (upper bounds: rounded up to whole voxels)
CLEAN_SHAPE = (6, 48, 65)
CLEAN_FOV = (89.0, -61.0)     # fov_up, fov_down (degrees): the columns are seen at a pitch of 87.6 to 88.5
CLEAN_HW = (16, 4096)
CLEAN_ROWS = (127, 128)


def clean_blocks_images():
    """(label image [H, W, 3], depth image, remission image) of the observation above"""
    H, W = CLEAN_HW
    depth = np.zeros((H, W), np.float32)
    for row in CLEAN_ROWS:
        x, y = divmod(row, CLEAN_SHAPE[1])
        wx, wy = CLEAN_BOUNDS[0, 0] + 0.1 * x, CLEAN_BOUNDS[1, 0] + 0.1 * y
        yaw = -np.arctan2(wy, wx)
        depth[:, int(np.floor(0.5 * (yaw / np.pi + 1.0) * W))] = 23.0
    label = np.zeros((H, W, 3), np.float32)
    label[:, :, 2] = 40.0
    return label, depth, np.full((H, W), 0.5, np.float32)


def written_rows(tsdf, weight):
    """rows (x * ny + y) of the columns that an integration wrote into"""
    return np.flatnonzero(((tsdf != 1) | (weight != 0)).any(axis=2).reshape(-1))
