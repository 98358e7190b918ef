"""``sequence._Tally``: the cells per code and one float64 sum a run keeps per chain for a model that is on -- on CPU
tensors, against ``numpy.bincount`` and a float64 sum."""
import numpy as np
import torch

from lidar_transfer_amd.sequence import _Tally


def _scans(n_codes, seed, scans=4, n=1000):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, n_codes, n).astype(np.uint8), rng.standard_normal(n).astype(np.float32)) for _ in range(scans)]


def test_tally_equals_bincount_and_a_float64_sum_and_starts_again_from_zero():
    for n_codes in (3, 6):
        t = _Tally(n_codes, "cpu")
        assert t.read() == ([0] * n_codes, 0.0) and t.counts is None          # (nothing allocated before the first add)
        for run in range(2):                                                 # (the second run starts from zero)
            want, total, given = np.zeros(n_codes, np.int64), np.float64(0.0), []
            for codes, values in _scans(n_codes, 10 * n_codes + run):
                value = torch.from_numpy(values).sum(dtype=torch.float64)
                given.append((value, float(value)))
                t.add(torch.from_numpy(codes), value)
                want += np.bincount(codes, minlength=n_codes)
                total += np.float64(float(value))
            counts, value = t.read()
            assert counts == want.tolist() and all(type(c) is int for c in counts) and sum(counts) == 4000
            assert type(value) is float and value == float(total)            # (the same float64 additions in the same order)
            assert all(float(v) == was for v, was in given)                  # the caller's tensors are not written to
            t.reset()
            assert t.read() == ([0] * n_codes, 0.0)
    t.add(torch.tensor([0, 2, 2], dtype=torch.uint8))                        # codes alone: no sum is kept
    assert t.read() == ([1, 0, 2, 0, 0, 0], 0.0) and t.sum is None


def test_tally_of_clamped_echo_counts_puts_three_and_more_with_two():
    rng = np.random.default_rng(5)
    n_echoes = rng.integers(0, 6, 1000).astype(np.uint8)                     # up to five echoes: three and more count as several
    fraction = rng.random(1000).astype(np.float32)
    assert (n_echoes > 2).sum() > 100
    image = torch.from_numpy(n_echoes)
    t = _Tally(3, "cpu")
    for _ in range(2):                                                       # what the sequence's worker adds per scan
        t.add(image.clamp(max=2), torch.from_numpy(fraction).sum(dtype=torch.float64))
    counts, share = t.read()
    assert counts == (2 * np.bincount(np.minimum(n_echoes, 2), minlength=3)).tolist() and sum(counts) == 2000
    assert share == 2 * float(torch.from_numpy(fraction).sum(dtype=torch.float64))
    assert int(image.max()) > 2                                              # (the clamp left the image itself alone)
