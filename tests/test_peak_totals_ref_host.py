"""tests/peak_totals_ref.py against the literal expressions of the reference's experiments on random peak lists:
hd_model.py:120-125            firing_rates[i] = [len([j for j in peaks[n] if j <= i and j > i - window]) for n ...], i = 0, window, ...
pipeline_setup.py:230          [len([j for j in i if j >= first_window]) for i in peaks]"""
import numpy as np
import pytest

import peak_totals_ref


def random_peaks(rng, steps, n):
    return [sorted(rng.choice(steps, size=int(rng.integers(0, min(steps, 40))), replace=False).tolist()) for _ in range(n)]


@pytest.mark.parametrize("seed", range(6))
def test_windows_are_the_experiments_firing_rates(seed):
    rng = np.random.default_rng(seed)
    steps, n = int(rng.integers(50, 400)), 7
    window = int(rng.integers(1, 25))                                       # (at least two whole windows in 50 steps)
    peaks = random_peaks(rng, steps, n)
    firing_rates = {}
    for i in range(0, steps, window):                                       # hd_model.py:120-125
        firing_rates[i] = [len([j for j in peaks[k] if j <= i and j > i - window]) for k in range(n)]
    n_windows = (steps - 1) // window
    assert n_windows >= 2
    got = peak_totals_ref.bucket_lists(peaks, 1, window, n_windows)
    for k in range(1, n_windows + 1):
        assert got[k - 1].tolist() == firing_rates[k * window], (k, window)


@pytest.mark.parametrize("seed", range(6))
def test_open_bucket_is_the_pipelines_count(seed):
    rng = np.random.default_rng(100 + seed)
    steps, n = int(rng.integers(50, 400)), 9
    first_window = int(rng.integers(0, steps))
    peaks = random_peaks(rng, steps, n)
    want = [len([j for j in i if j >= first_window]) for i in peaks]        # pipeline_setup.py:230
    assert peak_totals_ref.bucket_lists(peaks, first_window, 0, 1)[0].tolist() == want


def test_raster_form_and_edges():
    raster = np.zeros((20, 2), bool)
    raster[[2, 3, 7, 8, 12, 13], 0] = True
    raster[[0, 19], 1] = True
    got = peak_totals_ref.bucket(raster, 3, 5, 2)              # buckets [3, 8) and [8, 13); 2 is before the origin, 13 past the end
    assert got.tolist() == [[2, 0], [2, 0]]
    assert peak_totals_ref.bucket(raster, 0, 0, 1).tolist() == [[6, 2]]
    with pytest.raises(ValueError):
        peak_totals_ref.bucket(raster, 0, 0, 2)
    with pytest.raises(ValueError):
        peak_totals_ref.bucket(raster, 0, 5, 0)
