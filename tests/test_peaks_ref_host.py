"""The numpy twin of the voltage-peak record (tests/peaks_ref.py) against the expression of the reference's experiments:
scipy.signal.find_peaks(series) with no arguments, then series[index] > threshold.  Pins the DEFINITION the GPU tests compare the
device with; needs no GPU."""
import numpy as np
import pytest

import peaks_ref

scipy_signal = pytest.importorskip("scipy.signal")

THRESHOLD = 20.0
LEVELS = np.array([-70.0, -50.0, 0.0, 20.0, 25.0, 30.0, 40.0], np.float32)      # one level IS the threshold
NAN = np.float32(np.nan)


def experiments_expression(series, threshold):
    """find_peaks_above_threshold of interface_gpu/experiments, on a float32 series"""
    found, _ = scipy_signal.find_peaks(np.array(series))
    return [int(i) for i in found if series[i] > threshold]


def crafted():
    """series that hold each edge case for certain"""
    f = lambda *v: np.array(v, np.float32)
    return [f(30.0),                                               # length 1
            f(0.0, 30.0), f(30.0, 0.0),                            # length 2
            f(0.0, 30.0, 0.0),                                     # plain peak
            f(0.0, 30.0, 30.0, 0.0),                               # plateau of even length: index (1 + 2) // 2
            f(0.0, 30.0, 30.0, 30.0, 0.0),                         # ... of odd length
            f(0.0, 25.0, 0.0, 30.0, 30.0),                         # a plateau that reaches the end of the series
            f(0.0, 30.0, NAN, 0.0, 40.0, 0.0),                     # NaN ends a candidate
            f(0.0, NAN, 30.0, 0.0),                                # a rise out of NaN is none
            f(0.0, 20.0, 0.0, 25.0, 0.0),                          # a peak whose value equals the threshold
            f(40.0, 0.0, 0.0, 40.0),                               # first and last sample
            f(*([0.0] + [30.0] * 70 + [0.0]))]                     # a long plateau


def random_series(count=4000, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(1, 40))
        x = LEVELS[rng.integers(0, LEVELS.size, n)]
        if k % 3 == 0:
            x[rng.integers(0, n)] = NAN
        out.append(x)
    return out


def open_plateau_at_the_end(x):
    """the series rises to a value above the threshold and stays there, two samples or more, until it ends"""
    j = x.size - 1
    while j > 0 and x[j - 1] == x[-1]:
        j -= 1
    return bool(x.size - j >= 2 and j >= 1 and x[j - 1] < x[-1] and x[-1] > np.float32(THRESHOLD))


def test_twin_equals_scipy_find_peaks_above_threshold():
    seen = {"even plateau": False, "odd plateau": False, "plateau at the end": False, "nan": False, "equals threshold": False,
            "length 1": False, "length 2": False}
    total = 0
    for x in crafted() + random_series():
        want = experiments_expression(x, THRESHOLD)
        got = peaks_ref.peaks(x, THRESHOLD)
        assert got == want, (x.tolist(), got, want)
        total += len(want)
        # what this input covers, read off scipy's own description of its plateaus
        every, props = scipy_signal.find_peaks(x, plateau_size=0)
        sizes = props["plateau_sizes"]
        seen["even plateau"] |= bool(np.any((sizes > 1) & (sizes % 2 == 0)))
        seen["odd plateau"] |= bool(np.any((sizes > 1) & (sizes % 2 == 1)))
        seen["plateau at the end"] |= open_plateau_at_the_end(x)
        seen["nan"] |= bool(np.isnan(x).any())
        seen["equals threshold"] |= bool(np.any(x[every] == np.float32(THRESHOLD)))
        seen["length 1"] |= x.size == 1
        seen["length 2"] |= x.size == 2
    assert all(seen.values()), seen
    assert total > 1000


def test_raster_counts_and_lists_agree():
    rng = np.random.default_rng(5)
    h = LEVELS[rng.integers(0, LEVELS.size, (60, 9))]
    h[7, 3] = NAN
    raster = peaks_ref.peak_raster(h, THRESHOLD)
    for i in range(h.shape[1]):
        assert np.nonzero(raster[:, i])[0].tolist() == experiments_expression(h[:, i], THRESHOLD)
    for first in (0, 13, 60):
        lists = peaks_ref.peak_lists(raster, first)
        counts = peaks_ref.peak_counts(raster, first)
        for i in range(h.shape[1]):
            want = [j for j in experiments_expression(h[:, i], THRESHOLD) if j >= first]
            assert lists[i].tolist() == want and counts[i] == len(want)
    assert peaks_ref.peak_raster(np.zeros((0, 4), np.float32), THRESHOLD).shape == (0, 4)
