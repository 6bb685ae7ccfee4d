"""Numpy twin of the voltage-peak record (include/snn_amd.h, snn_set_peak_history): the streaming form the device keeps, applied to
a recorded voltage history.  Per neuron `prev` (the previous sample) and `left` (the index at which the series last rose, NONE
once it has fallen); at sample t >= 1 with value v:

    v > prev   left = t
    v == prev  nothing
    otherwise  a peak at (left + t - 1) // 2 if left is set, v < prev and prev > threshold; then left = NONE

then prev = v.  Sample 0 sets prev and clears left.  Everything in binary32.  tests/test_peaks_ref_host.py holds this to
scipy.signal.find_peaks + `series[index] > threshold`, the expression of the reference's experiments."""
import numpy as np

NONE = -1


def peak_raster(history, threshold):
    """bool[T, N]: the peaks of every column of history (float32[T, N], one row per recorded step) above `threshold`"""
    x = np.asarray(history, np.float32)
    if x.ndim == 1:
        x = x[:, None]
    steps, n = x.shape
    thr = np.float32(threshold)
    out = np.zeros((steps, n), bool)
    if steps == 0:
        return out
    prev = x[0].copy()
    left = np.full(n, NONE, np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(1, steps):
            v = x[t]
            up, flat = v > prev, v == prev
            other = ~(up | flat)
            hit = other & (left != NONE) & (v < prev) & (prev > thr)
            out[(left[hit] + t - 1) // 2, np.nonzero(hit)[0]] = True
            left[other] = NONE
            left[up] = t
            prev = v.copy()
    return out


def peaks(series, threshold):
    """the peak indices of ONE series, ascending, as a list of int"""
    return np.nonzero(peak_raster(np.asarray(series, np.float32).reshape(-1, 1), threshold)[:, 0])[0].tolist()


def peak_counts(raster, first_step=0):
    """uint32[N]: per neuron the peaks at step indices >= first_step"""
    return raster[int(first_step):].sum(axis=0).astype(np.uint32)


def peak_lists(raster, first_step=0):
    """per neuron the ascending step indices >= first_step"""
    return [(np.nonzero(raster[int(first_step):, i])[0] + int(first_step)).astype(np.int64) for i in range(raster.shape[1])]
