"""Numpy twin of the voltage-peak totals (include/snn_amd.h, snn_set_peak_totals): the peaks of tests/peaks_ref.py counted per
neuron and bucket.  A peak at index p: p < origin is not counted; window 0 is one open-ended bucket; otherwise bucket
(p - origin) // window, and buckets >= n_windows are not counted.  tests/test_peak_totals_ref_host.py holds it to the literal
expressions of the reference's experiments."""
import numpy as np


def bucket_lists(peak_lists, origin, window, n_windows):
    """uint32[n_windows, N] from per-neuron lists of peak indices"""
    origin, window, n_windows = int(origin), int(window), int(n_windows)
    if n_windows < 1 or (window == 0 and n_windows != 1):
        raise ValueError("n_windows >= 1, and exactly 1 with window 0")
    out = np.zeros((n_windows, len(peak_lists)), np.uint32)
    for n, peaks in enumerate(peak_lists):
        for p in peaks:
            p = int(p)
            if p < origin:
                continue
            b = 0 if window == 0 else (p - origin) // window
            if b < n_windows:
                out[b, n] += 1
    return out


def bucket(raster, origin, window, n_windows):
    """uint32[n_windows, N] from a peak raster bool[T, N] (peaks_ref.peak_raster)"""
    raster = np.asarray(raster, bool)
    return bucket_lists([np.nonzero(raster[:, i])[0] for i in range(raster.shape[1])], origin, window, n_windows)
