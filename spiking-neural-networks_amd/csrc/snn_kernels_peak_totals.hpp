// Voltage-peak totals (snn_set_peak_totals / snn_get_peak_totals): per neuron and caller-chosen window the NUMBER of peaks the
// peak record (snn_kernels_peaks.hpp) would set bits for -- the experiments' firing_rates[i][n] and their counts after a window --
// formed where the neuron is updated, in every step form, with no raster and no launch of its own.  The series of a neuron is its
// voltage after EVERY step since the totals were last restarted (sample t = 0, 1, ...), whatever the other records do.
//
// The streaming rule both readouts share, per neuron `prev` (the previous sample) and `left` (a mark of the sample at which the
// series last rose, PEAK_NONE when it has fallen since); at sample t with value v:
//     v > prev : left = mark(t)
//     v == prev: nothing (a plateau goes on)
//     else     : if (left != NONE) the plateau [left, t - 1] has ended; it is a peak when v < prev && prev > threshold;  left = NONE
//                (a NaN sample lands here and ends the candidate without a peak)
// then prev = v.  The first sample of a series has nothing to rise from: the raster's kernel sets left = NONE at t = 0, the totals
// restart with prev = NaN (nothing rises from a NaN), so neither counts a plateau across a restart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snn {

constexpr uint32_t PEAK_NONE = 0xFFFFFFFFu;

struct PeakClosed {
    bool ended;          // a plateau ended at this sample ...
    bool hit;            // ... and it is a peak above the threshold
    uint32_t left;       // the mark of its first sample
};

__device__ __forceinline__ PeakClosed peak_rule(float v, float prev, uint32_t &left, uint32_t mark, float threshold)
{
    PeakClosed c{false, false, PEAK_NONE};
    if (v > prev) {
        left = mark;
    } else if (!(v == prev)) {
        if (left != PEAK_NONE) {
            c.ended = true;
            c.hit = v < prev && prev > threshold;
            c.left = left;
            left = PEAK_NONE;
        }
    }
    return c;
}

// The totals' per-neuron block, [PT_ROWS][n_pad] words: the streaming state and, per neuron, the setting of its lattice (a lane
// finds everything it needs at its own index).  A neuron whose lattice has its totals off holds a NaN threshold: nothing is above it.
enum PeakTotalsRow { PT_PREV = 0, PT_LEFT, PT_THRESHOLD, PT_ORIGIN_LO, PT_ORIGIN_HI, PT_WINDOW, PT_N_WINDOWS, PT_ROWS };

// Part of UpdateArgs (24 bytes).  block == null: totals off for the whole handle, behind one wave-uniform branch.
struct PeakTotalsArgs {
    uint32_t *block;                // [PT_ROWS][n_pad]
    uint32_t *counts;               // [n_windows of the handle][n_pad]
    unsigned long long t0;          // sample index of the launch's first step
};

// The sample index travels as 64 bits, the mark of a rise as its low 31: a plateau is shorter than 2^31 samples.
__device__ __forceinline__ uint32_t peak_totals_mark(unsigned long long t) { return (uint32_t)t & 0x7FFFFFFFu; }

// The plateau that began at mark `left` ended at sample t (its last sample is t - 1) and is a peak: one more in its bucket.  With
// d = t - left >= 1 samples since the rise the peak's index is (left + t - 1) / 2 = t - (d + 2) / 2.  A peak before the origin or
// past the last window is not counted; window 0 is one open-ended bucket.  The lane that updates neuron q is the only one that
// touches its column of the counts: plain loads and stores.
__device__ __forceinline__ void peak_totals_count(const PeakTotalsArgs &pt, uint32_t n_pad, uint32_t q, uint32_t left, unsigned long long t)
{
    const uint32_t *cfg = pt.block + q;
    const unsigned long long origin = ((unsigned long long)cfg[(size_t)PT_ORIGIN_HI * n_pad] << 32) | cfg[(size_t)PT_ORIGIN_LO * n_pad];
    const uint32_t window = cfg[(size_t)PT_WINDOW * n_pad], n_windows = cfg[(size_t)PT_N_WINDOWS * n_pad];
    const uint32_t d = ((uint32_t)t - left) & 0x7FFFFFFFu;
    const unsigned long long p = t - ((d + 2u) >> 1);
    if (p < origin) return;
    unsigned long long b = p - origin;
    if (window) b /= window; else b = 0;
    if (b >= n_windows) return;
    pt.counts[(size_t)b * n_pad + q] += 1u;
}

// state in registers (the one-launch run keeps it there for the whole launch): one sample
__device__ __forceinline__ void peak_totals_step(const PeakTotalsArgs &pt, uint32_t n_pad, uint32_t q, float v, unsigned long long t,
                                                 float &prev, uint32_t &left, float threshold)
{
    const PeakClosed c = peak_rule(v, prev, left, peak_totals_mark(t), threshold);
    if (c.hit) peak_totals_count(pt, n_pad, q, c.left, t);
    prev = v;
}

// state in memory (every other step form): one sample of neuron q
__device__ __forceinline__ void peak_totals_sample(const PeakTotalsArgs &pt, uint32_t n_pad, uint32_t q, float v, unsigned long long t)
{
    uint32_t *s = pt.block + q;
    const float threshold = __uint_as_float(s[(size_t)PT_THRESHOLD * n_pad]);
    float prev = __uint_as_float(s[(size_t)PT_PREV * n_pad]);
    const uint32_t left0 = s[(size_t)PT_LEFT * n_pad];
    if (threshold != threshold) return;
    uint32_t left = left0;
    peak_totals_step(pt, n_pad, q, v, t, prev, left, threshold);
    if (left != left0) s[(size_t)PT_LEFT * n_pad] = left;
    s[(size_t)PT_PREV * n_pad] = __float_as_uint(v);
}

} // namespace snn
