// Voltage-peak record (snn_set_peak_history / snn_get_peak_raster / snn_get_peak_counts / snn_get_peaks): per neuron and recorded
// step one bit, set where scipy.signal.find_peaks(x) reports a local maximum of the neuron's recorded voltage series x and
// x[index] > threshold -- the readout of the reference's GPU experiments (find_peaks_above_threshold over the [T, N] voltage
// history), without the history.  Streaming form, per neuron `prev` (the previous recorded sample) and `left` (the sample index at
// which the series last rose, PEAK_NONE when it has fallen since): the rule of snn_kernels_peak_totals.hpp (peak_rule), which the
// peak totals share, with mark(t) = t; a plateau that ends at recorded sample t is a peak at (left + t - 1) / 2; sample 0 sets
// prev = v, left = NONE.  A peak is known only when its plateau has ended: its bit goes into a PAST row of the raster.  The raster
// has the spike raster's layout, [rows][n_pad / 64] words of 64 bits, neuron q at bit q % 64 of word q / 64.
#pragma once
#include "snn_kernels_peak_totals.hpp"
#include "snn_layout.hpp"

namespace snn {

struct PeakArgs {
    const float *xbuf;                // the voltage plane this step's history row was written from
    XLayout xl;
    const uint32_t *lattice_slot;     // [n_pad] neuron -> lattice slot
    const uint2 *cfg;                 // [n_lattices] {record on, bits of the binary32 threshold}
    float *prev;                      // [n_pad]
    uint32_t *left;                   // [n_pad]
    unsigned long long *raster;       // [cap][words]
    uint32_t n_neurons, n_pad, words;
    uint32_t t;                       // index of the sample being recorded (the row the other records write now)
};

// One thread per neuron; a wavefront owns word column q / 64 of every row, so neither lanes of other wavefronts nor other launches
// (stream order) touch the words it rewrites.  Lanes of a wavefront may close plateaus of different lengths in one step: the rows
// are taken one distinct value at a time, the lanes of that row as one ballot word, OR-ed in by one lane with vector loads and stores.
__global__ __launch_bounds__(256) void k_peak_detect(const PeakArgs a)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= a.n_pad) return;                                   // (n_pad is a multiple of 256: whole wavefronts leave)
    const uint32_t lane = threadIdx.x & 63u, word = q >> 6;
    if (lane == 0) a.raster[(size_t)a.t * a.words + word] = 0ull;      // this sample's row: nothing can be set in it before t + 1
    bool hit = false;
    uint32_t row = 0;
    if (q < a.n_neurons) {
        const uint2 c = a.cfg[a.lattice_slot[q]];
        if (c.x) {
            const float v = a.xbuf[a.xl.at(q, PLANE_V)];
            if (a.t == 0) {
                a.left[q] = PEAK_NONE;
            } else {
                const uint32_t l0 = a.left[q];
                uint32_t l = l0;
                const PeakClosed e = peak_rule(v, a.prev[q], l, a.t, __uint_as_float(c.y));
                hit = e.hit;
                if (e.ended) row = (e.left + a.t - 1u) >> 1;    // left >= 1, t <= 2^32 - 2: no wrap below 2^32 rows (grow_history)
                if (l != l0) a.left[q] = l;
            }
            a.prev[q] = v;
        }
    }
    unsigned long long pending = __ballot(hit);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const uint32_t r = (uint32_t)__shfl((int)row, leader, 64);
        const unsigned long long same = __ballot(hit && row == r);
        if ((int)lane == leader) a.raster[(size_t)r * a.words + word] |= same;
        pending &= ~same;
    }
}

// Neuron i of the lattice [first, first + count): its bits over rows [first_step, steps).  One thread per neuron; a lattice starts
// at any bit of a word, so a wavefront reads one or two words per row.
__global__ __launch_bounds__(256) void k_peak_counts(const unsigned long long *raster, uint32_t words, uint32_t first, uint32_t count,
                                                    uint64_t first_step, uint64_t steps, uint32_t *counts)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t q = first + i, bit = q & 63u;
    const unsigned long long *col = raster + (q >> 6);
    uint32_t n = 0;
    for (uint64_t t = first_step; t < steps; ++t) n += (uint32_t)((col[t * words] >> bit) & 1ull);
    counts[i] = n;
}

// ... and the same bits as ascending step indices, neuron i's from offset[i] on (the exclusive prefix sum of the counts)
__global__ __launch_bounds__(256) void k_peak_fill(const unsigned long long *raster, uint32_t words, uint32_t first, uint32_t count,
                                                  uint64_t first_step, uint64_t steps, const uint32_t *offset, uint32_t *out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t q = first + i, bit = q & 63u;
    const unsigned long long *col = raster + (q >> 6);
    uint32_t at = offset[i];
    for (uint64_t t = first_step; t < steps; ++t)
        if ((col[t * words] >> bit) & 1ull) out[at++] = (uint32_t)t;
}

} // namespace snn
