// The reference's Graph trait on the device matrix (graph/mod.rs:42-72): lookup_weight / edit_weight for lists of pairs and
// get_incoming_connections / get_outgoing_connections as ordered (index, weight) lists -- snn_graph_lookup, snn_graph_edit,
// snn_graph_incoming, snn_graph_outgoing.  Queries: a few KB to a few MB per call, bounded by launch and copy latency.
#pragma once
#include "snn_kernels_misc.hpp"

namespace snn {

typedef float graph_v4f __attribute__((ext_vector_type(4)));

// One pair per thread.  pre[k] < n_tot and q0 <= post[k] < q0 + n_loc were checked on the host for every pair of the call.
// Some(w): weight w / connected 1; None (the quiet NaN of the matrix): 0.0f / 0 -- what k_graph_export writes for the element.
__global__ __launch_bounds__(256) void k_graph_lookup(const float *W, uint32_t ld, uint32_t q0, const uint32_t *pre, const uint32_t *post,
                                                      uint32_t n, float *weights, uint8_t *connected)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const float w = W[widx(pre[k], post[k] - q0, ld)];
    const bool edge = (w == w);
    weights[k] = edge ? w : 0.0f;
    connected[k] = edge ? 1 : 0;
}

// One pair per thread; `value` holds the weight, or the quiet NaN for None.  The host lists every (pre, post) once (the last
// occurrence of a call): no two threads write one element.  trace / dw / counter of an edited pair restart at 0 where the handle
// carries them (null: it does not).
__global__ __launch_bounds__(256) void k_graph_edit(float *W, float *trace, float *pending, float *edge_counter, uint32_t ld, uint32_t q0,
                                                    const uint32_t *pre, const uint32_t *post, const float *value, uint32_t n)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const size_t i = widx(pre[k], post[k] - q0, ld);
    W[i] = value[k];
    if (trace) trace[i] = 0.0f;
    if (pending) pending[i] = 0.0f;
    if (edge_counter) edge_counter[i] = 0.0f;
}

// Ordered compaction of one line of W into (index, weight) lists, ONE workgroup of 256 threads.
//   COLUMN: local column `line`, presynaptic rows [0, n) (n = n_tot).  A column is 16 contiguous bytes per group of four rows at a
//           stride of ld * 16 B: a lane reads group g with one dwordx4 and holds the candidate rows 4g .. 4g+3; rows >= n of the
//           last group are never listed, whatever the padding holds.  The index listed is the row.
//   row:    presynaptic row `line`, local columns [0, n) (n = n_loc; the columns [n_loc, ld) are padding and never read).  A row
//           is one dword per column at a stride of 16 B.  The index listed is q0 + column.
// Ascending order: candidates are taken in index order -- lane l of pass t holds the indices right after lane l - 1's -- and
// each gets the slot `running + edges before it in the pass`: the wave-ballot / popcount prefix of k_spike_compact per
// candidate, the waves' totals through LDS, and a running offset every thread carries across the passes (all add the same
// pass total).  Entries are stored only below `capacity` (the staging lists hold no more); *count is the full number.
template <bool COLUMN>
__global__ __launch_bounds__(256) void k_graph_line(const float *W, uint32_t ld, uint32_t q0, uint32_t line, uint32_t n, uint32_t *index,
                                                    float *weights, uint32_t capacity, uint32_t *count)
{
    constexpr uint32_t PER = COLUMN ? 4u : 1u;
    __shared__ uint32_t wave_total[2][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t items = (n + PER - 1u) / PER;                 // quad groups of the column / columns of the row
    uint32_t running = 0;
    for (uint32_t first = 0, pass = 0; first < items; first += 256u, ++pass) {         // (uniform trip count: barriers inside)
        const uint32_t item = first + threadIdx.x;
        float w[PER];
        bool on[PER];
        if (COLUMN) {
            graph_v4f unit = {0.0f, 0.0f, 0.0f, 0.0f};
            if (item < items) unit = *(reinterpret_cast<const graph_v4f *>(W) + (size_t)item * ld + line);
#pragma unroll
            for (uint32_t k = 0; k < PER; ++k) {
                w[k] = unit[k];
                on[k] = item < items && item * 4u + k < n && w[k] == w[k];
            }
        } else {
            w[0] = item < items ? W[widx(line, item, ld)] : 0.0f;
            on[0] = item < items && w[0] == w[0];
        }
        // edges of this wave in front of each candidate of this lane, and the wave's total
        uint32_t before = 0, mine = 0, total = 0;
        uint32_t slot[PER];
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
            const unsigned long long mask = __ballot(on[k]);
            before += (uint32_t)__popcll(mask & below);
            total += (uint32_t)__popcll(mask);
            slot[k] = mine;
            mine += on[k] ? 1u : 0u;
        }
        uint32_t *totals = wave_total[pass & 1u];                // (two sets: a fast wave's next pass does not overwrite this one's)
        if (lane == 0) totals[wave] = total;
        __syncthreads();
        uint32_t base = running;
#pragma unroll
        for (uint32_t v = 0; v < 4u; ++v) {
            if (v < wave) base += totals[v];
            running += totals[v];
        }
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
            const uint32_t at = base + before + slot[k];
            if (on[k] && at < capacity) {
                index[at] = COLUMN ? item * 4u + k : q0 + item;
                weights[at] = w[k];
            }
        }
    }
    if (threadIdx.x == 0) *count = running;
}

} // namespace snn
