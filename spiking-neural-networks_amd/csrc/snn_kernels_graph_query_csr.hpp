// The reference's Graph trait on a SPARSE handle (graph/mod.rs:42-72) -- snn_graph_csr_lookup, snn_graph_csr_edit,
// snn_graph_csr_incoming, snn_graph_csr_outgoing -- on the arrays snn_set_graph_csr leaves on the device: SELL-64 rows (entry k of
// local row r at slice_ptr[r / 64] + 64 k + r % 64, presynaptic indices strictly ascending in k, row_len[r] real entries, SELL_PAD
// behind them) and the transpose (t_ptr / t_edge over CSR edges, edge_post / edge_slot per CSR edge).  Queries: bounded by launch
// and copy latency; nothing here reads or writes more than the pairs or the line asked for.
#pragma once
#include "snn_kernels_csr.hpp"

namespace snn {

constexpr uint32_t GRAPH_CSR_NONE = 0xFFFFFFFFu;            // `slot` of a pair that is no stored edge
constexpr unsigned long long GRAPH_CSR_ALL_FINE = ~0ull;    // *first_bad while no pair broke the edit rule

// One pair per thread.  pre[k] < n_tot and q0 <= post[k] < q0 + n_loc were checked on the host for every pair of the call.
// A binary search over the row_len entries of row post[k] - q0, 64 words apart: the entry whose presynaptic index is pre[k].
//   slot       (may be null) the SELL entry of the pair, GRAPH_CSR_NONE for an absent pair
//   weights / connected  (may be null, together) Some(w): w / 1; None: 0.0f / 0
//   want       (may be null) the resolve pass of an edit: want[k] != 0 asks for a stored edge, 0 for an absent pair -- the structure
//              is fixed, so anything else breaks the rule, and the smallest position `at + k` that does ends up in *first_bad
//              (the one word of these kernels with more than one writer: an atomic minimum, issued by offending pairs only)
__global__ __launch_bounds__(256) void k_graph_csr_find(const uint32_t *slice_ptr, const uint32_t *sell_pre, const float *sell_w,
                                                        const uint32_t *row_len, uint32_t q0, const uint32_t *pre, const uint32_t *post,
                                                        uint32_t n, uint32_t *slot, float *weights, uint8_t *connected, const uint8_t *want,
                                                        unsigned long long at, unsigned long long *first_bad)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint32_t r = post[k] - q0, p = pre[k];
    const uint32_t base = slice_ptr[r >> 6] + (r & 63u);
    uint32_t lo = 0, hi = row_len[r];                       // the first entry with index >= p lies in [lo, hi]
    const uint32_t len = hi;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sell_pre[base + mid * 64u] < p) lo = mid + 1u; else hi = mid;
    }
    const bool edge = lo < len && sell_pre[base + lo * 64u] == p;
    const uint32_t s = edge ? base + lo * 64u : GRAPH_CSR_NONE;
    if (slot) slot[k] = s;
    if (weights) {
        weights[k] = edge ? sell_w[s] : 0.0f;
        connected[k] = edge ? 1 : 0;
    }
    if (want && (want[k] != 0) != edge) atomicMin(first_bad, at + k);
}

// One resolved pair per thread: the weight into its SELL entry; trace / dw / counter of the entry restart at 0 where the handle
// carries them (null: it does not).  `sel` (may be null): the pair's position in `slot`, else k.  The host lists every pair once
// (the last occurrence of a call): no two threads write one entry.  A pair without an entry (an accepted "stay absent") is skipped.
__global__ __launch_bounds__(256) void k_graph_csr_store(float *sell_w, float *trace, float *pending, float *edge_counter,
                                                         const uint32_t *slot, const unsigned long long *sel, const float *value, uint32_t n)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint32_t s = slot[sel ? sel[k] : (unsigned long long)k];
    if (s == GRAPH_CSR_NONE) return;
    sell_w[s] = value[k];
    if (trace) trace[s] = 0.0f;
    if (pending) pending[s] = 0.0f;
    if (edge_counter) edge_counter[s] = 0.0f;
}

// The incoming list of local row r: its `len` = row_len[r] entries, already ascending, copied to (index, weights).  Entry k is one
// 4-byte word 256 B behind entry k - 1 (the 63 rows of the slice lie in between): a lane reads one word of each 256-byte line, the
// layout the step kernels want and a line query pays for; the stores are contiguous.
__global__ __launch_bounds__(256) void k_graph_csr_row(const uint32_t *slice_ptr, const uint32_t *sell_pre, const float *sell_w, uint32_t r,
                                                       uint32_t len, uint32_t *index, float *weights)
{
    const uint32_t base = slice_ptr[r >> 6] + (r & 63u);
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < len; k += gridDim.x * 256u) {
        index[k] = sell_pre[base + k * 64u];
        weights[k] = sell_w[base + k * 64u];
    }
}

// The outgoing list of presynaptic index `pre`: the `len` CSR edges t_edge[first ..], first = t_ptr[pre].  t_edge lists the edges of
// a source in ascending edge order and the CSR edges run row by row, so the list is ascending by postsynaptic index as it stands.
__global__ __launch_bounds__(256) void k_graph_csr_out(const uint32_t *t_edge, const uint32_t *edge_post, const uint32_t *edge_slot,
                                                       const float *sell_w, uint32_t q0, uint32_t first, uint32_t len, uint32_t *index,
                                                       float *weights)
{
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < len; k += gridDim.x * 256u) {
        const uint32_t e = t_edge[first + k];
        index[k] = q0 + edge_post[e];
        weights[k] = sell_w[edge_slot[e]];
    }
}

} // namespace snn
