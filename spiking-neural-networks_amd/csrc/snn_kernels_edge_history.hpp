// Edge-weight histories (snn_set_edge_history / snn_get_edge_history): the weights of a caller-chosen list of (pre, post) pairs per
// recorded step, on dense and sparse handles -- the connecting graph's history (LatticeNetwork::iterate*, neuron/mod.rs:2463-2465)
// and a lattice's own (graph/mod.rs:278-280) where the count x count snapshot of k_weight_snapshot cannot exist.
// The recorder's list is kept in RECORD order, not in the caller's: the pairs of order 1 (after the step's weight updates), then
// the pairs of order 2 (before them) from a multiple of 64 on, each group ascending by the weight-array offset the pair had when
// the list was installed.  Record slot i of a row is column i of the stored row: the recorder's stores are contiguous per wavefront
// (256 B per instruction at one slot per lane) and so are its offset loads; the gather from the weight array is ascending, and for
// "every edge of a sparse lattice" it walks the SELL-64 entries in storage order -- contiguous as well, except over the padding
// entries.  The caller's order comes back at download, on the host.
#pragma once
#include "snn_kernels_graph_query_csr.hpp"

namespace snn {

constexpr unsigned long long EDGE_HISTORY_ABSENT = ~0ull;   // offset of a pair without a SELL entry
constexpr uint32_t EDGE_HISTORY_NAN = 0x7FC00000u;          // what an absent pair records: the absent-edge sentinel of the dense matrix

typedef unsigned long long edge_history_v2u64 __attribute__((ext_vector_type(2)));
typedef float edge_history_v2f __attribute__((ext_vector_type(2)));

// Dense handles: one pair per thread, its element of W (q0 = 0: unsharded handles only).  Absent is decided per recorded step from
// the value read: NaN is the sentinel there.
__global__ __launch_bounds__(256) void k_edge_history_resolve_dense(const uint32_t *pre, const uint32_t *post, uint32_t n, uint32_t ld,
                                                                   unsigned long long *offset)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    offset[k] = (unsigned long long)widx(pre[k], post[k], ld);
}

// Sparse handles: one pair per thread, from the SELL entry k_graph_csr_find left (GRAPH_CSR_NONE: no stored edge) to the 64-bit
// offset into sell_w, or the absent mark.
__global__ __launch_bounds__(256) void k_edge_history_resolve_csr(const uint32_t *slot, uint32_t n, unsigned long long *offset)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint32_t s = slot[k];
    offset[k] = s == GRAPH_CSR_NONE ? EDGE_HISTORY_ABSENT : (unsigned long long)s;
}

// The per-step recorder: record slots [0, n) of one order, two per lane -- 16 B of offsets, two gathered weights, 8 B stored.
// `offset` and `row` point at the group's first slot, which is a multiple of 64 slots into allocations aligned to 256 B.
// weights: W of a dense handle, sell_w of a sparse one.  12 B read, 4 B written per pair.
__global__ __launch_bounds__(256) void k_edge_history(const float *weights, const unsigned long long *offset, uint32_t n, float *row)
{
    const uint32_t i = (blockIdx.x * 256u + threadIdx.x) * 2u;
    if (i >= n) return;
    const float absent = __uint_as_float(EDGE_HISTORY_NAN);
    if (i + 1u < n) {
        const edge_history_v2u64 o = *reinterpret_cast<const edge_history_v2u64 *>(offset + i);
        edge_history_v2f v;
        v.x = o.x == EDGE_HISTORY_ABSENT ? absent : weights[o.x];
        v.y = o.y == EDGE_HISTORY_ABSENT ? absent : weights[o.y];
        *reinterpret_cast<edge_history_v2f *>(row + i) = v;
    } else {
        const unsigned long long o = offset[i];
        row[i] = o == EDGE_HISTORY_ABSENT ? absent : weights[o];
    }
}

} // namespace snn
