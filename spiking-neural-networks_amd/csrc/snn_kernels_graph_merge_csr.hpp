// Structural edits of a SPARSE graph (snn_graph_csr_edit_structure: the reference's edit_weight(pre, post, Option<f32>),
// graph/mod.rs:42-72, 204-213, with Some(w) on an absent pair and None on a stored one): the handle's SELL-64 rows and a sorted
// edit list merged into plain CSR on the device, row by row, every element placed on its own by the formulas of
// snn_graph_merge.hpp.  Nothing of size N^2; O(old entries * log(edits of the row) + edits * log(row length)).
//
// The edit list, all of it on the device: edit_pre / edit_post sorted by (post, pre), no pair twice; edit_w the weight of a
// connected edit; slot the SELL entry of the pair as k_graph_csr_find left it (GRAPH_CSR_NONE: not stored); ins_before / rem_before
// the exclusive prefix sums of the insert / remove flags (k_connect_scan_*), n_edits + 1 words each.
#pragma once
#include "snn_graph_merge.hpp"
#include "snn_kernels_graph_query_csr.hpp"

namespace snn {

static_assert(GRAPH_MERGE_NONE == GRAPH_CSR_NONE, "one sentinel for \"no entry\"");

// One edit per thread: its insert and remove flags, as words for the scan.
__global__ __launch_bounds__(256) void k_graph_merge_flags(const uint32_t *slot, const uint8_t *connected, uint32_t n_edits,
                                                           uint32_t *ins, uint32_t *rem)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_edits) return;
    const bool stored = slot[t] != GRAPH_CSR_NONE, on = connected[t] != 0;
    ins[t] = graph_merge_inserts(on, stored) ? 1u : 0u;
    rem[t] = graph_merge_removes(on, stored) ? 1u : 0u;
}

struct GraphMergeArgs {
    const uint32_t *slice_ptr, *sell_pre, *row_len;      // the stored graph (all three null: the empty one)
    const float *sell_w;
    const uint32_t *edit_pre, *edit_post, *ins_before, *rem_before;
    const float *edit_w;
    uint32_t n_edits, n_rows, q0;
    uint32_t *new_len;                                   // [n_rows], written by k_graph_merge_count
    const uint32_t *new_ptr;                             // [n_rows + 1], read by k_graph_merge_fill
    uint32_t *new_pre, *new_src;                         // [new nnz]: presynaptic index; the old SELL entry, GRAPH_CSR_NONE for an
    float *new_w;                                        //            inserted or reweighed edge; weight
};

// One local row per thread: the length of the merged row.  grid (rows / 256 rounded up), 256 threads
__global__ __launch_bounds__(256) void k_graph_merge_count(const GraphMergeArgs a)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.n_rows) return;
    const GraphMergeSpan s = graph_merge_span(a.edit_post, a.n_edits, a.q0 + r);
    a.new_len[r] = graph_merge_row_length(a.row_len ? a.row_len[r] : 0u, a.ins_before, a.rem_before, s);
}

// One wavefront per local row, rows strided over the grid: lane l takes old entries l, l + 64, ... and then edits lo + l,
// lo + l + 64, ... of the row's span; a lane beyond the row or the span reads and writes nothing.  Every merged entry is written
// once, by the old entry or the inserting edit that becomes it; the merged row is strictly ascending as the formulas place it.
// grid (any), 256 threads = 4 rows per round
__global__ __launch_bounds__(256) void k_graph_merge_fill(const GraphMergeArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6); r < a.n_rows; r += gridDim.x * 4u) {
        const GraphMergeSpan s = graph_merge_span(a.edit_post, a.n_edits, a.q0 + r);
        const uint32_t len = a.row_len ? a.row_len[r] : 0u, at = a.new_ptr[r];
        const uint32_t base = len ? a.slice_ptr[r >> 6] + (r & 63u) : 0u;
        for (uint32_t j = lane; j < len; j += 64u) {
            const uint32_t entry = base + j * 64u, p = a.sell_pre[entry];
            const GraphMergeOld o = graph_merge_old_entry(a.edit_pre, a.ins_before, a.rem_before, s, j, p);
            if (o.what == GRAPH_MERGE_DROP) continue;
            const bool kept = o.what == GRAPH_MERGE_KEEP;
            a.new_pre[at + o.at] = p;
            a.new_w[at + o.at] = kept ? a.sell_w[entry] : a.edit_w[o.edit];
            a.new_src[at + o.at] = kept ? entry : GRAPH_CSR_NONE;
        }
        for (uint32_t t = s.lo + lane; t < s.hi; t += 64u) {
            if (!graph_merge_edit_inserts(a.ins_before, t)) continue;
            const uint32_t p = a.edit_pre[t];
            const uint32_t smaller = len ? graph_merge_lower_bound(a.sell_pre + base, 0u, len, 64u, p) : 0u;
            const uint32_t to = at + graph_merge_insert_at(a.ins_before, a.rem_before, s, t, smaller);
            a.new_pre[to] = p;
            a.new_w[to] = a.edit_w[t];
            a.new_src[to] = GRAPH_CSR_NONE;
        }
    }
}

// Per-edge state across the commit: one new CSR edge per thread, every plane the handle carries (null: it does not) from the old
// SELL entry of the edge to its new one.  Inserted and reweighed edges have no source and keep the 0 the new planes start with.
__global__ __launch_bounds__(256) void k_graph_merge_carry(const uint32_t *src, const uint32_t *edge_slot, uint32_t nnz, const float *old_trace,
                                                           float *trace, const float *old_pending, float *pending,
                                                           const float *old_counter, float *counter)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= nnz) return;
    const uint32_t from = src[e];
    if (from == GRAPH_CSR_NONE) return;
    const uint32_t to = edge_slot[e];
    if (trace) trace[to] = old_trace[from];
    if (pending) pending[to] = old_pending[from];
    if (counter) counter[to] = old_counter[from];
}

} // namespace snn
