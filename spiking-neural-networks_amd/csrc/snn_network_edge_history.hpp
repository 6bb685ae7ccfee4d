// snn_set_edge_history / snn_get_edge_history / snn_edge_history_count, host side: the recorder's list in record order
// (snn_kernels_edge_history.hpp), the resolve step that turns its pairs into offsets -- at install time and after every commit of a
// sparse structure (set_graph_csr_impl) --, the download in the caller's order.  The per-step launches are step_end's
// (snn_network_step.hpp, `snapshots`).  Included by snn_network.hip only (one translation unit).
#pragma once
#include "snn_network_graph.hpp"

namespace {

// Offsets of the n record slots whose pairs are pre_d / post_d, into offset_d: elements of W, SELL entries of the stored graph, or
// the absent mark everywhere while a sparse handle holds no graph.  Waited for.
int edge_history_offsets(snn_network *net, const uint32_t *pre_d, const uint32_t *post_d, uint32_t n, unsigned long long *offset_d)
{
    const dim3 grid((n + 255u) / 256u);
    dev_ptr<uint32_t> slot_d;
    if (!net->csr) {
        hipLaunchKernelGGL(k_edge_history_resolve_dense, grid, dim3(256), 0, net->stream, pre_d, post_d, n, net->ld, offset_d);
    } else if (!net->csr_ptr) {
        HIP_TRY(hipMemsetAsync(offset_d, 0xFF, (size_t)n * 8, net->stream), SNN_ERR_BUFFER_WRITE);
    } else {
        TRY(sized(&slot_d, (size_t)n * 4));
        launch_csr_find(net, pre_d, post_d, n, slot_d, nullptr, nullptr, nullptr, 0, nullptr);
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
        hipLaunchKernelGGL(k_edge_history_resolve_csr, grid, dim3(256), 0, net->stream, (const uint32_t *)slot_d, n, offset_d);
    }
    HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    HIP_TRY(hipStreamSynchronize(net->stream), SNN_ERR_WAIT);
    return SNN_OK;
}

// after a commit of a sparse structure: every pair of the installed list finds its entry again, or none -- the record goes on
int edge_history_resolve(snn_network *net)
{
    if (!net->eh_ld) return SNN_OK;
    return edge_history_offsets(net, net->eh_pre, net->eh_post, net->eh_ld, net->eh_offset);
}

void edge_history_clear(snn_network *net)
{
    net->eh_slot = hvec<uint32_t>();
    net->eh_n1 = net->eh_n2 = net->eh_first2 = net->eh_ld = 0;
    net->eh_pre = nullptr; net->eh_post = nullptr; net->eh_offset = nullptr; net->eh_hist = nullptr;
}

int set_edge_history(snn_network *net, const uint32_t *pre, const uint32_t *post, const uint8_t *when, size_t n)
{
    if (!net) return fail(SNN_ERR_BAD_ARG, "net is null");
    if (!net->finalized) return fail(SNN_ERR_BAD_STATE, "network not finalized: edge histories are installed on a finalized handle");
    if (net->sharded) return fail(SNN_ERR_BAD_STATE, "edge histories need an unsharded handle: shard handles of any kind are not covered");
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    if (n == 0) {
        TRY(end_run(net));
        if (net->eh_ld) { net->cur.hist_steps = 0; net->cur.hist_tick = 0; }      // all recorded rows must cover the same steps
        edge_history_clear(net);
        return SNN_OK;
    }
    if (!pre || !post) return fail(SNN_ERR_BAD_ARG, "null pointer with n > 0");
    if (n >= 0xFFFFFF00ull) return fail(SNN_ERR_DIM_MISMATCH, "more than 2^32-257 pairs in one list");
    // every pair is checked before anything changes: a refused call leaves the installed list and its record as they were
    TRY(graph_pairs_accept(net, pre, post, nullptr, nullptr, n, nullptr, nullptr));
    for (size_t k = 0; when && k < n; ++k)
        if (when[k] != 1 && when[k] != 2)
            return fail(SNN_ERR_BAD_ARG, graph_csr_pair(k, pre[k], post[k]) + ": when is " + std::to_string((unsigned)when[k]) +
                                             ", neither 1 (after the step's weight updates) nor 2 (before them)");
    TRY(end_run(net));                     // deferred STDP / R-STDP updates are applied before the step forms change
    // ---- the record order: order 1 first, order 2 from a multiple of 64; each group ascending by the offset the pair has now ----
    hvec<uint64_t> key(n);
    if (!net->csr) {
        for (size_t k = 0; k < n; ++k) key[k] = (uint64_t)widx(pre[k], post[k], net->ld);
    } else if (!net->csr_ptr) {
        for (size_t k = 0; k < n; ++k) key[k] = (uint64_t)post[k] << 32 | pre[k];
    } else {
        const size_t hop = std::min(n, GRAPH_PAIRS_HOP);
        GraphCallLists l;
        dev_ptr<uint32_t> slot_d;
        hvec<uint32_t> slot_h(hop);
        TRY(sized(&l.pre, hop * 4));
        TRY(sized(&l.post, hop * 4));
        TRY(sized(&slot_d, hop * 4));
        for (size_t k = 0; k < n; k += hop) {
            const uint32_t m = (uint32_t)std::min(hop, n - k);
            TRY(l.upload(net, 0, pre + k, post + k, nullptr, nullptr, m));
            launch_csr_find(net, l.pre, l.post, m, slot_d, nullptr, nullptr, nullptr, 0, nullptr);
            HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
            HIP_TRY(copy_sync(net, slot_h.data(), slot_d, (size_t)m * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
            for (uint32_t j = 0; j < m; ++j) key[k + j] = slot_h[j];      // (absent pairs, all ones, go last)
        }
    }
    hvec<uint32_t> order(n);
    for (size_t k = 0; k < n; ++k) order[k] = (uint32_t)k;
    auto second = [&](uint32_t k) { return when && when[k] == 2; };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (second(a) != second(b)) return second(b);
        return key[a] != key[b] ? key[a] < key[b] : a < b;
    });
    uint32_t n1 = 0;
    for (size_t k = 0; k < n; ++k) n1 += second((uint32_t)k) ? 0u : 1u;
    const uint32_t n2 = (uint32_t)n - n1, first2 = (n1 + 63u) & ~63u, ld = (first2 + n2 + 63u) & ~63u;
    hvec<uint32_t> slot(n), pre_rec(ld, 0u), post_rec(ld, 0u);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t k = order[i], at = i < n1 ? (uint32_t)i : first2 + (uint32_t)(i - n1);
        slot[k] = at; pre_rec[at] = pre[k]; post_rec[at] = post[k];
    }
    // ---- the new list into locals, resolved; the commit below only moves ----
    dev_ptr<uint32_t> pre_d, post_d;
    dev_ptr<unsigned long long> offset_d;
    TRY(sized(&pre_d, (size_t)ld * 4));
    TRY(sized(&post_d, (size_t)ld * 4));
    TRY(sized(&offset_d, (size_t)ld * 8));
    HIP_TRY(copy_sync(net, pre_d, pre_rec.data(), (size_t)ld * 4, hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
    HIP_TRY(copy_sync(net, post_d, post_rec.data(), (size_t)ld * 4, hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
    TRY(edge_history_offsets(net, pre_d, post_d, ld, offset_d));
    // ---- the commit: installing or replacing a list restarts the record ----
    net->eh_slot.swap(slot);
    net->eh_n1 = n1; net->eh_n2 = n2; net->eh_first2 = first2; net->eh_ld = ld;
    net->eh_pre = std::move(pre_d); net->eh_post = std::move(post_d); net->eh_offset = std::move(offset_d);
    net->eh_hist = nullptr;                // (sized by the next run: grow_history)
    net->cur.hist_steps = 0; net->cur.hist_tick = 0;
    return SNN_OK;
}

int get_edge_history(snn_network *net, float *weights, uint8_t *connected, size_t steps)
{
    if (!net) return fail(SNN_ERR_BAD_ARG, "net is null");
    if (!net->finalized) return fail(SNN_ERR_BAD_STATE, "network not finalized");
    if (!net->eh_ld) return fail(SNN_ERR_BAD_STATE, "no edge history list is installed (snn_set_edge_history)");
    if (steps != net->cur.hist_steps) return fail(SNN_ERR_DIM_MISMATCH, "history size mismatch");
    if (steps == 0) return SNN_OK;
    if (!weights) return fail(SNN_ERR_BAD_ARG, "weights is null");
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));
    // stored rows in hops of at most 64 MiB; the caller's order, and the split into weight and flag, on the way out
    const size_t n = net->eh_slot.size(), ld = net->eh_ld;
    const size_t hop = std::max<size_t>(1, std::min<size_t>(steps, ((size_t)64 << 20) / (ld * 4)));
    hvec<float> rows(hop * ld);
    for (size_t t = 0; t < steps; t += hop) {
        const size_t m = std::min(hop, steps - t);
        HIP_TRY(copy_sync(net, rows.data(), net->eh_hist.get() + t * ld, m * ld * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
        for (size_t r = 0; r < m; ++r) {
            const float *row = rows.data() + r * ld;
            float *w = weights + (t + r) * n;
            uint8_t *c = connected ? connected + (t + r) * n : nullptr;
            for (size_t k = 0; k < n; ++k) {
                const float v = row[net->eh_slot[k]];
                const bool edge = v == v;
                w[k] = edge ? v : 0.0f;
                if (c) c[k] = edge ? 1 : 0;
            }
        }
    }
    return SNN_OK;
}

} // namespace
