// Option "verify" (passive tooling): the steps of a run call executed twice from one snapshot and the two outcomes compared
// on the device, word for word; on a mismatch of a handle without weight updates a third execution says which one was odd.
// Included by snn_network.hip only (one translation unit), which defines run_steps.
#pragma once
#include "snn_network_step.hpp"

namespace {

int run_steps(snn_network *net, uint64_t iterations);

// what a rollback (or the second pass of "verify") puts back on the host: cursors, one-launch run counters, profiling events handed out
struct RunCursors { Cursors cur; Stats::Run run; size_t ev_used; };

// "verify": the matrices a run with weight updates rewrites (the snapshot table holds the small arrays only): synapse matrix or
// sparse weights, traces, dw, counters, the weights a one-launch run with STDP leaves behind
hvec<std::pair<void *, size_t>> verify_matrices(const snn_network *net)
{
    hvec<std::pair<void *, size_t>> m;
    if (!net->any_plasticity && !net->any_modulation && !net->any_conn_kind) return m;
    if (net->csr) { if (net->csr_w && net->sell_entries) m.emplace_back(net->csr_w, (size_t)net->sell_entries * 4); }
    else if (net->W) m.emplace_back(net->W, wcount(net->n_tot, net->ld) * 4);
    const size_t edges = std::max<size_t>(net->csr ? (size_t)net->sell_entries : wcount(net->n_tot, net->ld), 64) * 4;
    for (void *a : {(void *)net->trace, (void *)net->pending, (void *)net->edge_counter})
        if (a) m.emplace_back(a, edges);
    return m;
}

// "verify": what may be stepped twice from one snapshot -- nothing measured, the handle's own stream, unsharded; with weight updates
// only while the matrices fit a side buffer (64 MiB: the networks of the randomized tests)
bool verify_applies(const snn_network *net)
{
    if (!net->opt.verify || net->profile || net->external_stream || net->sharded || !net->nn) return false;
    size_t bytes = 0;
    for (const auto &m : verify_matrices(net)) bytes += m.second;
    return bytes <= ((size_t)64 << 20);
}

// name of the array a snapshot entry covers, for the report of a "verify" mismatch
std::string describe_array(const snn_network *net, const void *ptr, uint32_t word)
{
    const char *p = static_cast<const char *>(ptr);
    auto inside = [&](const void *base, size_t bytes) { return base && p >= (const char *)base && p < (const char *)base + bytes; };
    const size_t plane = (size_t)net->xl.stride * 4;
    if (inside(net->xbuf, plane * NUM_PLANES)) return "exchange buffer, plane " + std::to_string(word / net->xl.stride) + ", neuron " + std::to_string(word % net->xl.stride);
    for (int i = 0; i < 2; ++i)
        if (inside(net->shadow[i], plane * NUM_PLANES)) return "shadow " + std::to_string(i) + ", plane " + std::to_string(word / net->xl.stride) + ", neuron " + std::to_string(word % net->xl.stride);
    for (int i = 0; i < 2; ++i)
        if (inside(net->cell_view[i], (size_t)net->c_pad * 8)) return "cell view " + std::to_string(i) + ", word " + std::to_string(word);
    if (inside(net->pt_counts, (size_t)net->pt_rows * net->n_pad * 4))       // (one snapshot entry per row)
        return "peak totals: counts, bucket " + std::to_string((size_t)(p - (const char *)net->pt_counts) / 4 / net->n_pad) + ", neuron " + std::to_string(word);
    if (inside(net->pt_block, (size_t)PT_ROWS * net->n_pad * 4))             // (row 0: previous sample, row 1: left edge, then settings)
        return "peak totals: block, row " + std::to_string((size_t)(p - (const char *)net->pt_block) / 4 / net->n_pad) + ", neuron " + std::to_string(word);
    const struct { const void *base; const char *name; } known[] = {
        {net->part_i, "part_i"}, {net->part_t, "part_t"}, {net->n_in, "n_in"}, {net->tcount, "tcount"}, {net->W, "W"}, {net->w24, "24-bit image of W"},
        {net->spike_counts, "spike_counts"}, {net->spike_count, "spike_count"}, {net->st_clock_dev, "st_clock_dev"},
        {net->uni_neuron, "uniform table (neurons)"}, {net->uni_cell, "uniform table (cells)"}, {net->ca.presyn_value, "cells: presyn_value"},
        {net->ca.seed, "cells: seed"}, {net->ca.step, "cells: step"}, {net->ca.counter, "cells: counter"}, {net->lattice_slot, "lattice_slot"},
        {net->csr_w, "sparse weights"}, {net->trace, "traces"}, {net->pending, "dw of reward-modulated connections"},
        {net->edge_counter, "counters of reward-modulated connections"},
        {net->pk_prev, "peak record: previous sample"}, {net->pk_left, "peak record: left edge"}};
    for (const auto &k : known)
        if (k.base == ptr) return std::string(k.name) + ", word " + std::to_string(word);
    for (const auto *table : {&net->neuron_attrs, &net->cell_attrs})
        for (const auto &kv : *table) {
            const Attr &a = kv.second;
            if (!a.base) continue;
            const uint32_t pad = table == &net->neuron_attrs ? net->n_pad : net->c_pad;
            const size_t bytes = (size_t)pad * 4 * ((a.store == S_PLAIN_K) ? K_TYPES : 1);
            if (inside(a.base, bytes))
                return std::string(table == &net->neuron_attrs ? "neurons: " : "cells: ") + kv.first + ", word " +
                       std::to_string(word + (uint32_t)((p - (const char *)a.base) / 4));
        }
    char buf[64];
    snprintf(buf, sizeof buf, "array at %p, word %u", ptr, word);
    return buf;
}

// Left out of the comparison of two passes (a, b: what each left of the caches): the chunk partials (scratch of the two-kernel step
// only), and the shadows / cell views unless both passes left the same copy valid -- a pass that fell back from the one-launch run to one launch per step leaves
// them in another state than a pass that did not, and the validity flags say so
SkipSet verify_skip_set(const snn_network *net, const CacheState &a, const CacheState &b)
{
    SkipSet skip{};
    auto leave_out = [&](const void *array) {
        for (size_t k = 0; array && k < net->snap_table_host.size() && skip.n < 8; ++k)
            if ((const void *)net->snap_table_host[k].src == array) skip.entry[skip.n++] = (uint32_t)k + 1u;
    };
    leave_out(net->part_i); leave_out(net->part_t);
    if (!(a.shadow_valid && b.shadow_valid && a.shadow_cur == b.shadow_cur)) { leave_out(net->shadow[0]); leave_out(net->shadow[1]); }
    if (!(!a.view_dirty && !b.view_dirty && a.cell_view_cur == b.cell_view_cur)) { leave_out(net->cell_view[0]); leave_out(net->cell_view[1]); }
    return skip;
}

// The steps of a run call (between begin_run and end_run) for a handle verify_applies to: the same steps twice from the same
// snapshot, the outcomes compared on the device.  The handle keeps the outcome of the last execution.
int run_verified(snn_network *net, uint64_t iterations)
{
    // (weight updates a previous call deferred are applied first: the delta vectors they read are rewritten by the steps below)
    TRY(flush_rstdp(net));
    TRY(flush_stdp(net));
    TRY(run_snapshot(net, /*restore=*/false));                    // (builds the table; its own copy of S(t) is not used here)
    if (!net->verify_buf || net->verify_words < net->snap_words) {
        dev_replace(net, net->verify_buf);
        net->verify_buf = nullptr;
        net->verify_words = net->snap_words + net->snap_words / 4 + 1024;
        TRY(dev_alloc_t(net, &net->verify_buf, 2 * net->verify_words, /*scratch=*/true));
        TRY(run_snapshot(net, /*restore=*/false));                // the handle has allocated: the table is laid out anew
    }
    if (!net->verify_report) HIP_TRY(snn_malloc(&net->verify_report, 256), SNN_ERR_BUFFER_CREATE);
    if (!net->snap_entries || net->snap_words > net->verify_words) return run_steps(net, iterations);
    const CopyEntry *table = net->snap_table;
    const uint32_t *base = net->snap_buf;
    const uint64_t generation = net->snap_generation;
    const dim3 grid(std::max(1u, std::min(16u, (net->snap_max_words + 1023u) / 1024u)), net->snap_entries);
    uint32_t *start = net->verify_buf, *first = net->verify_buf + net->verify_words;
    const RunCursors c0{net->cur, net->stat.run, net->ev_used};
    const CacheState f0 = net->cache;
    // the matrices (runs with weight updates): [start state | first outcome], one after the other in a side buffer
    const auto matrices = verify_matrices(net);
    size_t big = 0;
    for (const auto &m : matrices) big += m.second;
    if (big > net->verify_big_bytes) {
        net->verify_big = nullptr; net->verify_big_bytes = 0;
        HIP_TRY(snn_malloc(&net->verify_big, 2 * big), SNN_ERR_BUFFER_CREATE);
        net->verify_big_bytes = big;
    }
    auto matrices_copy = [&](int half, bool restore) -> int {
        size_t off = (size_t)half * net->verify_big_bytes;
        if (restore) { net->img_stale = net->img_stale_direct = true; w24_invalidate(net); }
        for (const auto &m : matrices) {
            void *side = net->verify_big + off;
            HIP_TRY(hipMemcpyAsync(restore ? m.first : side, restore ? side : m.first, m.second, hipMemcpyDeviceToDevice, net->stream), SNN_ERR_BUFFER_WRITE);
            off += m.second;
        }
        return SNN_OK;
    };
    // the small arrays of the pass just executed go to `outcome`; arrays, cursors and cache flags back to the start state
    auto rewind = [&](uint32_t *outcome) -> int {
        hipLaunchKernelGGL(k_copy_table_alt, grid, dim3(256), 0, net->stream, table, base, outcome, 0);
        hipLaunchKernelGGL(k_copy_table_alt, grid, dim3(256), 0, net->stream, table, base, start, 1);
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
        net->cur = c0.cur; net->stat.run = c0.run; net->ev_used = c0.ev_used;
        net->cache.shadow_cur = f0.shadow_cur; net->cache.shadow_valid = f0.shadow_valid; net->cache.cell_view_cur = f0.cell_view_cur;
        net->cells_stepped = false; net->local_inputs_done = false;
        return SNN_OK;
    };
    // words in which the handle differs from `outcome` (and its matrices from the first outcome's): report[0], an example in [1..4]
    auto compare = [&](const uint32_t *outcome, const SkipSet &skip, uint32_t (&report)[8]) -> int {
        HIP_TRY(hipMemsetAsync(net->verify_report, 0, 32, net->stream), SNN_ERR_BUFFER_WRITE);
        hipLaunchKernelGGL(k_compare_table_alt, grid, dim3(256), 0, net->stream, table, base, outcome, net->verify_report, skip);
        // the matrices of the two outcomes, word for word (entry numbers past the table's: 2^20 + matrix index)
        size_t off = net->verify_big_bytes;
        uint32_t k = 0;
        for (const auto &m : matrices) {
            hipLaunchKernelGGL(k_compare_words, dim3(std::min<size_t>(1024, (m.second / 4 + 255) / 256)), dim3(256), 0, net->stream,
                               reinterpret_cast<const uint32_t *>(net->verify_big + off), static_cast<const uint32_t *>(m.first), m.second / 4,
                               (1u << 20) + k, net->verify_report);
            off += m.second;
            ++k;
        }
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
        HIP_TRY(copy_sync(net, report, net->verify_report, 32, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
        return SNN_OK;
    };
    hipLaunchKernelGGL(k_copy_table_alt, grid, dim3(256), 0, net->stream, table, base, start, 0);
    HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    TRY(matrices_copy(0, false));
    const uint64_t gave_up_0 = net->stat.run_fallbacks;
    TRY(run_steps(net, iterations));
    // what the first pass left of the caches and how it stepped: compared only where both passes agree
    const CacheState f1 = net->cache;
    const uint64_t launches_1 = net->stat.run.launches - c0.run.launches, gave_up_1 = net->stat.run_fallbacks;
    if (net->snap_generation != generation) {
        // the run allocated and laid the table out anew (first one-launch run of a handle): nothing to compare with this time
        net->stat.verify_skipped += 1;
        return SNN_OK;
    }
    // (a deferred weight update still pending at the end of the first pass belongs to its outcome: applied before the copy)
    TRY(flush_rstdp(net));
    TRY(flush_stdp(net));
    TRY(rewind(first));
    TRY(matrices_copy(1, false));
    TRY(matrices_copy(0, true));
    TRY(run_steps(net, iterations));
    TRY(flush_rstdp(net));
    TRY(flush_stdp(net));
    net->stat.verify_runs += 1;
    if (net->snap_generation != generation) {
        net->stat.verify_skipped += 1;
        return SNN_OK;
    }
    if (net->opt.verify_fault) {          // option "verify_fault" (test hook): the second outcome is not the first
        // (values from 2^30: that word of the first matrix -- the weights -- of a handle with weight updates)
        const bool in_matrix = net->opt.verify_fault >= (1u << 30) && !matrices.empty();
        hipLaunchKernelGGL(k_flip_bit, dim3(1), dim3(1), 0, net->stream,
                           in_matrix ? static_cast<uint32_t *>(matrices[0].first) : reinterpret_cast<uint32_t *>(net->xbuf),
                           in_matrix ? (size_t)(net->opt.verify_fault - (1u << 30)) : (size_t)(net->opt.verify_fault - 1));
        if (in_matrix) w24_invalidate(net);
        net->opt.verify_fault = 0;
    }
    const CacheState f2 = net->cache;
    uint32_t report[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    TRY(compare(first, verify_skip_set(net, f1, f2), report));
    if (!report[0]) return SNN_OK;
    const uint32_t n = report[0], e = report[1], w = report[2];
    char vals[96];
    snprintf(vals, sizeof vals, "first pass 0x%08x (%g), second pass 0x%08x (%g)", report[3],
             (double)__builtin_bit_cast(float, report[3]), report[4], (double)__builtin_bit_cast(float, report[4]));
    const void *arr = (e >= 1 && e <= net->snap_table_host.size()) ? (const void *)net->snap_table_host[e - 1].src
                    : (e >= (1u << 20) && e - (1u << 20) < matrices.size()) ? matrices[e - (1u << 20)].first : nullptr;
    net->verify_text = "run of " + std::to_string(iterations) + " steps ending at clock " + std::to_string(net->cur.clock) + ": " +
                       std::to_string(n) + " words differ between two executions from the same state; e.g. " +
                       describe_array(net, arr, w) + ": " + vals;
    net->verify_text += "; first pass: " + std::to_string(launches_1) + " one-launch launches, " + std::to_string(gave_up_1 - gave_up_0) +
                        " gave up; second pass: " + std::to_string(net->stat.run.launches - c0.run.launches) + " one-launch launches, " +
                        std::to_string(net->stat.run_fallbacks - gave_up_1) + " gave up";
    net->stat.verify_mismatches += 1;
    // Which of the two repeats?  A THIRD execution from the same start (handles without weight updates): the handle keeps its
    // outcome.
    if (matrices.empty()) {
        if (net->verify_third_words < net->verify_words) {
            net->verify_third = nullptr; net->verify_third_words = 0;
            HIP_TRY(snn_malloc(&net->verify_third, net->verify_words * 4), SNN_ERR_BUFFER_CREATE);
            net->verify_third_words = net->verify_words;
        }
        TRY(rewind(net->verify_third));
        TRY(run_steps(net, iterations));
        const CacheState f3 = net->cache;
        uint32_t from_first[8] = {}, from_second[8] = {};
        TRY(compare(first, verify_skip_set(net, f1, f3), from_first));
        TRY(compare(net->verify_third, verify_skip_set(net, f2, f3), from_second));
        const uint32_t differ[2] = {from_first[0], from_second[0]};
        net->verify_text += "; a third execution differs from the first in " + std::to_string(differ[0]) + " words, from the second in " +
                            std::to_string(differ[1]) + (differ[0] && !differ[1] ? ": the FIRST execution was the odd one"
                                                         : !differ[0] && differ[1] ? ": the SECOND execution was the odd one"
                                                         : differ[0] && differ[1] ? ": no two executions agree" : "");
    }
    fprintf(stderr, "[snn verify] MISMATCH %s\n", net->verify_text.c_str());
    if (const char *path = getenv("SNN_AMD_VERIFY_LOG")) {
        if (FILE *f = fopen(path, "a")) { fprintf(f, "%s\n", net->verify_text.c_str()); fclose(f); }
    }
    return SNN_OK;
}

} // namespace
