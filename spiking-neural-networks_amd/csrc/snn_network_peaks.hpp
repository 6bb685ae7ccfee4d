// snn_set_peak_history / snn_get_peak_raster / snn_get_peak_counts / snn_get_peaks, host side: which lattices record and against
// which threshold, the streaming state and the raster (snn_kernels_peaks.hpp), the readout as a raster, as counts and as step lists.
// The per-step launch is step_end's, the raster grows in grow_history (snn_network_step.hpp).  Included by snn_network.hip only
// (one translation unit).
#pragma once
#include "snn_network_graph.hpp"

namespace {

int set_peak_history(snn_network *net, uint32_t id, int enable, float threshold)
{
    if (!net) return fail(SNN_ERR_BAD_ARG, "net is null");
    if (!net->finalized) return fail(SNN_ERR_BAD_STATE, "network not finalized: peak records are switched on a finalized handle");
    const LatticeInfo *l = find_lattice(net, id);
    if (!l || l->spike_train) return fail(SNN_ERR_BAD_ARG, "peak records belong to neuron lattices");
    if (threshold != threshold) return fail(SNN_ERR_BAD_ARG, "the threshold is NaN: no voltage is above it");
    if (net->sharded && net->n_shards > 1)
        return fail(SNN_ERR_BAD_STATE, "peak records need an unsharded handle or a single shard: one of several shards is not covered");
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));                     // deferred STDP / R-STDP updates are applied before the step forms change
    const size_t nl = std::max<size_t>(1, net->lattices.size());
    const uint2 want = make_uint2(enable ? 1u : 0u, enable ? __builtin_bit_cast(uint32_t, threshold) : 0u);
    if (net->pk_cfg_host.size() == nl && net->pk_cfg_host[l->slot].x == want.x && net->pk_cfg_host[l->slot].y == want.y) return SNN_OK;
    if (!enable && net->pk_cfg_host.empty()) return SNN_OK;
    // ---- everything that can fail, into locals: a refused call leaves the handle as it was ----
    hvec<uint2> cfg(net->pk_cfg_host);
    if (cfg.empty()) cfg.assign(nl, make_uint2(0u, 0u));
    cfg[l->slot] = want;
    TRY(ensure_copy_stage(net));
    dev_ptr<uint2> cfg_d;
    TRY(sized(&cfg_d, nl * sizeof(uint2)));
    HIP_TRY(copy_sync(net, cfg_d, cfg.data(), nl * sizeof(uint2), hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
    float *prev = net->pk_prev;
    uint32_t *left = net->pk_left;
    if (!prev) {
        // registered arrays: the snapshot of "verify" and snn_debug_checkpoint carry the streaming state
        TRY(dev_alloc_t(net, &prev, (size_t)net->n_pad));
        int rc = dev_alloc_t(net, &left, (size_t)net->n_pad);
        if (rc == SNN_OK && (hipMemsetAsync(prev, 0, (size_t)net->n_pad * 4, net->stream) != hipSuccess ||
                             hipMemsetAsync(left, 0xFF, (size_t)net->n_pad * 4, net->stream) != hipSuccess ||
                             hipStreamSynchronize(net->stream) != hipSuccess))
            rc = fail(SNN_ERR_BUFFER_WRITE, "the fill of the peak record's state failed");
        if (rc != SNN_OK) {
            dev_replace(net, prev);
            dev_replace(net, left);
            return rc;
        }
    }
    // ---- the commit (nothing below fails): switching a lattice's record or changing its threshold restarts the shared cursor ----
    net->pk_cfg_host.swap(cfg);
    net->pk_cfg = std::move(cfg_d);
    net->pk_prev = prev; net->pk_left = left;
    net->want_peaks = false;
    for (const uint2 &c : net->pk_cfg_host) net->want_peaks = net->want_peaks || c.x != 0;
    net->pk_epoch += 1;
    net->cur.hist_steps = 0; net->cur.hist_tick = 0;
    return SNN_OK;
}

// what the three getters share: the lattice, its record, the handle at rest
int peak_query_begin(snn_network *net, uint32_t id, const LatticeInfo **lattice)
{
    if (!net) return fail(SNN_ERR_BAD_ARG, "net is null");
    if (!net->finalized) return fail(SNN_ERR_BAD_STATE, "network not finalized");
    const LatticeInfo *l = find_lattice(net, id);
    if (!l || l->spike_train) return fail(SNN_ERR_BAD_ARG, "peak records belong to neuron lattices");
    if (net->pk_cfg_host.empty() || !net->pk_cfg_host[l->slot].x)
        return fail(SNN_ERR_BAD_STATE, "the peak record of this lattice is off (snn_set_peak_history)");
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));
    *lattice = l;
    return SNN_OK;
}

int get_peak_raster(snn_network *net, uint32_t id, uint8_t *dst, size_t steps)
{
    const LatticeInfo *l = nullptr;
    TRY(peak_query_begin(net, id, &l));
    if (steps != net->cur.hist_steps) return fail(SNN_ERR_DIM_MISMATCH, "history size mismatch");
    if (steps == 0 || l->count == 0) return SNN_OK;
    if (!dst) return fail(SNN_ERR_BAD_ARG, "dst is null");
    // the packed rows in hops of at most 8 MiB, unpacked on the way out
    const size_t words = net->n_pad / 64;
    const size_t hop = std::max<size_t>(1, std::min<size_t>(steps, ((size_t)8 << 20) / (words * 8)));
    hvec<unsigned long long> rows(hop * words);
    for (size_t t = 0; t < steps; t += hop) {
        const size_t m = std::min(hop, steps - t);
        HIP_TRY(copy_sync(net, rows.data(), net->pk_raster.get() + t * words, m * words * 8, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
        for (size_t r = 0; r < m; ++r)
            for (uint32_t i = 0; i < l->count; ++i) {
                const uint32_t q = l->first + i;
                dst[(t + r) * l->count + i] = (uint8_t)((rows[r * words + (q >> 6)] >> (q & 63)) & 1ull);
            }
    }
    return SNN_OK;
}

// the lattice's counts over rows [first_step, hist_steps) into counts_d (count words; a first_step past the record counts nothing)
int peak_counts_device(snn_network *net, const LatticeInfo *l, uint64_t first_step, uint32_t *counts_d)
{
    const uint64_t steps = net->cur.hist_steps;
    if (steps == 0 || first_step >= steps) {
        HIP_TRY(hipMemsetAsync(counts_d, 0, (size_t)l->count * 4, net->stream), SNN_ERR_BUFFER_WRITE);
        return SNN_OK;
    }
    hipLaunchKernelGGL(k_peak_counts, dim3((l->count + 255u) / 256u), dim3(256), 0, net->stream,
                       (const unsigned long long *)net->pk_raster.get(), net->n_pad / 64, l->first, l->count, first_step, steps, counts_d);
    HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    return SNN_OK;
}

int get_peak_counts(snn_network *net, uint32_t id, uint64_t first_step, uint32_t *dst, size_t count)
{
    const LatticeInfo *l = nullptr;
    TRY(peak_query_begin(net, id, &l));
    if (count != l->count) return fail(SNN_ERR_DIM_MISMATCH, "count must equal rows*cols");
    if (count == 0) return SNN_OK;
    if (!dst) return fail(SNN_ERR_BAD_ARG, "dst is null");
    dev_ptr<uint32_t> counts_d;
    TRY(sized(&counts_d, count * 4));
    TRY(peak_counts_device(net, l, first_step, counts_d));
    HIP_TRY(copy_sync(net, dst, counts_d, count * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    return SNN_OK;
}

int get_peaks(snn_network *net, uint32_t id, uint64_t first_step, uint64_t *ptr, uint32_t *steps, uint64_t capacity, uint64_t *total)
{
    if (!total) return fail(SNN_ERR_BAD_ARG, "total is null");
    *total = 0;
    const LatticeInfo *l = nullptr;
    TRY(peak_query_begin(net, id, &l));
    const uint32_t count = l->count;
    // every buffer of the call first: counts -> offsets (count + 1 words, scanned in place), the scan's words, the host's offsets
    dev_ptr<uint32_t> offset_d, list_d;
    dev_ptr<unsigned long long> sums_d;
    hvec<uint32_t> offset_h((size_t)count + 1, 0u);
    TRY(sized(&offset_d, ((size_t)count + 1) * 4));
    TRY(sized(&sums_d, ((size_t)(count + 255u) / 256u + 1) * 8));
    TRY(ensure_copy_stage(net));
    uint64_t found = 0;
    if (count) {
        TRY(peak_counts_device(net, l, first_step, offset_d));
        TRY(device_scan(net, offset_d, offset_d, count, sums_d, &found));
    }
    if (found > 0xFFFFFFFFull)
        return fail(SNN_ERR_DIM_MISMATCH, "more than 2^32-1 peaks in one call: ask for a later first_step or use snn_get_peak_counts");
    *total = found;
    if (found > capacity) return SNN_OK;                   // nothing partial: the caller sizes `steps` from *total and calls again
    if (!ptr || (found && !steps)) return fail(SNN_ERR_BAD_ARG, "null list pointer with capacity >= total");
    if (found) {
        TRY(sized(&list_d, found * 4));
        hipLaunchKernelGGL(k_peak_fill, dim3((count + 255u) / 256u), dim3(256), 0, net->stream,
                           (const unsigned long long *)net->pk_raster.get(), net->n_pad / 64, l->first, count, first_step,
                           (uint64_t)net->cur.hist_steps, (const uint32_t *)offset_d.get(), list_d.get());
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    }
    if (count) HIP_TRY(copy_sync(net, offset_h.data(), offset_d, ((size_t)count + 1) * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    if (found) HIP_TRY(copy_sync(net, steps, list_d, found * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    for (size_t i = 0; i <= count; ++i) ptr[i] = offset_h[i];
    return SNN_OK;
}

// ---- voltage-peak totals (snn_set_peak_totals / snn_get_peak_totals / snn_peak_totals_steps; snn_kernels_peak_totals.hpp) ----

// The series starts over: no sample seen, nothing to rise from (prev = NaN, left = NONE: both all-ones words), counts zero.
int peak_totals_restart(snn_network *net)
{
    if (!net->pt_block) return SNN_OK;
    if (hipMemsetAsync(net->pt_block, 0xFF, (size_t)2 * net->n_pad * 4, net->stream) != hipSuccess ||
        hipMemsetAsync(net->pt_counts, 0, (size_t)net->pt_rows * net->n_pad * 4, net->stream) != hipSuccess ||
        hipStreamSynchronize(net->stream) != hipSuccess)
        return fail(SNN_ERR_BUFFER_WRITE, "the fill of the peak totals' state failed");
    net->cur.pt_steps = 0;
    return SNN_OK;
}

int set_peak_totals(snn_network *net, uint32_t id, int enable, float threshold, uint64_t origin, uint32_t window, uint32_t n_windows)
{
    static_assert(PT_PREV == 0 && PT_LEFT == 1, "peak_totals_restart fills the first two rows of the block");
    if (!net) return fail(SNN_ERR_BAD_ARG, "net is null");
    if (!net->finalized) return fail(SNN_ERR_BAD_STATE, "network not finalized: peak totals are switched on a finalized handle");
    const LatticeInfo *l = find_lattice(net, id);
    if (!l || l->spike_train) return fail(SNN_ERR_BAD_ARG, "peak totals belong to neuron lattices");
    if (threshold != threshold) return fail(SNN_ERR_BAD_ARG, "the threshold is NaN: no voltage is above it");
    if (enable && n_windows == 0) return fail(SNN_ERR_BAD_ARG, "n_windows is 0: nothing to count into");
    if (enable && window == 0 && n_windows != 1) return fail(SNN_ERR_BAD_ARG, "window 0 is one open-ended bucket: n_windows must be 1");
    if (net->sharded && net->n_shards > 1)
        return fail(SNN_ERR_BAD_STATE, "peak totals need an unsharded handle or a single shard: one of several shards is not covered");
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));
    using Setting = snn_network::PeakTotalsSetting;
    const size_t nl = std::max<size_t>(1, net->lattices.size()), np = net->n_pad;
    Setting want;
    if (enable) { want.on = true; want.threshold = threshold; want.origin = origin; want.window = window; want.n_windows = n_windows; }
    if (net->pt_cfg_host.empty() && !enable) return SNN_OK;
    if (net->pt_cfg_host.size() == nl) {
        const Setting &have = net->pt_cfg_host[l->slot];
        if (have.on == want.on && __builtin_bit_cast(uint32_t, have.threshold) == __builtin_bit_cast(uint32_t, want.threshold) &&
            have.origin == want.origin && have.window == want.window && have.n_windows == want.n_windows)
            return SNN_OK;
    }
    // ---- everything that can fail, into locals: a refused call leaves the handle as it was ----
    hvec<Setting> cfg(net->pt_cfg_host);
    if (cfg.empty()) cfg.assign(nl, Setting{});
    cfg[l->slot] = want;
    // the block as a restarted series finds it: state rows all ones, every neuron the setting of its lattice (off: a NaN threshold)
    hvec<uint32_t> block((size_t)PT_ROWS * np, 0u);
    std::fill(block.begin(), block.begin() + (size_t)(PT_THRESHOLD + 1) * np, 0xFFFFFFFFu);
    uint32_t rows = 1;
    bool any = false;
    for (const auto &lat : net->lattices) {
        const Setting &c = cfg[lat.slot];
        if (lat.spike_train || !c.on) continue;
        any = true;
        rows = std::max(rows, c.n_windows);
        const uint32_t word[PT_ROWS] = {0xFFFFFFFFu, 0xFFFFFFFFu, __builtin_bit_cast(uint32_t, c.threshold), (uint32_t)c.origin,
                                        (uint32_t)(c.origin >> 32), c.window, c.n_windows};
        for (int r = PT_THRESHOLD; r < PT_ROWS; ++r)
            std::fill(block.begin() + (size_t)r * np + lat.first, block.begin() + (size_t)r * np + lat.first + lat.count, word[r]);
    }
    TRY(ensure_copy_stage(net));
    // registered arrays, fresh ones: snapshots, "verify" and snn_debug_checkpoint carry the state and the counts, row by row
    uint32_t *block_d = nullptr, *counts_d = nullptr;
    int rc = dev_alloc(net, reinterpret_cast<void **>(&block_d), (size_t)PT_ROWS * np * 4, /*scratch=*/false, /*slice=*/np * 4);
    if (rc == SNN_OK) rc = dev_alloc(net, reinterpret_cast<void **>(&counts_d), (size_t)rows * np * 4, /*scratch=*/false, /*slice=*/np * 4);
    if (rc == SNN_OK && copy_sync(net, block_d, block.data(), block.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(SNN_ERR_BUFFER_WRITE, "the upload of the peak totals' settings failed");
    if (rc == SNN_OK && (hipMemsetAsync(counts_d, 0, (size_t)rows * np * 4, net->stream) != hipSuccess || hipStreamSynchronize(net->stream) != hipSuccess))
        rc = fail(SNN_ERR_BUFFER_WRITE, "the fill of the peak totals' counts failed");
    if (rc != SNN_OK) {
        dev_replace(net, block_d);
        dev_replace(net, counts_d);
        return rc;
    }
    // ---- the commit (nothing below fails): the series of every lattice starts over ----
    dev_replace(net, net->pt_block);
    dev_replace(net, net->pt_counts);
    net->pt_cfg_host.swap(cfg);
    net->pt_block = block_d; net->pt_counts = counts_d; net->pt_rows = rows;
    net->want_pt = any;
    net->pk_epoch += 1;                    // (a checkpoint taken before this call no longer fits the handle)
    net->cur.pt_steps = 0;
    return SNN_OK;
}

int get_peak_totals(snn_network *net, uint32_t id, uint32_t *dst, size_t n_windows, size_t count)
{
    if (!net) return fail(SNN_ERR_BAD_ARG, "net is null");
    if (!net->finalized) return fail(SNN_ERR_BAD_STATE, "network not finalized");
    const LatticeInfo *l = find_lattice(net, id);
    if (!l || l->spike_train) return fail(SNN_ERR_BAD_ARG, "peak totals belong to neuron lattices");
    if (net->pt_cfg_host.empty() || !net->pt_cfg_host[l->slot].on)
        return fail(SNN_ERR_BAD_STATE, "the peak totals of this lattice are off (snn_set_peak_totals)");
    if (n_windows != net->pt_cfg_host[l->slot].n_windows) return fail(SNN_ERR_DIM_MISMATCH, "n_windows must equal the lattice's setting");
    if (count != l->count) return fail(SNN_ERR_DIM_MISMATCH, "count must equal rows*cols");
    if (count == 0) return SNN_OK;
    if (!dst) return fail(SNN_ERR_BAD_ARG, "dst is null");
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));
    HIP_TRY(copy2d_sync(net, dst, count * 4, net->pt_counts + l->first, (size_t)net->n_pad * 4, count * 4, n_windows, hipMemcpyDeviceToHost),
            SNN_ERR_BUFFER_READ);
    return SNN_OK;
}

} // namespace
