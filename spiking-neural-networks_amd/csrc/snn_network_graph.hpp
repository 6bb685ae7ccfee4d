// The graph calls of the C ABI, host side (the extern "C" definitions, thin, are in snn_network.hip): graph setters, connect by rule
// (dense and sparse), the Graph trait on dense and sparse handles, the structural edit of a sparse graph -- and what they share: the
// device lists of a call, the walk over a pair list and its last-wins order (snn_graph_pairs.hpp, host only), the prefix sum on the
// device, the commit of a CSR built on the device.  Kernels: snn_kernels_connect*.hpp, _graph_query*.hpp, _graph_merge_csr.hpp.
#pragma once
#include "snn_graph_pairs.hpp"
#include "snn_network_step.hpp"

namespace {

constexpr size_t GRAPH_PAIRS_HOP = (size_t)1 << 20;         // pairs per launch: the lists of a call go to the device in hops of so many

// a device buffer of a call, never of size 0
template <typename T>
int sized(dev_ptr<T> *dst, size_t bytes)
{
    HIP_TRY(snn_malloc(dst, std::max<size_t>(bytes, 256)), SNN_ERR_BUFFER_CREATE);
    return SNN_OK;
}

// the staging buffer of copy_sync, allocated before the first write of a call: no allocation can fail between two writes
int ensure_copy_stage(snn_network *net)
{
    if (net->opt.pinned_copies) HIP_TRY(copy_stage_alloc(net), SNN_ERR_BUFFER_CREATE);
    return SNN_OK;
}

// the lists of a lookup or an edit on the device: index pairs, a value and a flag per pair; a call allocates those it uses (sized)
struct GraphCallLists {
    dev_ptr<uint32_t> pre, post;
    dev_ptr<float> value;
    dev_ptr<uint8_t> flag;
    // one hop: m entries of every host list given, to position `at` of its device list
    int upload(snn_network *net, size_t at, const uint32_t *pre_s, const uint32_t *post_s, const float *value_s, const uint8_t *flag_s, uint32_t m)
    {
        if (pre_s) HIP_TRY(copy_sync(net, pre.get() + at, pre_s, (size_t)m * 4, hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
        if (post_s) HIP_TRY(copy_sync(net, post.get() + at, post_s, (size_t)m * 4, hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
        if (value_s) HIP_TRY(copy_sync(net, value.get() + at, value_s, (size_t)m * 4, hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
        if (flag_s) HIP_TRY(copy_sync(net, flag.get() + at, flag_s, m, hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
        return SNN_OK;
    }
};

// Exclusive prefix sum of count words on the device: out[0 .. count] (count + 1 offsets), the 64-bit total read back.  in == out is fine
// (every thread reads its word before the block's first write).  sums_d: (count + 255) / 256 block sums of 64 bit, then the total.
int device_scan(snn_network *net, const uint32_t *in, uint32_t *out, uint32_t count, unsigned long long *sums_d, uint64_t *total)
{
    *total = 0;
    if (count == 0) return hipMemsetAsync(out, 0, 4, net->stream) == hipSuccess ? SNN_OK : fail(SNN_ERR_BUFFER_WRITE, "hipMemsetAsync failed");
    const uint32_t blocks = (count + 255u) / 256u;
    unsigned long long *total_d = sums_d + blocks;
    hipLaunchKernelGGL(k_connect_scan_local, dim3(blocks), dim3(256), 0, net->stream, in, count, out, sums_d);
    hipLaunchKernelGGL(k_connect_scan_sums, dim3(1), dim3(256), 0, net->stream, sums_d, blocks, total_d);
    hipLaunchKernelGGL(k_connect_scan_add, dim3(blocks), dim3(256), 0, net->stream, out, count, (const unsigned long long *)sums_d,
                       (const unsigned long long *)total_d);
    HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    unsigned long long t = 0;
    HIP_TRY(copy_sync(net, &t, total_d, 8, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    *total = t;
    return SNN_OK;
}

// snn_set / snn_get_graph_rows (rows [pre_begin, pre_begin + pre_count), n_neurons columns on the host) and, `whole`,
// snn_set / snn_get_graph_dense (the n_tot x n_tot matrix)
int graph_io(snn_network *net, bool set, bool whole, uint32_t pre_begin, uint32_t pre_count, float *weights, uint32_t *connections, size_t n_tot)
{
    if (net && set) net->cross_checked = false;
    if (!net) return fail(SNN_ERR_BAD_ARG, "net is null");
    if (!whole) return graph_rows_io(net, pre_begin, pre_count, weights, connections, net->nn, set);
    if (!net->finalized) return fail(SNN_ERR_BAD_STATE, "network not finalized");
    if (n_tot != net->n_tot) return fail(SNN_ERR_DIM_MISMATCH, "graph size does not match the network");
    return graph_rows_io(net, 0, net->n_tot, weights, connections, net->n_tot, set);
}

// the arguments of one connection by rule, checked (snn_connect_by_rule; `where` = "record k: " for snn_connect_by_rules_csr)
// weight_rules: how many weight rules the call takes (CONNECT_RULE_WEIGHTS; CONNECT_SPEC_WEIGHTS for the spec calls)
int connect_check(const snn_network *net, const std::string &where, const snn_connect_record &r, uint32_t weight_rules,
                  const LatticeInfo **pre_out, const LatticeInfo **post_out)
{
    const LatticeInfo *pre = find_lattice(net, r.pre_id), *post = find_lattice(net, r.post_id);
    if (!pre) return fail(SNN_ERR_BAD_ARG, where + "pre_id: unknown lattice id " + std::to_string(r.pre_id));
    if (!post) return fail(SNN_ERR_BAD_ARG, where + "post_id: unknown lattice id " + std::to_string(r.post_id));
    if (post->spike_train)   // LatticeNetworkError::PostsynapticLatticeCannotBeSpikeTrain, neuron/mod.rs:1852-1854
        return fail(SNN_ERR_BAD_ARG, where + "post_id: lattice " + std::to_string(r.post_id) + " is a spike-train lattice, which is never postsynaptic");
    if (r.rule >= CONNECT_RULES) return fail(SNN_ERR_BAD_ARG, where + "rule: unknown connection rule " + std::to_string(r.rule));
    if (r.weight_rule >= weight_rules) return fail(SNN_ERR_BAD_ARG, where + "weight_rule: unknown weight rule " + std::to_string(r.weight_rule));
    if (r.probability != r.probability) return fail(SNN_ERR_BAD_ARG, where + "probability is NaN");
    *pre_out = pre; *post_out = post;
    if (r.weight_rule == CONNECT_DISPLACEMENT || r.weight_rule == CONNECT_FACTORS) return SNN_OK;      // (w_lo, w_hi are not read)
    if (r.w_lo - r.w_lo != 0.0f) return fail(SNN_ERR_BAD_ARG, where + "w_lo is not finite (NaN is the absent-edge sentinel of the device matrix)");
    if (r.w_hi - r.w_hi != 0.0f) return fail(SNN_ERR_BAD_ARG, where + "w_hi is not finite (NaN is the absent-edge sentinel of the device matrix)");
    if (r.weight_rule == CONNECT_UNIFORM && (r.w_hi - r.w_lo) - (r.w_hi - r.w_lo) != 0.0f)      // (lo + inf * u24 is +-inf, or NaN where u24 is 0)
        return fail(SNN_ERR_BAD_ARG, where + "w_hi - w_lo is not finite: the uniform weights would be infinite or the absent-edge sentinel");
    return SNN_OK;
}

// what a spec adds to connect_check: the wrap flags, and for SNN_WEIGHT_DISPLACEMENT the table -- its dimensions follow from the
// two grids and the flags, and every entry is finite or NaN (None).  `ext`: the kernels' form of it, the table still on the host.
int connect_spec_check(const snn_network *net, const std::string &where, const snn_connect_spec &s, const LatticeInfo **pre_out,
                              const LatticeInfo **post_out, ConnectSpecExt *ext, uint32_t weight_rules = CONNECT_SPEC_WEIGHTS)
{
    const snn_connect_record &r = s.record;
    TRY(connect_check(net, where, r, weight_rules, pre_out, post_out));
    if (s.wrap > (SNN_WRAP_ROWS | SNN_WRAP_COLS)) return fail(SNN_ERR_BAD_ARG, where + "wrap: unknown flags " + std::to_string(s.wrap));
    const LatticeInfo *pre = *pre_out, *post = *post_out;
    *ext = ConnectSpecExt{};
    ext->period_r = (s.wrap & SNN_WRAP_ROWS) ? std::max(pre->rows, post->rows) : 0u;
    ext->period_c = (s.wrap & SNN_WRAP_COLS) ? std::max(pre->cols, post->cols) : 0u;
    if (r.weight_rule != CONNECT_DISPLACEMENT) return SNN_OK;        // (table, table_rows and table_cols are not read)
    ext->u_bias = pre->rows ? pre->rows - 1u : 0u;
    ext->v_bias = pre->cols ? pre->cols - 1u : 0u;
    const uint64_t rows = ext->period_r ? ext->period_r : (uint64_t)pre->rows + post->rows - (pre->rows && post->rows ? 1u : 0u);
    const uint64_t cols = ext->period_c ? ext->period_c : (uint64_t)pre->cols + post->cols - (pre->cols && post->cols ? 1u : 0u);
    if (!s.table) return fail(SNN_ERR_BAD_ARG, where + "table is null: SNN_WEIGHT_DISPLACEMENT reads its weights from it");
    if (s.table_rows != rows)
        return fail(SNN_ERR_BAD_ARG, where + "table_rows: " + std::to_string(s.table_rows) + " given, these lattices and flags take " + std::to_string(rows));
    if (s.table_cols != cols)
        return fail(SNN_ERR_BAD_ARG, where + "table_cols: " + std::to_string(s.table_cols) + " given, these lattices and flags take " + std::to_string(cols));
    for (uint64_t k = 0; k < rows * cols; ++k)
        if (s.table[k] == s.table[k] && s.table[k] - s.table[k] != 0.0f)
            return fail(SNN_ERR_BAD_ARG, where + "table: entry " + std::to_string(k) + " is infinite (a weight is finite; NaN marks the pairs without an edge)");
    ext->table_cols = s.table_cols;
    return SNN_OK;
}

// the table of a checked spec in a device buffer of the handle's allocator (the caller's dev_ptr frees it); ext->table points at it
int connect_spec_upload(snn_network *net, const snn_connect_spec &s, ConnectSpecExt *ext, dev_ptr<float> *table_d)
{
    if (s.record.weight_rule != CONNECT_DISPLACEMENT) return SNN_OK;
    const size_t bytes = (size_t)s.table_rows * s.table_cols * 4;
    HIP_TRY(snn_malloc(table_d, std::max<size_t>(bytes, 256)), SNN_ERR_BUFFER_CREATE);
    if (bytes) HIP_TRY(copy_sync(net, table_d->get(), s.table, bytes, hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
    ext->table = table_d->get();
    return SNN_OK;
}

// what snn_connect_by_factors adds to connect_spec_check, for a record with SNN_WEIGHT_FACTORS (with another weight rule nothing of
// it is read): the factor count, both arrays finite and the bound that keeps every weight inside binary32 --
// |w64| <= n_factors * max|U| * max|V| * |scale| up to rounding, far below the 2^128 a conversion would need to overflow.
int connect_factors_check(const std::string &where, const snn_connect_factors &f, const LatticeInfo *pre, const LatticeInfo *post)
{
    if (f.spec.record.weight_rule != CONNECT_FACTORS) return SNN_OK;
    if (f.n_factors == 0 || f.n_factors > 65536u)
        return fail(SNN_ERR_BAD_ARG, where + "n_factors: " + std::to_string(f.n_factors) + " given, a factors record takes 1 .. 65536");
    if (!f.pre_factors) return fail(SNN_ERR_BAD_ARG, where + "pre_factors is null: SNN_WEIGHT_FACTORS reads its weights from it");
    if (!f.post_factors) return fail(SNN_ERR_BAD_ARG, where + "post_factors is null: SNN_WEIGHT_FACTORS reads its weights from it");
    if (f.scale - f.scale != 0.0) return fail(SNN_ERR_BAD_ARG, where + "scale is not finite");
    double largest[2] = {0.0, 0.0};
    const double *arrays[2] = {f.pre_factors, f.post_factors};
    const size_t counts[2] = {(size_t)f.n_factors * pre->count, (size_t)f.n_factors * post->count};
    for (int s = 0; s < 2; ++s)
        for (size_t k = 0; k < counts[s]; ++k) {
            const double v = arrays[s][k];
            if (v - v != 0.0)
                return fail(SNN_ERR_BAD_ARG, where + (s ? "post_factors" : "pre_factors") + ": entry " + std::to_string(k) + " is not finite");
            largest[s] = std::max(largest[s], std::fabs(v));
        }
    const double bound = (double)f.n_factors * largest[0] * largest[1] * std::fabs(f.scale);
    if (!(bound < 0x1p127))
        return fail(SNN_ERR_BAD_ARG, where + "scale: n_factors * max|pre_factors| * max|post_factors| * |scale| is not below 2^127: a weight "
                                             "could leave binary32");
    return SNN_OK;
}

// the factor arrays of a checked factors record in device buffers of the handle's allocator (the caller's dev_ptrs free them)
int connect_factors_upload(snn_network *net, const snn_connect_factors &f, const LatticeInfo *pre, const LatticeInfo *post,
                           ConnectFactorsExt *ext, dev_ptr<double> *pre_d, dev_ptr<double> *post_d)
{
    *ext = ConnectFactorsExt{};
    if (f.spec.record.weight_rule != CONNECT_FACTORS) return SNN_OK;
    const size_t pre_bytes = (size_t)f.n_factors * pre->count * 8, post_bytes = (size_t)f.n_factors * post->count * 8;
    HIP_TRY(snn_malloc(pre_d, std::max<size_t>(pre_bytes, 256)), SNN_ERR_BUFFER_CREATE);
    HIP_TRY(snn_malloc(post_d, std::max<size_t>(post_bytes, 256)), SNN_ERR_BUFFER_CREATE);
    if (pre_bytes) HIP_TRY(copy_sync(net, pre_d->get(), f.pre_factors, pre_bytes, hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
    if (post_bytes) HIP_TRY(copy_sync(net, post_d->get(), f.post_factors, post_bytes, hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
    ext->U = pre_d->get(); ext->V = post_d->get();
    ext->n_factors = f.n_factors; ext->drop_zero = f.drop_zero != 0; ext->scale = f.scale;
    return SNN_OK;
}

// one record as the kernels take it: all of lattice `pre`, the columns (rows of a sparse graph) [c_begin, c_end) of lattice `post`
ConnectArgs connect_args(const snn_network *net, const snn_connect_record &r, const LatticeInfo *pre, const LatticeInfo *post, uint32_t c_begin,
                         uint32_t c_end)
{
    ConnectArgs a{};
    a.col0 = c_begin - net->q0; a.n_cols = c_end - c_begin; a.post_i0 = c_begin - post->first;
    a.post_cols = post->cols; a.post_count = post->count;
    a.pre_first = pre->first; a.pre_count = pre->count; a.pre_rows = pre->rows; a.pre_cols = pre->cols;
    a.extent = r.extent; a.probability = r.probability; a.edge_seed = r.edge_seed; a.weight_seed = r.weight_seed;
    a.w_lo = r.w_lo; a.w_hi = r.w_hi;
    return a;
}

// snn_connect_by_rule, snn_connect_by_spec and snn_connect_by_factors (`factors` set: s is its spec): one body.  A plain spec (no
// table, no distance on a ring) launches k_connect_rule, a factors record k_connect_factors.
int connect_dense(snn_network_t *net, const snn_connect_spec &s, uint32_t weight_rules, const snn_connect_factors *factors = nullptr)
{
    if (!net) return fail(SNN_ERR_BAD_ARG, "net is null");
    if (!net->finalized) return fail(SNN_ERR_BAD_STATE, "network not finalized");
    if (net->csr) return fail(SNN_ERR_BAD_STATE, "connecting by rule is for dense handles only: this handle holds a sparse graph");
    const snn_connect_record &r = s.record;
    const LatticeInfo *pre = nullptr, *post = nullptr;
    ConnectSpecExt x{};
    if (weight_rules == CONNECT_RULE_WEIGHTS)
        TRY(connect_check(net, "", r, CONNECT_RULE_WEIGHTS, &pre, &post));
    else
        TRY(connect_spec_check(net, "", s, &pre, &post, &x, weight_rules));
    if (factors) TRY(connect_factors_check("", *factors, pre, post));
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));                     // a deferred reward-modulated update belongs to the OLD weights: apply it first
    dev_ptr<float> table_d;                // (freed when the call returns; a failure here leaves the graph as it was)
    TRY(connect_spec_upload(net, s, &x, &table_d));
    dev_ptr<double> pre_factors_d, post_factors_d;
    ConnectFactorsExt fx{};
    if (factors) TRY(connect_factors_upload(net, *factors, pre, post, &fx, &pre_factors_d, &post_factors_d));
    net->cross_checked = false;
    net->cache.counts_dirty = true;        // stale from here on, whichever way the call ends (as graph_rows_io marks them on every exit of a set)
    w24_invalidate(net);
    // the block's columns this handle owns, as local columns
    const uint32_t c_begin = std::max(post->first, net->q0), c_end = std::min(post->first + post->count, net->q0 + net->n_loc);
    if (pre->count && c_begin < c_end) {
        ConnectArgs a = connect_args(net, r, pre, post, c_begin, c_end);
        a.W = net->W; a.ld = net->ld;
        const uint32_t groups = ((a.pre_first + a.pre_count - 1u) >> 2) - (a.pre_first >> 2) + 1u;
        const uint32_t blocks_x = (a.col0 + a.n_cols - (a.col0 & ~63u) + 255u) / 256u;
        const dim3 grid(blocks_x, std::min<uint32_t>(groups, 4096));
        const bool thin = r.probability < 1.0f, self = r.self_edges != 0, wrap = x.period_r || x.period_c;
        // (probability <= 0: the draw is made and never succeeds)
        if (r.weight_rule == CONNECT_FACTORS) {
            // row tiles in y: enough workgroups to fill the device, each walking many tiles with the V tile it staged once
            a.w_lo = 0.0f;                 // (connect_factors_on asks connect_spec_value for a constant: 0 or None)
            const uint32_t tiles = (groups + 3u) / 4u;
            const dim3 grid_f(blocks_x, std::min<uint32_t>(tiles, std::max<uint32_t>(1u, 8192u / blocks_x)));
            hipLaunchKernelGGL(connect_factors_kernel((int)r.rule, thin, self), grid_f, dim3(256), 0, net->stream, ConnectFactorsArgs{a, x, fx});
        } else if (connect_spec_is_plain((int)r.rule, (int)r.weight_rule, wrap))
            hipLaunchKernelGGL(connect_kernel((int)r.rule, (int)r.weight_rule, thin, self), grid, dim3(256), 0, net->stream, a);
        else
            hipLaunchKernelGGL(connect_spec_kernel((int)r.rule, (int)r.weight_rule, wrap, thin, self), grid, dim3(256), 0, net->stream,
                               ConnectSpecArgs{a, x});
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
        // a replaced edge starts with a fresh TraceRSTDP; the other blocks keep theirs
        for (float *m : {net->trace.get(), net->pending.get(), net->edge_counter.get()})
            if (m) {
                hipLaunchKernelGGL(k_connect_clear, grid, dim3(256), 0, net->stream, m, net->ld, a.col0, a.n_cols, a.pre_first, a.pre_count);
                HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
            }
        HIP_TRY(hipStreamSynchronize(net->stream), SNN_ERR_WAIT);
    }
    return SNN_OK;
}

// ---- the Graph trait (graph/mod.rs:42-72): lookup_weight, edit_weight, incoming / outgoing connections.  On a dense handle on the
// matrix; on a sparse one on the SELL-64 arrays and the transpose as they lie on the device: no table of size nnz is read, built or
// moved by any of the four (no edge_slot_host, no download of the SELL arrays) ----
// what the calls check first, as graph_rows_io does: a finalized handle of the form the call is for
int graph_begin(const snn_network *net, bool sparse)
{
    if (!net) return fail(SNN_ERR_BAD_ARG, "net is null");
    if (!net->finalized) return fail(SNN_ERR_BAD_STATE, "network not finalized");
    if (!sparse && net->csr)
        return fail(SNN_ERR_BAD_STATE, "handle holds a CSR graph, whose structure is fixed: read it with snn_get_graph_csr_structure / "
                                       "snn_get_graph_csr (12 bytes per edge on the host)");
    if (sparse && !net->csr)
        return fail(SNN_ERR_BAD_STATE, "handle holds a dense graph: ask it with snn_graph_lookup / snn_graph_edit / snn_graph_incoming / "
                                       "snn_graph_outgoing");
    if (sparse && net->block_mode)
        return fail(SNN_ERR_BAD_STATE, "the graph queries do not cover shards by lattice (range-set ownership): not covered");
    return SNN_OK;
}
// one index pair of a call: inside the matrix, and in a column this handle owns (`what`: "pair k" / "post")
int graph_pair_check(const snn_network *net, const std::string &what, uint32_t pre, uint32_t post)
{
    const std::string where = what + " (pre " + std::to_string(pre) + ", post " + std::to_string(post) + "): ";
    if (pre >= net->n_tot) return fail(SNN_ERR_BAD_ARG, where + "pre is not below n_tot = " + std::to_string(net->n_tot));
    if (post >= net->nn) return fail(SNN_ERR_BAD_ARG, where + "post is not below n_neurons = " + std::to_string(net->nn));
    if (post < net->q0 || post >= net->q0 + net->n_loc)
        return fail(SNN_ERR_BAD_ARG, where + "post is outside the columns this shard owns, [" + std::to_string(net->q0) + ", " +
                                     std::to_string(net->q0 + net->n_loc) + ")");
    return SNN_OK;
}
// one column (incoming) or one row (outgoing) of W as ascending (index, weight) lists: the two-call idiom of snn_halo_needs
int graph_line(snn_network *net, bool column, uint32_t line, uint32_t *index, float *weights, uint64_t capacity, uint64_t *count)
{
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));
    const uint32_t n = column ? net->n_tot : net->n_loc;
    if (n == 0 || net->n_loc == 0) return SNN_OK;
    const uint32_t room = index && weights ? (uint32_t)std::min<uint64_t>(capacity, n) : 0u;
    dev_ptr<uint32_t> index_d, count_d;
    dev_ptr<float> w_d;
    HIP_TRY(snn_malloc(&index_d, std::max<size_t>((size_t)room * 4, 256)), SNN_ERR_BUFFER_CREATE);
    HIP_TRY(snn_malloc(&w_d, std::max<size_t>((size_t)room * 4, 256)), SNN_ERR_BUFFER_CREATE);
    HIP_TRY(snn_malloc(&count_d, 256), SNN_ERR_BUFFER_CREATE);
    hipLaunchKernelGGL(column ? k_graph_line<true> : k_graph_line<false>, dim3(1), dim3(256), 0, net->stream, net->W, net->ld, net->q0, line, n,
                       index_d, w_d, room, count_d);
    HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    uint32_t found = 0;
    HIP_TRY(copy_sync(net, &found, count_d, 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    *count = found;
    if (found == 0 || found > capacity) return SNN_OK;
    if (!index || !weights) return fail(SNN_ERR_BAD_ARG, "null list pointer with capacity >= count > 0");
    HIP_TRY(copy_sync(net, index, index_d, (size_t)found * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    HIP_TRY(copy_sync(net, weights, w_d, (size_t)found * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    return SNN_OK;
}

std::string graph_csr_pair(size_t k, uint32_t pre, uint32_t post)
{
    return "pair " + std::to_string(k) + " (pre " + std::to_string(pre) + ", post " + std::to_string(post) + ")";
}
int graph_csr_fixed(size_t k, uint32_t pre, uint32_t post, bool connect)
{
    return fail(SNN_ERR_BAD_ARG, graph_csr_pair(k, pre, post) + (connect ? ": no stored edge, and an edit cannot connect it" : ": a stored edge, and an edit cannot remove it") +
                                     ": the structure of a sparse graph is fixed (snn_connect_by_rules_csr / snn_set_graph_csr replace it).  "
                                     "Nothing of this call was applied");
}

// one row of the SELL arrays (incoming) or one source of the transpose (outgoing) as ascending (index, weight) lists: the count
// is one or two words read from the device, the lists are copied when there is room for them
int graph_csr_line(snn_network *net, bool incoming, uint32_t line, uint32_t *index, float *weights, uint64_t capacity, uint64_t *count)
{
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));
    if (!net->csr_ptr || net->n_loc == 0) return SNN_OK;          // no graph set yet: the empty one
    uint32_t span[2] = {0, 0};
    if (incoming) HIP_TRY(copy_sync(net, &span[1], net->csr_row_len.get() + line, 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    else HIP_TRY(copy_sync(net, span, net->csr_t_ptr.get() + line, 8, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    if (span[1] < span[0]) return fail(SNN_ERR_BAD_STATE, "the stored transpose offsets are not monotone");
    const uint32_t found = span[1] - span[0];
    *count = found;
    if (found == 0 || found > capacity) return SNN_OK;
    if (!index || !weights) return fail(SNN_ERR_BAD_ARG, "null list pointer with capacity >= count > 0");
    dev_ptr<uint32_t> index_d;
    dev_ptr<float> w_d;
    HIP_TRY(snn_malloc(&index_d, std::max<size_t>((size_t)found * 4, 256)), SNN_ERR_BUFFER_CREATE);
    HIP_TRY(snn_malloc(&w_d, std::max<size_t>((size_t)found * 4, 256)), SNN_ERR_BUFFER_CREATE);
    const dim3 grid(std::min<uint32_t>((found + 255u) / 256u, 1024u));
    if (incoming)
        hipLaunchKernelGGL(k_graph_csr_row, grid, dim3(256), 0, net->stream, (const uint32_t *)net->csr_ptr, (const uint32_t *)net->csr_pre,
                           (const float *)net->csr_w, line, found, index_d.get(), w_d.get());
    else
        hipLaunchKernelGGL(k_graph_csr_out, grid, dim3(256), 0, net->stream, (const uint32_t *)net->csr_t_edge, (const uint32_t *)net->csr_post,
                           (const uint32_t *)net->csr_edge_slot, (const float *)net->csr_w, net->q0, span[0], found, index_d.get(), w_d.get());
    HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    HIP_TRY(copy_sync(net, index, index_d, (size_t)found * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    HIP_TRY(copy_sync(net, weights, w_d, (size_t)found * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    return SNN_OK;
}

// ---- what the calls of the two forms share ----
// how the refusal of a connected edge with a NaN weight ends, by the form of the handle
const char *const GRAPH_NAN_DENSE = "sentinel of the device matrix, such an edge cannot be stored (graph/mod.rs:204-213).  "
                                           "Nothing of this call was applied";
const char *const GRAPH_NAN_SPARSE = "sentinel of the dense form, which the sparse form refuses alike (graph/mod.rs:204-213).  "
                                            "Nothing of this call was applied";

// The pair list of a call, walked before anything is written (graph_pairs_check), and the refusal of its first offender in words.
// weights == nullptr: a lookup, no NaN test.  ascending (may be null): strictly by (pre, post), no pair twice.
int graph_pairs_accept(const snn_network *net, const uint32_t *pre, const uint32_t *post, const float *weights, const uint8_t *connected,
                              size_t n, const char *nan_tail, bool *ascending)
{
    const GraphPairsCheck r = graph_pairs_check(pre, post, weights, connected, n, net->n_tot, net->nn, net->q0, net->n_loc);
    if (ascending) *ascending = r.ascending;
    if (r.why == GRAPH_PAIR_FINE) return SNN_OK;
    const size_t k = r.at;
    if (r.why == GRAPH_PAIR_NAN_WEIGHT)
        return fail(SNN_ERR_BAD_ARG, graph_csr_pair(k, pre[k], post[k]) + ": a connected edge carries a NaN weight; NaN is the absent-edge " + nan_tail);
    return graph_pair_check(net, "pair " + std::to_string(k), pre[k], post[k]);
}

// k_graph_csr_find over m pairs of device lists: the entry of every pair (slot), or its weight and whether it is stored (w, c); with
// `want`, every pair is held to the fixed structure and the first offender's position base + j goes to *bad.  Null: not asked for.
void launch_csr_find(snn_network *net, const uint32_t *pre_d, const uint32_t *post_d, uint32_t m, uint32_t *slot, float *w, uint8_t *c,
                            const uint8_t *want, unsigned long long base, unsigned long long *bad)
{
    hipLaunchKernelGGL(k_graph_csr_find, dim3((m + 255u) / 256u), dim3(256), 0, net->stream, (const uint32_t *)net->csr_ptr,
                       (const uint32_t *)net->csr_pre, (const float *)net->csr_w, (const uint32_t *)net->csr_row_len, net->q0, pre_d, post_d, m,
                       slot, w, c, want, base, bad);
}

// snn_graph_lookup and snn_graph_csr_lookup: one body
int graph_lookup(snn_network *net, bool sparse, const uint32_t *pre, const uint32_t *post, size_t n, float *weights, uint8_t *connected)
{
    TRY(graph_begin(net, sparse));
    if (n == 0) return SNN_OK;
    if (!pre || !post || !weights || !connected) return fail(SNN_ERR_BAD_ARG, "null pointer with n > 0");
    TRY(graph_pairs_accept(net, pre, post, nullptr, nullptr, n, nullptr, nullptr));
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));                     // deferred STDP / R-STDP updates belong to the weights a lookup sees
    if (sparse && !net->csr_ptr) {         // no graph set yet: the empty one
        std::fill(weights, weights + n, 0.0f);
        std::fill(connected, connected + n, (uint8_t)0);
        return SNN_OK;
    }
    const size_t hop = std::min(n, GRAPH_PAIRS_HOP);
    GraphCallLists l;                      // value, flag: the answers
    TRY(sized(&l.pre, hop * 4));
    TRY(sized(&l.post, hop * 4));
    TRY(sized(&l.value, hop * 4));
    TRY(sized(&l.flag, hop));
    for (size_t k = 0; k < n; k += hop) {
        const uint32_t m = (uint32_t)std::min(hop, n - k);
        TRY(l.upload(net, 0, pre + k, post + k, nullptr, nullptr, m));
        if (sparse)
            launch_csr_find(net, l.pre, l.post, m, nullptr, l.value, l.flag, nullptr, 0, nullptr);
        else
            hipLaunchKernelGGL(k_graph_lookup, dim3((m + 255u) / 256u), dim3(256), 0, net->stream, net->W, net->ld, net->q0, l.pre, l.post, m,
                               l.value, l.flag);
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
        HIP_TRY(copy_sync(net, weights + k, l.value, (size_t)m * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
        HIP_TRY(copy_sync(net, connected + k, l.flag, m, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    }
    return SNN_OK;
}

// The write pass of an in-place sparse edit, one launch: value_d[j] goes to the entry slot_d[sel_d ? sel_d[j] : j], j < m, and the
// per-edge state of that entry starts afresh.  The structure stays; the step image's records are packed again before the next
// image step.
int graph_csr_store(snn_network *net, const uint32_t *slot_d, const unsigned long long *sel_d, const float *value_d, uint32_t m)
{
    net->cross_checked = false;
    net->img_stale = net->img_stale_direct = true;
    hipLaunchKernelGGL(k_graph_csr_store, dim3((m + 255u) / 256u), dim3(256), 0, net->stream, net->csr_w.get(), net->trace.get(),
                       net->pending.get(), net->edge_counter.get(), slot_d, sel_d, value_d, m);
    HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    HIP_TRY(hipStreamSynchronize(net->stream), SNN_ERR_WAIT);
    return SNN_OK;
}

// what the four line queries check after the handle: `count`, and the line -- incoming: a neuron this handle owns, outgoing: a source
int graph_line_check(const snn_network *net, bool incoming, uint32_t line, uint64_t *count)
{
    if (!count) return fail(SNN_ERR_BAD_ARG, "count is null");
    *count = 0;
    if (!incoming) {
        if (line >= net->n_tot) return fail(SNN_ERR_BAD_ARG, "pre " + std::to_string(line) + " is not below n_tot = " + std::to_string(net->n_tot));
        return SNN_OK;
    }
    if (line >= net->nn) return fail(SNN_ERR_BAD_ARG, "post " + std::to_string(line) + " is not below n_neurons = " + std::to_string(net->nn));
    if (line < net->q0 || line >= net->q0 + net->n_loc)
        return fail(SNN_ERR_BAD_ARG, "post " + std::to_string(line) + " is outside the columns this shard owns, [" + std::to_string(net->q0) +
                                     ", " + std::to_string(net->q0 + net->n_loc) + ")");
    return SNN_OK;
}

// the four line queries: one body.  A dense handle compacts a column or a row of W, a sparse one copies a row or a transposed list
int graph_line_query(snn_network *net, bool sparse, bool incoming, uint32_t line, uint32_t *index, float *weights, uint64_t capacity,
                     uint64_t *count)
{
    TRY(graph_begin(net, sparse));
    TRY(graph_line_check(net, incoming, line, count));
    if (incoming) line -= net->q0;         // (the local column, the local row)
    return sparse ? graph_csr_line(net, incoming, line, index, weights, capacity, count) : graph_line(net, incoming, line, index, weights, capacity, count);
}

// snn_graph_edit
int graph_edit(snn_network *net, const uint32_t *pre, const uint32_t *post, const float *weights, const uint8_t *connected, size_t n)
{
    TRY(graph_begin(net, false));
    if (n == 0) return SNN_OK;
    if (!pre || !post || !weights || !connected) return fail(SNN_ERR_BAD_ARG, "null pointer with n > 0");
    // every pair is checked before anything is written: a refused call leaves the graph as it was
    bool ascending = true;
    TRY(graph_pairs_accept(net, pre, post, weights, connected, n, GRAPH_NAN_DENSE, &ascending));
    // "as if one after another": of a pair that occurs more than once the LAST occurrence is kept, decided here -- every element is
    // written by one thread, whatever the order the threads run in.  An ascending list has no pair twice: no table is built
    hvec<uint64_t> order;
    const size_t kept = ascending ? n : graph_pairs_last_wins(pre, post, n, GRAPH_KEY_PRE_POST, order);
    const size_t hop = std::min(kept, GRAPH_PAIRS_HOP);
    GraphCallLists l;                      // value: the weight, NaN for a pair that is not connected
    hvec<uint32_t> pre_h(hop), post_h(hop);
    hvec<float> value_h(hop);
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));                     // a deferred update belongs to the OLD weights: applied now, it cannot overwrite the edit
    TRY(sized(&l.pre, hop * 4));
    TRY(sized(&l.post, hop * 4));
    TRY(sized(&l.value, hop * 4));
    TRY(ensure_copy_stage(net));
    net->cross_checked = false;
    net->cache.counts_dirty = true;        // stale from here on, whichever way the call ends
    w24_invalidate(net);
    const float absent = std::nanf("");
    for (size_t k = 0; k < kept; k += hop) {
        const uint32_t m = (uint32_t)std::min(hop, kept - k);
        for (uint32_t j = 0; j < m; ++j) {
            const size_t src = ascending ? k + j : (size_t)order[k + j];
            pre_h[j] = pre[src]; post_h[j] = post[src];
            value_h[j] = connected[src] ? weights[src] : absent;
        }
        TRY(l.upload(net, 0, pre_h.data(), post_h.data(), value_h.data(), nullptr, m));
        hipLaunchKernelGGL(k_graph_edit, dim3((m + 255u) / 256u), dim3(256), 0, net->stream, net->W, net->trace.get(), net->pending.get(),
                           net->edge_counter.get(), net->ld, net->q0, l.pre, l.post, l.value, m);
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
        HIP_TRY(hipStreamSynchronize(net->stream), SNN_ERR_WAIT);
    }
    return SNN_OK;
}

// snn_graph_csr_edit: the weights of stored edges; the structure stays
int graph_csr_edit(snn_network *net, const uint32_t *pre, const uint32_t *post, const float *weights, const uint8_t *connected, size_t n)
{
    TRY(graph_begin(net, true));
    if (n == 0) return SNN_OK;
    if (!pre || !post || !weights || !connected) return fail(SNN_ERR_BAD_ARG, "null pointer with n > 0");
    // every pair is checked before anything is written: a refused call leaves the graph as it was
    bool ascending = true;
    TRY(graph_pairs_accept(net, pre, post, weights, connected, n, GRAPH_NAN_SPARSE, &ascending));
    if (!net->csr_ptr) {                   // no graph set yet: every pair is absent, and stays so
        for (size_t k = 0; k < n; ++k)
            if (connected[k]) return graph_csr_fixed(k, pre[k], post[k], true);
        return SNN_OK;
    }
    // "as if one after another": the structure never changes, so every occurrence of a pair is held to the rule on its own (the
    // resolve pass, in the order of the call), and of a pair that occurs more than once the LAST occurrence is written, decided
    // here -- every entry is written by one thread, whatever the order the threads run in.  An ascending list: no table is built
    hvec<uint64_t> order;
    const size_t kept = ascending ? n : graph_pairs_last_wins(pre, post, n, GRAPH_KEY_PRE_POST, order);
    const size_t hop = std::min(n, GRAPH_PAIRS_HOP);
    GraphCallLists l;                      // flag: connected, for the resolve pass; value: the weights of the write pass
    hvec<float> value_h(ascending ? 0 : hop);
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));                     // a deferred update belongs to the OLD weights: applied now, it cannot overwrite the edit
    dev_ptr<uint32_t> slot_d;              // the entry of every pair of the call, in its order: n of them, not a hop
    dev_ptr<unsigned long long> sel_d, bad_d;
    TRY(sized(&l.pre, hop * 4));
    TRY(sized(&l.post, hop * 4));
    TRY(sized(&l.flag, hop));
    TRY(sized(&slot_d, n * 4));
    TRY(sized(&l.value, hop * 4));
    if (!ascending) TRY(sized(&sel_d, hop * 8));
    TRY(sized(&bad_d, 256));
    TRY(ensure_copy_stage(net));
    // ---- the resolve pass: read only; hop k fills slot_d[k ..] ----
    unsigned long long bad = GRAPH_CSR_ALL_FINE;
    HIP_TRY(copy_sync(net, bad_d, &bad, 8, hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
    for (size_t k = 0; k < n; k += hop) {
        const uint32_t m = (uint32_t)std::min(hop, n - k);
        TRY(l.upload(net, 0, pre + k, post + k, nullptr, connected + k, m));
        launch_csr_find(net, l.pre, l.post, m, slot_d.get() + k, nullptr, nullptr, l.flag, k, bad_d);
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
        HIP_TRY(hipStreamSynchronize(net->stream), SNN_ERR_WAIT);
    }
    HIP_TRY(copy_sync(net, &bad, bad_d, 8, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    if (bad != GRAPH_CSR_ALL_FINE) {
        if (bad >= n) return fail(SNN_ERR_BAD_STATE, "the resolve pass named a pair the call does not have");
        return graph_csr_fixed((size_t)bad, pre[bad], post[bad], connected[bad] != 0);
    }
    // ---- the write pass: the kept entries in hops.  Ascending, hop k writes the entries slot_d[k ..]; otherwise order[k ..] selects
    // them from the slots of the whole call ----
    for (size_t k = 0; k < kept; k += hop) {
        const uint32_t m = (uint32_t)std::min(hop, kept - k);
        if (ascending) {
            TRY(l.upload(net, 0, nullptr, nullptr, weights + k, nullptr, m));
        } else {
            for (uint32_t j = 0; j < m; ++j) value_h[j] = weights[order[k + j]];
            TRY(l.upload(net, 0, nullptr, nullptr, value_h.data(), nullptr, m));
            HIP_TRY(copy_sync(net, sel_d, order.data() + k, (size_t)m * 8, hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
        }
        TRY(graph_csr_store(net, ascending ? slot_d.get() + k : slot_d.get(), sel_d, l.value, m));
    }
    return SNN_OK;
}

int ensure_traces(snn_network *net), ensure_pending(snn_network *net);       // (with the plasticity calls, in snn_network.hip)
int edge_history_resolve(snn_network *net);                                  // (snn_network_edge_history.hpp)

// All or nothing: a failed call leaves the previous graph in place, intact -- except that the traces / dw / counters of a handle
// with modulation or connection kinds are sized by the new graph and allocated after the commit: if THAT fails, the handle holds
// the new graph without them.  Device memory peaks at old graph + new graph while the call runs.
// `keep` (may be null): at the commit the planes of the replaced edges move there instead of being freed -- a structural edit
// carries them over to the edges it keeps (snn_graph_csr_edit_structure).  Untouched when the call fails before the commit.
struct CsrEdgePlanes { dev_ptr<float> trace, pending, edge_counter; };

int set_graph_csr_impl(snn_network_t *net, const uint64_t *row_ptr, const uint32_t *pre_index, const float *weights,
                              uint64_t nnz, CsrEdgePlanes *keep = nullptr)
{
    if (!net) return fail(SNN_ERR_BAD_ARG, "net is null");
    if (!net->finalized) return fail(SNN_ERR_BAD_STATE, "network not finalized");
    if (!net->csr) return fail(SNN_ERR_BAD_STATE, "handle holds a dense graph: call snn_network_use_csr before finalize");
    if (!row_ptr || (nnz && (!pre_index || !weights))) return fail(SNN_ERR_BAD_ARG, "null graph pointer");
    if (nnz >= 0xFFFFFFFFull) return fail(SNN_ERR_DIM_MISMATCH, "more than 2^32-1 stored synapses per handle");
    if ((uint64_t)net->nn + net->nc >= PLAN_CODE) return fail(SNN_ERR_DIM_MISMATCH, "the gather plan addresses fewer than 2^31-1 presynaptic rows");
    // the caller's rows are the OWNED neurons in ascending order; a range-set shard places them on its local rows
    // (global 64-blocks, holes in between keep length 0)
    const uint32_t n_loc = net->n_loc, n_rows = net->n_owned;
    auto local = [&](uint32_t k) { return net->block_mode ? net->owned_local_host[k] : k; };
    if (row_ptr[0] != 0 || row_ptr[n_rows] != nnz) return fail(SNN_ERR_DIM_MISMATCH, "row_ptr must run from 0 to nnz");
    const uint32_t n_slices = (n_loc + 63) / 64;
    hvec<uint32_t> slice_ptr((size_t)n_slices + 1, 0), row_len((size_t)n_slices * 64, 0), post(nnz),
        t_ptr((size_t)net->n_tot + 1, 0), t_edge(nnz), edge_slot(nnz);
    for (uint32_t k = 0; k < n_rows; ++k) {
        const uint32_t q = local(k);
        if (row_ptr[k + 1] < row_ptr[k]) return fail(SNN_ERR_DIM_MISMATCH, "row_ptr is not monotone");
        row_len[q] = (uint32_t)(row_ptr[k + 1] - row_ptr[k]);
        for (uint64_t e = row_ptr[k]; e < row_ptr[k + 1]; ++e) {
            if (pre_index[e] >= net->n_tot) return fail(SNN_ERR_DIM_MISMATCH, "presynaptic index out of range");
            if (e > row_ptr[k] && pre_index[e] <= pre_index[e - 1])
                return fail(SNN_ERR_BAD_ARG, "presynaptic indices of a row must be strictly ascending");
            if (weights[e] != weights[e])          // (the dense form cannot hold such an edge: the two forms refuse alike)
                return fail(SNN_ERR_BAD_ARG, "stored edge " + std::to_string(e) + " (pre " + std::to_string(pre_index[e]) + ") carries a NaN weight");
            post[e] = q;
            ++t_ptr[pre_index[e] + 1];
        }
    }
    // SELL-64: every slice (64 rows) is padded to its longest row
    uint64_t entries = 0;
    for (uint32_t sl = 0; sl < n_slices; ++sl) {
        uint32_t width = 0;
        for (uint32_t r = sl * 64; r < sl * 64 + 64; ++r) width = std::max(width, row_len[r]);
        slice_ptr[sl] = (uint32_t)entries;
        entries += (uint64_t)width * 64;
        if (entries >= 0xFFFFFFFFull) return fail(SNN_ERR_DIM_MISMATCH, "sparse graph too large for 32-bit slots");
    }
    slice_ptr[n_slices] = (uint32_t)entries;
    hvec<uint32_t> sell_pre(entries, SELL_PAD);
    hvec<float> sell_w(entries, 0.0f);
    for (uint32_t k = 0; k < n_rows; ++k) {
        const uint32_t q = local(k);
        const uint32_t base = slice_ptr[q >> 6] + (q & 63u);
        for (uint64_t e = row_ptr[k]; e < row_ptr[k + 1]; ++e) {
            const uint32_t slot = base + (uint32_t)(e - row_ptr[k]) * 64;
            sell_pre[slot] = pre_index[e];
            sell_w[slot] = weights[e];
            edge_slot[e] = slot;
        }
    }
    for (size_t p = 0; p < net->n_tot; ++p) t_ptr[p + 1] += t_ptr[p];
    {
        hvec<uint32_t> fill(t_ptr.begin(), t_ptr.end() - 1);
        for (uint64_t e = 0; e < nnz; ++e) t_edge[fill[pre_index[e]]++] = (uint32_t)e;
    }
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));
    // everything of the new graph goes into locals first (device arrays, gather plan, step image, halo lists, cell list); the
    // commit below only moves and swaps
    dev_ptr<uint32_t> slice_ptr_d, pre_d, row_len_d, edge_slot_d, post_d, t_ptr_d, t_edge_d, plan_d, img_hdr_d, plan_win_d;
    dev_ptr<float> w_d;
    dev_ptr<uint4> img_rec_d;
    auto up = [&](auto *dst, const void *src, size_t bytes) -> int {
        HIP_TRY(snn_malloc(dst, std::max<size_t>(bytes, 256)), SNN_ERR_BUFFER_CREATE);
        if (bytes) HIP_TRY(copy_sync(net, *dst, src, bytes, hipMemcpyHostToDevice), SNN_ERR_BUFFER_WRITE);
        return SNN_OK;
    };
    TRY(up(&slice_ptr_d, slice_ptr.data(), slice_ptr.size() * 4));
    TRY(up(&pre_d, sell_pre.data(), entries * 4));
    TRY(up(&w_d, sell_w.data(), entries * 4));
    TRY(up(&row_len_d, row_len.data(), row_len.size() * 4));
    TRY(up(&edge_slot_d, edge_slot.data(), nnz * 4));
    TRY(up(&post_d, post.data(), nnz * 4));
    TRY(up(&t_ptr_d, t_ptr.data(), t_ptr.size() * 4));
    TRY(up(&t_edge_d, t_edge.data(), nnz * 4));
    HIP_TRY(snn_malloc(&plan_d, std::max<size_t>(entries * 4, 256)), SNN_ERR_BUFFER_CREATE);
    uint64_t img_records = 0, img_staged_slices = 0;
    {
        // the step image's host-built half: slice headers with the window pieces, and the plan words that go with them
        hvec<uint32_t> img_hdr, plan_win;
        build_step_image_plan(net->nn, net->nc, slice_ptr, sell_pre, n_slices, img_hdr, plan_win, img_records, img_staged_slices);
        TRY(up(&img_hdr_d, img_hdr.data(), img_hdr.size() * 4));
        TRY(up(&plan_win_d, plan_win.data(), plan_win.size() * 4));
        HIP_TRY(snn_malloc(&img_rec_d, (size_t)img_records * 16 + 4096), SNN_ERR_BUFFER_CREATE);    // (+ a wavefront's load of slack)
    }
    if (n_slices) {
        SellGraph g = csr_graph(net);                 // (the handle's geometry, the new arrays)
        g.slice_ptr = slice_ptr_d; g.pre = pre_d; g.w = w_d; g.row_len = row_len_d;
        g.edge_slot = edge_slot_d; g.edge_post = post_d; g.t_ptr = t_ptr_d; g.t_edge = t_edge_d; g.plan = plan_d;
        hipLaunchKernelGGL(k_csr_plan, dim3((n_slices * 64 + 255) / 256), dim3(256), 0, net->stream, g,
                           plan_d, (const uint32_t *)nullptr, net->nn, PLAN_CODE);
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    }
    // the new rows decide what is read from the other shards, and which spike-train cells this rank reads at all
    hvec<hvec<uint32_t>> halo_need(net->n_shards), halo_send(net->n_shards);
    halo_needs_from_rows(net, pre_index, nnz, halo_need);
    const bool list_cells = net->sharded && net->n_shards > 1 && net->nc;
    hvec<uint32_t> cells;
    dev_ptr<uint32_t> cells_d;
    if (list_cells) {
        hvec<uint8_t> seen(net->nc, 0);
        for (uint64_t e = 0; e < nnz; ++e)
            if (pre_index[e] >= net->nn) seen[pre_index[e] - net->nn] = 1;
        for (uint32_t s = 0; s < net->nc; ++s)
            if (seen[s]) cells.push_back(s);
        TRY(upload_table(net, &cells_d, cells));
    }
    // ---- the commit ----
    net->csr_ptr = std::move(slice_ptr_d); net->csr_pre = std::move(pre_d); net->csr_w = std::move(w_d);
    net->csr_row_len = std::move(row_len_d); net->csr_edge_slot = std::move(edge_slot_d); net->csr_post = std::move(post_d);
    net->csr_t_ptr = std::move(t_ptr_d); net->csr_t_edge = std::move(t_edge_d); net->csr_plan = std::move(plan_d);
    net->csr_img_hdr = std::move(img_hdr_d); net->csr_plan_win = std::move(plan_win_d); net->csr_img_rec = std::move(img_rec_d);
    net->img_records = img_records; net->img_staged_slices = img_staged_slices;
    net->img_stale = net->img_stale_direct = true;
    if (keep) { keep->trace = std::move(net->trace); keep->pending = std::move(net->pending); keep->edge_counter = std::move(net->edge_counter); }
    net->trace = nullptr;                                        // traces belong to the replaced edges
    net->pending = nullptr; net->edge_counter = nullptr;         // ... and so do dw and the counters of its connections
    net->cross_checked = false;
    net->nnz = nnz;
    net->sell_entries = entries;
    net->edge_slot_host.swap(edge_slot);
    if (net->sharded && net->n_shards > 1) { net->sell_pre_host.swap(sell_pre); net->slice_ptr_host.swap(slice_ptr); }
    else { net->sell_pre_host.clear(); net->slice_ptr_host.clear(); }
    net->cache.counts_dirty = true;
    net->halo_need.swap(halo_need); net->halo_send.swap(halo_send);
    net->halo_committed = false; net->x_dirty = true;
    if (list_cells) {
        net->cell_list_host.swap(cells);
        net->cell_list_dev = std::move(cells_d);
        net->n_cells_listed = (uint32_t)net->cell_list_host.size();
        net->cache.view_dirty = true;
    }
    // a reward-modulated handle keeps modulating: zeroed traces for the new edges, sized by the committed graph (see above)
    if (net->any_modulation || net->any_conn_kind) TRY(ensure_traces(net));
    if (net->any_conn_kind) TRY(ensure_pending(net));
    // the pairs of an installed edge history are identities, not entries: each finds its entry in the committed arrays, or none
    return edge_history_resolve(net);
}

// A CSR built on the device (rows + 1 32-bit offsets, nnz presynaptic indices and weights) becomes the handle's graph: one download,
// then the host builder of snn_set_graph_csr -- all or nothing from here as before here.  The three buffers are freed between the
// two, and the caller has freed every other working buffer by now (edit lists, flags, scan words, row lengths, the CSR set its last
// merge read; the source word per new edge of a structural edit may stay): device memory peaks at old graph + new graph.
// built (may be null): when set_graph_csr_impl began and ended -- what precedes is the download, and the host arrays are freed after.
int commit_device_csr(snn_network *net, dev_ptr<uint32_t> &ptr_d, dev_ptr<uint32_t> &pre_d, dev_ptr<float> &w_d, uint32_t rows, uint64_t nnz,
                      CsrEdgePlanes *keep, std::chrono::steady_clock::time_point *built = nullptr)
{
    hvec<uint32_t> ptr32((size_t)rows + 1), pre_h((size_t)nnz);
    hvec<float> w_h((size_t)nnz);
    HIP_TRY(copy_sync(net, ptr32.data(), ptr_d, ptr32.size() * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    if (nnz) {
        HIP_TRY(copy_sync(net, pre_h.data(), pre_d, nnz * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
        HIP_TRY(copy_sync(net, w_h.data(), w_d, nnz * 4, hipMemcpyDeviceToHost), SNN_ERR_BUFFER_READ);
    }
    ptr_d.reset(); pre_d.reset(); w_d.reset();
    hvec<uint64_t> ptr64(ptr32.begin(), ptr32.end());
    hvec<uint32_t>().swap(ptr32);
    uint32_t no_pre = 0;                   // (an empty graph: the builder still wants pointers)
    float no_w = 0.0f;
    const auto t_builder = std::chrono::steady_clock::now();
    const int rc = set_graph_csr_impl(net, ptr64.data(), nnz ? pre_h.data() : &no_pre, nnz ? w_h.data() : &no_w, nnz, keep);
    if (built) { built[0] = t_builder; built[1] = std::chrono::steady_clock::now(); }
    return rc;
}

// snn_connect_by_rules_csr (specs == nullptr: every record plain), snn_connect_by_specs_csr (records == nullptr) and
// snn_connect_by_factors_csr (factors_form: the list is `items`, the spec of record k is items[k].spec): one body
int connect_csr(snn_network_t *net, const snn_connect_record *records, const snn_connect_spec *specs, uint32_t n_records,
                const snn_connect_factors *items = nullptr, bool factors_form = false)
{
    if (!net) return fail(SNN_ERR_BAD_ARG, "net is null");
    if (!net->finalized) return fail(SNN_ERR_BAD_STATE, "network not finalized");
    if (!net->csr) return fail(SNN_ERR_BAD_STATE, "handle holds a dense graph: connect it with snn_connect_by_rule");
    if (net->block_mode) return fail(SNN_ERR_BAD_STATE, "connecting by rule does not cover shards by lattice (range-set ownership): not covered");
    if (n_records == 0) return SNN_OK;
    if (!records && !specs && !items) return fail(SNN_ERR_BAD_ARG, factors_form ? "items is null" : "records is null");
    auto spec_of = [&](uint32_t k) -> const snn_connect_spec & { return items ? items[k].spec : specs[k]; };
    hvec<std::pair<const LatticeInfo *, const LatticeInfo *>> ends(n_records);
    hvec<ConnectSpecExt> exts(n_records);
    for (uint32_t k = 0; k < n_records; ++k) {
        const std::string where = (factors_form ? "item " : "record ") + std::to_string(k) + ": ";
        if (items) {
            TRY(connect_spec_check(net, where, items[k].spec, &ends[k].first, &ends[k].second, &exts[k], CONNECT_FACTOR_WEIGHTS));
            TRY(connect_factors_check(where, items[k], ends[k].first, ends[k].second));
        } else if (specs) TRY(connect_spec_check(net, where, specs[k], &ends[k].first, &ends[k].second, &exts[k]));
        else TRY(connect_check(net, where, records[k], CONNECT_RULE_WEIGHTS, &ends[k].first, &ends[k].second));
    }
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));                     // a deferred update belongs to the weights the merge is about to read
    const uint32_t n = net->n_loc, scan_blocks = (n + 255u) / 256u;
    // two sets of working CSR (the merge of a record reads one and writes the other), the row lengths and the scan's words: all
    // locals, freed on every exit
    dev_ptr<uint32_t> ptr[2], pre[2], len_d;
    dev_ptr<float> w[2];
    dev_ptr<unsigned long long> sums_d;              // the words of device_scan
    for (int s = 0; s < 2; ++s) TRY(sized(&ptr[s], ((size_t)n + 1) * 4));
    TRY(sized(&len_d, (size_t)n * 4));
    TRY(sized(&sums_d, ((size_t)scan_blocks + 1) * 8));
    // ---- the current graph, from SELL-64 (weights as plasticity left them) ----
    int cur = 0;
    uint64_t nnz = 0;
    if (net->csr_ptr && n) {
        TRY(device_scan(net, net->csr_row_len, ptr[cur], n, sums_d, &nnz));
        if (nnz != net->nnz) return fail(SNN_ERR_BAD_STATE, "stored row lengths do not add up to the stored edge count");
        TRY(sized(&pre[cur], nnz * 4));
        TRY(sized(&w[cur], nnz * 4));
        hipLaunchKernelGGL(k_connect_csr_export, dim3(scan_blocks), dim3(256), 0, net->stream, (const uint32_t *)net->csr_ptr,
                           (const uint32_t *)net->csr_pre, (const float *)net->csr_w, (const uint32_t *)net->csr_row_len,
                           (const uint32_t *)ptr[cur], n, pre[cur].get(), w[cur].get());
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    } else {
        HIP_TRY(hipMemsetAsync(ptr[cur], 0, ((size_t)n + 1) * 4, net->stream), SNN_ERR_BUFFER_WRITE);
        TRY(sized(&pre[cur], 0));
        TRY(sized(&w[cur], 0));
    }
    // ---- record by record: count, scan, check the total, fill, swap ----
    for (uint32_t k = 0; k < n_records; ++k) {
        const snn_connect_record &r = records ? records[k] : spec_of(k).record;
        const LatticeInfo *lp = ends[k].first, *lq = ends[k].second;
        // the block's rows this handle owns, as local rows (the dense form: its columns)
        const uint32_t c_begin = std::max(lq->first, net->q0), c_end = std::min(lq->first + lq->count, net->q0 + n);
        if (!n || c_begin >= c_end) continue;          // (an empty pre lattice still clears nothing: the block has no pair)
        if (!lp->count) continue;
        ConnectCsrArgs a{};
        a.c = connect_args(net, r, lp, lq, c_begin, c_end);
        a.n_rows = n;
        a.window = connect_window_extent(r.rule, r.extent, std::max(std::max(lp->rows, lp->cols), std::max(lq->rows, lq->cols)));
        a.old_ptr = ptr[cur]; a.old_pre = pre[cur]; a.old_w = w[cur];
        a.new_len = len_d;
        const bool thin = r.probability < 1.0f, self = r.self_edges != 0, wrap = exts[k].period_r || exts[k].period_c;
        const bool plain = connect_spec_is_plain((int)r.rule, (int)r.weight_rule, wrap);
        dev_ptr<float> table_d;                        // (read by both passes; freed after the wait that ends this record)
        if (!records) TRY(connect_spec_upload(net, spec_of(k), &exts[k], &table_d));
        dev_ptr<double> pre_factors_d, post_factors_d;     // (likewise)
        ConnectFactorsExt fx{};
        if (items) TRY(connect_factors_upload(net, items[k], lp, lq, &fx, &pre_factors_d, &post_factors_d));
        const bool by_factors = r.weight_rule == CONNECT_FACTORS;
        if (by_factors) a.c.w_lo = 0.0f;               // (connect_factors_on asks connect_spec_value for a constant: 0 or None)
        const dim3 grid(std::min<uint32_t>((n + 3u) / 4u, 16384u));
        if (by_factors)
            hipLaunchKernelGGL(connect_csr_factors_kernel<false>((int)r.rule, thin, self), grid, dim3(256), 0, net->stream,
                               ConnectCsrFactorsArgs{a, exts[k], fx});
        else if (plain)
            hipLaunchKernelGGL(connect_csr_kernel<false>((int)r.rule, (int)r.weight_rule, thin, self), grid, dim3(256), 0, net->stream, a);
        else
            hipLaunchKernelGGL(connect_csr_spec_kernel<false>((int)r.rule, (int)r.weight_rule, wrap, thin, self), grid, dim3(256), 0, net->stream,
                               ConnectCsrSpecArgs{a, exts[k]});
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
        uint64_t total = 0;
        TRY(device_scan(net, len_d, ptr[cur ^ 1], n, sums_d, &total));     // lengths -> n + 1 offsets
        if (total >= 0xFFFFFFFFull)
            return fail(SNN_ERR_DIM_MISMATCH, (factors_form ? "item " : "record ") + std::to_string(k) + ": the graph would hold " + std::to_string(total) +
                                                  " stored synapses, more than 2^32-2 per handle");
        TRY(sized(&pre[cur ^ 1], total * 4));
        TRY(sized(&w[cur ^ 1], total * 4));
        a.new_ptr = ptr[cur ^ 1]; a.new_pre = pre[cur ^ 1]; a.new_w = w[cur ^ 1];
        if (by_factors)
            hipLaunchKernelGGL(connect_csr_factors_kernel<true>((int)r.rule, thin, self), grid, dim3(256), 0, net->stream,
                               ConnectCsrFactorsArgs{a, exts[k], fx});
        else if (plain)
            hipLaunchKernelGGL(connect_csr_kernel<true>((int)r.rule, (int)r.weight_rule, thin, self), grid, dim3(256), 0, net->stream, a);
        else
            hipLaunchKernelGGL(connect_csr_spec_kernel<true>((int)r.rule, (int)r.weight_rule, wrap, thin, self), grid, dim3(256), 0, net->stream,
                               ConnectCsrSpecArgs{a, exts[k]});
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
        HIP_TRY(hipStreamSynchronize(net->stream), SNN_ERR_WAIT);      // (the set just read is freed when it is next sized)
        cur ^= 1;
        nnz = total;
    }
    // ---- the commit: the set the last merge read, the row lengths and the scan's words go first ----
    ptr[cur ^ 1].reset(); pre[cur ^ 1].reset(); w[cur ^ 1].reset(); len_d.reset(); sums_d.reset();
    return commit_device_csr(net, ptr[cur], pre[cur], w[cur], n, nnz, nullptr);
}

// edit_weight(pre, post, Option<f32>) on a sparse handle, structure included (graph/mod.rs:42-72, 204-213): the sorted edit list
// merged into the stored rows on the device (snn_kernels_graph_merge_csr.hpp), committed as connect_csr commits.  Nothing of the
// handle is written before the commit -- or, when no pair inserts or removes, before the in-place store of snn_graph_csr_edit.
int graph_csr_edit_structure(snn_network *net, const uint32_t *pre, const uint32_t *post, const float *weights, const uint8_t *connected,
                             size_t n)
{
    TRY(graph_begin(net, true));
    if (n == 0) return SNN_OK;
    if (!pre || !post || !weights || !connected) return fail(SNN_ERR_BAD_ARG, "null pointer with n > 0");
    // every pair is checked before anything is written: a refused call leaves the graph as it was
    TRY(graph_pairs_accept(net, pre, post, weights, connected, n, GRAPH_NAN_SPARSE, nullptr));
    // "as if one after another": of a pair listed more than once the last occurrence decides, whatever the earlier ones asked for;
    // the list sorted by (post, pre) is the order the rows of the merge read it in (sorted always: the merge needs that order)
    hvec<uint64_t> order;
    const size_t kept = graph_pairs_last_wins(pre, post, n, GRAPH_KEY_POST_PRE, order);
    if (kept >= 0xFFFFFFFFull) return fail(SNN_ERR_DIM_MISMATCH, "more than 2^32-2 distinct pairs in one call");
    const uint32_t m = (uint32_t)kept, rows = net->n_loc;
    const size_t hop = std::min(kept, GRAPH_PAIRS_HOP);
    GraphCallLists l;                      // the whole sorted list on the device; flag: connected
    hvec<uint32_t> pre_h(hop), post_h(hop);
    hvec<float> value_h(hop);
    hvec<uint8_t> on_h(hop);
    HIP_TRY(hipSetDevice(net->device), SNN_ERR_GET_DEVICE);
    TRY(end_run(net));                     // a deferred update belongs to the weights the merge is about to read
    const bool timing = getenv("SNN_DEBUG_EDIT_TIMING") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    typedef std::chrono::steady_clock::time_point Instant;
    auto ms = [](Instant from, Instant to) { return std::chrono::duration<double, std::milli>(to - from).count(); };
    const auto t_begin = now();
    const uint32_t scan_edits = (m + 255u) / 256u, scan_rows = (rows + 255u) / 256u;
    dev_ptr<uint32_t> slot_d, ins_d, rem_d, len_d, new_pre_d, src_d;
    dev_ptr<float> new_w_d;
    dev_ptr<unsigned long long> sums_d;              // the words of device_scan, for the longer of its two inputs
    TRY(sized(&l.pre, kept * 4));
    TRY(sized(&l.post, kept * 4));
    TRY(sized(&l.value, kept * 4));
    TRY(sized(&l.flag, kept));
    TRY(sized(&slot_d, kept * 4));
    TRY(sized(&ins_d, (kept + 1) * 4));
    TRY(sized(&rem_d, (kept + 1) * 4));
    TRY(sized(&sums_d, ((size_t)std::max(scan_edits, scan_rows) + 1) * 8));
    TRY(ensure_copy_stage(net));
    // ---- the resolve pass: read only.  The sorted list goes up in hops; every pair finds its entry ----
    for (size_t k = 0; k < kept; k += hop) {
        const uint32_t h = (uint32_t)std::min(hop, kept - k);
        for (uint32_t j = 0; j < h; ++j) {
            const size_t src = (size_t)order[k + j];
            pre_h[j] = pre[src]; post_h[j] = post[src]; value_h[j] = weights[src]; on_h[j] = connected[src] ? 1 : 0;
        }
        TRY(l.upload(net, k, pre_h.data(), post_h.data(), value_h.data(), on_h.data(), h));
        if (net->csr_ptr) launch_csr_find(net, l.pre.get() + k, l.post.get() + k, h, slot_d.get() + k, nullptr, nullptr, nullptr, 0, nullptr);
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    }
    if (!net->csr_ptr)                     // no graph set yet: the empty one, no pair has an entry (GRAPH_CSR_NONE is all ones)
        HIP_TRY(hipMemsetAsync(slot_d, 0xFF, kept * 4, net->stream), SNN_ERR_BUFFER_WRITE);
    hipLaunchKernelGGL(k_graph_merge_flags, dim3(scan_edits), dim3(256), 0, net->stream, (const uint32_t *)slot_d, (const uint8_t *)l.flag, m,
                       ins_d.get(), rem_d.get());
    HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    // flags -> m + 1 offsets, in place
    uint64_t inserts = 0, removes = 0;
    TRY(device_scan(net, ins_d, ins_d, m, sums_d, &inserts));
    TRY(device_scan(net, rem_d, rem_d, m, sums_d, &removes));
    if (inserts == 0 && removes == 0) {
        // ---- nothing inserts, nothing removes: the write pass of snn_graph_csr_edit, in place ("stay absent" has no entry and is
        // skipped; no pair is listed twice) ----
        if (!net->csr_ptr) return SNN_OK;
        return graph_csr_store(net, slot_d, nullptr, l.value, m);
    }
    // ---- the structural path: lengths, offsets, the 2^32-2 check, then every entry placed on its own ----
    TRY(sized(&len_d, ((size_t)rows + 1) * 4));
    GraphMergeArgs a{};
    if (net->csr_ptr) { a.slice_ptr = net->csr_ptr; a.sell_pre = net->csr_pre; a.row_len = net->csr_row_len; a.sell_w = net->csr_w; }
    a.edit_pre = l.pre; a.edit_post = l.post; a.ins_before = ins_d; a.rem_before = rem_d; a.edit_w = l.value;
    a.n_edits = m; a.n_rows = rows; a.q0 = net->q0;
    a.new_len = len_d;
    hipLaunchKernelGGL(k_graph_merge_count, dim3(scan_rows), dim3(256), 0, net->stream, a);
    HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    uint64_t nnz = 0;
    TRY(device_scan(net, len_d, len_d, rows, sums_d, &nnz));       // lengths -> rows + 1 offsets, in place
    if (nnz >= 0xFFFFFFFFull)
        return fail(SNN_ERR_DIM_MISMATCH, "the graph would hold " + std::to_string(nnz) + " stored synapses, more than 2^32-2 per handle");
    if (nnz != net->nnz + inserts - removes) return fail(SNN_ERR_BAD_STATE, "the merged row lengths do not add up to stored + inserted - removed");
    TRY(sized(&new_pre_d, nnz * 4));
    TRY(sized(&new_w_d, nnz * 4));
    TRY(sized(&src_d, nnz * 4));
    a.new_ptr = len_d; a.new_pre = new_pre_d; a.new_w = new_w_d; a.new_src = src_d;
    hipLaunchKernelGGL(k_graph_merge_fill, dim3(std::min<uint32_t>((rows + 3u) / 4u, 16384u)), dim3(256), 0, net->stream, a);
    HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
    HIP_TRY(hipStreamSynchronize(net->stream), SNN_ERR_WAIT);
    const double ms_merge = ms(t_begin, now());
    // ---- the commit: everything but the new CSR and the source of every new edge goes first ----
    const auto t_download = now();
    l = GraphCallLists{};
    slot_d.reset(); ins_d.reset(); rem_d.reset(); sums_d.reset();
    CsrEdgePlanes old;
    Instant built[2];
    TRY(commit_device_csr(net, len_d, new_pre_d, new_w_d, rows, nnz, &old, built));
    const auto t_carry = now();
    // ---- per-edge state: the planes the handle carried, from the old entry of every kept edge to its new one (a handle with
    // modulation or connection kinds has zeroed planes again by now; planes set without either are allocated here) ----
    if (old.trace) TRY(ensure_traces(net));
    if (old.pending) TRY(ensure_pending(net));
    if (nnz && (old.trace || old.pending)) {
        hipLaunchKernelGGL(k_graph_merge_carry, dim3(((uint32_t)nnz + 255u) / 256u), dim3(256), 0, net->stream, (const uint32_t *)src_d,
                           (const uint32_t *)net->csr_edge_slot, (uint32_t)nnz, (const float *)old.trace, old.trace ? net->trace.get() : nullptr,
                           (const float *)old.pending, old.pending ? net->pending.get() : nullptr, (const float *)old.edge_counter,
                           old.edge_counter ? net->edge_counter.get() : nullptr);
        HIP_TRY(hipGetLastError(), SNN_ERR_QUEUE);
        HIP_TRY(hipStreamSynchronize(net->stream), SNN_ERR_WAIT);
    }
    if (timing)
        fprintf(stderr, "[snn] edit_structure: %u edits (%llu inserts, %llu removes), %llu edges: resolve+merge %.3f ms, download %.3f ms, "
                        "host builder %.3f ms, carry %.3f ms\n", m, (unsigned long long)inserts, (unsigned long long)removes,
                (unsigned long long)nnz, ms_merge, ms(t_download, built[0]), ms(built[0], built[1]), ms(t_carry, now()));
    return SNN_OK;
}

} // namespace

