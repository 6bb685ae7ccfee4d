// Connection rules on SPARSE handles (snn_connect_by_rules_csr): the graph is merged record by record on the device in plain
// CSR -- row_ptr[n_loc + 1] of 32-bit offsets, pre[nnz], w[nnz], rows sorted by presynaptic index -- and handed to the host
// builder of snn_set_graph_csr once, at the end.  Nothing of size N^2 exists: a row costs its old entries plus the candidates of
// the rule's window.  The pair formulas are connect_value of snn_kernels_connect.hpp, the one definition the dense kernel uses.
#pragma once
#include "snn_connect_window.hpp"
#include "snn_kernels_connect.hpp"

namespace snn {

struct ConnectCsrArgs {
    // what connect_value reads (extent, probability, seeds, w_lo, w_hi) and the geometry of the block, with the meaning the dense
    // kernel gives them: col0 / n_cols the LOCAL rows of this handle inside the postsynaptic lattice, post_i0 the lattice-local
    // index of the first of them (W and ld are unused)
    ConnectArgs c;
    uint32_t n_rows;                 // local rows of the handle
    uint32_t window;                 // connect_window_extent of the rule
    const uint32_t *old_ptr, *old_pre;
    const float *old_w;
    uint32_t *new_len;               // FILL == false: [n_rows]
    const uint32_t *new_ptr;         // FILL == true: [n_rows + 1], the scan of new_len
    uint32_t *new_pre;
    float *new_w;
};

// One wavefront per local row, grid-stride over rows; the same body counts (FILL == false: the row's new length) and fills
// (FILL == true: its entries from new_ptr[row] on), so that the two passes cannot disagree about a pair.  A row outside the
// record's postsynaptic block is copied.  A row inside it becomes: its old entries below pre_first, the rule's entries, its old
// entries from pre_first + pre_count on -- the lattice is contiguous in the presynaptic index and the old row is sorted, so the
// two cut points are counts (a ballot over the old row) and the result is sorted without a sort.  Candidates are visited in
// ascending lattice-local pre index, 64 per round, one per lane: all of them (ALL), the window of rows rb-e..rb+e and columns
// cb-e..cb+e clipped to the pre grid, row-major (the distance rules), the one cell at the post position (SAME_POSITION).  A
// lane's place among the round's survivors is the popcount of the ballot below it (as k_spike_compact ranks spikes): each round
// stores to consecutive words.
// grid (min(rows / 4 rounded up, 16384)), 256 threads
template <int RULE, int WEIGHT, bool THIN, bool SELF, bool FILL>
__global__ __launch_bounds__(256) void k_connect_csr(const ConnectCsrArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t waves = gridDim.x * 4u;
    const uint32_t pre_end = a.c.pre_first + a.c.pre_count;
    for (uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6); row < a.n_rows; row += waves) {
        const uint32_t o0 = a.old_ptr[row], o1 = a.old_ptr[row + 1];
        uint32_t out = FILL ? a.new_ptr[row] : 0u;                 // wave-uniform from here on
        if (row < a.c.col0 || row >= a.c.col0 + a.c.n_cols) {
            if (FILL)
                for (uint32_t k = o0 + lane; k < o1; k += 64u) { a.new_pre[out + (k - o0)] = a.old_pre[k]; a.new_w[out + (k - o0)] = a.old_w[k]; }
            else if (lane == 0) a.new_len[row] = o1 - o0;
            continue;
        }
        // the old row: [o0, o0 + n_low) lies below the block, [o0 + n_mid, o1) above it
        uint32_t n_low = 0, n_mid = 0;
        for (uint32_t k0 = o0; k0 < o1; k0 += 64u) {
            const uint32_t k = k0 + lane;
            const bool have = k < o1;
            const uint32_t p = have ? a.old_pre[k] : 0xFFFFFFFFu;
            const bool low = have && p < a.c.pre_first;
            n_low += (uint32_t)__popcll(__ballot(low));
            n_mid += (uint32_t)__popcll(__ballot(have && p < pre_end));
            if (FILL && low) { a.new_pre[out + (k - o0)] = p; a.new_w[out + (k - o0)] = a.old_w[k]; }
        }
        out += n_low;
        // the rule's entries
        const uint32_t j = a.c.post_i0 + (row - a.c.col0);
        const uint32_t rb = j / a.c.post_cols, cb = j - rb * a.c.post_cols;
        const uint32_t i_same = (cb < a.c.pre_cols && rb < a.c.pre_rows) ? rb * a.c.pre_cols + cb : 0xFFFFFFFFu;
        uint32_t n_cand, r0 = 0, c0 = 0, width = 1;
        if (RULE == CONNECT_CHEBYSHEV || RULE == CONNECT_EUCLIDEAN) {
            const ConnectSpan rs = connect_window_span(rb, a.window, a.c.pre_rows), cs = connect_window_span(cb, a.window, a.c.pre_cols);
            r0 = rs.first; c0 = cs.first; width = cs.count;
            n_cand = rs.count * cs.count;
        } else if (RULE == CONNECT_SAME_POSITION) {
            n_cand = i_same != 0xFFFFFFFFu ? 1u : 0u;
        } else {
            n_cand = a.c.pre_count;
        }
        for (uint32_t t0 = 0; t0 < n_cand; t0 += 64u) {
            const uint32_t t = t0 + lane;
            uint32_t i = t, ra = 0, ca = 0;
            if (RULE == CONNECT_CHEBYSHEV || RULE == CONNECT_EUCLIDEAN) {
                const uint32_t wr = t / width;
                ra = r0 + wr; ca = c0 + (t - wr * width);
                i = ra * a.c.pre_cols + ca;
            }
            if (RULE == CONNECT_SAME_POSITION) i = i_same;
            float v = quiet_nan();
            if (t < n_cand) v = connect_value<RULE, WEIGHT, THIN, SELF>(a.c, i, i_same, ra, ca, rb, cb, (uint64_t)i * a.c.post_count + j);
            const bool on = v == v;                                // NaN: absent
            const unsigned long long mask = __ballot(on);
            if (FILL && on) {
                const uint32_t at = out + (uint32_t)__popcll(mask & below);
                a.new_pre[at] = a.c.pre_first + i;
                a.new_w[at] = v;
            }
            out += (uint32_t)__popcll(mask);
        }
        // the old entries above the block
        if (FILL) {
            for (uint32_t k = o0 + n_mid + lane; k < o1; k += 64u) { a.new_pre[out + (k - o0 - n_mid)] = a.old_pre[k]; a.new_w[out + (k - o0 - n_mid)] = a.old_w[k]; }
        } else if (lane == 0) {
            a.new_len[row] = out + (o1 - o0 - n_mid);
        }
    }
}

// snn_connect_by_specs_csr: the merge of k_connect_csr, statement for statement, for the records it does not cover
// (connect_spec_is_plain): the table with every rule, WRAP with the two distance rules.  A kernel of its own so that the
// instantiations of k_connect_csr stay what they are.  WRAP: the window of a wrapped dimension is at most two ascending runs of
// cells (connect_window_spans), so candidate t is still (row ordinal, column ordinal) over sorted rows x sorted columns, ascending
// in the pre index.  A displacement record takes its candidates from its rule -- every presynaptic cell under CONNECT_ALL, the
// window under a radius -- and a NaN entry of the table drops the pair.  Grid and block as k_connect_csr.
struct ConnectCsrSpecArgs { ConnectCsrArgs c; ConnectSpecExt x; };
template <int RULE, int WEIGHT, bool THIN, bool SELF, bool WRAP, bool FILL>
__global__ __launch_bounds__(256) void k_connect_csr_spec(const ConnectCsrSpecArgs s)
{
    const ConnectCsrArgs &a = s.c;
    const ConnectSpecExt &x = s.x;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t waves = gridDim.x * 4u;
    const uint32_t pre_end = a.c.pre_first + a.c.pre_count;
    for (uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6); row < a.n_rows; row += waves) {
        const uint32_t o0 = a.old_ptr[row], o1 = a.old_ptr[row + 1];
        uint32_t out = FILL ? a.new_ptr[row] : 0u;                 // wave-uniform from here on
        if (row < a.c.col0 || row >= a.c.col0 + a.c.n_cols) {
            if (FILL)
                for (uint32_t k = o0 + lane; k < o1; k += 64u) { a.new_pre[out + (k - o0)] = a.old_pre[k]; a.new_w[out + (k - o0)] = a.old_w[k]; }
            else if (lane == 0) a.new_len[row] = o1 - o0;
            continue;
        }
        // the old row: [o0, o0 + n_low) lies below the block, [o0 + n_mid, o1) above it
        uint32_t n_low = 0, n_mid = 0;
        for (uint32_t k0 = o0; k0 < o1; k0 += 64u) {
            const uint32_t k = k0 + lane;
            const bool have = k < o1;
            const uint32_t p = have ? a.old_pre[k] : 0xFFFFFFFFu;
            const bool low = have && p < a.c.pre_first;
            n_low += (uint32_t)__popcll(__ballot(low));
            n_mid += (uint32_t)__popcll(__ballot(have && p < pre_end));
            if (FILL && low) { a.new_pre[out + (k - o0)] = p; a.new_w[out + (k - o0)] = a.old_w[k]; }
        }
        out += n_low;
        // the rule's entries
        const uint32_t j = a.c.post_i0 + (row - a.c.col0);
        const uint32_t rb = j / a.c.post_cols, cb = j - rb * a.c.post_cols;
        const uint32_t i_same = (cb < a.c.pre_cols && rb < a.c.pre_rows) ? rb * a.c.pre_cols + cb : 0xFFFFFFFFu;
        uint32_t n_cand, r0 = 0, c0 = 0, width = 1;
        ConnectSpans rs2{}, cs2{};
        if ((RULE == CONNECT_CHEBYSHEV || RULE == CONNECT_EUCLIDEAN) && WRAP) {
            rs2 = connect_window_spans(rb, a.window, a.c.pre_rows, x.period_r);
            cs2 = connect_window_spans(cb, a.window, a.c.pre_cols, x.period_c);
            width = cs2.a.count + cs2.b.count;
            n_cand = (rs2.a.count + rs2.b.count) * width;
        } else if (RULE == CONNECT_CHEBYSHEV || RULE == CONNECT_EUCLIDEAN) {
            const ConnectSpan rs = connect_window_span(rb, a.window, a.c.pre_rows), cs = connect_window_span(cb, a.window, a.c.pre_cols);
            r0 = rs.first; c0 = cs.first; width = cs.count;
            n_cand = rs.count * cs.count;
        } else if (RULE == CONNECT_SAME_POSITION) {
            n_cand = i_same != 0xFFFFFFFFu ? 1u : 0u;
        } else {
            n_cand = a.c.pre_count;
        }
        for (uint32_t t0 = 0; t0 < n_cand; t0 += 64u) {
            const uint32_t t = t0 + lane;
            uint32_t i = t, ra = 0, ca = 0;
            if (RULE == CONNECT_CHEBYSHEV || RULE == CONNECT_EUCLIDEAN) {
                const uint32_t wr = t / width;
                if (WRAP) {
                    if (t < n_cand) { ra = connect_spans_cell(rs2, wr); ca = connect_spans_cell(cs2, t - wr * width); }
                } else {
                    ra = r0 + wr; ca = c0 + (t - wr * width);
                }
                i = ra * a.c.pre_cols + ca;
            }
            if (RULE == CONNECT_SAME_POSITION) i = i_same;
            if (WEIGHT == CONNECT_DISPLACEMENT && (RULE == CONNECT_ALL || RULE == CONNECT_SAME_POSITION) && t < n_cand) {
                ra = i / a.c.pre_cols; ca = i - ra * a.c.pre_cols;          // (the table is indexed by position under every rule)
            }
            float v = quiet_nan();
            if (t < n_cand)
                v = connect_spec_value<RULE, WEIGHT, THIN, SELF, WRAP>(a.c, x, i, i_same, ra, ca, rb, cb, (uint64_t)i * a.c.post_count + j);
            const bool on = v == v;                                // NaN: absent
            const unsigned long long mask = __ballot(on);
            if (FILL && on) {
                const uint32_t at = out + (uint32_t)__popcll(mask & below);
                a.new_pre[at] = a.c.pre_first + i;
                a.new_w[at] = v;
            }
            out += (uint32_t)__popcll(mask);
        }
        // the old entries above the block
        if (FILL) {
            for (uint32_t k = o0 + n_mid + lane; k < o1; k += 64u) { a.new_pre[out + (k - o0 - n_mid)] = a.old_pre[k]; a.new_w[out + (k - o0 - n_mid)] = a.old_w[k]; }
        } else if (lane == 0) {
            a.new_len[row] = out + (o1 - o0 - n_mid);
        }
    }
}

// The handle's SELL-64 graph as plain CSR: entry k of row r sits at slice_ptr[r / 64] + 64 k + r % 64.  One thread per row, a
// wavefront = the 64 columns of one slice: its loads of entry k are one contiguous 256 bytes, as the step kernels read them.
// grid (rows / 256 rounded up), 256 threads
__global__ __launch_bounds__(256) void k_connect_csr_export(const uint32_t *slice_ptr, const uint32_t *sell_pre, const float *sell_w,
                                                            const uint32_t *row_len, const uint32_t *row_ptr, uint32_t n_rows,
                                                            uint32_t *pre, float *w)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t base = slice_ptr[r >> 6] + (r & 63u), len = row_len[r], at = row_ptr[r];
    for (uint32_t k = 0; k < len; ++k) {
        pre[at + k] = sell_pre[base + k * 64u];
        w[at + k] = sell_w[base + k * 64u];
    }
}

// ---- exclusive sum of the row lengths, three launches: 32-bit offsets per row (the host refuses a total they cannot hold before
// anything reads them), block sums and the total in 64 bits ----
__device__ __forceinline__ unsigned long long scan256_exclusive(unsigned long long v, unsigned long long *sh, unsigned long long *total)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256u; d <<= 1) {
        const unsigned long long add = t >= d ? sh[t - d] : 0ull;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const unsigned long long inclusive = sh[t];
    *total = sh[255];
    __syncthreads();
    return inclusive - v;
}

// (1) offsets inside each block of 256 rows, and the block's sum.  grid (rows / 256 rounded up), 256 threads
__global__ __launch_bounds__(256) void k_connect_scan_local(const uint32_t *len, uint32_t n, uint32_t *ptr, unsigned long long *block_sum)
{
    __shared__ unsigned long long sh[256];
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    unsigned long long total;
    const unsigned long long ex = scan256_exclusive(r < n ? len[r] : 0u, sh, &total);
    if (r < n) ptr[r] = (uint32_t)ex;
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// (2) the block sums to block offsets, in place, and the total.  One block of 256 threads: a contiguous run of blocks per thread
__global__ __launch_bounds__(256) void k_connect_scan_sums(unsigned long long *block_sum, uint32_t n_blocks, unsigned long long *total_out)
{
    __shared__ unsigned long long sh[256];
    const uint32_t per = (n_blocks + 255u) / 256u;
    const uint32_t b0 = min(threadIdx.x * per, n_blocks), b1 = min(b0 + per, n_blocks);
    unsigned long long mine = 0;
    for (uint32_t b = b0; b < b1; ++b) mine += block_sum[b];
    unsigned long long total;
    unsigned long long run = scan256_exclusive(mine, sh, &total);
    for (uint32_t b = b0; b < b1; ++b) { const unsigned long long s = block_sum[b]; block_sum[b] = run; run += s; }
    if (threadIdx.x == 0) *total_out = total;
}

// (3) block offsets onto the rows; ptr[n] = the total.  grid (rows / 256 rounded up), 256 threads
__global__ __launch_bounds__(256) void k_connect_scan_add(uint32_t *ptr, uint32_t n, const unsigned long long *block_off, const unsigned long long *total)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r < n) ptr[r] += (uint32_t)block_off[blockIdx.x];
    if (r == 0) ptr[n] = (uint32_t)*total;
}

typedef void (*connect_csr_kernel_t)(const ConnectCsrArgs);

template <int RULE, int WEIGHT, bool FILL>
inline connect_csr_kernel_t connect_csr_kernel_flags(bool thin, bool self)
{
    if (thin) return self ? k_connect_csr<RULE, WEIGHT, true, true, FILL> : k_connect_csr<RULE, WEIGHT, true, false, FILL>;
    return self ? k_connect_csr<RULE, WEIGHT, false, true, FILL> : k_connect_csr<RULE, WEIGHT, false, false, FILL>;
}
template <int RULE, bool FILL>
inline connect_csr_kernel_t connect_csr_kernel_weight(int weight, bool thin, bool self)
{
    return weight == CONNECT_UNIFORM ? connect_csr_kernel_flags<RULE, CONNECT_UNIFORM, FILL>(thin, self)
                                     : connect_csr_kernel_flags<RULE, CONNECT_CONSTANT, FILL>(thin, self);
}
// the instantiation for a record: which template arguments a launch takes
template <bool FILL>
inline connect_csr_kernel_t connect_csr_kernel(int rule, int weight, bool thin, bool self)
{
    switch (rule) {
    case CONNECT_CHEBYSHEV: return connect_csr_kernel_weight<CONNECT_CHEBYSHEV, FILL>(weight, thin, self);
    case CONNECT_EUCLIDEAN: return connect_csr_kernel_weight<CONNECT_EUCLIDEAN, FILL>(weight, thin, self);
    case CONNECT_SAME_POSITION: return connect_csr_kernel_weight<CONNECT_SAME_POSITION, FILL>(weight, thin, self);
    default: return connect_csr_kernel_weight<CONNECT_ALL, FILL>(weight, thin, self);
    }
}


typedef void (*connect_csr_spec_kernel_t)(const ConnectCsrSpecArgs);

template <int RULE, int WEIGHT, bool WRAP, bool FILL>
inline connect_csr_spec_kernel_t connect_csr_spec_kernel_flags(bool thin, bool self)
{
    if (thin) return self ? k_connect_csr_spec<RULE, WEIGHT, true, true, WRAP, FILL> : k_connect_csr_spec<RULE, WEIGHT, true, false, WRAP, FILL>;
    return self ? k_connect_csr_spec<RULE, WEIGHT, false, true, WRAP, FILL> : k_connect_csr_spec<RULE, WEIGHT, false, false, WRAP, FILL>;
}
template <int RULE, bool FILL>
inline connect_csr_spec_kernel_t connect_csr_spec_kernel_table(bool wrap, bool thin, bool self)
{
    return wrap ? connect_csr_spec_kernel_flags<RULE, CONNECT_DISPLACEMENT, true, FILL>(thin, self)
                : connect_csr_spec_kernel_flags<RULE, CONNECT_DISPLACEMENT, false, FILL>(thin, self);
}
template <int RULE, bool FILL>
inline connect_csr_spec_kernel_t connect_csr_spec_kernel_ring(int weight, bool thin, bool self)
{
    return weight == CONNECT_UNIFORM ? connect_csr_spec_kernel_flags<RULE, CONNECT_UNIFORM, true, FILL>(thin, self)
                                     : connect_csr_spec_kernel_flags<RULE, CONNECT_CONSTANT, true, FILL>(thin, self);
}
// the instantiation for a record that is not plain (connect_spec_is_plain)
template <bool FILL>
inline connect_csr_spec_kernel_t connect_csr_spec_kernel(int rule, int weight, bool wrap, bool thin, bool self)
{
    if (weight == CONNECT_DISPLACEMENT)
        switch (rule) {
        case CONNECT_CHEBYSHEV: return connect_csr_spec_kernel_table<CONNECT_CHEBYSHEV, FILL>(wrap, thin, self);
        case CONNECT_EUCLIDEAN: return connect_csr_spec_kernel_table<CONNECT_EUCLIDEAN, FILL>(wrap, thin, self);
        case CONNECT_SAME_POSITION: return connect_csr_spec_kernel_table<CONNECT_SAME_POSITION, FILL>(wrap, thin, self);
        default: return connect_csr_spec_kernel_table<CONNECT_ALL, FILL>(wrap, thin, self);
        }
    return rule == CONNECT_CHEBYSHEV ? connect_csr_spec_kernel_ring<CONNECT_CHEBYSHEV, FILL>(weight, thin, self)
                                     : connect_csr_spec_kernel_ring<CONNECT_EUCLIDEAN, FILL>(weight, thin, self);
}

} // namespace snn
