// Connection rules evaluated on the device, straight into the quad-row matrix (snn_connect_by_rule): the reference's
// Lattice::connect / LatticeNetwork::connect (backend/src/neuron/mod.rs:1134-1157, 1845-1935) for the handful of predicates its
// users write -- everything, a distance bound, position to position, a coin flip -- without a matrix of size N^2 on the host.
#pragma once
#include "snn_kernels_misc.hpp"

namespace snn {

enum ConnectRule { CONNECT_ALL = 0, CONNECT_CHEBYSHEV = 1, CONNECT_EUCLIDEAN = 2, CONNECT_SAME_POSITION = 3, CONNECT_RULES = 4 };
enum ConnectWeight { CONNECT_CONSTANT = 0, CONNECT_UNIFORM = 1, CONNECT_DISPLACEMENT = 2 };
// how many of them a call takes: snn_connect_by_rule / snn_connect_by_rules_csr the first two, the spec calls the table too
enum ConnectWeightCount { CONNECT_RULE_WEIGHTS = 2, CONNECT_SPEC_WEIGHTS = 3 };

// One block of W: presynaptic rows [pre_first, pre_first + pre_count) -- lattice-local index i = row - pre_first -- and the
// local columns [col0, col0 + n_cols) of this handle, whose lattice-local postsynaptic indices are post_i0 ...
struct ConnectArgs {
    float *W;
    uint32_t ld;
    uint32_t col0, n_cols, post_i0;
    uint32_t post_cols, post_count;         // grid width and cell count of the postsynaptic lattice
    uint32_t pre_first, pre_count, pre_rows, pre_cols;
    uint32_t extent;
    float probability;
    uint64_t edge_seed, weight_seed;
    float w_lo, w_hi;
};

// What snn_connect_by_spec adds to a block: wrap-around and the displacement table.  period_r / period_c: the ring a wrapped
// dimension closes on (max of the two grids' rows / columns), 0 where that dimension does not wrap.  table[u * table_cols + v]
// with u = rb - ra mod period_r where rows wrap, rb - ra + u_bias (u_bias = pre_rows - 1) where they do not; v likewise.
struct ConnectSpecExt {
    uint32_t period_r, period_c;
    const float *table;
    uint32_t table_cols, u_bias, v_bias;
};

typedef float connect_v4f __attribute__((ext_vector_type(4)));

// Some(weight) or None (the quiet NaN) of the pair (pre index i at position (ra, ca), post position (rb, cb));
// idx = i * post_count + i_post.  i_same: the pre index whose position IS the post position (0xFFFFFFFF: the pre grid has no such
// cell) -- `a == b` and `a != b` are one comparison of indices, and only the distance rules look at positions at all.
// WRAP: distances on the rings of x (a dimension with period 0 stays a line).  WEIGHT == CONNECT_DISPLACEMENT: the weight is
// the table's entry for the displacement b - a, read where the pair is connected only -- one word per pair from an array that
// fits L2; a wavefront's lanes are consecutive post columns, so consecutive words.  A NaN entry is None whatever the rule says.
// Without WRAP and without the table nothing of x is read.
template <int RULE, int WEIGHT, bool THIN, bool SELF, bool WRAP>
__device__ __forceinline__ float connect_spec_value(const ConnectArgs &a, const ConnectSpecExt &x, uint32_t i, uint32_t i_same, uint32_t ra,
                                                    uint32_t ca, uint32_t rb, uint32_t cb, uint64_t idx)
{
    bool on = true;
    if (RULE == CONNECT_CHEBYSHEV || RULE == CONNECT_EUCLIDEAN) {
        uint32_t dr = ra > rb ? ra - rb : rb - ra, dc = ca > cb ? ca - cb : cb - ca;
        if (WRAP) {                                                // (dr < period: both positions lie on the ring)
            if (x.period_r) dr = min(dr, x.period_r - dr);
            if (x.period_c) dc = min(dc, x.period_c - dc);
        }
        if (RULE == CONNECT_CHEBYSHEV) on = max(dr, dc) <= a.extent;
        else on = (uint64_t)dr * dr + (uint64_t)dc * dc <= (uint64_t)a.extent;
    }
    if (RULE == CONNECT_SAME_POSITION) on = i == i_same;
    if (!SELF) on = on && i != i_same;
    if (THIN) on = on && (float)(hash32(a.edge_seed, idx) >> 8) * (1.0f / 16777216.0f) < a.probability;
    if (WEIGHT == CONNECT_DISPLACEMENT) {
        uint32_t u = rb + x.u_bias - ra, v = cb + x.v_bias - ca;
        if (WRAP) {
            if (x.period_r) u = rb >= ra ? rb - ra : rb + x.period_r - ra;
            if (x.period_c) v = cb >= ca ? cb - ca : cb + x.period_c - ca;
        }
        return on ? x.table[(size_t)u * x.table_cols + v] : quiet_nan();
    }
    const float w = WEIGHT == CONNECT_UNIFORM ? uniform_from_hash(a.weight_seed, idx, a.w_lo, a.w_hi) : a.w_lo;
    return on ? w : quiet_nan();
}
template <int RULE, int WEIGHT, bool THIN, bool SELF>
__device__ __forceinline__ float connect_value(const ConnectArgs &a, uint32_t i, uint32_t i_same, uint32_t ra, uint32_t ca, uint32_t rb,
                                               uint32_t cb, uint64_t idx)
{
    return connect_spec_value<RULE, WEIGHT, THIN, SELF, false>(a, ConnectSpecExt{}, i, i_same, ra, ca, rb, cb, idx);
}

// One thread = one unit of W (4 consecutive presynaptic rows of one local column), as in k_graph_synthetic: a wavefront's
// 16-byte stores are 1 KiB contiguous (the grid starts at the 64-column boundary at or below col0), non-temporal -- the stream
// is written once and is as large as W.  The row groups of a column are a grid-stride loop in y; the post position is
// computed once per thread, the pre position advances by additions.  A group that straddles the block's first or last row is
// read, has its in-block rows replaced and is stored back; interior groups are stores only.  Nothing outside the block is touched.
// RULE / WEIGHT / THIN (the Bernoulli draw) / SELF (pairs at equal positions allowed): the all-to-all and position-to-position
// forms carry no geometry (the pre position is dead code there), a constant weight without the draw no hash.
// grid (columns / 256 rounded up, min(row groups, 4096)), 256 threads
template <int RULE, int WEIGHT, bool THIN, bool SELF>
__global__ __launch_bounds__(256) void k_connect_rule(const ConnectArgs a)
{
    const uint32_t q = (a.col0 & ~63u) + blockIdx.x * 256u + threadIdx.x;
    if (q < a.col0 || q >= a.col0 + a.n_cols) return;
    const uint32_t j = a.post_i0 + (q - a.col0);
    const uint32_t rb = j / a.post_cols, cb = j - rb * a.post_cols;
    const uint32_t i_same = (cb < a.pre_cols && rb < a.pre_rows) ? rb * a.pre_cols + cb : 0xFFFFFFFFu;
    const uint32_t g_first = a.pre_first >> 2, g_last = (a.pre_first + a.pre_count - 1u) >> 2;
    const uint32_t stride = gridDim.y * 4u;                        // rows between two groups of this thread
    const uint32_t step_r = stride / a.pre_cols, step_c = stride - step_r * a.pre_cols;
    uint32_t g = g_first + blockIdx.y;
    long long i = (long long)g * 4 - (long long)a.pre_first;       // lattice-local index of the group's first row: -3 .. pre_count - 1
    // (r, c): position of row i -- of the thread's NEXT group while i < 0 (the group that straddles the block's first row)
    const uint32_t i_pos = (uint32_t)(i < 0 ? i + stride : i);
    uint32_t r = i_pos / a.pre_cols, c = i_pos - r * a.pre_cols;
    uint64_t idx = (uint64_t)i * a.post_count + j;                 // (wraps while i < 0; used from i >= 0 on)
    const uint64_t idx_step = (uint64_t)stride * a.post_count;
    connect_v4f *unit = reinterpret_cast<connect_v4f *>(a.W) + (size_t)g * a.ld + q;
    const size_t unit_step = (size_t)gridDim.y * a.ld;
    for (; g <= g_last; g += gridDim.y, i += stride, idx += idx_step, unit += unit_step) {
        connect_v4f out;
        if (i >= 0 && i + 3 < (long long)a.pre_count) {
            uint32_t rr = r, cc = c;
            uint64_t e = idx;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                out[k] = connect_value<RULE, WEIGHT, THIN, SELF>(a, (uint32_t)i + k, i_same, rr, cc, rb, cb, e);
                e += a.post_count;
                if (++cc == a.pre_cols) { cc = 0; ++rr; }
            }
        } else {
            out = *unit;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long ik = i + k;
                if (ik >= 0 && ik < (long long)a.pre_count) {
                    const uint32_t ra = (uint32_t)ik / a.pre_cols, ca = (uint32_t)ik - ra * a.pre_cols;
                    out[k] = connect_value<RULE, WEIGHT, THIN, SELF>(a, (uint32_t)ik, i_same, ra, ca, rb, cb, (uint64_t)ik * a.post_count + j);
                }
            }
        }
        __builtin_nontemporal_store(out, unit);
        if (i >= 0) {
            c += step_c; r += step_r;
            if (c >= a.pre_cols) { c -= a.pre_cols; ++r; }
        }
    }
}

// snn_connect_by_spec: the walk of k_connect_rule, statement for statement, with wrap-around distances and / or weights from the
// displacement table (connect_spec_value).  A kernel of its own so that the instantiations of k_connect_rule stay what they
// are; instantiated for what those do not cover: the table with every rule, WRAP with the two distance rules -- a wrap-free
// instantiation computes no ring distance, a table-free one loads nothing.  Grid and block as k_connect_rule.
struct ConnectSpecArgs { ConnectArgs c; ConnectSpecExt x; };
template <int RULE, int WEIGHT, bool THIN, bool SELF, bool WRAP>
__global__ __launch_bounds__(256) void k_connect_spec(const ConnectSpecArgs s)
{
    const ConnectArgs &a = s.c;
    const uint32_t q = (a.col0 & ~63u) + blockIdx.x * 256u + threadIdx.x;
    if (q < a.col0 || q >= a.col0 + a.n_cols) return;
    const uint32_t j = a.post_i0 + (q - a.col0);
    const uint32_t rb = j / a.post_cols, cb = j - rb * a.post_cols;
    const uint32_t i_same = (cb < a.pre_cols && rb < a.pre_rows) ? rb * a.pre_cols + cb : 0xFFFFFFFFu;
    const uint32_t g_first = a.pre_first >> 2, g_last = (a.pre_first + a.pre_count - 1u) >> 2;
    const uint32_t stride = gridDim.y * 4u;                        // rows between two groups of this thread
    const uint32_t step_r = stride / a.pre_cols, step_c = stride - step_r * a.pre_cols;
    uint32_t g = g_first + blockIdx.y;
    long long i = (long long)g * 4 - (long long)a.pre_first;       // lattice-local index of the group's first row: -3 .. pre_count - 1
    // (r, c): position of row i -- of the thread's NEXT group while i < 0 (the group that straddles the block's first row)
    const uint32_t i_pos = (uint32_t)(i < 0 ? i + stride : i);
    uint32_t r = i_pos / a.pre_cols, c = i_pos - r * a.pre_cols;
    uint64_t idx = (uint64_t)i * a.post_count + j;                 // (wraps while i < 0; used from i >= 0 on)
    const uint64_t idx_step = (uint64_t)stride * a.post_count;
    connect_v4f *unit = reinterpret_cast<connect_v4f *>(a.W) + (size_t)g * a.ld + q;
    const size_t unit_step = (size_t)gridDim.y * a.ld;
    for (; g <= g_last; g += gridDim.y, i += stride, idx += idx_step, unit += unit_step) {
        connect_v4f out;
        if (i >= 0 && i + 3 < (long long)a.pre_count) {
            uint32_t rr = r, cc = c;
            uint64_t e = idx;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                out[k] = connect_spec_value<RULE, WEIGHT, THIN, SELF, WRAP>(a, s.x, (uint32_t)i + k, i_same, rr, cc, rb, cb, e);
                e += a.post_count;
                if (++cc == a.pre_cols) { cc = 0; ++rr; }
            }
        } else {
            out = *unit;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long ik = i + k;
                if (ik >= 0 && ik < (long long)a.pre_count) {
                    const uint32_t ra = (uint32_t)ik / a.pre_cols, ca = (uint32_t)ik - ra * a.pre_cols;
                    out[k] = connect_spec_value<RULE, WEIGHT, THIN, SELF, WRAP>(a, s.x, (uint32_t)ik, i_same, ra, ca, rb, cb, (uint64_t)ik * a.post_count + j);
                }
            }
        }
        __builtin_nontemporal_store(out, unit);
        if (i >= 0) {
            c += step_c; r += step_r;
            if (c >= a.pre_cols) { c -= a.pre_cols; ++r; }
        }
    }
}

// zeroes the block's entries of a matrix in the layout of W (traces, dw and counters of replaced edges start afresh): the shape of
// k_connect_rule -- one thread per 16-byte unit, interior groups one dwordx4 store, the groups that straddle the block's first or
// last row read, patched and stored back.  grid (columns from the 64-column boundary / 256 rounded up, min(row groups, 4096)), 256 threads
__global__ __launch_bounds__(256) void k_connect_clear(float *M, uint32_t ld, uint32_t col0, uint32_t n_cols, uint32_t pre_first, uint32_t pre_count)
{
    const uint32_t q = (col0 & ~63u) + blockIdx.x * 256u + threadIdx.x;
    if (q < col0 || q >= col0 + n_cols) return;
    const uint32_t g_last = (pre_first + pre_count - 1u) >> 2;
    for (uint32_t g = (pre_first >> 2) + blockIdx.y; g <= g_last; g += gridDim.y) {
        connect_v4f *unit = reinterpret_cast<connect_v4f *>(M) + (size_t)g * ld + q;
        const long long i = (long long)g * 4 - (long long)pre_first;
        connect_v4f out = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i < 0 || i + 3 >= (long long)pre_count) {
            out = *unit;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k >= 0 && i + k < (long long)pre_count) out[k] = 0.0f;
        }
        *unit = out;
    }
}

typedef void (*connect_kernel_t)(const ConnectArgs);

template <int RULE, int WEIGHT>
inline connect_kernel_t connect_kernel_flags(bool thin, bool self)
{
    if (thin) return self ? k_connect_rule<RULE, WEIGHT, true, true> : k_connect_rule<RULE, WEIGHT, true, false>;
    return self ? k_connect_rule<RULE, WEIGHT, false, true> : k_connect_rule<RULE, WEIGHT, false, false>;
}
template <int RULE>
inline connect_kernel_t connect_kernel_weight(int weight, bool thin, bool self)
{
    return weight == CONNECT_UNIFORM ? connect_kernel_flags<RULE, CONNECT_UNIFORM>(thin, self) : connect_kernel_flags<RULE, CONNECT_CONSTANT>(thin, self);
}
// the instantiation for a rule: which template arguments a launch takes
inline connect_kernel_t connect_kernel(int rule, int weight, bool thin, bool self)
{
    switch (rule) {
    case CONNECT_CHEBYSHEV: return connect_kernel_weight<CONNECT_CHEBYSHEV>(weight, thin, self);
    case CONNECT_EUCLIDEAN: return connect_kernel_weight<CONNECT_EUCLIDEAN>(weight, thin, self);
    case CONNECT_SAME_POSITION: return connect_kernel_weight<CONNECT_SAME_POSITION>(weight, thin, self);
    default: return connect_kernel_weight<CONNECT_ALL>(weight, thin, self);
    }
}


typedef void (*connect_spec_kernel_t)(const ConnectSpecArgs);

template <int RULE, int WEIGHT, bool WRAP>
inline connect_spec_kernel_t connect_spec_kernel_flags(bool thin, bool self)
{
    if (thin) return self ? k_connect_spec<RULE, WEIGHT, true, true, WRAP> : k_connect_spec<RULE, WEIGHT, true, false, WRAP>;
    return self ? k_connect_spec<RULE, WEIGHT, false, true, WRAP> : k_connect_spec<RULE, WEIGHT, false, false, WRAP>;
}
template <int RULE>
inline connect_spec_kernel_t connect_spec_kernel_table(bool wrap, bool thin, bool self)
{
    return wrap ? connect_spec_kernel_flags<RULE, CONNECT_DISPLACEMENT, true>(thin, self) : connect_spec_kernel_flags<RULE, CONNECT_DISPLACEMENT, false>(thin, self);
}
template <int RULE>
inline connect_spec_kernel_t connect_spec_kernel_ring(int weight, bool thin, bool self)
{
    return weight == CONNECT_UNIFORM ? connect_spec_kernel_flags<RULE, CONNECT_UNIFORM, true>(thin, self) : connect_spec_kernel_flags<RULE, CONNECT_CONSTANT, true>(thin, self);
}
// does a spec need k_connect_spec at all: the table, or a distance on a ring (all-to-all and position-to-position have no distance)
inline bool connect_spec_is_plain(int rule, int weight, bool wrap)
{
    return weight != CONNECT_DISPLACEMENT && !(wrap && (rule == CONNECT_CHEBYSHEV || rule == CONNECT_EUCLIDEAN));
}
// the instantiation for a spec that is not plain
inline connect_spec_kernel_t connect_spec_kernel(int rule, int weight, bool wrap, bool thin, bool self)
{
    if (weight == CONNECT_DISPLACEMENT)
        switch (rule) {
        case CONNECT_CHEBYSHEV: return connect_spec_kernel_table<CONNECT_CHEBYSHEV>(wrap, thin, self);
        case CONNECT_EUCLIDEAN: return connect_spec_kernel_table<CONNECT_EUCLIDEAN>(wrap, thin, self);
        case CONNECT_SAME_POSITION: return connect_spec_kernel_table<CONNECT_SAME_POSITION>(wrap, thin, self);
        default: return connect_spec_kernel_table<CONNECT_ALL>(wrap, thin, self);
        }
    return rule == CONNECT_CHEBYSHEV ? connect_spec_kernel_ring<CONNECT_CHEBYSHEV>(weight, thin, self)
                                     : connect_spec_kernel_ring<CONNECT_EUCLIDEAN>(weight, thin, self);
}

} // namespace snn
