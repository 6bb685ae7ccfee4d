// Connect by rule with FACTORED weights (snn_connect_by_factors / snn_connect_by_factors_csr): the weight of a pair is
// w(i, j) = scale * sum_p U[p][i] * V[p][j] -- the auto-associative (Hopfield) matrix of the reference's experiments
// (interface_gpu/experiments/pipeline_setup.py:44-64: U = pattern - b, V = pattern - a) and, with one factor, a table indexed by
// the post or the pre position alone -- from O(P N) numbers on the device where the graph has O(N^2).  The per-pair arithmetic is
// connect_factors_weight below, in binary64 and in the order numpy adds the patterns; which pairs exist at all is
// connect_spec_value of snn_kernels_connect.hpp (the one definition of rule, self edges, draw and wrap), asked for a constant 0.
#pragma once
#include "snn_kernels_connect_csr.hpp"

namespace snn {

// SNN_WEIGHT_FACTORS, the weight rule after ConnectWeight's three (snn_kernels_connect.hpp, whose instantiation sets are pinned and
// which therefore stays as it is), and how many weight rules the two factors calls take (after ConnectWeightCount's two counts)
enum ConnectFactorsWeight { CONNECT_FACTORS = 3 };
enum ConnectFactorsWeightCount { CONNECT_FACTOR_WEIGHTS = 4 };

constexpr uint32_t FACTOR_CHUNK = 32;               // factors staged at a time (dense): V as [FACTOR_CHUNK][256 columns] is 64 KiB
constexpr uint32_t FACTOR_TILE_ROWS = 16;           // presynaptic rows per tile: four 16-byte units per thread, 16 sums in registers
constexpr uint32_t FACTOR_CSR_CHUNK = 128;          // factors of one post row staged at a time (sparse): 1 KiB per wavefront

// U: [n_factors][pre_count], V: [n_factors][post_count] (the FULL postsynaptic lattice, also on a shard), lattice-local indices
struct ConnectFactorsExt {
    const double *U, *V;
    uint32_t n_factors;
    int drop_zero;
    double scale;
};
struct ConnectFactorsArgs { ConnectArgs c; ConnectSpecExt x; ConnectFactorsExt f; };          // (c.w_lo is 0: see connect_factors_on)
struct ConnectCsrFactorsArgs { ConnectCsrArgs c; ConnectSpecExt x; ConnectFactorsExt f; };

// one step of the sum: the product is rounded, then the sum -- never a fused multiply-add, whatever the translation unit's setting
__device__ __forceinline__ double connect_factors_step(double s, double u, double v)
{
#pragma clang fp contract(off)
    const double product = u * v;
    return s + product;
}

// rule, self edges, draw and ring distances of the pair: connect_spec_value with a constant weight (0 or NaN).  WRAP is on: a
// dimension whose period is 0 stays a line.
template <int RULE, bool THIN, bool SELF>
__device__ __forceinline__ bool connect_factors_on(const ConnectArgs &a, const ConnectSpecExt &x, uint32_t i, uint32_t i_same, uint32_t ra,
                                                   uint32_t ca, uint32_t rb, uint32_t cb, uint64_t idx)
{
    const float v = connect_spec_value<RULE, CONNECT_CONSTANT, THIN, SELF, true>(a, x, i, i_same, ra, ca, rb, cb, idx);
    return v == v;
}

// Some(weight) or None (the quiet NaN) from the finished sum: w64 = s * scale, dropped where drop_zero is set and w64 == 0
__device__ __forceinline__ float connect_factors_weight(const ConnectFactorsExt &f, bool on, double sum)
{
    const double w64 = sum * f.scale;
    if (f.drop_zero && w64 == 0.0) on = false;
    return on ? (float)w64 : quiet_nan();
}

// The store shape of k_connect_rule -- one thread per 16-byte unit (4 presynaptic rows of one local column), a wavefront's stores
// 1 KiB contiguous and non-temporal, the units that straddle the block's first or last row read, patched and stored back, nothing
// outside the block touched -- around an inner loop of P binary64 multiplies and adds per element.  A workgroup owns 256 columns
// and walks tiles of FACTOR_TILE_ROWS rows (grid-stride in y).  The factors come from LDS: V[p0 .. p0 + chunk) of the workgroup's
// columns as v_sh[p][column] (one ds_read_b64 per lane and factor, consecutive lanes consecutive banks), the tile's U rows as
// u_sh[p][row], which every lane reads at the same address (a broadcast).  With P <= FACTOR_CHUNK the V tile is staged ONCE per
// workgroup and serves every row tile it walks; beyond, the chunks of a tile are staged in turn and the 16 partial sums stay in
// registers across them -- per element the additions run p ascending either way.
// grid (columns from the 64-column boundary / 256 rounded up, row tiles capped by the host), 256 threads; 68 KiB of LDS: two
// workgroups per CU
template <int RULE, bool THIN, bool SELF>
__global__ __launch_bounds__(256) void k_connect_factors(const ConnectFactorsArgs s)
{
    __shared__ double v_sh[FACTOR_CHUNK][256];
    __shared__ double u_sh[FACTOR_CHUNK][FACTOR_TILE_ROWS];
    const ConnectArgs &a = s.c;
    const ConnectFactorsExt &f = s.f;
    const uint32_t q = (a.col0 & ~63u) + blockIdx.x * 256u + threadIdx.x;
    const bool mine = q >= a.col0 && q < a.col0 + a.n_cols;       // (the others stage and wait with the workgroup, and store nothing)
    const uint32_t j = mine ? a.post_i0 + (q - a.col0) : 0u;
    const uint32_t rb = j / a.post_cols, cb = j - rb * a.post_cols;
    const uint32_t i_same = (cb < a.pre_cols && rb < a.pre_rows) ? rb * a.pre_cols + cb : 0xFFFFFFFFu;
    const uint32_t g_first = a.pre_first >> 2, g_last = (a.pre_first + a.pre_count - 1u) >> 2;
    const uint32_t n_tiles = (g_last - g_first) / 4u + 1u;
    const uint32_t n_chunks = (f.n_factors + FACTOR_CHUNK - 1u) / FACTOR_CHUNK;
    for (uint32_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const uint32_t g0 = g_first + tile * 4u;
        const long long i0 = (long long)g0 * 4 - (long long)a.pre_first;      // lattice-local index of the tile's first row: -3 ..
        double sum[FACTOR_TILE_ROWS];
#pragma unroll
        for (uint32_t k = 0; k < FACTOR_TILE_ROWS; ++k) sum[k] = 0.0;
        for (uint32_t chunk = 0; chunk < n_chunks; ++chunk) {
            const uint32_t p0 = chunk * FACTOR_CHUNK, pc = min(FACTOR_CHUNK, f.n_factors - p0);
            __syncthreads();                                       // the tile staged before this one has been read
            if (n_chunks > 1u || tile == blockIdx.y)
                for (uint32_t p = 0; p < pc; ++p) v_sh[p][threadIdx.x] = mine ? f.V[(size_t)(p0 + p) * a.post_count + j] : 0.0;
            for (uint32_t e = threadIdx.x; e < pc * FACTOR_TILE_ROWS; e += 256u) {
                const uint32_t p = e / FACTOR_TILE_ROWS, k = e % FACTOR_TILE_ROWS;
                const long long ik = i0 + k;
                u_sh[p][k] = (ik >= 0 && ik < (long long)a.pre_count) ? f.U[(size_t)(p0 + p) * a.pre_count + (size_t)ik] : 0.0;
            }
            __syncthreads();
            for (uint32_t p = 0; p < pc; ++p) {
                const double v = v_sh[p][threadIdx.x];
#pragma unroll
                for (uint32_t k = 0; k < FACTOR_TILE_ROWS; ++k) sum[k] = connect_factors_step(sum[k], u_sh[p][k], v);
            }
        }
        if (!mine) continue;
#pragma unroll
        for (uint32_t u = 0; u < FACTOR_TILE_ROWS / 4u; ++u) {
            const uint32_t g = g0 + u;
            if (g <= g_last) {
                const long long i = i0 + 4 * (long long)u;
                connect_v4f *unit = reinterpret_cast<connect_v4f *>(a.W) + (size_t)g * a.ld + q;
                connect_v4f out;
                if (!(i >= 0 && i + 3 < (long long)a.pre_count)) out = *unit;
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    const long long ik = i + k;
                    if (ik >= 0 && ik < (long long)a.pre_count) {
                        uint32_t ra = 0, ca = 0;
                        if (RULE == CONNECT_CHEBYSHEV || RULE == CONNECT_EUCLIDEAN) { ra = (uint32_t)ik / a.pre_cols; ca = (uint32_t)ik - ra * a.pre_cols; }
                        const bool on = connect_factors_on<RULE, THIN, SELF>(a, s.x, (uint32_t)ik, i_same, ra, ca, rb, cb, (uint64_t)ik * a.post_count + j);
                        out[k] = connect_factors_weight(f, on, sum[u * 4u + k]);
                    }
                }
                __builtin_nontemporal_store(out, unit);
            }
        }
    }
}

// A wave-uniform word held in a vector register: the sparse kernel below has many more scalar values alive across its loops than
// vector ones (every argument of the merge, of the rule and of the sum, and the masks of five nested loops), and what the draw and
// the ring distances read moves over so that no scalar register spills.
__device__ __forceinline__ uint32_t connect_in_vgpr(uint32_t x)
{
    uint32_t v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}

// The merge of k_connect_csr_spec, statement for statement -- count and fill from the same body, candidates from the rule's window
// (on a ring at most two runs of rows by two of columns), ballot compaction -- with the factor sum as the candidate's weight.  One
// wavefront owns one post row j, so V[:, j] is staged once per row in the wavefront's own 1 KiB of LDS (FACTOR_CSR_CHUNK factors;
// a longer sum stages chunk after chunk per round of 64 candidates and carries the lane's partial sum); U[p][i] is read straight
// from memory, consecutive lanes consecutive candidates.  The count pass computes the sum only where drop_zero can drop the pair.
// Grid and block as k_connect_csr.
template <int RULE, bool THIN, bool SELF, bool FILL>
__global__ __launch_bounds__(256) void k_connect_csr_factors(const ConnectCsrFactorsArgs s)
{
    __shared__ double v_sh[4][FACTOR_CSR_CHUNK];
    const ConnectCsrArgs &a = s.c;
    const ConnectFactorsExt &f = s.f;
    ConnectArgs rule = a.c;                                        // what connect_factors_on reads, its draw in vector registers
    ConnectSpecExt x = s.x;
    if (THIN) {
        rule.edge_seed = (uint64_t)connect_in_vgpr((uint32_t)(a.c.edge_seed >> 32)) << 32 | connect_in_vgpr((uint32_t)a.c.edge_seed);
        rule.probability = __uint_as_float(connect_in_vgpr(__float_as_uint(a.c.probability)));
    }
    if (RULE == CONNECT_CHEBYSHEV || RULE == CONNECT_EUCLIDEAN) {
        rule.extent = connect_in_vgpr(a.c.extent);
        x.period_r = connect_in_vgpr(s.x.period_r); x.period_c = connect_in_vgpr(s.x.period_c);
    }
    const uint32_t lane = threadIdx.x & 63u;
    double *const vs = v_sh[threadIdx.x >> 6];
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t waves = gridDim.x * 4u;
    const uint32_t pre_end = a.c.pre_first + a.c.pre_count;
    const bool weigh = FILL || f.drop_zero;
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
        uint32_t n_cand, width = 1;
        ConnectSpans rs2{}, cs2{};
        if (RULE == CONNECT_CHEBYSHEV || RULE == CONNECT_EUCLIDEAN) {
            rs2 = connect_window_spans(rb, a.window, a.c.pre_rows, x.period_r);
            cs2 = connect_window_spans(cb, a.window, a.c.pre_cols, x.period_c);
            width = cs2.a.count + cs2.b.count;
            n_cand = (rs2.a.count + rs2.b.count) * width;
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
                if (t < n_cand) { ra = connect_spans_cell(rs2, wr); ca = connect_spans_cell(cs2, t - wr * width); }
                i = ra * a.c.pre_cols + ca;
            }
            if (RULE == CONNECT_SAME_POSITION) i = i_same;
            double sum = 0.0;
            if (weigh) {
                const double *u = f.U + (t < n_cand ? i : 0u);     // the lane's candidate; factor p is p * pre_count further on
                for (uint32_t p0 = 0; p0 < f.n_factors; p0 += FACTOR_CSR_CHUNK) {
                    const uint32_t pc = min(FACTOR_CSR_CHUNK, f.n_factors - p0);
                    if (f.n_factors > FACTOR_CSR_CHUNK || t0 == 0u) {      // (wave-uniform) the row's V, once; chunk by chunk when it is longer
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        for (uint32_t p = lane; p < pc; p += 64u) vs[p] = f.V[(size_t)(p0 + p) * a.c.post_count + j];
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    }
                    if (t < n_cand)
                        for (uint32_t p = 0; p < pc; ++p, u += a.c.pre_count) sum = connect_factors_step(sum, *u, vs[p]);
                }
            }
            float v = quiet_nan();
            if (t < n_cand)
                v = connect_factors_weight(f, connect_factors_on<RULE, THIN, SELF>(rule, x, i, i_same, ra, ca, rb, cb, (uint64_t)i * a.c.post_count + j), sum);
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

typedef void (*connect_factors_kernel_t)(const ConnectFactorsArgs);

template <int RULE>
inline connect_factors_kernel_t connect_factors_kernel_flags(bool thin, bool self)
{
    if (thin) return self ? k_connect_factors<RULE, true, true> : k_connect_factors<RULE, true, false>;
    return self ? k_connect_factors<RULE, false, true> : k_connect_factors<RULE, false, false>;
}
// the instantiation for a factors record: which template arguments a launch takes
inline connect_factors_kernel_t connect_factors_kernel(int rule, bool thin, bool self)
{
    switch (rule) {
    case CONNECT_CHEBYSHEV: return connect_factors_kernel_flags<CONNECT_CHEBYSHEV>(thin, self);
    case CONNECT_EUCLIDEAN: return connect_factors_kernel_flags<CONNECT_EUCLIDEAN>(thin, self);
    case CONNECT_SAME_POSITION: return connect_factors_kernel_flags<CONNECT_SAME_POSITION>(thin, self);
    default: return connect_factors_kernel_flags<CONNECT_ALL>(thin, self);
    }
}

typedef void (*connect_csr_factors_kernel_t)(const ConnectCsrFactorsArgs);

template <int RULE, bool FILL>
inline connect_csr_factors_kernel_t connect_csr_factors_kernel_flags(bool thin, bool self)
{
    if (thin) return self ? k_connect_csr_factors<RULE, true, true, FILL> : k_connect_csr_factors<RULE, true, false, FILL>;
    return self ? k_connect_csr_factors<RULE, false, true, FILL> : k_connect_csr_factors<RULE, false, false, FILL>;
}
template <bool FILL>
inline connect_csr_factors_kernel_t connect_csr_factors_kernel(int rule, bool thin, bool self)
{
    switch (rule) {
    case CONNECT_CHEBYSHEV: return connect_csr_factors_kernel_flags<CONNECT_CHEBYSHEV, FILL>(thin, self);
    case CONNECT_EUCLIDEAN: return connect_csr_factors_kernel_flags<CONNECT_EUCLIDEAN, FILL>(thin, self);
    case CONNECT_SAME_POSITION: return connect_csr_factors_kernel_flags<CONNECT_SAME_POSITION, FILL>(thin, self);
    default: return connect_csr_factors_kernel_flags<CONNECT_ALL, FILL>(thin, self);
    }
}

} // namespace snn
