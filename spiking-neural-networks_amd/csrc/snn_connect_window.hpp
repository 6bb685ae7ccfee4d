// The candidate window of a distance rule (snn_connect_by_rules_csr): which cells of the presynaptic grid can lie within the
// rule's extent of a postsynaptic position at all.  Integer arithmetic only; plain C++ that host and device code share, and that
// tests/cpp/connect_window_test.cpp includes alone.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SNN_WINDOW_FN __host__ __device__ inline
#else
#define SNN_WINDOW_FN inline
#endif

namespace snn {

// floor(sqrt(x)) for every uint32_t: bit by bit from the top, no floating point
SNN_WINDOW_FN uint32_t isqrt_u32(uint32_t x)
{
    uint32_t r = 0;
    for (uint32_t bit = 1u << 15; bit; bit >>= 1) {
        const uint32_t t = r | bit;                 // t <= 0xFFFF: t * t fits
        if (t * t <= x) r = t;
    }
    return r;
}

// Half-width of the window in cells: the Chebyshev extent itself, the integer square root of the squared Euclidean one (dr <= e
// and dc <= e are necessary for dr*dr + dc*dc <= extent), 0 otherwise -- clipped to `largest_dim`, the largest row or column
// count of the two grids (no two positions are further apart), so that position + e never leaves 32 bits (grids hold < 2^31 cells).
SNN_WINDOW_FN uint32_t connect_window_extent(uint32_t rule, uint32_t extent, uint32_t largest_dim)
{
    const uint32_t e = rule == 1u /* Chebyshev */ ? extent : rule == 2u /* Euclidean */ ? isqrt_u32(extent) : 0u;
    return e < largest_dim ? e : largest_dim;
}

struct ConnectSpan { uint32_t first, count; };

// the cells [first, first + count) of 0 .. size-1 within e of `center` (which may lie outside the grid: count is 0 when none is)
SNN_WINDOW_FN ConnectSpan connect_window_span(uint32_t center, uint32_t e, uint32_t size)
{
    ConnectSpan s{center > e ? center - e : 0u, 0u};
    if (size == 0u) return s;
    const uint64_t reach = (uint64_t)center + e;
    const uint32_t last = reach < (uint64_t)size - 1u ? (uint32_t)reach : size - 1u;
    if (s.first <= last) s.count = last - s.first + 1u;
    return s;
}

} // namespace snn
