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

// The same window on a ring of `period` cells (snn_connect_by_spec with a wrap flag; period >= size, center < period): the cells
// x of 0 .. size-1 with min(|x - center|, period - |x - center|) <= e.  They are the union of [0, center+e-period],
// [max(0, center-e), min(size-1, center+e)] and [center-e+period, size-1].  With 2e + 1 >= period that is every cell; otherwise
// the first piece needs center + e >= period and the last center < e, which together give 2e > period: at most two pieces hold a
// cell, and as 2e + 1 < period no two of them touch.  Returned as two ascending runs, a below b, either of which may be empty.
// period == 0: no wrap-around -- a = connect_window_span, b empty.
struct ConnectSpans { ConnectSpan a, b; };

SNN_WINDOW_FN ConnectSpans connect_window_spans(uint32_t center, uint32_t e, uint32_t size, uint32_t period)
{
    ConnectSpans s{connect_window_span(center, e, size), ConnectSpan{size, 0u}};
    if (period == 0u || size == 0u) return s;
    if (2ull * e + 1ull >= (uint64_t)period) { s.a = ConnectSpan{0u, size}; return s; }
    const uint64_t reach = (uint64_t)center + e;
    if (reach >= (uint64_t)period) {                 // the window runs over the end of the ring: cells 0 .. reach - period, below the middle piece
        const uint64_t last = reach - period;
        s.b = s.a;
        s.a = ConnectSpan{0u, last < (uint64_t)size - 1u ? (uint32_t)last + 1u : size};
    } else if (center < e) {                         // ... or below cell 0: cells center - e + period .., above the middle piece
        const uint64_t first = (uint64_t)center + period - e;
        if (first < (uint64_t)size) s.b = ConnectSpan{(uint32_t)first, size - (uint32_t)first};
    }
    return s;
}

// the cell with ordinal `k` (0 <= k < a.count + b.count) of the two runs taken in ascending order
SNN_WINDOW_FN uint32_t connect_spans_cell(const ConnectSpans &s, uint32_t k)
{
    return k < s.a.count ? s.a.first + k : s.b.first + (k - s.a.count);
}

} // namespace snn
