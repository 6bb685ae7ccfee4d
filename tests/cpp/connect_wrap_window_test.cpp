// The wrapped window of the sparse connection rules (csrc/snn_connect_window.hpp: connect_window_spans, connect_spans_cell), the
// header included alone: for every size, post_dim <= 24, every centre c < post_dim and every e <= period + 1 (period =
// max(size, post_dim)) the two runs hold exactly the cells x of 0 .. size-1 with min(|x - c|, period - |x - c|) <= e -- compared
// with the brute-force set cell by cell --, in ascending order, without duplicates, and their counts add up to the set's size.
// period == 0 must be connect_window_span.  Prints the number of cases and "connect wrap window ok".
#include "snn_connect_window.hpp"

#include <cstdio>
#include <cstdlib>

static void fail(const char *what, uint32_t size, uint32_t post_dim, uint32_t c, uint32_t e)
{
    std::printf("FAILED %s: size %u post_dim %u center %u e %u\n", what, size, post_dim, c, e);
    std::exit(1);
}

int main()
{
    unsigned long cases = 0, two_runs = 0, everything = 0;
    for (uint32_t size = 1; size <= 24; ++size)
        for (uint32_t post_dim = 1; post_dim <= 24; ++post_dim) {
            const uint32_t period = size > post_dim ? size : post_dim;
            for (uint32_t c = 0; c < post_dim; ++c)
                for (uint32_t e = 0; e <= period + 1; ++e) {
                    bool want[24];
                    uint32_t n_want = 0;
                    for (uint32_t x = 0; x < size; ++x) {
                        const uint32_t d = x > c ? x - c : c - x;
                        want[x] = (d < period - d ? d : period - d) <= e;
                        n_want += want[x];
                    }
                    const snn::ConnectSpans s = snn::connect_window_spans(c, e, size, period);
                    if (s.a.count + s.b.count != n_want) fail("count", size, post_dim, c, e);
                    if (s.a.count && s.b.count && s.a.first + s.a.count > s.b.first) fail("runs overlap or descend", size, post_dim, c, e);
                    bool seen[24] = {};
                    uint32_t last = 0;
                    for (uint32_t k = 0; k < n_want; ++k) {
                        const uint32_t x = snn::connect_spans_cell(s, k);
                        if (x >= size) fail("cell outside the grid", size, post_dim, c, e);
                        if (k && x <= last) fail("not ascending", size, post_dim, c, e);
                        if (seen[x]) fail("duplicate", size, post_dim, c, e);
                        if (!want[x]) fail("cell outside the window", size, post_dim, c, e);
                        seen[x] = true;
                        last = x;
                    }
                    two_runs += s.a.count && s.b.count;
                    everything += n_want == size;
                    // no wrap: the single clipped span, b empty
                    const snn::ConnectSpans flat = snn::connect_window_spans(c, e, size, 0);
                    const snn::ConnectSpan one = snn::connect_window_span(c, e, size);
                    if (flat.a.first != one.first || flat.a.count != one.count || flat.b.count != 0) fail("period 0", size, post_dim, c, e);
                    ++cases;
                }
        }
    // the format's edge: positions and extents near 2^31 must not overflow
    const snn::ConnectSpans big = snn::connect_window_spans(0x7FFFFFF0u, 0x7FFFFFFFu, 0x7FFFFFFFu, 0x7FFFFFFFu);
    if (big.a.first != 0 || big.a.count != 0x7FFFFFFFu || big.b.count != 0) fail("large", 0, 0, 0, 0);
    const snn::ConnectSpans edge = snn::connect_window_spans(0x7FFFFFFEu, 3, 0x7FFFFFFFu, 0x7FFFFFFFu);
    if (edge.a.first != 0 || edge.a.count != 3 || edge.b.first != 0x7FFFFFFBu || edge.b.count != 4) fail("large, two runs", 0, 0, 0, 0);
    std::printf("cases %lu two_runs %lu everything %lu\nconnect wrap window ok\n", cases, two_runs, everything);
    return 0;
}
