// csrc/snn_connect_window.hpp on the host, included alone: prints what the helpers return -- the integer square root for every
// extent 0 .. 2^16, the format edges and every perfect square +- 1; the window half-width per rule; the clipped span of a window
// for small grids and for the largest positions -- one line each, for tests/test_connect_window.py to compare with math.isqrt and
// a brute-force count.  Also checks r*r <= x < (r+1)*(r+1) in 64 bits on a stride through all of uint32.
#include <cinttypes>
#include <cstdio>
#include <initializer_list>

#include "snn_connect_window.hpp"

using namespace snn;

int main()
{
    for (uint32_t x = 0; x <= 65536u; ++x) std::printf("isqrt %" PRIu32 " %" PRIu32 "\n", x, isqrt_u32(x));
    for (uint64_t r = 1; r <= 65535u; ++r) {
        for (int64_t d = -1; d <= 1; ++d) {
            const uint64_t x = r * r + d;
            if (x <= 0xFFFFFFFFull) std::printf("isqrt %" PRIu64 " %" PRIu32 "\n", x, isqrt_u32((uint32_t)x));
        }
    }
    for (uint32_t x : {0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFE0001u, 0xFFFE0000u, 0xFFFE0002u, 0x80000000u, 0x7FFFFFFFu, 0x40000000u, 0x3FFFFFFFu})
        std::printf("isqrt %" PRIu32 " %" PRIu32 "\n", x, isqrt_u32(x));
    for (uint64_t x = 0; x <= 0xFFFFFFFFull; x += 65521u) {
        const uint64_t r = isqrt_u32((uint32_t)x);
        if (r * r > x || (r + 1) * (r + 1) <= x) { std::printf("isqrt_u32(%" PRIu64 ") = %" PRIu64 " is not the floor of the root\n", x, r); return 1; }
    }
    for (uint32_t rule = 0; rule < 4; ++rule)
        for (uint32_t extent : {0u, 1u, 4u, 5u, 24u, 25u, 1000u, 0xFFFFFFFFu})
            for (uint32_t largest : {1u, 5u, 512u, 0x7FFFFFFFu})
                std::printf("extent %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", rule, extent, largest, connect_window_extent(rule, extent, largest));
    for (uint32_t size = 0; size <= 6; ++size)
        for (uint32_t center = 0; center <= 9; ++center)
            for (uint32_t e = 0; e <= 8; ++e) {
                const ConnectSpan s = connect_window_span(center, e, size);
                std::printf("span %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", center, e, size, s.first, s.count);
            }
    for (uint32_t center : {0u, 0x7FFFFFFEu, 0x7FFFFFFFu})
        for (uint32_t e : {0u, 1u, 0x7FFFFFFFu})
            for (uint32_t size : {1u, 0x7FFFFFFFu}) {
                const ConnectSpan s = connect_window_span(center, e, size);
                std::printf("span %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", center, e, size, s.first, s.count);
            }
    std::printf("connect window ok\n");
    return 0;
}
