// Host check of csrc/snn_w24.hpp, included alone: the 24-bit code round trip, the encodability rule, and the image layout
// (tests/test_w24_codec.py builds and runs it, plain and under the address / undefined-behaviour sanitizers).
#include "snn_w24.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace snn;

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) {                                                            \
            if (++failures <= 10) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                         \
    } while (0)

// every code of the 24-bit space against `base`: present codes give the bit pattern back and encode to themselves, alone and
// through the lane's 12 dwords
static void round_trip(uint32_t base)
{
    uint32_t code[16], dw[12];
    for (uint32_t c0 = 0; c0 < (1u << 24); c0 += 16) {
        for (uint32_t i = 0; i < 16; ++i) code[i] = c0 + i;
        w24_pack16(code, dw);
        for (int i = 0; i < 16; ++i) {
            const uint32_t c = w24_unpack(dw, i);
            CHECK(c == code[i], "base %08x: code %06x unpacks as %06x", base, code[i], c);
            if (c == W24_ABSENT) {
                CHECK(!w24_present(c), "the absent code reads as present");
                continue;
            }
            CHECK(w24_present(c), "code %06x reads as absent", c);
            const uint32_t bits = w24_decode(c, base);
            CHECK(bits == base + c, "base %08x code %06x decodes to %08x", base, c, bits);
            CHECK(w24_encode(bits, base) == c, "base %08x bits %08x encodes to %06x, not %06x", base, bits, w24_encode(bits, base), c);
        }
    }
}

static void encodability()
{
    const uint32_t bases[] = {0u, 0x3F000000u, 0xBF000000u, 0xFF000001u};
    for (uint32_t b : bases) {
        CHECK(w24_encodable(b, b), "span 0 at %08x", b);
        CHECK(w24_base(b, b) == b, "base of a single pattern");
        if (b <= 0xFFFFFFFFu - 0xFFFFFEu) {
            CHECK(w24_encodable(b, b + 0xFFFFFEu), "span 0xFFFFFE at %08x", b);
            CHECK(w24_encode(b + 0xFFFFFEu, b) == 0xFFFFFEu && w24_present(w24_encode(b + 0xFFFFFEu, b)), "the largest code is present");
        }
        if (b <= 0xFFFFFFFFu - 0xFFFFFFu) CHECK(!w24_encodable(b, b + 0xFFFFFFu), "span 0xFFFFFF at %08x must not be encodable", b);
    }
    CHECK(W24_MAX_SPAN == 0xFFFFFEu && W24_ABSENT == 0xFFFFFFu, "constants");
    CHECK(w24_encodable(0xFFFFFFFFu, 0u) && w24_base(0xFFFFFFFFu, 0u) == 0u, "no present edge: encodable with base 0");
    CHECK(!w24_encodable(0x3F000000u, 0xBF000000u), "mixed signs");
    CHECK(w24_encodable(0x3F000000u, 0x3FBFFFFFu), "U[0.5, 1.5)");
    CHECK(!w24_encodable(0x00000000u, 0x3F800000u), "U[0, 1]");
}

// the three bytes of every (row, column) of the unpadded matrix: inside the image without its slack, no byte taken twice
static void bijection(uint32_t n_tot, uint32_t n_loc, size_t ld)
{
    const size_t bytes = w24_image_bytes(n_tot, ld);
    CHECK(bytes == w24_row_units(n_tot) * (ld / 64) * 3072 + W24_SLACK, "image size");
    std::vector<uint8_t> seen(bytes - W24_SLACK, 0);
    size_t taken = 0;
    for (uint32_t p = 0; p < n_tot; ++p)
        for (uint32_t q = 0; q < n_loc; ++q)
            for (uint32_t k = 0; k < 3; ++k) {
                const size_t at = w24_byte_index(p, q, ld, k);
                if (at >= seen.size()) { CHECK(false, "(%u, %u) byte %u at %zu, past the image of %zu bytes", p, q, k, at, seen.size()); return; }
                if (seen[at]) { CHECK(false, "(%u, %u) byte %u at %zu: taken twice", p, q, k, at); return; }
                seen[at] = 1;
                ++taken;
            }
    CHECK(taken == (size_t)3 * n_tot * n_loc, "bytes taken");
}

// an image written the way the pack kernel writes it (a lane's 16 codes -> 12 dwords -> three 16-byte pieces, one per plane)
// holds the code of (row, column) at the bytes w24_byte_index names
static void layout(uint32_t n_tot, uint32_t n_loc, size_t ld)
{
    std::vector<uint8_t> image(w24_image_bytes(n_tot, ld), 0xEE);
    auto code_of = [&](uint32_t p, uint32_t q) { return (p < n_tot && q < n_loc && (p * 31u + q * 7u) % 5u != 0u) ? (p * 2654435761u + q * 40503u) % 0xFFFFFFu : W24_ABSENT; };
    for (size_t ru = 0; ru < w24_row_units(n_tot); ++ru)
        for (uint32_t q = 0; q < ld; ++q) {
            uint32_t code[16], dw[12];
            for (uint32_t r = 0; r < 16; ++r) code[r] = code_of((uint32_t)ru * 16 + r, q);
            w24_pack16(code, dw);
            uint8_t *unit = image.data() + w24_unit_offset(ru, q / 64, ld);
            for (int plane = 0; plane < 3; ++plane)
                for (int d = 0; d < 4; ++d)
                    for (int b = 0; b < 4; ++b)      // little-endian dwords
                        unit[plane * W24_PLANE_BYTES + (q % 64) * 16 + d * 4 + b] = (uint8_t)(dw[plane * 4 + d] >> (8 * b));
        }
    for (uint32_t p = 0; p < n_tot; ++p)
        for (uint32_t q = 0; q < n_loc; ++q) {
            uint32_t c = 0;
            for (uint32_t k = 0; k < 3; ++k) c |= (uint32_t)image[w24_byte_index(p, q, ld, k)] << (8 * k);
            CHECK(c == code_of(p, q), "(%u, %u): %06x in the image, %06x packed", p, q, c, code_of(p, q));
        }
    // rows past n_tot of the last unit and columns past n_loc read as absent
    const uint32_t last = (uint32_t)w24_row_units(n_tot) * 16 - 1;
    uint32_t c = 0;
    for (uint32_t k = 0; k < 3; ++k) c |= (uint32_t)image[w24_byte_index(last, 0, ld, k)] << (8 * k);
    CHECK(n_tot % 16 == 0 || c == W24_ABSENT, "padding row");
}

int main()
{
    round_trip(0u);
    round_trip(0x3F000000u);
    round_trip(0xBF000000u);          // negative weights: the sign bit is part of the base
    encodability();
    bijection(5183, 5183, 5184);
    bijection(4101, 4101, 4160);
    bijection(37, 100, 128);
    layout(37, 100, 128);
    layout(64, 64, 64);
    printf(failures ? "w24 codec: %d failures\n" : "w24 codec ok\n", failures);
    return failures ? 1 : 0;
}
