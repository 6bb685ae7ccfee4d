// Host check of the fit predicate of the region hand-over (csrc/snn_w24.hpp: w24_fits_matrix), included alone: may the 24-bit
// image of a matrix take over that matrix's own allocation?  (tests/test_w24_region.py builds and runs it, plain and under the
// address / undefined-behaviour sanitizers.)
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

// W as the library allocates it (snn_layout.hpp, wcount): rows padded to groups of four, then 4096 floats of slack
constexpr size_t MATRIX_SLACK_BYTES = 4096 * 4;
static size_t body_bytes(uint32_t n_rows, size_t ld) { return (size_t)((n_rows + 3u) / 4u) * 4u * ld * 4u; }

// one past the last byte the image kernel may touch, restated from the layout: every unit of every row unit and column block,
// and the slack tile of 16 units behind the last one
static size_t image_end(uint32_t n_rows, size_t ld)
{
    const size_t rus = ((size_t)n_rows + 15) / 16, cbs = ld / 64;
    return w24_unit_offset(rus - 1, cbs - 1, ld) + W24_UNIT_BYTES + 16 * W24_UNIT_BYTES;
}

static void predicate_over_ragged_sizes()
{
    size_t fits = 0, total = 0;
    for (uint32_t n = 1; n <= 4200; ++n)
        for (size_t ld = 64; ld <= 4224; ld += 64) {
            const bool want = image_end(n, ld) <= body_bytes(n, ld);
            const bool got = w24_fits_matrix(n, ld);
            CHECK(got == want, "n_tot %u ld %zu: predicate %d, image ends at %zu of a body of %zu", n, ld, (int)got, image_end(n, ld), body_bytes(n, ld));
            CHECK(image_end(n, ld) == w24_image_bytes(n, ld), "n_tot %u ld %zu: w24_image_bytes %zu, layout ends at %zu", n, ld, w24_image_bytes(n, ld), image_end(n, ld));
            CHECK(w24_matrix_body_bytes(n, ld) == body_bytes(n, ld), "n_tot %u ld %zu: body", n, ld);
            // the last code of the last (padded) row and column lies inside the image proper, before its slack
            const uint32_t p_last = (uint32_t)(((size_t)n + 15) / 16 * 16 - 1);
            CHECK(w24_byte_index(p_last, (uint32_t)ld - 1, ld, 2) < w24_image_bytes(n, ld) - W24_SLACK, "n_tot %u ld %zu: last code outside", n, ld);
            fits += got;
            ++total;
        }
    CHECK(fits > 0 && fits < total, "the predicate must hold for some sizes and fail for others (%zu of %zu)", fits, total);
    CHECK(!w24_fits_matrix(1, 64) && !w24_fits_matrix(12, 4224) && !w24_fits_matrix(400, 64),"few rows: padding to 16 and the slack outweigh the quarter saved");
    CHECK(w24_fits_matrix(5183, 5184) && w24_fits_matrix(4099, 4160) && w24_fits_matrix(65536, 65536), "the sizes the library hands over");
    CHECK(!w24_fits_matrix(5183, 5000) && !w24_fits_matrix(5183, 0), "ld must be a positive multiple of 64");
}

// The real thing in small: a buffer exactly as large as W with its slack, the slack filled with a canary; every byte of the
// image's extent (slack tile included) is written through the layout's own offsets.  The canary must survive, and under the
// address sanitizer no write may leave the buffer.
static void image_written_into_a_matrix(uint32_t n, size_t ld)
{
    CHECK(w24_fits_matrix(n, ld), "n_tot %u ld %zu should fit", n, ld);
    if (!w24_fits_matrix(n, ld)) return;
    const size_t body = body_bytes(n, ld);
    std::vector<uint8_t> w(body + MATRIX_SLACK_BYTES, 0xC5);
    const size_t rus = w24_row_units(n), cbs = ld / W24_UNIT_COLS;
    for (size_t ru = 0; ru < rus; ++ru)
        for (size_t cb = 0; cb < cbs; ++cb) memset(w.data() + w24_unit_offset(ru, cb, ld), 0x11, W24_UNIT_BYTES);
    memset(w.data() + w24_unit_offset(rus, 0, ld), 0x22, W24_SLACK);       // the image's own slack, behind its last unit
    for (uint32_t p : {0u, n - 1}) for (uint32_t q : {0u, (uint32_t)ld - 1}) for (uint32_t k = 0; k < 3; ++k) w[w24_byte_index(p, q, ld, k)] = 0x33;
    size_t hurt = 0;
    for (size_t i = body; i < w.size(); ++i) hurt += w[i] != 0xC5;
    CHECK(hurt == 0, "n_tot %u ld %zu: %zu bytes of W's slack overwritten by the image", n, ld, hurt);
}

int main()
{
    predicate_over_ragged_sizes();
    // the two ragged shapes of the GPU tests, and for a few ld the FIRST n_tot that fits (the tightest case)
    image_written_into_a_matrix(5183, 5184);
    image_written_into_a_matrix(4099, 4160);
    for (size_t ld : {64, 320, 1024, 4224})
        for (uint32_t n = 1; n <= 4200; ++n)
            if (w24_fits_matrix(n, ld)) { image_written_into_a_matrix(n, ld); break; }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("w24 region ok\n");
    return 0;
}
