// The 24-bit image of a static dense synapse matrix: what k_inputs_dense_w24 streams instead of W.
//
// Code.    code = bits(w) - base as u32, base = the smallest bit pattern (compared unsigned) over the PRESENT edges of the
//          handle's n_tot x n_loc block; an absent edge is W24_ABSENT.  The matrix is encodable iff max_bits - base <=
//          W24_MAX_SPAN, so every present code is below W24_ABSENT and bits = code + base gives every weight back exactly.
// Layout.  A unit is 16 presynaptic rows x 64 columns = 3 KiB, stored as three 1 KiB planes: lane L (= column % 64) owns the
//          16-byte pieces at plane * 1024 + L * 16, and inside those 48 bytes its 16 codes are consecutive and little-endian,
//          the code of row r at byte 3 r.  A wavefront reads a plane with ONE fully coalesced dwordx4 load (1 KiB), as it reads
//          a row group of W.  Units are ordered [row unit][column block of 64]; rows are padded to 16 with absent codes, columns
//          go to ld (a multiple of 64).  CHUNK = 256 rows is 16 units, so the chunked ascending order of the sums is untouched.
//          The image ends with W24_SLACK bytes the last column tile may read past the last row unit (never used).
// Plain C++17: tests/cpp/w24_codec.cpp compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SNN_W24_HD __host__ __device__
#else
#define SNN_W24_HD
#endif

namespace snn {

constexpr uint32_t W24_ABSENT = 0xFFFFFFu;          // code of an absent edge
constexpr uint32_t W24_MAX_SPAN = 0xFFFFFEu;        // largest max_bits - base an image can hold
constexpr uint32_t W24_UNIT_ROWS = 16, W24_UNIT_COLS = 64;
constexpr size_t W24_PLANE_BYTES = 1024, W24_UNIT_BYTES = 3 * W24_PLANE_BYTES;
constexpr size_t W24_SLACK = 16 * W24_UNIT_BYTES;   // one column tile (1024 columns) of units, as WMATRIX_SLACK for W

// min_bits / max_bits over the present edges (min_bits > max_bits: there is none -- encodable with base 0)
SNN_W24_HD inline bool w24_encodable(uint32_t min_bits, uint32_t max_bits)
{
    return min_bits > max_bits || max_bits - min_bits <= W24_MAX_SPAN;
}
SNN_W24_HD inline uint32_t w24_base(uint32_t min_bits, uint32_t max_bits) { return min_bits > max_bits ? 0u : min_bits; }

SNN_W24_HD inline uint32_t w24_encode(uint32_t bits, uint32_t base) { return bits - base; }      // of a present edge
SNN_W24_HD inline bool w24_present(uint32_t code) { return code != W24_ABSENT; }
SNN_W24_HD inline uint32_t w24_decode(uint32_t code, uint32_t base) { return code + base; }

SNN_W24_HD inline size_t w24_row_units(uint32_t n_rows) { return ((size_t)n_rows + W24_UNIT_ROWS - 1) / W24_UNIT_ROWS; }
// bytes of the image of a matrix with n_rows rows and ld columns (ld a multiple of 64), slack included
SNN_W24_HD inline size_t w24_image_bytes(uint32_t n_rows, size_t ld)
{
    return w24_row_units(n_rows) * (ld / W24_UNIT_COLS) * W24_UNIT_BYTES + W24_SLACK;
}
// Region hand-over (ensure_w24): the image may take over the allocation of the matrix it was packed from.  The body of W is its
// rows padded to groups of four, 4 bytes per entry; W's own slack follows the body and is left out, so that the image -- its own
// slack included -- never reaches into it.  3 bytes against 4 per entry, but rows padded to 16 against 4 and 48 KiB of slack:
// false for matrices of few rows or few columns, whose padding and slack outweigh the quarter saved.
SNN_W24_HD inline size_t w24_matrix_body_bytes(uint32_t n_rows, size_t ld) { return (((size_t)n_rows + 3) / 4) * 4 * ld * 4; }
SNN_W24_HD inline bool w24_fits_matrix(uint32_t n_rows, size_t ld)
{
    return ld >= W24_UNIT_COLS && ld % W24_UNIT_COLS == 0 && w24_image_bytes(n_rows, ld) <= w24_matrix_body_bytes(n_rows, ld);
}
// byte offset of unit (row unit ru, column block cb)
SNN_W24_HD inline size_t w24_unit_offset(size_t ru, size_t cb, size_t ld) { return (ru * (ld / W24_UNIT_COLS) + cb) * W24_UNIT_BYTES; }
// byte offset of byte k (0 = least significant .. 2) of the code of (row p, column q); a code may straddle two planes
SNN_W24_HD inline size_t w24_byte_index(uint32_t p, uint32_t q, size_t ld, uint32_t k = 0)
{
    const uint32_t in_lane = 3u * (p % W24_UNIT_ROWS) + k;   // byte inside the lane's 48
    return w24_unit_offset(p / W24_UNIT_ROWS, q / W24_UNIT_COLS, ld) + (size_t)(in_lane / 16u) * W24_PLANE_BYTES +
           (size_t)(q % W24_UNIT_COLS) * 16u + in_lane % 16u;
}

// 16 codes -> the lane's 12 little-endian dwords (dword d holds bytes 4 d .. 4 d + 3 of the 48), and back
SNN_W24_HD inline void w24_pack16(const uint32_t (&code)[16], uint32_t (&dw)[12])
{
    for (int d = 0; d < 12; ++d) dw[d] = 0u;
    for (int r = 0; r < 16; ++r)
        for (int k = 0; k < 3; ++k) {
            const int byte = 3 * r + k;
            dw[byte >> 2] |= ((code[r] >> (8 * k)) & 0xFFu) << (8 * (byte & 3));
        }
}
SNN_W24_HD inline uint32_t w24_unpack(const uint32_t (&dw)[12], int r)
{
    uint32_t c = 0;
    for (int k = 0; k < 3; ++k) {
        const int byte = 3 * r + k;
        c |= ((dw[byte >> 2] >> (8 * (byte & 3))) & 0xFFu) << (8 * k);
    }
    return c;
}

} // namespace snn
