// The host-built half of the step image of a sparse graph (snn_kernels_csr.hpp, "STEP IMAGE"): the slice headers with their
// window pieces and the plan words that go with them, from the SELL arrays.  Plain C++, no HIP and no handle;
// tests/cpp/step_image_plan_test.cpp includes it alone and emulates the kernel's window on the host.
#pragma once
#include <cstddef>
#include <cstdint>
#include <algorithm>

namespace snn {

constexpr uint32_t SELL_PAD = 0xFFFFFFFFu;     // presynaptic index of a padding entry
constexpr uint32_t PLAN_CODE = 0x7FFFFFFFu;    // gather-plan word: the source code (all ones = padding), bit 31 = new chunk
constexpr uint32_t PLAN_CHUNK = 256;           // the canonical reduction chunk (snn_layout.hpp CHUNK) the chunk bits follow

constexpr uint32_t IMG_HDR_WORDS = 40, IMG_MAX_PIECES = 16, IMG_PIECE_WORDS = 64, IMG_CELL_BIT = 0x40000000u;
constexpr uint32_t IMG_WIN_WORDS = IMG_MAX_PIECES * IMG_PIECE_WORDS;           // LDS words per wavefront

// Per slice: the sorted set of everything its 64 rows gather, cut greedily into pieces -- a piece starts at the first source not
// yet covered and spans at most 64 LDS words of consecutive sources of one kind (a neuron is one word, a spike-train cell the two
// words of its view entry), trimmed to the last source it holds.  A slice that needs more than IMG_MAX_PIECES pieces stays
// unstaged (no pieces, plain codes).
// nn, nc: neurons and spike-train cells of the network (a presynaptic index below nn is a neuron, below nn + nc a cell).
// halo_word (shard handles, the image of direct runs): per neuron the word of the receive buffer that carries it (0xFFFFFFFF: read
// from the exchanged state); such a source has code nn + nc + word, a third kind of piece next to neurons and cells.
// slice_ptr, sell_pre, hdr, plan_win: any vectors of uint32_t.
template <typename VecIn, typename VecOut>
inline void build_step_image_plan(uint32_t nn, uint32_t nc, const VecIn &slice_ptr, const VecIn &sell_pre, uint32_t n_slices,
                                  VecOut &hdr, VecOut &plan_win, uint64_t &records, uint64_t &staged_slices,
                                  const uint32_t *halo_word = nullptr)
{
    const uint32_t halo_base = nn + nc;
    auto code_of = [&](uint32_t p) { return (halo_word && p < nn && halo_word[p] != 0xFFFFFFFFu) ? halo_base + halo_word[p] : p; };
    auto kind_of = [&](uint32_t code) { return code < nn ? 0 : (code < halo_base ? 1 : 2); };
    hdr.assign((size_t)n_slices * IMG_HDR_WORDS, 0u);
    plan_win.assign(sell_pre.size(), PLAN_CODE);
    records = 0; staged_slices = 0;
    VecOut codes, offs;
    for (uint32_t sl = 0; sl < n_slices; ++sl) {
        const uint32_t s0 = slice_ptr[sl], s1 = slice_ptr[sl + 1], width = (s1 - s0) >> 6;
        uint32_t *h = &hdr[(size_t)sl * IMG_HDR_WORDS];
        h[0] = (uint32_t)records; h[1] = (width + 1) / 2;
        records += (uint64_t)h[1] * 64;
        if (width == 0) continue;
        codes.clear();
        for (uint32_t e = s0; e < s1; ++e)
            if (sell_pre[e] != SELL_PAD) codes.push_back(code_of(sell_pre[e]));
        std::sort(codes.begin(), codes.end());
        codes.erase(std::unique(codes.begin(), codes.end()), codes.end());
        offs.assign(codes.size(), 0u);
        uint32_t n_pieces = 0;
        bool staged = !codes.empty();
        for (size_t i = 0; i < codes.size() && staged;) {
            const uint32_t start = codes[i];
            const int kind = kind_of(start);
            const uint32_t per = kind == 1 ? 2u : 1u, span = IMG_PIECE_WORDS / per;
            if (n_pieces == IMG_MAX_PIECES) { staged = false; break; }
            size_t j = i;
            while (j < codes.size() && codes[j] - start < span && kind_of(codes[j]) == kind) {
                offs[j] = n_pieces * IMG_PIECE_WORDS + (codes[j] - start) * per;
                ++j;
            }
            h[4 + 2 * n_pieces] = start;
            h[5 + 2 * n_pieces] = (codes[j - 1] - start + 1) * per;
            ++n_pieces;
            i = j;
        }
        if (!staged) {
            n_pieces = 0;
            for (uint32_t k = 0; k < 2 * IMG_MAX_PIECES; ++k) h[4 + k] = 0u;
        }
        h[2] = n_pieces;
        staged_slices += staged ? 1 : 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            uint32_t prev = 0;
            for (uint32_t k = 0; k < width; ++k) {
                const size_t e = s0 + lane + (size_t)k * 64;
                const uint32_t p = sell_pre[e];
                if (p == SELL_PAD) break;                   // padding only ever trails a row
                const uint32_t chunk_bit = (k == 0 || p / PLAN_CHUNK != prev / PLAN_CHUNK) ? 0x80000000u : 0u;
                prev = p;
                const uint32_t code = code_of(p);
                if (staged) {
                    const size_t at = std::lower_bound(codes.begin(), codes.end(), code) - codes.begin();
                    plan_win[e] = offs[at] | (kind_of(code) == 1 ? IMG_CELL_BIT : 0u) | chunk_bit;
                } else {
                    plan_win[e] = code | chunk_bit;
                }
            }
        }
    }
}

} // namespace snn
