// csrc/snn_step_image_plan.hpp on the host, included alone: the slice headers, window pieces and plan words of the step image,
// checked by EMULATING the kernel (csr_row_sums_img / csr_img_sums<true> in snn_kernels_csr.hpp) and against a naive restatement.
//   window:  per slice a 1024-word window is poisoned and filled from the header's pieces exactly as the LDS-DMA loop fills it
//            (win[u * 64 + lane] = src[lane] for lane < words) out of source arrays with a distinct value in every word (neuron
//            words, the cells' view word pairs, the words of the receive buffer); then every entry's plan word is walked: a staged
//            entry's window word is its source's word and never poison, a staged cell's off and off + 1 are the two words of its
//            view entry in order and off + 1 is inside the window; an unstaged entry's word is the plain code.
//   pieces:  at most 16 per slice, each 1 .. 64 words (an even number for cells), sources of one kind, never past the end of
//            its array (code + words <= nn; 2 * (code - nn) + words <= 2 * nc; the receive buffer's word count), the header's
//            unused pieces zero.
//   header:  [0] = the running record count, [1] = (width + 1) / 2, [2] = pieces, [3] = 0; `records` and `staged_slices`.
//   staging: a slice is unstaged exactly when the greedy cut, restated here over a std::set (take the smallest source left, erase
//            what its span and kind cover, count), needs more than 16 pieces; then plain codes and no pieces.
//   chunks:  bit 31 on the first entry of a row and on every change of p / 256 (the presynaptic INDEX, as in the plain plan).
//   padding: entries behind a row's end stay PLAN_CODE.
// Inputs: every subset of 14 sources around nn - 1 | nn (neuron | cell), nn + nc - 1 | halo_base (cell | receive buffer) and the
// span ends of either kind; the same without cells (neuron | receive buffer); directed slices (1024 and 1025 consecutive neurons
// from 37, 1024 neurons in 16 pieces with gaps, trimmed pieces, 512 cells up to the LAST cell, 513 cells, a run through neuron,
// cell and receive buffer, the last cell alone, empty slices in the middle and at the end) with and without a halo; random slices.
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "snn_step_image_plan.hpp"

using namespace snn;

typedef std::vector<uint32_t> U32;
typedef std::vector<U32> Slice;                 // 64 rows, each the ascending presynaptic indices of its entries

static const uint32_t POISON = 0xDEADBEEFu, NO_HALO = 0xFFFFFFFFu;

struct Net {
    uint32_t nn, nc;
    U32 halo_word;                              // empty: no halo; else per neuron the word of the receive buffer or NO_HALO
    uint32_t n_halo;                            // words of the receive buffer
};

struct Expect { int staged; int pieces; int max_off; };          // per slice, -1 = not asserted

static unsigned long long g_slices = 0;

#define FAIL(...) do { std::printf("%s, slice %u: ", what, sl); std::printf(__VA_ARGS__); std::printf("\n"); return false; } while (0)

static int kind_of(const Net &n, uint32_t code) { return code < n.nn ? 0 : code < n.nn + n.nc ? 1 : 2; }

// the greedy cut, naively: pieces needed for a set of codes
static uint32_t naive_pieces(const Net &n, std::set<uint32_t> left)
{
    uint32_t pieces = 0;
    while (!left.empty()) {
        const uint32_t c0 = *left.begin();
        const int kind = kind_of(n, c0);
        uint64_t end = (uint64_t)c0 + (kind == 1 ? 32 : 64);                  // a cell takes two of a piece's 64 words
        if (kind == 0) end = std::min<uint64_t>(end, n.nn);                  // a piece never leaves its array
        if (kind == 1) end = std::min<uint64_t>(end, (uint64_t)n.nn + n.nc);
        left.erase(left.begin(), left.lower_bound((uint32_t)std::min<uint64_t>(end, 0xFFFFFFFFu)));
        ++pieces;
    }
    return pieces;
}

static bool check(const Net &n, const std::vector<Slice> &slices, const std::vector<Expect> &expect, const char *what)
{
    const uint32_t n_slices = (uint32_t)slices.size(), halo_base = n.nn + n.nc;
    // SELL-64: entry k of a slice's lane at slice_ptr + k * 64 + lane, rows padded to the slice's longest
    U32 slice_ptr(1, 0u), sell_pre;
    for (const Slice &s : slices) {
        size_t width = 0;
        for (const U32 &row : s) width = std::max(width, row.size());
        const size_t s0 = sell_pre.size();
        sell_pre.resize(s0 + width * 64, SELL_PAD);
        for (uint32_t lane = 0; lane < 64; ++lane)
            for (size_t k = 0; k < s[lane].size(); ++k) sell_pre[s0 + k * 64 + lane] = s[lane][k];
        slice_ptr.push_back((uint32_t)sell_pre.size());
    }
    U32 hdr(3, 77u), plan_win(5, 99u);                                    // (whatever they held before)
    uint64_t records = 12345, staged_slices = 678;
    build_step_image_plan(n.nn, n.nc, slice_ptr, sell_pre, n_slices, hdr, plan_win, records, staged_slices,
                          n.halo_word.empty() ? nullptr : n.halo_word.data());
    uint32_t sl = 0;
    if (hdr.size() != (size_t)n_slices * IMG_HDR_WORDS || plan_win.size() != sell_pre.size()) FAIL("sizes of the outputs");
    // the sources, a distinct value in every word
    U32 xv(n.nn), cv(2 * (size_t)n.nc), halo(n.n_halo);
    for (uint32_t i = 0; i < n.nn; ++i) xv[i] = 0x10000000u + i;
    for (size_t i = 0; i < cv.size(); ++i) cv[i] = 0x20000000u + (uint32_t)i;
    for (uint32_t i = 0; i < n.n_halo; ++i) halo[i] = 0x30000000u + i;
    auto code_of = [&](uint32_t p) { return (!n.halo_word.empty() && p < n.nn && n.halo_word[p] != NO_HALO) ? halo_base + n.halo_word[p] : p; };
    auto source_word = [&](uint32_t code) { return code < n.nn ? xv[code] : code < halo_base ? cv[2 * (size_t)(code - n.nn)] : halo[code - halo_base]; };
    uint64_t want_records = 0, want_staged = 0;
    for (sl = 0; sl < n_slices; ++sl, ++g_slices) {
        const Slice &s = slices[sl];
        const uint32_t s0 = slice_ptr[sl], width = (slice_ptr[sl + 1] - s0) / 64;
        const uint32_t *h = &hdr[(size_t)sl * IMG_HDR_WORDS];
        if (h[0] != want_records || h[1] != (width + 1) / 2 || h[3] != 0u) FAIL("header {%u, %u, %u, %u}, %llu records before it, width %u", h[0], h[1], h[2], h[3], (unsigned long long)want_records, width);
        want_records += (uint64_t)((width + 1) / 2) * 64;
        std::set<uint32_t> codes;
        for (const U32 &row : s) for (uint32_t p : row) codes.insert(code_of(p));
        const uint32_t need = naive_pieces(n, codes);
        const bool staged = need >= 1 && need <= IMG_MAX_PIECES;
        want_staged += staged;
        const uint32_t n_pieces = h[2];
        if (n_pieces > IMG_MAX_PIECES) FAIL("%u pieces", n_pieces);
        if (n_pieces != (staged ? need : 0u)) FAIL("%u pieces where the naive cut needs %u", n_pieces, need);
        if (sl < expect.size() && expect[sl].staged >= 0 && (int)staged != expect[sl].staged) FAIL("the case is not what it was built to be: %u pieces needed", need);
        if (sl < expect.size() && expect[sl].pieces >= 0 && (int)need != expect[sl].pieces) FAIL("the case is not what it was built to be: %u pieces needed, not %d", need, expect[sl].pieces);
        // the window, as the LDS-DMA loop fills it (all 16 header pieces are walked: the kernel does)
        U32 win(IMG_WIN_WORDS, POISON);
        for (uint32_t u = 0; u < IMG_MAX_PIECES; ++u) {
            const uint32_t code = h[4 + 2 * u], words = h[5 + 2 * u];
            if (u >= n_pieces) {
                if (code || words) FAIL("piece %u of %u is {%u, %u}", u, n_pieces, code, words);
                continue;
            }
            if (words < 1 || words > IMG_PIECE_WORDS) FAIL("piece %u has %u words", u, words);
            const int kind = kind_of(n, code);
            const uint32_t *src;
            if (kind == 0) {
                if ((uint64_t)code + words > n.nn) FAIL("piece %u {%u, %u} reads past the %u neurons", u, code, words, n.nn);
                src = xv.data() + code;
            } else if (kind == 1) {
                if (words % 2 || 2 * (uint64_t)(code - n.nn) + words > 2 * (uint64_t)n.nc) FAIL("piece %u {%u, %u} of cells: odd, or past the %u cells", u, code, words, n.nc);
                src = cv.data() + 2 * (size_t)(code - n.nn);
            } else {
                if ((uint64_t)(code - halo_base) + words > n.n_halo) FAIL("piece %u {%u, %u} reads past the %u words of the receive buffer", u, code, words, n.n_halo);
                src = halo.data() + (code - halo_base);
            }
            for (uint32_t lane = 0; lane < 64; ++lane)
                if (lane < words) win[u * IMG_PIECE_WORDS + lane] = src[lane];
        }
        // every entry's plan word
        int max_off = -1;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            for (uint32_t k = 0; k < width; ++k) {
                const size_t e = s0 + lane + (size_t)k * 64;
                const uint32_t w = plan_win[e];
                if (k >= s[lane].size()) {
                    if (w != PLAN_CODE) FAIL("lane %u entry %u is padding with plan word %08x", lane, k, w);
                    continue;
                }
                const uint32_t p = s[lane][k], code = code_of(p);
                const bool chunk = k == 0 || p / 256 != s[lane][k - 1] / 256;
                if ((w >> 31) != (chunk ? 1u : 0u)) FAIL("lane %u entry %u (source %u): chunk bit %u", lane, k, p, w >> 31);
                if (!staged) {
                    if ((w & PLAN_CODE) != code) FAIL("lane %u entry %u: plain code %u expected, plan word %08x", lane, k, code, w);
                    continue;
                }
                const bool cell = kind_of(n, code) == 1;
                const uint32_t off = w & 0xFFFFu;
                if ((w & 0x7FFFFFFFu) != (off | (cell ? IMG_CELL_BIT : 0u))) FAIL("lane %u entry %u: plan word %08x of a %s", lane, k, w, cell ? "cell" : "neuron");
                if (off >= IMG_WIN_WORDS || win[off] == POISON || win[off] != source_word(code))
                    FAIL("lane %u entry %u (code %u): window word %u holds %08x, its source is %08x", lane, k, code, off, off < IMG_WIN_WORDS ? win[off] : 0u, source_word(code));
                if (cell && (off + 1 >= IMG_WIN_WORDS || win[off + 1] != cv[2 * (size_t)(code - n.nn) + 1]))
                    FAIL("lane %u entry %u (cell %u): the second view word is not at window word %u + 1", lane, k, code - n.nn, off);
                max_off = std::max(max_off, (int)off);
            }
        }
        if (sl < expect.size() && expect[sl].max_off >= 0 && max_off != expect[sl].max_off) FAIL("the case is not what it was built to be: largest offset %d, not %d", max_off, expect[sl].max_off);
    }
    sl = n_slices;
    if (records != want_records || staged_slices != want_staged) FAIL("%llu records and %llu staged slices, not %llu and %llu", (unsigned long long)records, (unsigned long long)staged_slices, (unsigned long long)want_records, (unsigned long long)want_staged);
    return true;
}

static Slice empty_slice() { return Slice(64); }

// sources dealt to the 64 rows in turn (each row ascending), `per_row` to a row; all of them also to nobody twice
static Slice deal(const U32 &sources, size_t per_row)
{
    Slice s(64);
    for (size_t i = 0; i < sources.size(); ++i) s[std::min<size_t>(i / per_row, 63)].push_back(sources[i]);
    return s;
}

static bool exhaustive(const Net &n, const U32 &sources, unsigned long long &cases)
{
    for (uint32_t mask = 0; mask < (1u << sources.size()); ++mask, ++cases) {
        Slice s(64);
        for (size_t i = 0; i < sources.size(); ++i)
            if (mask >> i & 1u) {
                s[0].push_back(sources[i]);                     // one row reads all of them,
                if (i % 2) s[5 + i].push_back(sources[i]);      // a few rows one each,
                s[63].push_back(sources[i]);
            }
        if (!s[63].empty()) s[63].pop_back();                   // and the last row all but the largest
        for (U32 &row : s) std::sort(row.begin(), row.end());
        if (!check(n, {s}, {}, "exhaustive")) { std::printf("(subset %x)\n", mask); return false; }
    }
    return true;
}

static U32 range(uint32_t from, uint32_t count, uint32_t step = 1)
{
    U32 r;
    for (uint32_t i = 0; i < count; ++i) r.push_back(from + i * step);
    return r;
}

static bool directed(bool with_halo, unsigned long long &count)
{
    Net n{2000, 600, {}, 0};
    if (with_halo) {
        // neurons 1500 .. 1599 arrive by the receive buffer, neighbours in words that are NOT neighbours (1500 + i in word 7 * i mod 100)
        n.halo_word.assign(n.nn, NO_HALO);
        for (uint32_t i = 0; i < 100; ++i) n.halo_word[1500 + i] = (7 * i) % 100;
        n.n_halo = 100;
    }
    const uint32_t nn = n.nn, nc = n.nc;
    std::vector<Slice> s;
    std::vector<Expect> x;
    s.push_back(deal(range(0, 640), 10)); x.push_back({1, 10, 639});
    s.push_back(deal(range(37, 1024), 16)); x.push_back({1, 16, 1023});          // the window full, from a start that is no multiple of 64
    s.push_back(empty_slice()); x.push_back({0, 0, -1});                            // empty, in the middle
    s.push_back(deal(range(37, 1025), 16)); x.push_back({0, 17, -1});             // one source more
    {   // 1024 neurons in 16 full pieces with gaps of 6 between them
        U32 src;
        for (uint32_t u = 0; u < 16; ++u) for (uint32_t i = 0; i < 64; ++i) src.push_back(37 + u * 70 + i);
        s.push_back(deal(src, 16)); x.push_back({1, 16, 1023});
        src.push_back(37 + 16 * 70);                                                  // ... and a 17th piece of one word
        s.push_back(deal(src, 17)); x.push_back({0, 17, -1});
    }
    {   // trimmed pieces: three sources within a span of 40, sixteen times; the piece's words end at its last source
        U32 src;
        for (uint32_t u = 0; u < 16; ++u) for (uint32_t i : {0u, 10u, 39u}) src.push_back(5 + u * 90 + i);
        s.push_back(deal(src, 3)); x.push_back({1, 16, 15 * 64 + 39});
    }
    s.push_back(deal(range(nn + nc - 512, 512), 8)); x.push_back({1, 16, 1022});   // 512 cells up to the LAST cell: words 1022 / 1023
    s.push_back(deal(range(nn + nc - 513, 513), 9)); x.push_back({0, 17, -1});
    s.push_back(deal(range(nn + 3, 512), 8)); x.push_back({1, 16, 1022});
    {   // consecutive codes, three kinds: neurons nn - 3 .. nn - 1 | cells 0 .. 2, and the last cells | the receive buffer's first words
        U32 src = range(nn - 3, 6);
        for (uint32_t c : range(nn + nc - 2, 2)) src.push_back(c);
        Slice sl = deal(src, 4);
        sl[7] = {1500, 1501, 1515, nn - 1, nn};                                       // (with a halo: words 0, 7 and 5 -- the fourth piece)
        s.push_back(sl); x.push_back({1, 4, with_halo ? 3 * 64 + 7 : 3 * 64 + 2});
    }
    {   // the last cell of the array alone, and the last neuron alone
        Slice sl = empty_slice();
        sl[63] = {nn + nc - 1};
        s.push_back(sl); x.push_back({1, 1, 0});
        sl[63] = {nn - 1};
        s.push_back(sl); x.push_back({1, 1, 0});
    }
    s.push_back(deal(range(1450, 200), 4)); x.push_back({1, 4, -1});                  // through the halo's neurons
    s.push_back(deal(range(0, 17), 17)); x.push_back({1, 1, 16});                 // odd width: half a record of padding
    s.push_back(empty_slice()); x.push_back({0, 0, -1});                            // the LAST slice is empty
    count += s.size();
    return check(n, s, x, with_halo ? "directed, with a halo" : "directed");
}

static bool random_nets(unsigned long long &nets)
{
    std::mt19937 rng(20240611u);
    auto below = [&](uint32_t m) { return m ? (uint32_t)(rng() % m) : 0u; };
    auto shuffle = [&](U32 &v) { for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[below((uint32_t)i)]); };
    for (int t = 0; t < 400; ++t, ++nets) {
        Net n{1 + below(t % 3 ? 3000 : 90), t % 4 == 1 ? 0u : 1 + below(t % 5 ? 700 : 40), {}, 0};
        if (t % 2) {
            // a halo: some neurons, their words a random permutation (every word carries one neuron)
            const uint32_t count = 1 + below(std::min(n.nn, 300u));
            U32 who(n.nn), word(count);
            for (uint32_t i = 0; i < n.nn; ++i) who[i] = i;
            for (uint32_t i = 0; i < count; ++i) word[i] = i;
            if (t % 4 == 3) shuffle(who);       // (else: the first `count` neurons, a contiguous band)
            if (t % 8 >= 4) shuffle(word);
            n.halo_word.assign(n.nn, NO_HALO);
            for (uint32_t i = 0; i < count; ++i) n.halo_word[who[i]] = word[i];
            n.n_halo = count;
        }
        const uint32_t n_tot = n.nn + n.nc;
        std::vector<Slice> slices(1 + below(6));
        for (Slice &s : slices) {
            s = empty_slice();
            const uint32_t mix = below(6);
            if (mix == 0) continue;                                          // an empty slice
            // a band [base, base + reach) the rows draw from: of neurons, of cells, across the boundary, or everything
            uint32_t base, reach;
            if (mix == 1) { reach = 1 + below(std::min(n.nn, 1400u)); base = below(n.nn - reach + 1); }
            else if (mix == 2 && n.nc) { reach = 1 + below(std::min(n.nc, 600u)); base = n.nn + below(n.nc - reach + 1); }
            else if (mix == 3) { reach = 1 + below(std::min(n_tot, 700u)); base = n.nn > reach / 2 ? std::min(n.nn - reach / 2, n_tot - reach) : 0u; }
            else if (mix == 4) { reach = std::min(n_tot, 1024u + below(3)); base = below(n_tot - reach + 1); }
            else { reach = n_tot; base = 0; }
            const uint32_t longest = below(3) ? 1 + below(20) : 1 + below(60);
            for (U32 &row : s) {
                std::set<uint32_t> pick;
                const uint32_t len = below(4) ? below(longest + 1) : longest;
                for (uint32_t i = 0; i < len; ++i) pick.insert(base + below(reach));
                row.assign(pick.begin(), pick.end());
            }
        }
        if (!check(n, slices, {}, "random")) { std::printf("(network %d)\n", t); return false; }
    }
    return true;
}

int main()
{
    unsigned long long subsets = 0, directed_slices = 0, nets = 0;
    {
        // nn = 100, nc = 70, the receive buffer 80 words.  Around nn - 1 | nn: neurons 98, 99, cells 0, 1; a neuron piece's span end
        // seen from 36 (36 + 63 = 99, 36 + 64 = 100 is no neuron) and 35; a cell piece's span end seen from cell 0: cells 31, 32;
        // around nn + nc - 1 | halo_base: cells 68, 69 and the neurons in words 0, 1; the halo's span end: words 63, 64
        Net n{100, 70, U32(100, NO_HALO), 80};
        n.halo_word[10] = 0; n.halo_word[11] = 1; n.halo_word[3] = 63; n.halo_word[50] = 64;
        if (!exhaustive(n, {98, 99, 100, 101, 35, 36, 131, 132, 168, 169, 10, 11, 3, 50}, subsets)) return 1;
        // no cells: nn - 1 | halo_base
        Net m{100, 0, U32(100, NO_HALO), 80};
        m.halo_word[10] = 0; m.halo_word[11] = 1; m.halo_word[3] = 63; m.halo_word[50] = 64;
        if (!exhaustive(m, {98, 99, 35, 36, 10, 11, 3, 50}, subsets)) return 1;
    }
    if (!directed(false, directed_slices) || !directed(true, directed_slices)) return 1;
    if (!random_nets(nets)) return 1;
    std::printf("step image plan ok: %llu exhaustive subsets, %llu directed slices, %llu random networks, %llu slices in all\n", subsets,
                directed_slices, nets, g_slices);
    return 0;
}
