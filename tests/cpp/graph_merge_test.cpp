// csrc/snn_graph_merge.hpp on the host, included alone: a sparse graph (SELL-64 rows, as the device holds them) and a list of
// edits merged twice -- by the header's formulas, statement for statement as k_graph_merge_count / k_graph_merge_fill use them
// (sorted list with last-wins, resolve, prefix sums of the insert / remove flags, every element placed on its own), and by a naive
// std::map that applies the edits one after another -- and compared: row lengths, presynaptic indices, weights, the source of
// every new edge; every output position written exactly once; rows strictly ascending.
//   exhaustive: every old row over a universe of 6 presynaptic indices x every edit list of at most 3 edits (index, kind), so
//               duplicates of every kind and order occur;
//   random:     1 .. 70 rows (two slices) of 0 .. 300 entries, 0 .. 200 edits per row, shuffled over the call, with repeats.
#include <cinttypes>
#include <cstdio>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "snn_graph_merge.hpp"
#include "snn_graph_pairs.hpp"

using namespace snn;

struct Edit { uint32_t pre, post; float w; bool on; };
struct Entry { uint32_t pre; float w; uint32_t src; };
typedef std::vector<std::vector<std::pair<uint32_t, float>>> Rows;

static bool same(const Entry &a, const Entry &b) { return a.pre == b.pre && a.w == b.w && a.src == b.src; }

// the stored rows as SELL-64: entry k of row r at slice_ptr[r / 64] + 64 k + r % 64
struct Sell {
    std::vector<uint32_t> slice_ptr, pre, row_len;
    std::vector<float> w;
    explicit Sell(const Rows &rows)
    {
        const size_t n_slices = (rows.size() + 63) / 64;
        row_len.assign(n_slices * 64, 0);
        for (size_t r = 0; r < rows.size(); ++r) row_len[r] = (uint32_t)rows[r].size();
        slice_ptr.assign(n_slices + 1, 0);
        for (size_t s = 0; s < n_slices; ++s) {
            uint32_t width = 0;
            for (size_t r = s * 64; r < s * 64 + 64; ++r) width = std::max(width, row_len[r]);
            slice_ptr[s + 1] = slice_ptr[s] + width * 64;
        }
        pre.assign(slice_ptr[n_slices], 0xFFFFFFFFu);
        w.assign(slice_ptr[n_slices], 0.0f);
        for (size_t r = 0; r < rows.size(); ++r)
            for (size_t k = 0; k < rows[r].size(); ++k) {
                pre[slot(r, k)] = rows[r][k].first;
                w[slot(r, k)] = rows[r][k].second;
            }
    }
    uint32_t slot(size_t r, size_t k) const { return slice_ptr[r / 64] + (uint32_t)(64 * k + r % 64); }
};

// the merge as the device does it; false (and a line on stdout) when a position is written twice, never, or out of range
static bool merge_by_formulas(const Rows &rows, const std::vector<Edit> &edits, std::vector<std::vector<Entry>> &out)
{
    const uint32_t n_rows = (uint32_t)rows.size();
    const Sell g(rows);
    std::vector<uint32_t> call_pre(edits.size()), call_post(edits.size());
    for (size_t k = 0; k < edits.size(); ++k) { call_pre[k] = edits[k].pre; call_post[k] = edits[k].post; }
    std::vector<uint64_t> order;
    const uint32_t m = (uint32_t)graph_pairs_last_wins(call_pre.data(), call_post.data(), edits.size(), GRAPH_KEY_POST_PRE, order);
    std::vector<uint32_t> e_pre(m), e_post(m), slot(m), ins(m + 1, 0), rem(m + 1, 0);
    std::vector<float> e_w(m);
    for (uint32_t t = 0; t < m; ++t) {
        const Edit &e = edits[order[t]];
        e_pre[t] = e.pre; e_post[t] = e.post; e_w[t] = e.w;
        if (t && !(e_post[t - 1] < e_post[t] || (e_post[t - 1] == e_post[t] && e_pre[t - 1] < e_pre[t]))) {
            std::printf("the ordered list is not strictly ascending at %" PRIu32 "\n", t);
            return false;
        }
        // the resolve pass (k_graph_csr_find): the entry of the pair, or none
        const uint32_t r = e.post, len = g.row_len[r], base = g.slot(r, 0);
        const uint32_t k = len ? graph_merge_lower_bound(g.pre.data() + base, 0u, len, 64u, e.pre) : 0u;
        const bool stored = k < len && g.pre[base + 64u * k] == e.pre;
        slot[t] = stored ? base + 64u * k : GRAPH_MERGE_NONE;
        ins[t] = graph_merge_inserts(e.on, stored) ? 1u : 0u;
        rem[t] = graph_merge_removes(e.on, stored) ? 1u : 0u;
    }
    for (uint32_t t = 0, i = 0, d = 0; t <= m; ++t) {       // exclusive prefix sums, m + 1 words
        const uint32_t fi = t < m ? ins[t] : 0u, fd = t < m ? rem[t] : 0u;
        ins[t] = i; rem[t] = d;
        i += fi; d += fd;
    }
    std::vector<uint32_t> new_ptr(n_rows + 1, 0);
    for (uint32_t r = 0; r < n_rows; ++r) {
        const GraphMergeSpan s = graph_merge_span(e_post.data(), m, r);
        new_ptr[r + 1] = new_ptr[r] + graph_merge_row_length(g.row_len[r], ins.data(), rem.data(), s);
    }
    const uint32_t nnz = new_ptr[n_rows];
    std::vector<Entry> flat(nnz);
    std::vector<uint32_t> written(nnz, 0);
    auto put = [&](uint32_t at, uint32_t row, Entry e) {
        if (at < new_ptr[row] || at >= new_ptr[row + 1]) { std::printf("row %" PRIu32 ": position %" PRIu32 " outside the row\n", row, at); return false; }
        flat[at] = e;
        ++written[at];
        return true;
    };
    for (uint32_t r = 0; r < n_rows; ++r) {
        const GraphMergeSpan s = graph_merge_span(e_post.data(), m, r);
        const uint32_t len = g.row_len[r], base = g.slot(r, 0), at = new_ptr[r];
        for (uint32_t j = 0; j < len; ++j) {
            const uint32_t entry = base + 64u * j, p = g.pre[entry];
            const GraphMergeOld o = graph_merge_old_entry(e_pre.data(), ins.data(), rem.data(), s, j, p);
            if (o.what == GRAPH_MERGE_DROP) continue;
            const bool kept = o.what == GRAPH_MERGE_KEEP;
            if (!put(at + o.at, r, Entry{p, kept ? g.w[entry] : e_w[o.edit], kept ? entry : GRAPH_MERGE_NONE})) return false;
        }
        for (uint32_t t = s.lo; t < s.hi; ++t) {
            if (!graph_merge_edit_inserts(ins.data(), t)) continue;
            const uint32_t smaller = len ? graph_merge_lower_bound(g.pre.data() + base, 0u, len, 64u, e_pre[t]) : 0u;
            if (!put(at + graph_merge_insert_at(ins.data(), rem.data(), s, t, smaller), r, Entry{e_pre[t], e_w[t], GRAPH_MERGE_NONE})) return false;
        }
    }
    for (uint32_t k = 0; k < nnz; ++k)
        if (written[k] != 1) { std::printf("position %" PRIu32 " written %" PRIu32 " times\n", k, written[k]); return false; }
    out.assign(n_rows, {});
    for (uint32_t r = 0; r < n_rows; ++r) out[r].assign(flat.begin() + new_ptr[r], flat.begin() + new_ptr[r + 1]);
    return true;
}

// the edits one after another on a map: Some(w) sets or inserts (a new edge either way: no source), None erases
static void merge_naive(const Rows &rows, const std::vector<Edit> &edits, std::vector<std::vector<Entry>> &out)
{
    const Sell g(rows);
    std::vector<std::map<uint32_t, Entry>> maps(rows.size());
    for (size_t r = 0; r < rows.size(); ++r)
        for (size_t k = 0; k < rows[r].size(); ++k) maps[r][rows[r][k].first] = Entry{rows[r][k].first, rows[r][k].second, g.slot(r, k)};
    for (const Edit &e : edits) {
        if (e.on) maps[e.post][e.pre] = Entry{e.pre, e.w, GRAPH_MERGE_NONE};
        else maps[e.post].erase(e.pre);
    }
    out.assign(rows.size(), {});
    for (size_t r = 0; r < rows.size(); ++r)
        for (const auto &kv : maps[r]) out[r].push_back(kv.second);
}

static bool check(const Rows &rows, const std::vector<Edit> &edits, const char *what, unsigned long long id)
{
    std::vector<std::vector<Entry>> got, want;
    if (!merge_by_formulas(rows, edits, got)) { std::printf("%s %llu: the merge is not a placement\n", what, id); return false; }
    merge_naive(rows, edits, want);
    for (size_t r = 0; r < rows.size(); ++r) {
        bool ok = got[r].size() == want[r].size();
        for (size_t k = 0; ok && k < got[r].size(); ++k) ok = same(got[r][k], want[r][k]) && (k == 0 || got[r][k - 1].pre < got[r][k].pre);
        if (!ok) {
            std::printf("%s %llu: row %zu differs: %zu entries against %zu\n", what, id, r, got[r].size(), want[r].size());
            return false;
        }
    }
    return true;
}

int main()
{
    // ---- exhaustive: one row over 6 presynaptic indices, edit lists of 0 .. 3 edits of 12 kinds (index x connected) ----
    unsigned long long cases = 0;
    for (uint32_t old = 0; old < 64u; ++old) {
        Rows rows(1);
        for (uint32_t p = 0; p < 6u; ++p)
            if (old >> p & 1u) rows[0].push_back({p, 10.0f + (float)p});
        for (uint32_t n = 0; n <= 3u; ++n) {
            uint32_t lists = 1;
            for (uint32_t k = 0; k < n; ++k) lists *= 12u;
            for (uint32_t code = 0; code < lists; ++code) {
                std::vector<Edit> edits;
                for (uint32_t k = 0, c = code; k < n; ++k, c /= 12u) edits.push_back(Edit{c % 12u % 6u, 0u, 100.0f + (float)k, c % 12u >= 6u});
                if (!check(rows, edits, "exhaustive", cases)) return 1;
                ++cases;
            }
        }
    }
    if (cases != 64ull * (1 + 12 + 144 + 1728)) { std::printf("%llu exhaustive cases\n", cases); return 1; }
    // ---- random: rows of two slices, long rows, long spans, shuffled calls with repeats ----
    std::mt19937 rng(20240607u);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    unsigned long long inserted = 0, removed = 0, longest_row = 0, longest_span = 0;
    for (uint32_t round = 0; round < 150u; ++round) {
        const uint32_t n_rows = round < 4u ? 1u : 1u + below(70u), universe = round % 3u ? 512u : 320u;
        Rows rows(n_rows);
        std::vector<Edit> edits;
        for (uint32_t r = 0; r < n_rows; ++r) {
            const uint32_t len = below(4u) ? below(301u) : 0u;
            std::vector<uint8_t> in(universe, 0);
            for (uint32_t k = 0; k < len;) {                 // exactly len distinct indices
                const uint32_t p = below(universe);
                k += in[p] ? 0u : 1u;
                in[p] = 1;
            }
            for (uint32_t p = 0; p < universe; ++p)
                if (in[p]) rows[r].push_back({p, (float)(r * 1000u + p)});
            const uint32_t n_edits = below(3u) ? below(201u) : 0u;
            longest_row = std::max<unsigned long long>(longest_row, rows[r].size());
            longest_span = std::max<unsigned long long>(longest_span, n_edits);
            for (uint32_t k = 0; k < n_edits; ++k) {
                // stored and absent pairs alike; every fourth a repeat of an earlier edit's pair with another kind
                Edit e{below(universe), r, -1.0f - (float)edits.size(), below(2u) != 0};
                if (k % 4u == 3u && !edits.empty()) { const Edit &again = edits[below((uint32_t)edits.size())]; e.pre = again.pre; e.post = again.post; }
                edits.push_back(e);
            }
        }
        for (size_t k = edits.size(); k > 1; --k) std::swap(edits[k - 1], edits[below((uint32_t)k)]);
        for (size_t k = 0; k < edits.size(); ++k) edits[k].w = -1.0f - (float)k;       // (the weight names the position in the call)
        if (!check(rows, edits, "random", round)) return 1;
        std::vector<std::vector<Entry>> after;
        merge_naive(rows, edits, after);
        for (uint32_t r = 0; r < n_rows; ++r) {
            size_t kept = 0;
            for (const Entry &e : after[r]) kept += e.src != GRAPH_MERGE_NONE;
            removed += rows[r].size() - kept;
            inserted += after[r].size() - kept;
        }
    }
    if (longest_row <= 256 || longest_span <= 128 || inserted < 1000 || removed < 1000) {
        std::printf("the random cases are thinner than meant: %llu %llu %llu %llu\n", longest_row, longest_span, inserted, removed);
        return 1;
    }
    std::printf("graph merge ok: %llu exhaustive cases, 150 random graphs\n", cases);
    return 0;
}
