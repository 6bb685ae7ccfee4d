// The index arithmetic of a structural edit of a sparse graph (snn_graph_csr_edit_structure): where every entry of a merged row
// lands, computed per element with no serial chain.  Integer arithmetic only; plain C++ that host and device code share, and that
// tests/cpp/graph_merge_test.cpp includes alone.
//
// The edit list is sorted by (post, pre) with no pair twice (graph_pairs_last_wins of snn_graph_pairs.hpp: of a pair listed more
// than once the LAST occurrence is kept).  Every edit is resolved against the stored row: it INSERTS (connected, not stored), REMOVES (not
// connected, stored), REWEIGHS (connected, stored) or does nothing (not connected, not stored).  ins_before / rem_before are the
// exclusive prefix sums of the insert / remove flags over the sorted list, n_edits + 1 words each, so that the flag of edit t is
// x_before[t + 1] - x_before[t] and a span [lo, t) holds x_before[t] - x_before[lo] of them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <algorithm>

#if defined(__HIPCC__)
#define SNN_MERGE_FN __host__ __device__ inline
#else
#define SNN_MERGE_FN inline
#endif

namespace snn {

constexpr uint32_t GRAPH_MERGE_NONE = 0xFFFFFFFFu;          // "no edit" / "no old entry" (the value of GRAPH_CSR_NONE)

// the first k of [lo, hi) with a[k * stride] >= key, hi when there is none; a[lo * stride .. ] ascending.  stride 1: a sorted
// list; stride 64: the entries of one SELL-64 row
SNN_MERGE_FN uint32_t graph_merge_lower_bound(const uint32_t *a, uint32_t lo, uint32_t hi, uint32_t stride, uint32_t key)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[(size_t)mid * stride] < key) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

struct GraphMergeSpan { uint32_t lo, hi; };

// the edits of one row: the run of `post` in the sorted post list, by two binary searches
SNN_MERGE_FN GraphMergeSpan graph_merge_span(const uint32_t *edit_post, uint32_t n_edits, uint32_t post)
{
    GraphMergeSpan s;
    s.lo = graph_merge_lower_bound(edit_post, 0u, n_edits, 1u, post);
    s.hi = post == 0xFFFFFFFFu ? n_edits : graph_merge_lower_bound(edit_post, s.lo, n_edits, 1u, post + 1u);
    return s;
}

// what an edit does, from whether its pair is stored and whether it asks for an edge
SNN_MERGE_FN bool graph_merge_inserts(bool connected, bool stored) { return connected && !stored; }
SNN_MERGE_FN bool graph_merge_removes(bool connected, bool stored) { return !connected && stored; }

// old length - removes in the span + inserts in the span (a span removes stored entries only: the result is never negative)
SNN_MERGE_FN uint32_t graph_merge_row_length(uint32_t old_len, const uint32_t *ins_before, const uint32_t *rem_before, GraphMergeSpan s)
{
    return old_len - (rem_before[s.hi] - rem_before[s.lo]) + (ins_before[s.hi] - ins_before[s.lo]);
}

enum : uint32_t { GRAPH_MERGE_KEEP = 0u, GRAPH_MERGE_REWEIGH = 1u, GRAPH_MERGE_DROP = 2u };
struct GraphMergeOld { uint32_t at, edit, what; };

// Old entry j of a row, presynaptic index p: it moves down by the removes before it and up by the inserts before it.  `edit` is
// the edit of the span that names p (GRAPH_MERGE_NONE: none does, KEEP): a remove DROPs the entry (`at` means nothing then),
// anything else REWEIGHs it -- an edit that names a stored pair and does not remove it is connected.
SNN_MERGE_FN GraphMergeOld graph_merge_old_entry(const uint32_t *edit_pre, const uint32_t *ins_before, const uint32_t *rem_before,
                                                 GraphMergeSpan s, uint32_t j, uint32_t p)
{
    const uint32_t t = graph_merge_lower_bound(edit_pre, s.lo, s.hi, 1u, p);
    GraphMergeOld o;
    o.at = j - (rem_before[t] - rem_before[s.lo]) + (ins_before[t] - ins_before[s.lo]);
    o.edit = GRAPH_MERGE_NONE;
    o.what = GRAPH_MERGE_KEEP;
    if (t < s.hi && edit_pre[t] == p) {
        o.edit = t;
        o.what = rem_before[t + 1u] != rem_before[t] ? GRAPH_MERGE_DROP : GRAPH_MERGE_REWEIGH;
    }
    return o;
}

// does edit t insert?
SNN_MERGE_FN bool graph_merge_edit_inserts(const uint32_t *ins_before, uint32_t t) { return ins_before[t + 1u] != ins_before[t]; }

// An inserting edit t of the span, `smaller` = the old entries of the row with a smaller presynaptic index (a lower bound over the
// row): the inserts before it, plus those entries, minus the removes before it -- every remove before t names a smaller stored index.
SNN_MERGE_FN uint32_t graph_merge_insert_at(const uint32_t *ins_before, const uint32_t *rem_before, GraphMergeSpan s, uint32_t t,
                                            uint32_t smaller)
{
    return (ins_before[t] - ins_before[s.lo]) + smaller - (rem_before[t] - rem_before[s.lo]);
}

} // namespace snn
