// The pair list of a graph call (snn_graph_lookup / _edit and their sparse twins, snn_graph_csr_edit_structure) on the host: the
// walk over its arguments and the order its entries are applied in.  Plain C++, no HIP and no handle; tests/cpp/graph_pairs_test.cpp
// includes it alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <algorithm>

namespace snn {

// Why a pair is refused, in the order one pair is held to them: pre is not below n_tot; post is not below n_neurons; post is outside
// [q0, q0 + n_loc), the columns (rows of a sparse graph) the handle owns; a connected pair carries a NaN weight.
enum GraphPairFault : uint32_t { GRAPH_PAIR_FINE = 0u, GRAPH_PAIR_PRE_RANGE, GRAPH_PAIR_POST_RANGE, GRAPH_PAIR_POST_NOT_OWNED, GRAPH_PAIR_NAN_WEIGHT };

struct GraphPairsCheck {
    size_t at;                     // the first offending position (n when there is none)
    GraphPairFault why;
    bool ascending;                // strictly, by (pre, post): no pair twice.  Means nothing when a pair is refused
};

// The first pair that is refused, before any later one.  weights == nullptr: a lookup, which has no weights and no NaN test
// (`connected` is not read then).
inline GraphPairsCheck graph_pairs_check(const uint32_t *pre, const uint32_t *post, const float *weights, const uint8_t *connected,
                                         size_t n, uint32_t n_tot, uint32_t n_neurons, uint32_t q0, uint32_t n_loc)
{
    GraphPairsCheck r{n, GRAPH_PAIR_FINE, true};
    for (size_t k = 0; k < n; ++k) {
        if (pre[k] >= n_tot || post[k] - q0 >= n_loc) {          // (post < q0 wraps to a large number)
            r.at = k;
            r.why = pre[k] >= n_tot ? GRAPH_PAIR_PRE_RANGE : post[k] >= n_neurons ? GRAPH_PAIR_POST_RANGE : GRAPH_PAIR_POST_NOT_OWNED;
            return r;
        }
        if (weights && connected[k] && weights[k] != weights[k]) {
            r.at = k;
            r.why = GRAPH_PAIR_NAN_WEIGHT;
            return r;
        }
        if (k && (pre[k] < pre[k - 1] || (pre[k] == pre[k - 1] && post[k] <= post[k - 1]))) r.ascending = false;
    }
    return r;
}

enum GraphPairKey { GRAPH_KEY_PRE_POST, GRAPH_KEY_POST_PRE };        // which index sorts first

// "As if one after another": order[0 .. kept) = the positions in the call of the entries that count, ascending by the key -- of a
// pair listed more than once the LAST occurrence.  `order` is any vector of uint64_t; returns kept.
template <typename Vec>
inline size_t graph_pairs_last_wins(const uint32_t *pre, const uint32_t *post, size_t n, GraphPairKey by, Vec &order)
{
    const uint32_t *major = by == GRAPH_KEY_PRE_POST ? pre : post, *minor = by == GRAPH_KEY_PRE_POST ? post : pre;
    order.resize(n);
    for (size_t k = 0; k < n; ++k) order[k] = k;
    auto key = [&](uint64_t k) { return ((uint64_t)major[k] << 32) | minor[k]; };
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return key(a) != key(b) ? key(a) < key(b) : a < b; });
    size_t kept = 0;
    for (size_t k = 0; k < n; ++k)
        if (k + 1 == n || key(order[k + 1]) != key(order[k])) order[kept++] = order[k];
    return kept;
}

} // namespace snn
