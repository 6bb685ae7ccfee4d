// csrc/snn_graph_pairs.hpp on the host, included alone: the walk over the pair list of a graph call and the last-wins ordering,
// each against a naive restatement.
//   ordering: under both key orders against a std::map that is written one entry after another (the last occurrence of every
//             pair, the output strictly ascending by the key, `kept` = the number of distinct pairs) -- every list of at most 4
//             entries over 3 x 3 indices, and random lists of up to 5 000 entries over few pairs, so that most are repeats;
//   check:    against a loop that tests one pair after another in the order of the refusals -- every list of at most 3 entries
//             over pre in [0, 4) and post in [0, 7) for handles whose owned columns [q0, q0 + n_loc) start at 0 and above it
//             (post < q0: the unsigned wrap of post - q0) and end at and below n_neurons, with and without weights, and random
//             lists with one offender planted (or none).
#include <cmath>
#include <cstdio>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "snn_graph_pairs.hpp"

using namespace snn;

typedef std::vector<uint32_t> U32;

static bool check_order(const U32 &pre, const U32 &post, const char *what, unsigned long long id)
{
    for (GraphPairKey by : {GRAPH_KEY_PRE_POST, GRAPH_KEY_POST_PRE}) {
        std::map<std::pair<uint32_t, uint32_t>, size_t> last;          // key -> the position that wrote it last
        for (size_t k = 0; k < pre.size(); ++k)
            last[by == GRAPH_KEY_PRE_POST ? std::make_pair(pre[k], post[k]) : std::make_pair(post[k], pre[k])] = k;
        std::vector<uint64_t> order(7, 99u);                            // (whatever it held before)
        const size_t kept = graph_pairs_last_wins(pre.data(), post.data(), pre.size(), by, order);
        bool ok = kept == last.size() && order.size() >= kept;
        size_t t = 0;
        for (auto it = last.begin(); ok && it != last.end(); ++it, ++t) ok = order[t] == it->second;      // (a map iterates ascending)
        if (!ok) {
            std::printf("%s %llu, key order %d: %zu kept against %zu distinct pairs, or another position at %zu\n", what, id, (int)by, kept,
                        last.size(), t);
            return false;
        }
    }
    return true;
}

struct Shape { uint32_t n_tot, n_neurons, q0, n_loc; };

static GraphPairsCheck check_naive(const U32 &pre, const U32 &post, const float *w, const uint8_t *on, const Shape &s)
{
    GraphPairsCheck r{pre.size(), GRAPH_PAIR_FINE, true};
    for (size_t k = 0; k < pre.size(); ++k) {
        GraphPairFault why = GRAPH_PAIR_FINE;
        if (pre[k] >= s.n_tot) why = GRAPH_PAIR_PRE_RANGE;
        else if (post[k] >= s.n_neurons) why = GRAPH_PAIR_POST_RANGE;
        else if (post[k] < s.q0 || post[k] >= s.q0 + s.n_loc) why = GRAPH_PAIR_POST_NOT_OWNED;
        else if (w && on[k] && std::isnan(w[k])) why = GRAPH_PAIR_NAN_WEIGHT;
        if (why != GRAPH_PAIR_FINE) { r.at = k; r.why = why; return r; }
    }
    for (size_t k = 1; k < pre.size(); ++k)
        if (std::make_pair(pre[k - 1], post[k - 1]) >= std::make_pair(pre[k], post[k])) r.ascending = false;
    return r;
}

static bool check_list(const U32 &pre, const U32 &post, const float *w, const uint8_t *on, const Shape &s, const char *what, unsigned long long id)
{
    const GraphPairsCheck got = graph_pairs_check(pre.data(), post.data(), w, on, pre.size(), s.n_tot, s.n_neurons, s.q0, s.n_loc);
    const GraphPairsCheck want = check_naive(pre, post, w, on, s);
    if (got.at == want.at && got.why == want.why && (want.why != GRAPH_PAIR_FINE || got.ascending == want.ascending)) return true;
    std::printf("%s %llu (q0 %u, n_loc %u): position %zu reason %u ascending %d, the loop says %zu %u %d\n", what, id, s.q0, s.n_loc, got.at,
                (unsigned)got.why, (int)got.ascending, want.at, (unsigned)want.why, (int)want.ascending);
    return false;
}

int main()
{
    std::mt19937 rng(20240611u);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    // ---- the ordering, exhaustive: lists of 0 .. 4 entries over 3 x 3 pairs ----
    unsigned long long orders = 0;
    for (uint32_t n = 0, lists = 1; n <= 4u; ++n, lists *= 9u)
        for (uint32_t code = 0; code < lists; ++code, ++orders) {
            U32 pre(n), post(n);
            for (uint32_t k = 0, c = code; k < n; ++k, c /= 9u) { pre[k] = c % 9u / 3u; post[k] = c % 3u; }
            if (!check_order(pre, post, "ordering, exhaustive", orders)) return 1;
        }
    // ---- the ordering, random: many repeats; indices with the top bit set, so that the key is compared without a sign ----
    unsigned long long repeats = 0;
    for (uint32_t round = 0; round < 200u; ++round) {
        const uint32_t n = round < 2u ? round : 1u + below(5000u), span_pre = 1u + below(40u), span_post = 1u + below(40u);
        const uint32_t base = round % 4u == 3u ? 0xFFFFFF00u : 0u;
        U32 pre(n), post(n);
        for (uint32_t k = 0; k < n; ++k) { pre[k] = base + below(span_pre); post[k] = base + below(span_post); }
        if (!check_order(pre, post, "ordering, random", round)) return 1;
        std::vector<uint64_t> order;
        repeats += n - graph_pairs_last_wins(pre.data(), post.data(), n, GRAPH_KEY_POST_PRE, order);
    }
    if (orders != 1 + 9 + 81 + 729 + 6561 || repeats < 100000) { std::printf("%llu orderings, %llu repeats\n", orders, repeats); return 1; }
    // ---- the check, exhaustive: n_tot = 3 (pre 3 is out of range), n_neurons = 5 (post 5, 6 are), owned columns as below ----
    const Shape shapes[] = {{3, 5, 0, 5}, {3, 5, 0, 2}, {3, 5, 2, 2}, {3, 5, 2, 3}, {3, 5, 4, 1}, {3, 5, 1, 0}, {3, 5, 0xFFFFFFFEu, 1}};
    const float absent = std::nanf(""), weights[3] = {1.0f, absent, -0.0f};
    unsigned long long lists_checked = 0, reasons[5] = {0, 0, 0, 0, 0};
    for (const Shape &s : shapes)
        for (uint32_t n = 0, lists = 1; n <= 3u; ++n, lists *= 28u)
            for (uint32_t code = 0; code < lists; ++code) {
                U32 pre(n), post(n);
                for (uint32_t k = 0, c = code; k < n; ++k, c /= 28u) { pre[k] = c % 28u / 7u; post[k] = c % 7u; }
                if (!check_list(pre, post, nullptr, nullptr, s, "check without weights", lists_checked)) return 1;
                for (uint32_t flags = 0; flags < (1u << n); ++flags, ++lists_checked) {          // which pairs are connected; pair 1 is NaN
                    const uint8_t on[3] = {(uint8_t)(flags & 1u), (uint8_t)(flags & 2u), (uint8_t)(flags >> 2)};
                    if (!check_list(pre, post, weights, on, s, "check with weights", lists_checked)) return 1;
                    ++reasons[graph_pairs_check(pre.data(), post.data(), weights, on, n, s.n_tot, s.n_neurons, s.q0, s.n_loc).why];
                }
            }
    for (int why = 0; why < 5; ++why)
        if (!reasons[why]) { std::printf("no exhaustive list is refused for reason %d\n", why); return 1; }
    // ---- the check, random: long lists, ascending or with repeats, one offender (or none) planted anywhere ----
    unsigned long long ascending_seen = 0, refused = 0;
    for (uint32_t round = 0; round < 300u; ++round) {
        const Shape s = {40u + below(40u), 30u, below(10u), 1u + below(20u)};
        const uint32_t n = below(2000u);
        U32 pre(n), post(n);
        std::vector<float> w(n);
        std::vector<uint8_t> on(n);
        for (uint32_t k = 0; k < n; ++k) {
            pre[k] = below(s.n_tot); post[k] = s.q0 + below(s.n_loc); w[k] = below(50u) ? (float)k : absent; on[k] = !std::isnan(w[k]) || below(2u);
            if (std::isnan(w[k]) && round % 3u) on[k] = 0;                       // (a NaN of a pair that is not connected is not looked at)
        }
        if (round % 2u) {                                                       // strictly ascending by (pre, post): sorted, no pair twice
            std::vector<uint64_t> order;
            const size_t kept = graph_pairs_last_wins(pre.data(), post.data(), n, GRAPH_KEY_PRE_POST, order);
            U32 p(kept), q(kept);
            for (size_t t = 0; t < kept; ++t) { p[t] = pre[order[t]]; q[t] = post[order[t]]; }
            pre.swap(p); post.swap(q);
            if (round % 4u == 1u && kept > 1) { post[kept - 1] = post[kept - 2]; pre[kept - 1] = pre[kept - 2]; }      // ... but for the last pair
        }
        if (round % 5u == 0u && !pre.empty()) {
            const uint32_t k = below((uint32_t)pre.size());
            switch (round / 5u % 4u) {
            case 0: pre[k] = s.n_tot + below(3u); break;
            case 1: post[k] = s.n_neurons + below(3u); break;
            case 2: post[k] = s.q0 ? s.q0 - 1u : s.q0 + s.n_loc; break;
            default: post[k] = s.q0 + s.n_loc; break;
            }
        }
        if (!check_list(pre, post, w.data(), on.data(), s, "check, random", round)) return 1;
        const GraphPairsCheck r = graph_pairs_check(pre.data(), post.data(), w.data(), on.data(), pre.size(), s.n_tot, s.n_neurons, s.q0, s.n_loc);
        ascending_seen += r.why == GRAPH_PAIR_FINE && r.ascending && pre.size() > 1;
        refused += r.why != GRAPH_PAIR_FINE;
    }
    if (ascending_seen < 20 || refused < 50 || refused > 250) {
        std::printf("the random lists are not the mix that was meant: %llu ascending, %llu refused\n", ascending_seen, refused);
        return 1;
    }
    std::printf("graph pairs ok: %llu orderings and 200 random lists under both key orders, %llu exhaustive checks, 300 random lists\n", orders,
                lists_checked);
    return 0;
}
