"""Graph edits of more pairs than one launch takes (2^20: the device lists of a call hold no more, so the list goes up hop by
hop): snn_graph_edit, snn_graph_csr_edit and snn_graph_csr_edit_structure, held bit for bit to numpy with last-wins semantics and
to the dense twin.  The lookups of that length are in test_gpu_graph_query*.py ("three hops of the staging lists")."""
import numpy as np
import pytest

import test_gpu_connect_rule_csr as csr_tests
import test_gpu_graph_query as dense_tests
import test_gpu_graph_query_csr as query_tests
import test_gpu_graph_restructure_csr as structure_tests

pytestmark = pytest.mark.gpu

BAD_ARG = 11
HOP = 1 << 20
RAGGED, LONG = dense_tests.RAGGED, dense_tests.LONG
handle, pattern, all_pairs = dense_tests.handle, dense_tests.pattern, dense_tests.all_pairs
long_graph, edge_pairs, same_bits, digest = query_tests.long_graph, query_tests.edge_pairs, query_tests.same_bits, query_tests.digest
csr_of, assert_csr = csr_tests.csr_of, csr_tests.assert_csr


def last_of_every_pair(p, q, nn):
    """positions in the call of the entries that count: of a pair listed more than once the last one"""
    key = p.astype(np.int64) * nn + q
    _, first_from_the_end = np.unique(key[::-1], return_index=True)
    return key.size - 1 - first_from_the_end


def apply_last_wins(w, c, p, q, v, on):
    """edit_weight one pair after another on host matrices [n_tot, n_neurons], without the loop"""
    w, c = w.copy(), c.copy()
    k = last_of_every_pair(p, q, c.shape[1])
    c[p[k], q[k]] = on[k]
    w[p[k], q[k]] = np.where(on[k], v[k], np.float32(0))
    return w, c


# ---- 1. dense: every pair of LONG, each once; ascending, then shuffled with repeats appended ---------------------------------------
def test_dense_edit_of_every_pair_of_the_long_network(snn):
    dn = handle(snn, LONG)
    w, c = dense_tests.long_pattern()
    dn.set_graph_rows(0, w, c)
    pre, post = all_pairs(dn)                           # ascending by (pre, post): the path without the sort
    assert pre.size > 2 * HOP and pre.size % HOP != 0
    rng = np.random.default_rng(23)
    v = rng.uniform(-3.0, 3.0, pre.size).astype(np.float32)
    on = rng.random(pre.size) < 0.7
    dn.graph_edit(pre, post, v, on)
    w, c = apply_last_wins(w, c, pre, post, v, on)
    gw, gc = dn.get_graph_rows(0, dn.n_tot)
    assert np.array_equal(gc, c) and np.array_equal(gw.view(np.uint32), w.view(np.uint32)), "after the ascending call"
    assert (c != dense_tests.long_pattern()[1]).any()
    # shuffled, and 3 000 of the pairs again at the end (some of those twice): the last occurrence wins
    order = rng.permutation(pre.size)
    again = rng.integers(0, pre.size, 3000)
    again[2000:2500] = again[:500]
    pick = np.concatenate([order, again])
    p, q = pre[pick], post[pick]
    v = rng.uniform(-3.0, 3.0, p.size).astype(np.float32)
    on = rng.random(p.size) < 0.5
    dn.graph_edit(p, q, v, on)
    w, c = apply_last_wins(w, c, p, q, v, on)
    k = order.size + 2000                               # a pair listed three times: the value of the third
    assert on[k] == (c[p[k], q[k]] != 0) and (not on[k] or w[p[k], q[k]] == v[k])
    gw, gc = dn.get_graph_rows(0, dn.n_tot)
    assert np.array_equal(gc, c) and np.array_equal(gw.view(np.uint32), w.view(np.uint32)), "after the shuffled call"
    dn.close()


# ---- 2. sparse, in place -------------------------------------------------------------------------------------------------------------
def test_sparse_edit_of_stored_edges_repeated_past_a_hop(snn):
    """the resolve pass crosses a hop, and the one launch of the write pass selects entries of the second hop's slots"""
    w, c = pattern(RAGGED)
    dn = handle(snn, RAGGED, csr=True)
    csr = csr_of(w, c, dn.owned)
    dn.set_graph_csr(*csr)
    structure = dn.graph_csr_structure()
    pre, post = edge_pairs(csr, dn.owned)
    rng = np.random.default_rng(29)
    edges = rng.integers(0, pre.size, HOP + 1500)
    values = rng.uniform(-3.0, 3.0, edges.size).astype(np.float32)
    # the same list with one absent pair past the first hop: refused, that position named, nothing written
    before = digest(dn)
    absent = np.argwhere(c == 0)[77].astype(np.uint32)
    at = HOP + 613
    p, q = pre[edges].copy(), post[edges].copy()
    p[at], q[at] = absent
    with pytest.raises(snn.SnnError) as err:
        dn.graph_edit(p, q, values)
    assert err.value.code == BAD_ARG and f"pair {at} (pre {absent[0]}, post {absent[1]}): no stored edge" in str(err.value), str(err.value)
    assert digest(dn) == before
    dn.graph_edit(pre[edges], post[edges], values)
    last = np.full(pre.size, -1, np.int64)
    np.maximum.at(last, edges, np.arange(edges.size))
    assert (last >= 0).all() and (last >= HOP).any(), "every edge is listed, some for the last time past the first hop"
    want = values[last]
    assert same_bits(dn.get_graph_csr(), want)
    for x, y in zip(dn.graph_csr_structure(), structure):
        assert np.array_equal(x, y)
    dn.close()


@pytest.mark.parametrize("ascending", [True, False], ids=["ascending", "edge_order"])
def test_sparse_edit_of_every_stored_edge_of_the_long_network(snn, ascending):
    """the write pass crosses hops: by (pre, post) without the sort, in the edge order (by post) with the slots selected"""
    w, c = long_graph()
    dn = handle(snn, LONG, csr=True)
    csr = csr_of(w, c, dn.owned)
    dn.set_graph_csr(*csr)
    pre, post = edge_pairs(csr, dn.owned)
    assert pre.size > 2 * HOP and pre.size % HOP != 0
    edges = np.lexsort((post, pre)) if ascending else np.arange(pre.size)
    values = np.random.default_rng(31).uniform(-3.0, 3.0, pre.size).astype(np.float32)
    dn.graph_edit(pre[edges], post[edges], values)
    want = np.empty(pre.size, np.float32)
    want[edges] = values
    assert same_bits(dn.get_graph_csr(), want)
    dn.close()


# ---- 3. sparse, structure included -----------------------------------------------------------------------------------------------------
def test_structural_edit_of_more_entries_than_a_hop(snn):
    w, c = structure_tests.ragged_graph()
    sparse, dense = handle(snn, RAGGED, csr=True), handle(snn, RAGGED)
    sparse.set_graph_csr(*csr_of(w, c, sparse.owned))
    dense.set_graph_rows(0, w, c)
    rng = np.random.default_rng(37)
    n = HOP + 2500
    p = rng.integers(0, c.shape[0], n).astype(np.uint32)          # every pair of the matrix, hundreds of times each
    q = rng.integers(0, c.shape[1], n).astype(np.uint32)
    q[rng.random(n) < 0.02] = 3                                    # (the row without an incoming edge gets its share)
    v = rng.uniform(-3.0, 3.0, n).astype(np.float32)
    on = rng.random(n) < 0.5
    w1, c1 = apply_last_wins(w, c, p, q, v, on)
    k = last_of_every_pair(p, q, c.shape[1])
    stored = c[p[k], q[k]] != 0
    assert (on[k] & ~stored).sum() > 100 and (~on[k] & stored).sum() > 100 and (on[k] & stored).sum() > 100 and (~on[k] & ~stored).any(), \
        "inserts, removes, overwrites and stay-absent"
    assert (k >= HOP).any() and (k < HOP).any()
    sparse.graph_edit(p, q, v, on, structure=True)
    dense.graph_edit(p, q, v, on)
    want = csr_of(w1, c1, sparse.owned)
    assert sparse._nnz == want[1].size
    assert_csr(sparse, want, "after the long call")
    gw, gc = dense.get_graph_rows(0, dense.n_tot)
    assert np.array_equal(gc, c1) and np.array_equal(gw.view(np.uint32), w1.view(np.uint32))
    structure_tests.assert_equals_the_dense_twin(sparse, dense, p, q)
    sparse.close()
    dense.close()
