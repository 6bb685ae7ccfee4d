"""snn_graph_csr_lookup / _edit / _incoming / _outgoing under the allocation-failure hook (snn_debug_fail_alloc_at), as
tests/test_gpu_alloc_failures_connect_spec.py walks the connect calls: whichever allocation of a call fails -- a staging list on
the device, the host table that orders an unsorted edit -- the outcome is a status code with a message, the graph (structure and
weights) is readable and unchanged, and the same call succeeds afterwards with the same answer."""
import numpy as np
import pytest

import test_gpu_alloc_failures_connect_spec as model
import test_gpu_connect_rule_csr as csr_tests
import test_gpu_graph_query_csr as query_tests

pytestmark = pytest.mark.gpu

RAGGED = query_tests.RAGGED


def fresh_of(snn):
    return lambda: csr_tests.patterned(snn, RAGGED)[0]


def stored_edges(snn):
    dn, w, c = csr_tests.patterned(snn, RAGGED)
    csr = csr_tests.csr_of(w, c, dn.owned)
    pre, post = query_tests.edge_pairs(csr, dn.owned)
    dn.close()
    return csr, pre, post


def walk_reader(snn, call, allocations):
    """a call that changes nothing: every failure leaves the graph alone, and every answer given is the same one"""
    answers = []
    failed, total, messages = model.walk(snn, fresh_of(snn), lambda dn: answers.append(call(dn)), csr_tests.read, allocations)
    assert failed == total, (failed, total, messages)
    assert len(answers) == total + 1
    for answer in answers[1:]:
        assert all(query_tests.same_bits(x, y) for x, y in zip(answer, answers[0]))
    return answers[0]


def test_every_allocation_of_a_lookup_may_fail(snn):
    csr, pre, post = stored_edges(snn)
    p = np.concatenate([pre[::7], np.arange(56, dtype=np.uint32)])
    q = np.concatenate([post[::7], np.full(56, 49, np.uint32)])
    w, on = walk_reader(snn, lambda dn: dn.graph_lookup(p, q), 4)
    assert on[:pre[::7].size].all() and query_tests.same_bits(w[:pre[::7].size], csr[2][::7])


def test_every_allocation_of_a_line_query_may_fail(snn):
    csr, pre, post = stored_edges(snn)
    index, w = walk_reader(snn, lambda dn: dn.graph_incoming(17), 2)
    assert np.array_equal(index, pre[post == 17]) and query_tests.same_bits(w, csr[2][post == 17])
    index, w = walk_reader(snn, lambda dn: dn.graph_outgoing(52), 2)
    assert np.array_equal(index, post[pre == 52]) and query_tests.same_bits(w, csr[2][pre == 52])


@pytest.mark.parametrize("ascending", [False, True], ids=["shuffled", "ascending"])
def test_every_allocation_of_an_edit_may_fail(snn, ascending):
    csr, pre, post = stored_edges(snn)
    rng = np.random.default_rng(4)
    edges = np.unique(rng.choice(pre.size, 200, replace=False))
    edges = edges[np.lexsort((post[edges], pre[edges]))] if ascending else np.concatenate([edges, edges[:20]])[rng.permutation(edges.size + 20)]
    values = rng.uniform(-2.0, 2.0, edges.size).astype(np.float32)
    failed, total, messages = model.walk(snn, fresh_of(snn), lambda dn: dn.graph_edit(pre[edges], post[edges], values), csr_tests.read,
                                         6 if ascending else 9)
    assert failed == total, (failed, total, messages)
    want = csr[2].copy()
    for e, v in zip(edges, values):
        want[e] = v
    dn = fresh_of(snn)()
    dn.graph_edit(pre[edges], post[edges], values)
    csr_tests.assert_csr(dn, (csr[0], csr[1], want), "after the walk")
    dn.close()
