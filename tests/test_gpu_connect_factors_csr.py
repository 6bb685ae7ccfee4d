"""snn_connect_by_factors_csr: the factored weights merged into a sparse graph on the device -- structure and weights against the
CSR (np.nonzero order) of the float64 host twin patched into the uploaded pattern: the grids of tests/test_gpu_connect_factors.py,
a list that mixes record kinds committed once, edges outside the blocks kept, contiguous shards, an empty result, refusals."""
import ctypes as C

import numpy as np
import pytest

import connect_factors_cases as cases
import connect_spec_cases as spec_cases
import parity
import test_gpu_connect_factors as dense_factors
import test_gpu_connect_rule as dense_tests
import test_gpu_connect_rule_csr as csr_tests
from snn_amd import ConnectionRule, WeightRule, _lib

pytestmark = pytest.mark.gpu

BAD_ARG = 11
NO_SELF, PAIR, RULES = dense_factors.NO_SELF, dense_factors.PAIR, dense_factors.RULES
apply_host, random_factors = dense_factors.apply_host, dense_factors.random_factors
patterned, assert_csr, csr_of, read = csr_tests.patterned, csr_tests.assert_csr, csr_tests.csr_of, csr_tests.read
CSR_CHUNK = 128                                            # FACTOR_CSR_CHUNK of csrc/snn_kernels_connect_factors.hpp


def connect_and_compare(snn, layout, plan, what=""):
    dn, w, c = patterned(snn, layout)
    for k, record in enumerate(plan):
        dn.connect_sparse([record])
        apply_host(w, c, layout, [record])
        assert_csr(dn, csr_of(w, c, dn.owned), f"{what} after record {k}")
    dn.close()


@pytest.mark.parametrize("name", cases.CASES)
def test_fixture_case_between_two_other_lattices(snn, name):
    rows, cols = cases.GRIDS[name]
    layout = parity.Layout([(0, 3, 5), (1, rows, cols), (2, 2, 3)])
    connect_and_compare(snn, layout, [(1, 1, NO_SELF, cases.hopfield(WeightRule, name))], name)


@pytest.mark.parametrize("p", [1, 3, CSR_CHUNK + 1])
def test_several_candidate_rounds_and_more_than_one_chunk(snn, p):
    """420 candidates per row: seven ballot rounds, the last ragged; 423 rows: seven SELL slices"""
    u, v = random_factors(p, p, 420, 420)
    v[:, 7] = 0.0
    layout = parity.Layout([(0, 1, 3), (1, 20, 21)])
    connect_and_compare(snn, layout, [(1, 1, NO_SELF, WeightRule.factors(u, v, scale=0.25, drop_zero=True))], f"P = {p}")


@pytest.mark.parametrize("form", ["per_post", "per_pre", "general"])
def test_between_lattices_of_different_grids(snn, form):
    u, v = random_factors(5, 4, 15, 24)
    weight = {"per_post": WeightRule.per_post(v[0]), "per_pre": WeightRule.per_pre(u[0]),
              "general": WeightRule.factors(u, v, scale=-1.5)}[form]
    connect_and_compare(snn, PAIR, [(0, 1, rule, weight) for rule in RULES] +
                        [(2, 0, ConnectionRule.all_to_all(), WeightRule.per_post(np.arange(15.0) - 3.0))], form)


def mixed_plan():
    u, v = random_factors(6, 3, 15, 24)
    table = spec_cases.ramp(spec_cases.table_shape((4, 6), (4, 6), 3), 0.25, 1.0)
    return [(0, 1, ConnectionRule.all_to_all(probability=0.5, seed=3), WeightRule.factors(u, v, drop_zero=True)),
            (2, 1, ConnectionRule.all_to_all(), WeightRule.constant(0.75)),
            (1, 1, ConnectionRule.chebyshev(1, self_edges=False, wrap=True), WeightRule.displacement(table, wrap=True)),
            (0, 0, NO_SELF, WeightRule.hopfield(np.sign(u), a=0.25, b=0.5, scalar=0.125))]


def test_a_mixed_list_commits_once_and_equals_the_single_calls(snn):
    plan = mixed_plan()
    one, w, c = patterned(snn, PAIR)
    batch, _, _ = patterned(snn, PAIR)
    for record in plan:
        one.connect_sparse([record])
    batch.connect_sparse(plan)
    for x, y in zip(read(one), read(batch)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "the batch and the sequence of calls differ"
    apply_host(w, c, PAIR, plan)
    assert_csr(batch, csr_of(w, c, batch.owned), "after the mixed list")
    # the blocks no record names (1 -> 0, 2 -> 0) keep the pattern, with the weights they have now
    untouched, cu = dense_tests.pattern(PAIR)
    assert np.array_equal(w[15:, 0:15], untouched[15:, 0:15]) and np.array_equal(c[15:, 0:15], cu[15:, 0:15]) and cu[15:, 0:15].any()
    one.close()
    batch.close()


def test_contiguous_shards_write_the_rows_they_own(snn):
    layout, plan = dense_tests.SPLIT, dense_factors.split_plan()
    w, c = dense_tests.pattern(layout)
    apply_host(w, c, layout, plan)
    owned = 0
    for k in range(2):
        dn, _, _ = patterned(snn, layout, shard=(k, 2))
        dn.connect_sparse(plan)
        assert_csr(dn, csr_of(w, c, dn.owned), f"on shard {k}")
        owned += len(dn.owned)
        dn.close()
    assert owned == layout.n_neurons


def test_drop_zero_that_drops_everything_leaves_an_empty_graph(snn):
    dn = dense_tests.handle(snn, parity.Layout([(0, 5, 7)]), csr=True)
    dn.connect_sparse([(0, 0, ConnectionRule.all_to_all(), WeightRule.factors(np.zeros((2, 35)), np.ones((2, 35)), drop_zero=True))])
    rp, pi, w = read(dn)
    assert not rp.any() and pi.size == 0 and w.size == 0
    dn.connect_sparse([(0, 0, NO_SELF, WeightRule.factors(np.zeros((2, 35)), np.ones((2, 35))))])      # ... and without it 35 * 34 edges of weight 0
    rp, pi, w = read(dn)
    assert rp[-1] == 35 * 34 and not w.any()
    dn.close()


def test_refusals_name_the_item_and_leave_the_graph_alone(snn):
    dn, w, c = patterned(snn, PAIR)
    L, h = dn._L, dn._h
    before = read(dn)
    good, keep0 = dense_factors.item()
    for kw, name in dense_factors.refusals():
        bad, keep1 = dense_factors.item(**kw)
        items = (_lib.ConnectFactors * 2)(good, bad)
        code, msg = L.snn_connect_by_factors_csr(h, items, 2), (L.snn_last_error() or b"").decode()
        assert code == BAD_ARG and name in msg and "item 1: " in msg, (name, code, msg)
    assert L.snn_connect_by_factors_csr(h, None, 1) == BAD_ARG and "items" in L.snn_last_error().decode()
    assert L.snn_connect_by_factors_csr(h, None, 0) == 0
    for x, y in zip(read(dn), before):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    dense = dense_tests.handle(snn, PAIR)
    items = (_lib.ConnectFactors * 1)(good)
    assert L.snn_connect_by_factors_csr(dense._h, items, 1) == 12 and "dense" in L.snn_last_error().decode()
    dense.close()
    dn.close()
    # a shard by lattice: as the spec calls
    slab = dense_tests.handle(snn, PAIR, finalize=False)
    slab.finalize(0, 2, csr=True, by_lattice=True)
    slab.set_graph_csr(*csr_of(w, c, slab.owned))
    code, msg = L.snn_connect_by_factors_csr(slab._h, items, 1), (L.snn_last_error() or b"").decode()
    assert code == 12 and "not covered" in msg and "by lattice" in msg, msg
    assert_csr(slab, csr_of(w, c, slab.owned), "on the by-lattice shard after the refusal")
    slab.close()
    raw = dense_tests.handle(snn, PAIR, finalize=False)
    assert L.snn_connect_by_factors_csr(raw._h, items, 1) == 12 and "finalized" in L.snn_last_error().decode()
    raw.close()
