"""snn_connect_by_factors on the device (dense handles): every block against the float64 host twin (WeightRule.values, held to the
reference's own matrices by tests/test_connect_factors_host.py) and everything outside it still the uploaded pattern -- the
fixture cases alone and between two other lattices (boundary quads that straddle), more than one 256-column block and one factor
more than the kernel stages at a time, two different grids with every part of the rule, a spike-train pre lattice, drop_zero,
shard handles, a reward-modulated handle, the equivalence with snn_connect_by_spec and the refusals.  The pattern and the helpers
are test_gpu_connect_rule.py's; all comparisons are on bits."""
import ctypes as C

import numpy as np
import pytest

import connect_factors_cases as cases
import parity
import test_gpu_connect_rule as dense_tests
import test_gpu_connect_spec as spec_tests
from snn_amd import ConnectionRule, WeightRule, _lib
from snn_amd.network import rule_pairs

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_STATE = 11, 12
FACTORS = 3
CHUNK = 32                                                 # FACTOR_CHUNK of csrc/snn_kernels_connect_factors.hpp
handle, pattern, geometry, assert_rows = dense_tests.handle, dense_tests.pattern, dense_tests.geometry, dense_tests.assert_rows
NO_SELF = ConnectionRule.all_to_all(self_edges=False)
PAIR = parity.Layout([(0, 3, 5), (1, 4, 6)], [(2, 2, 3)])  # two grids of different shapes and a spike-train lattice


def apply_host(w, c, layout, plan):
    """the plan's blocks written into host rows [n_tot, n_neurons] from the host twins"""
    geo = geometry(layout)
    for pre, post, rule, weight in plan:
        (f0, s0), (f1, s1) = geo[pre], geo[post]
        on, ww = cases.expected(rule_pairs, rule, weight, s0, s1)
        w[f0:f0 + on.shape[0], f1:f1 + on.shape[1]] = ww
        c[f0:f0 + on.shape[0], f1:f1 + on.shape[1]] = on
    return w, c


def connect_and_compare(snn, layout, plan, what=""):
    dn = handle(snn, layout)
    w, c = pattern(layout)
    dn.set_graph_rows(0, w, c)
    for k, record in enumerate(plan):
        dn.connect_by_rule(*record)
        apply_host(w, c, layout, [record])
        assert_rows(dn, w, c, what=f"{what} after record {k}")
    dn.close()
    return w, c


def random_factors(seed, p, n_pre, n_post):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((p, n_pre)), rng.standard_normal((p, n_post))


@pytest.mark.parametrize("name", cases.CASES)
def test_fixture_case_alone_on_a_handle(snn, name):
    rows, cols = cases.GRIDS[name]
    w, c = connect_and_compare(snn, parity.Layout([(0, rows, cols)]), [(0, 0, NO_SELF, cases.hopfield(WeightRule, name))], name)
    want = cases.case(name)[4]
    assert np.array_equal(c != 0, want != 0) and np.array_equal(parity.bits(w), parity.bits(np.where(want != 0, want, 0).astype(np.float32)))


@pytest.mark.parametrize("name", cases.CASES)
def test_fixture_case_between_two_other_lattices(snn, name):
    """pre_first = 15 is no multiple of 4, and neither is the block's end: both boundary quads are read, patched and stored back"""
    rows, cols = cases.GRIDS[name]
    layout = parity.Layout([(0, 3, 5), (1, rows, cols), (2, 2, 3)])
    assert (15 + rows * cols) % 4 != 0
    connect_and_compare(snn, layout, [(1, 1, NO_SELF, cases.hopfield(WeightRule, name))], name)


@pytest.mark.parametrize("p", [1, 3, CHUNK + 1])
def test_more_than_one_column_block_and_more_than_one_chunk(snn, p):
    """20 x 21 = 420 columns: two workgroups in x, the second ragged; 105 row groups: 27 row tiles, the last ragged"""
    u, v = random_factors(p, p, 420, 420)
    v[:, 7] = 0.0                                          # a column of zeros: dropped
    layout = parity.Layout([(0, 1, 3), (1, 20, 21)])
    w, c = connect_and_compare(snn, layout, [(1, 1, NO_SELF, WeightRule.factors(u, v, scale=0.25, drop_zero=True))], f"P = {p}")
    assert c[3:, 3 + 7].sum() == 0 and c[3:, 3:].sum() == 420 * 419 - 419


RULES = [ConnectionRule.all_to_all(), ConnectionRule.all_to_all(self_edges=False), ConnectionRule.all_to_all(probability=0.5, seed=11),
         ConnectionRule.chebyshev(1), ConnectionRule.chebyshev(1, wrap=True), ConnectionRule.chebyshev(1, self_edges=False, wrap=(False, True)),
         ConnectionRule.euclidean(2, probability=0.5, seed=12), ConnectionRule.same_position()]


@pytest.mark.parametrize("form", ["per_post", "per_pre", "general"])
def test_between_lattices_of_different_grids(snn, form):
    u, v = random_factors(5, 4, 15, 24)
    weight = {"per_post": WeightRule.per_post(v[0]), "per_pre": WeightRule.per_pre(u[0]),
              "general": WeightRule.factors(u, v, scale=-1.5)}[form]
    connect_and_compare(snn, PAIR, [(0, 1, rule, weight) for rule in RULES], form)


def test_spike_train_pre_lattice(snn):
    u, v = random_factors(6, 2, 6, 15)
    connect_and_compare(snn, PAIR, [(2, 0, ConnectionRule.all_to_all(), WeightRule.factors(u, v)),
                                    (2, 1, ConnectionRule.chebyshev(1), WeightRule.per_post(np.arange(24.0) - 3.0))])


def test_drop_zero_is_none_and_without_it_zero_is_an_edge(snn):
    dn = handle(snn, parity.Layout([(0, 5, 7)]))
    patterns, a, b, scalar, want = cases.case("single")
    i, j = np.argwhere((want == 0) & ~np.eye(35, dtype=bool))[0]
    k, l = np.argwhere(want != 0)[0]
    pre, post = np.array([i, k, 3], np.uint32), np.array([j, l, 3], np.uint32)
    dn.connect_by_rule(0, 0, NO_SELF, cases.hopfield(WeightRule, "single"))
    w, on = dn.graph_lookup(pre, post)
    assert on.tolist() == [0, 1, 0] and w.tolist() == [0.0, np.float32(want[k, l]), 0.0]
    dn.connect_by_rule(0, 0, NO_SELF, cases.hopfield(WeightRule, "single", drop_zero=False))
    w, on = dn.graph_lookup(pre, post)
    assert on.tolist() == [1, 1, 0] and w.tolist() == [0.0, np.float32(want[k, l]), 0.0]          # Some(0.0), Some(w), None (the diagonal)
    dn.close()


def split_plan():
    """on test_gpu_connect_rule.py's SPLIT (9x9 and 10x11 neurons, 2x3 cells; the shards' cut at 128 lies inside lattice 1)"""
    u, v = random_factors(7, 3, 81, 110)
    return [(1, 1, NO_SELF, WeightRule.hopfield((v > 0).astype(np.float64), a=0.3, b=0.7, scalar=0.5)),
            (0, 1, ConnectionRule.chebyshev(2, wrap=True), WeightRule.factors(u, v)),
            (2, 1, ConnectionRule.all_to_all(), WeightRule.per_post(np.arange(110.0) / 8.0))]


def test_two_shard_handles_together_are_the_unsharded_matrix(snn):
    layout, plan = dense_tests.SPLIT, split_plan()
    whole = handle(snn, layout)
    shards = [handle(snn, layout, shard=(k, 2)) for k in range(2)]
    w, c = pattern(layout)
    for dn in [whole] + shards:
        dn.set_graph_rows(0, w, c)
        for record in plan:
            dn.connect_by_rule(*record)
    apply_host(w, c, layout, plan)
    assert_rows(whole, w, c, what="on the unsharded handle")
    owned = 0
    for k, dn in enumerate(shards):
        owned += dn.post_end - dn.post_begin
        assert_rows(dn, w, c, cols=slice(dn.post_begin, dn.post_end), what=f"on shard {k}")
    assert owned == layout.n_neurons and 81 < shards[0].post_end < 191
    for dn in [whole] + shards:
        dn.close()


def test_reward_modulated_handle_restarts_the_traces_of_the_block(snn):
    dn = handle(snn, PAIR)
    w, c = pattern(PAIR)
    dn.set_graph_rows(0, w, c)
    dn.set_reward_modulator(1, do_modulation=True)
    n_tot, nn = dn.n_tot, dn.n_neurons
    t = (np.float32(1.0) + np.arange(n_tot * nn, dtype=np.float32).reshape(n_tot, nn) / np.float32(4096.0)).astype(np.float32)
    dn.set_trace_rows(0, t)
    dn.set_pending_rows(0, -t)
    dn.set_counter_rows(0, np.ones((n_tot, nn), np.uint8))
    u, v = random_factors(8, 2, 15, 24)
    record = (0, 1, ConnectionRule.all_to_all(), WeightRule.factors(u, v))
    dn.connect_by_rule(*record)
    want = t.copy()
    want[0:15, 15:39] = 0
    assert np.array_equal(dn.get_trace_rows(0, n_tot).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dn.get_pending_rows(0, n_tot).view(np.uint32), (-want).view(np.uint32) * (want != 0))
    counters = np.ones((n_tot, nn), np.uint8)
    counters[0:15, 15:39] = 0
    assert np.array_equal(dn.get_counter_rows(0, n_tot), counters)
    apply_host(w, c, PAIR, [record])
    assert_rows(dn, w, c)
    dn.close()


def test_with_an_older_weight_rule_the_new_call_is_the_spec_call(snn):
    RAGGED = dense_tests.RAGGED
    old, new = handle(snn, RAGGED), handle(snn, RAGGED)
    w, c = pattern(RAGGED)
    for dn in (old, new):
        dn.set_graph_rows(0, w, c)
    junk = np.array([np.inf], np.float64)
    for pre, post, rule, weight in spec_tests.PLAN + dense_tests.PLAN:
        old.connect_by_rule(pre, post, rule, weight)
        spec = new._connect_spec(pre, post, rule, weight, "test")
        # the fields after the spec are not read: a count of 0, a scale of NaN, one infinite word behind each pointer
        item = _lib.ConnectFactors(spec, 0, 1, float("nan"), junk.ctypes.data_as(_lib.f64p), junk.ctypes.data_as(_lib.f64p))
        new._check(new._L.snn_connect_by_factors(new._h, C.byref(item)))
        assert_rows(new, *old.get_graph_rows(0, old.n_tot), what=f"{pre} -> {post}")
    old.close()
    new.close()


def item(u=None, v=None, n_factors=None, scale=0.5, drop_zero=0, **change):
    """a factors record 0 -> 1 of PAIR as a raw snn_connect_factors; the returned arrays must outlive the call"""
    f = dict(pre_id=0, post_id=1, rule=0, extent=0, self_edges=1, probability=1.0, edge_seed=0, weight_rule=FACTORS, w_lo=0.0, w_hi=0.0,
             weight_seed=0)
    f.update(change)
    uu, vv = random_factors(9, 2, 15, 24)
    u = uu if u is None else u
    v = vv if v is None else v
    spec = _lib.ConnectSpec(_lib.ConnectRecord(**f), 0, 0, 0, None)
    pointer = lambda x: None if x is False else x.ctypes.data_as(_lib.f64p)
    return _lib.ConnectFactors(spec, 2 if n_factors is None else n_factors, drop_zero, scale, pointer(u), pointer(v)), (u, v)


def refusals():
    """(keyword arguments of item, the argument the message names)"""
    uu, vv = random_factors(9, 2, 15, 24)
    out = [(dict(u=False), "pre_factors"), (dict(v=False), "post_factors"), (dict(n_factors=0), "n_factors"), (dict(n_factors=65537), "n_factors"),
           (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"),
           (dict(u=np.sign(uu) * 2.0 ** 62, v=np.sign(vv) * 2.0 ** 64, scale=1.0), "2^127"),           # 2 * 2^62 * 2^64 = 2^127 exactly
           (dict(pre_id=9), "pre_id"), (dict(post_id=2), "post_id"), (dict(rule=4), "rule"), (dict(weight_rule=4), "weight_rule"),
           (dict(probability=float("nan")), "probability")]
    for bad in (np.nan, np.inf, -np.inf):
        broken_u, broken_v = uu.copy(), vv.copy()
        broken_u[1, 14] = bad
        broken_v[0, 0] = bad
        out += [(dict(u=broken_u), "pre_factors"), (dict(v=broken_v), "post_factors")]
    return out


def test_refusals_leave_the_graph_alone(snn):
    dn = handle(snn, PAIR)
    L, h = dn._L, dn._h
    w, c = pattern(PAIR)
    dn.set_graph_rows(0, w, c)

    def call(handle_, **kw):
        it, keep = item(**kw)
        code = L.snn_connect_by_factors(handle_, C.byref(it))
        return code, (L.snn_last_error() or b"").decode()

    assert call(None)[0] == BAD_ARG
    assert L.snn_connect_by_factors(h, None) == BAD_ARG
    for kw, name in refusals():
        code, msg = call(h, **kw)
        assert code == BAD_ARG and name in msg, (name, code, msg)
    assert_rows(dn, w, c, what="after the refused calls")
    # w_lo / w_hi are not read; the accepted call, for contrast, changes the graph
    uu, vv = random_factors(9, 2, 15, 24)
    assert call(h, w_lo=float("nan"), w_hi=float("inf"))[0] == 0
    apply_host(w, c, PAIR, [(0, 1, ConnectionRule.all_to_all(), WeightRule.factors(uu, vv, scale=0.5))])
    assert_rows(dn, w, c, what="after the accepted call")
    # the four older calls do not take the factors
    code = L.snn_connect_by_rule(h, 0, 1, 0, 0, 1, 1.0, 0, FACTORS, 0.0, 0.0, 0)
    assert code == BAD_ARG and "weight_rule" in L.snn_last_error().decode()
    it, keep = item()
    assert L.snn_connect_by_spec(h, C.byref(it.spec)) == BAD_ARG and "weight_rule" in L.snn_last_error().decode()
    assert_rows(dn, w, c, what="after the older calls with weight_rule 3")
    dn.close()

    raw = handle(snn, PAIR, finalize=False)
    code, msg = call(raw._h)
    assert code == BAD_STATE and "finalized" in msg
    raw.close()

    sparse = handle(snn, PAIR, csr=True)
    n = PAIR.n_neurons
    row_ptr, pre_index, weights = np.arange(n + 1, dtype=np.uint64), np.arange(n, dtype=np.uint32)[::-1].copy(), np.full(n, 0.5, np.float32)
    sparse.set_graph_csr(row_ptr, pre_index, weights)
    code, msg = call(sparse._h)
    assert code == BAD_STATE and "dense handles only" in msg
    it, keep = item()
    assert L.snn_connect_by_rules_csr(sparse._h, C.byref(it.spec.record), 1) == BAD_ARG
    assert "weight_rule" in L.snn_last_error().decode() and "record 0" in L.snn_last_error().decode()
    assert L.snn_connect_by_specs_csr(sparse._h, C.byref(it.spec), 1) == BAD_ARG
    assert "weight_rule" in L.snn_last_error().decode() and "record 0" in L.snn_last_error().decode()
    assert np.array_equal(sparse.get_graph_csr(), weights)
    sparse.close()


def test_factor_lengths_that_do_not_fit_raise_on_the_host(snn):
    dn = handle(snn, PAIR)
    w, c = pattern(PAIR)
    dn.set_graph_rows(0, w, c)
    u, v = random_factors(10, 2, 15, 24)
    with pytest.raises(ValueError, match="fit grids"):
        dn.connect_by_rule(1, 0, ConnectionRule.all_to_all(), WeightRule.factors(u, v))       # the two lattices swapped
    with pytest.raises(ValueError, match="fit grids"):
        dn.connect_by_rule(0, 1, ConnectionRule.all_to_all(), WeightRule.per_post(np.ones(15)))
    assert_rows(dn, w, c, what="after the refused rules")
    dn.close()
