"""snn_connect_by_spec on the device: wrap-around distances and weights from a displacement table, every block against the
per-pair restatement of the header's formulas (connect_spec_cases), everything outside the block left alone, the equivalences
with the older call, the grid-stride loop, shard handles, run parity against the oracle, reward-modulated handles and the
refusals.  The ragged network, its pattern and its helpers are test_gpu_connect_rule.py's; all comparisons go through
get_graph_rows, on bits."""
import ctypes as C

import numpy as np
import pytest

import connect_spec_cases as cases
import parity
import test_gpu_connect_rule as dense_tests
from snn_amd import ConnectionRule, WeightRule, _lib

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_STATE = 11, 12
RAGGED, SPLIT = dense_tests.RAGGED, dense_tests.SPLIT
PLAN = cases.plan(ConnectionRule, WeightRule)
SPLIT_SPEC_PLAN = cases.plan(ConnectionRule, WeightRule, ((9, 9), (10, 11), (2, 3)))
handle, pattern, geometry, assert_rows = dense_tests.handle, dense_tests.pattern, dense_tests.geometry, dense_tests.assert_rows


def apply_host(w, c, layout, plan):
    """the plan's blocks written into host rows [n_tot, n_neurons] from the per-pair expectation"""
    geo = geometry(layout)
    for pre, post, rule, weight in plan:
        (f0, s0), (f1, s1) = geo[pre], geo[post]
        on, ww = cases.expected_for(rule, weight, s0, s1)
        w[f0:f0 + on.shape[0], f1:f1 + on.shape[1]] = ww
        c[f0:f0 + on.shape[0], f1:f1 + on.shape[1]] = on
    return w, c


def test_the_plan_says_what_it_is_meant_to_say():
    """conditions on the restatement, not on the device"""
    geo = geometry(RAGGED)
    tables = [weight.table.shape if weight.table is not None else None for _, _, _, weight in PLAN]
    assert tables == [(3, 5), (5, 11), (9, 13), None]
    for pre, post, rule, weight in PLAN:
        on, _ = cases.expected_for(rule, weight, geo[pre][1], geo[post][1])
        assert on.any() and not on.all(), (pre, post)
    # only the table removes pairs of the all-to-all block
    pre, post, rule, weight = PLAN[2]
    on, w = cases.expected_for(rule, weight, (5, 7), (5, 7))
    assert 0 < (~on).sum() == np.isnan(weight.values((5, 7), (5, 7))).sum() and (w[on] < 0).any()
    # the thinned block: some, not all, of the pairs its radius allows
    pre, post, rule, weight = PLAN[1]
    on, _ = cases.expected_for(rule, weight, (3, 5), (5, 7))
    full = cases.expected_block((3, 5), (5, 7), rule.kind, rule.extent, wrap=rule.wrap)[0]
    assert 0.1 < on.sum() / full.sum() < 0.9 and not (on & ~full).any()


def test_ragged_network_blocks_and_everything_outside_them(snn):
    dn = handle(snn, RAGGED)
    w, c = pattern(RAGGED)
    dn.set_graph_rows(0, w, c)
    for k, (pre, post, rule, weight) in enumerate(PLAN):
        dn.connect_by_rule(pre, post, rule, weight)
        apply_host(w, c, RAGGED, PLAN[k:k + 1])
        # the block as the per-pair loop has it; every entry outside the blocks written so far still the pattern
        assert_rows(dn, w, c, what=f"after connecting {pre} -> {post}")
    untouched, _ = pattern(RAGGED)
    assert np.array_equal(w[15:50, 0:15], untouched[15:50, 0:15]) and np.array_equal(w[50:, 0:15], untouched[50:, 0:15])
    dn.close()


def test_equivalences_on_a_ring(snn):
    lay = parity.Layout([(0, 12, 1)])
    dn = handle(snn, lay)
    weight = WeightRule.displacement(cases.ramp((12, 1), 0.5, 1.0), wrap=True)

    def rows_after(rule):
        dn.connect_by_rule(0, 0, rule, weight)
        on, w = cases.expected_for(rule, weight, (12, 1), (12, 1))
        assert_rows(dn, w, on.astype(np.uint32), what=f"after {rule!r}")
        return dn.get_graph_rows(0, 12)

    for e in (6, 7, 12, 2 ** 32 - 1):                          # 2 e + 1 >= P: every pair
        w0, c0 = rows_after(ConnectionRule.chebyshev(e, wrap=True))
        w1, c1 = rows_after(ConnectionRule.all_to_all(wrap=True))
        assert c0.all() and np.array_equal(c0, c1) and np.array_equal(parity.bits(w0), parity.bits(w1))
    w0, c0 = rows_after(ConnectionRule.chebyshev(5, wrap=True))
    assert c0.sum() == 12 * 11
    w0, c0 = rows_after(ConnectionRule.chebyshev(0, wrap=True))
    w1, c1 = rows_after(ConnectionRule.same_position(wrap=True))
    assert c0.sum() == 12 and np.array_equal(c0, c1) and np.array_equal(parity.bits(w0), parity.bits(w1))
    w0, c0 = rows_after(ConnectionRule.euclidean(0, wrap=True))
    assert np.array_equal(c0, c1) and np.array_equal(parity.bits(w0), parity.bits(w1))
    dn.close()


def test_without_wrap_and_table_the_new_call_is_the_old_call(snn):
    """two handles: snn_connect_by_rule on one, snn_connect_by_spec with an empty extension on the other"""
    old, new = handle(snn, RAGGED), handle(snn, RAGGED)
    w, c = pattern(RAGGED)
    for dn in (old, new):
        dn.set_graph_rows(0, w, c)
    for pre, post, rule, weight in dense_tests.PLAN:
        assert rule.wrap == 0 and weight.table is None
        old._check(old._L.snn_connect_by_rule(old._h, pre, post, rule.kind, rule.extent, int(rule.self_edges), rule.probability, rule.seed,
                                              weight.kind, weight.lo, weight.hi, weight.seed))
        new.connect_by_rule(pre, post, rule, weight)
        dense_tests.apply_host(w, c, RAGGED, [(pre, post, rule, weight)])
        assert_rows(old, w, c, what=f"by the old call, {pre} -> {post}")
        assert_rows(new, *old.get_graph_rows(0, old.n_tot), what=f"by the new call, {pre} -> {post}")
    # a table that is given with another weight rule is not read, whatever it points at
    record = _lib.ConnectRecord(0, 1, cases.CHEBYSHEV, 1, 1, 1.0, 0, cases.UNIFORM, 0.5, 1.5, 9)
    spec = _lib.ConnectSpec(record, 0, 7, 7, None)
    new._check(new._L.snn_connect_by_spec(new._h, C.byref(spec)))
    old.connect_by_rule(0, 1, ConnectionRule.chebyshev(1), WeightRule.uniform(0.5, 1.5, seed=9))
    assert_rows(new, *old.get_graph_rows(0, old.n_tot), what="with table dimensions that are not read")
    # ... nor is the pointer followed or scanned: one infinite word where the dimensions claim 7 x 7
    one = np.array([np.inf], np.float32)
    record.weight_seed = 10
    spec = _lib.ConnectSpec(record, 0, 7, 7, one.ctypes.data_as(_lib.f32p))
    new._check(new._L.snn_connect_by_spec(new._h, C.byref(spec)))
    old.connect_by_rule(0, 1, ConnectionRule.chebyshev(1), WeightRule.uniform(0.5, 1.5, seed=10))
    assert_rows(new, *old.get_graph_rows(0, old.n_tot), what="with a table pointer that is not read")
    old.close()
    new.close()


def test_grid_stride_loop_over_a_long_presynaptic_lattice(snn):
    """130 x 127 cells (16 510 rows: more row groups than the grid has blocks in y) onto 2 x 3 neurons, on a torus, with a table"""
    lay = parity.Layout([(0, 2, 3)], [(1, 130, 127)])
    dn = handle(snn, lay)
    w, c = pattern(lay)
    dn.set_graph_rows(0, w, c)
    u, v = np.arange(130, dtype=np.float32)[:, None], np.arange(127, dtype=np.float32)[None, :]
    table = (u * np.float32(128.0) + v + np.float32(0.5)).astype(np.float32)                 # every entry names its displacement
    table[(np.arange(130)[:, None] + np.arange(127)[None, :]) % 11 == 0] = np.nan
    record = (1, 0, ConnectionRule.chebyshev(40, wrap=True), WeightRule.displacement(table, wrap=True))
    dn.connect_by_rule(*record)
    apply_host(w, c, lay, [record])
    on = c[6:, :]
    assert (16510 + 3) // 4 > 4096 and 0 < on.sum() < on.size and on[-1].any() and on[0].any()
    assert_rows(dn, w, c, what="after the long block")
    untouched, cu = pattern(lay)
    assert np.array_equal(w[:6], untouched[:6]) and np.array_equal(c[:6], cu[:6])
    dn.close()


@pytest.mark.parametrize("layout,plan", [(RAGGED, PLAN), (SPLIT, SPLIT_SPEC_PLAN)], ids=["ragged", "split"])
def test_shard_handles_write_the_columns_they_own(snn, layout, plan):
    whole = handle(snn, layout)
    shards = [handle(snn, layout, shard=(k, 2)) for k in range(2)]
    w, c = pattern(layout)
    for dn in [whole] + shards:
        dn.set_graph_rows(0, w, c)
        for pre, post, rule, weight in plan:
            dn.connect_by_rule(pre, post, rule, weight)
    apply_host(w, c, layout, plan)
    assert_rows(whole, w, c, what="on the unsharded handle")
    owned = 0
    for k, dn in enumerate(shards):
        cols = slice(dn.post_begin, dn.post_end)
        owned += dn.post_end - dn.post_begin
        assert_rows(dn, w, c, cols=cols, what=f"on shard {k} (columns {dn.post_begin}..{dn.post_end})")
    assert owned == layout.n_neurons
    for dn in [whole] + shards:
        dn.close()


def test_run_parity_of_a_graph_built_by_spec(snn):
    net = dense_tests.ragged_oracle()
    dn = parity.device_from_oracle(snn, net)                 # no edge at all ...
    for pre, post, rule, weight in PLAN:
        dn.connect_by_rule(pre, post, rule, weight)          # ... then the graph, on the device
    apply_host(net["weights"], net["connections"], RAGGED, PLAN)            # the oracle is fed the expected host matrix
    assert (net["weights"] < 0).any()
    parity.assert_graph_equal(net, dn)
    dn.set_history(voltage=True, spikes=True)
    dn.run(20)
    net.run(20, voltage_history=True, spike_history=True)
    rng = RAGGED.ranges()
    for i, _, _ in RAGGED.lattices:
        first, count, _ = rng[i]
        assert np.array_equal(dn.spike_history(i), net.spike_history[:, first:first + count]), f"raster of lattice {i}"
        assert np.array_equal(parity.bits(dn.voltage_history(i)), parity.bits(net.voltage_history[:, first:first + count]))
    parity.assert_state_equal(net, parity.pull_state(dn, net))
    parity.assert_graph_equal(net, dn)
    assert net["st_last_firing_time"].max() > 0, "the spike trains must have fired"
    dn.close()


def spec(table=None, wrap=3, rows=None, cols=None, **change):
    """the first record of the plan as a raw snn_connect_spec; the returned table array must outlive the call"""
    f = dict(pre_id=0, post_id=0, rule=cases.CHEBYSHEV, extent=1, self_edges=0, probability=1.0, edge_seed=0,
             weight_rule=cases.DISPLACEMENT, w_lo=0.0, w_hi=0.0, weight_seed=0)
    f.update(change)
    table = cases.ramp((3, 5), 0.25, 1.0) if table is None else table
    pointer = table.ctypes.data_as(_lib.f32p) if table is not False else None
    shape = table.shape if table is not False else (3, 5)
    return _lib.ConnectSpec(_lib.ConnectRecord(**f), wrap, shape[0] if rows is None else rows, shape[1] if cols is None else cols, pointer), table


def test_refusals_leave_the_graph_alone(snn):
    dn = handle(snn, RAGGED)
    L, h = dn._L, dn._h
    w, c = pattern(RAGGED)
    dn.set_graph_rows(0, w, c)

    def call(handle_, *args, **change):
        s, keep = spec(*args, **change)
        code = L.snn_connect_by_spec(handle_, C.byref(s))
        return code, (L.snn_last_error() or b"").decode()

    assert call(None)[0] == BAD_ARG
    assert L.snn_connect_by_spec(h, None) == BAD_ARG and "spec" in L.snn_last_error().decode()
    inf = cases.ramp((3, 5))
    inf[2, 4] = np.inf
    minus_inf = cases.ramp((3, 5))
    minus_inf[0, 0] = -np.inf
    for args, change, name in [((), dict(wrap=4), "wrap"), ((), dict(wrap=0xFFFFFFFF), "wrap"), ((False,), {}, "table"),
                               ((), dict(rows=4), "table_rows"), ((), dict(rows=5), "table_rows"), ((), dict(cols=9), "table_cols"),
                               ((), dict(wrap=0), "table_rows"), ((), dict(wrap=1), "table_cols"),
                               ((inf,), {}, "table"), ((minus_inf,), {}, "table"), ((), dict(weight_rule=3), "weight_rule"),
                               ((), dict(rule=4), "rule"), ((), dict(pre_id=9), "pre_id"), ((), dict(post_id=2), "post_id"),
                               ((), dict(probability=float("nan")), "probability"),
                               ((), dict(weight_rule=cases.UNIFORM, w_lo=float("inf")), "w_lo")]:
        code, msg = call(h, *args, **change)
        assert code == BAD_ARG and name in msg, (change, code, msg)
    assert_rows(dn, w, c, what="after the refused calls")
    # w_lo / w_hi are not read with a table; the accepted call, for contrast, does change the graph
    assert call(h, w_lo=float("nan"), w_hi=float("inf"))[0] == 0
    apply_host(w, c, RAGGED, PLAN[:1])
    assert_rows(dn, w, c, what="after the accepted call")
    # the old calls do not take the table
    code = L.snn_connect_by_rule(h, 0, 0, cases.CHEBYSHEV, 1, 0, 1.0, 0, cases.DISPLACEMENT, 0.0, 0.0, 0)
    assert code == BAD_ARG and "weight_rule" in L.snn_last_error().decode()
    assert_rows(dn, w, c, what="after the old call with weight_rule 2")
    dn.close()

    raw = handle(snn, RAGGED, finalize=False)
    code, msg = call(raw._h)
    assert code == BAD_STATE and "finalized" in msg
    raw.close()

    sparse = handle(snn, RAGGED, csr=True)
    row_ptr, pre_index, weights = np.arange(51, dtype=np.uint64), np.arange(50, dtype=np.uint32)[::-1].copy(), np.full(50, 0.5, np.float32)
    sparse.set_graph_csr(row_ptr, pre_index, weights)
    code, msg = call(sparse._h)
    assert code == BAD_STATE and "dense handles only" in msg
    assert np.array_equal(sparse.get_graph_csr(), weights)
    record = _lib.ConnectRecord(0, 0, cases.CHEBYSHEV, 1, 0, 1.0, 0, cases.DISPLACEMENT, 0.0, 0.0, 0)
    code = L.snn_connect_by_rules_csr(sparse._h, C.byref(record), 1)
    assert code == BAD_ARG and "weight_rule" in L.snn_last_error().decode() and "record 0" in L.snn_last_error().decode()
    assert np.array_equal(sparse.get_graph_csr(), weights)
    sparse.close()


def test_reward_modulated_handle_restarts_the_traces_of_the_block(snn):
    dn = handle(snn, RAGGED)
    w, c = pattern(RAGGED)
    dn.set_graph_rows(0, w, c)
    dn.set_reward_modulator(1, do_modulation=True)
    n_tot, nn = dn.n_tot, dn.n_neurons
    t = (np.float32(1.0) + np.arange(n_tot * nn, dtype=np.float32).reshape(n_tot, nn) / np.float32(4096.0)).astype(np.float32)
    dn.set_trace_rows(0, t)
    dn.set_pending_rows(0, -t)
    dn.set_counter_rows(0, np.ones((n_tot, nn), np.uint8))
    dn.connect_by_rule(*PLAN[1])                             # 0 -> 1
    want = t.copy()
    want[0:15, 15:50] = 0
    assert np.array_equal(dn.get_trace_rows(0, n_tot).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dn.get_pending_rows(0, n_tot).view(np.uint32), (-want).view(np.uint32) * (want != 0))
    counters = np.ones((n_tot, nn), np.uint8)
    counters[0:15, 15:50] = 0
    assert np.array_equal(dn.get_counter_rows(0, n_tot), counters)
    apply_host(w, c, RAGGED, PLAN[1:2])
    assert_rows(dn, w, c)
    dn.close()
