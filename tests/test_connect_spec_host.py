"""The host twins of the spec calls (ConnectionRule.mask with wrap, WeightRule.displacement / from_displacement_function, values)
against the per-pair restatement of the header's formulas (connect_spec_cases), the restatement against the older one where the
two must agree, the rule-built facade lattice against the closure-built one, and the Python errors.  No device call."""
import itertools

import numpy as np
import pytest

import connect_rule_cases as old_cases
import connect_spec_cases as cases
import parity
import snn_amd
from snn_amd import ConnectionRule, WeightRule

# 3x5 -> 5x7: different shapes, both periods from the larger grid; a dimension of 1; even and odd periods (the tie dr0 == P / 2)
GRIDS = [((3, 5), (5, 7)), ((5, 7), (3, 5)), ((12, 1), (12, 1)), ((1, 12), (1, 12)), ((6, 6), (6, 6)), ((5, 5), (5, 5)), ((2, 3), (5, 7))]
WRAPS = [False, True, (True, False), (False, True)]


def old_plans():
    """every (shapes, rule, weight) of the plans of the existing device tests"""
    import test_gpu_connect_rule as dense_tests
    import test_gpu_connect_rule_csr as csr_tests
    out = []
    for layout, plan in [(dense_tests.RAGGED, csr_tests.RAGGED_PLAN), (dense_tests.SPLIT, dense_tests.SPLIT_PLAN), (csr_tests.WIDE, csr_tests.WIDE_PLAN)]:
        geo = dense_tests.geometry(layout)
        out += [(geo[pre][1], geo[post][1], rule, weight) for pre, post, rule, weight in plan]
    return out


def test_restatement_without_wrap_is_the_older_restatement():
    plans = old_plans()
    assert len(plans) == 15
    for pre_shape, post_shape, rule, weight in plans:
        assert rule.wrap == 0 and weight.table is None
        on, w = cases.expected_for(rule, weight, pre_shape, post_shape)
        on0, w0 = old_cases.expected_for(rule, weight, pre_shape, post_shape)
        assert np.array_equal(on, on0) and np.array_equal(parity.bits(w), parity.bits(w0)), (pre_shape, post_shape, rule)


@pytest.mark.parametrize("shapes", GRIDS, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_mask_and_values_with_wrap_and_tables(shapes):
    pre_shape, post_shape = shapes
    span = max(max(pre_shape), max(post_shape))
    for wrap in WRAPS:
        flags = snn_amd.network._wrap_flags(wrap)
        shape = WeightRule.table_shape(pre_shape, post_shape, wrap)
        assert shape == cases.table_shape(pre_shape, post_shape, flags)
        table = cases.holed(shape)
        assert np.isnan(table).any() and not np.isnan(table).all()
        weight = WeightRule.displacement(table, wrap=wrap)
        rules = [ConnectionRule.all_to_all(wrap=wrap), ConnectionRule.same_position(self_edges=True, wrap=wrap),
                 ConnectionRule.all_to_all(self_edges=False, probability=0.5, seed=7, wrap=wrap)]
        rules += [ConnectionRule.chebyshev(e, wrap=wrap) for e in (0, 1, span // 2, span)]
        rules += [ConnectionRule.euclidean(e2, self_edges=False, wrap=wrap) for e2 in (0, 1, 2, 5, (span // 2) ** 2)]
        for rule in rules:
            for wt in (weight, WeightRule.uniform(-1.0, 1.0, seed=3)):
                on, w = cases.expected_for(rule, wt, pre_shape, post_shape)
                got_on, got_w = snn_amd.network.rule_pairs(rule, wt, pre_shape, post_shape)
                assert np.array_equal(got_on, on), (rule, wt)
                assert np.array_equal(parity.bits(got_w), parity.bits(w)), (rule, wt)
                # mask alone is the geometry and the draw; values alone the table's entry, NaN where the table is NaN
                v = wt.values(pre_shape, post_shape)
                assert np.array_equal(rule.mask(pre_shape, post_shape) & ~np.isnan(v), on)
                # one row and one column of it cost O(N)
                i, j = on.shape[0] // 2, on.shape[1] - 1
                row = snn_amd.network.rule_pairs(rule, wt, pre_shape, post_shape, [i], None)
                col = snn_amd.network.rule_pairs(rule, wt, pre_shape, post_shape, None, [j])
                assert np.array_equal(row[0][0], on[i]) and np.array_equal(parity.bits(row[1][0]), parity.bits(w[i]))
                assert np.array_equal(col[0][:, 0], on[:, j]) and np.array_equal(parity.bits(col[1][:, 0]), parity.bits(w[:, j]))


def test_wrapped_distance_ties_and_equivalences():
    ring = ((12, 1), (12, 1))
    everything = cases.expected_block(*ring, cases.ALL)[0]
    assert everything.all()
    assert np.array_equal(ConnectionRule.chebyshev(6, wrap=True).mask(*ring), everything)        # dr0 == P / 2 is its own mirror image
    assert not ConnectionRule.chebyshev(5, wrap=True).mask(*ring).all()
    assert ConnectionRule.chebyshev(5, wrap=True).mask(*ring).sum() == 12 * 11
    assert np.array_equal(ConnectionRule.chebyshev(0, wrap=True).mask(*ring), ConnectionRule.same_position().mask(*ring))
    odd = ((5, 5), (5, 5))
    assert ConnectionRule.chebyshev(2, wrap=True).mask(*odd).all() and not ConnectionRule.chebyshev(1, wrap=True).mask(*odd).all()
    assert ConnectionRule.chebyshev(1, wrap=True).mask(*odd).sum() == 25 * 9
    # a dimension that does not wrap keeps its plain distance
    half = ConnectionRule.chebyshev(1, wrap=(True, False)).mask(*odd)
    assert half[0, 20] and not half[0, 4] and half.sum() == 5 * 3 * (2 + 3 + 3 + 3 + 2)
    assert repr(ConnectionRule.chebyshev(1)) == "ConnectionRule(kind=1, extent=1, self_edges=True, probability=1.0, seed=0)"
    assert "wrap=(True, False)" in repr(ConnectionRule.chebyshev(1, wrap=(True, False)))


def closure_lattice(shape, fn):
    lat = snn_amd.Lattice(0)
    lat.populate(snn_amd.IzhikevichNeuron(), *shape)
    lat.connect(lambda a, b: True, fn)
    return lat


@pytest.mark.parametrize("shape", [(12, 1), (6, 6), (5, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("form", ["bump", "scaled_bump", "shift"])
def test_displacement_function_builds_the_closure_graph(shape, form):
    fn = cases.attractor_forms(shape)[form]
    calls = []

    def counted(a, b):
        calls.append((a, b))
        return fn(a, b)
    weight = WeightRule.from_displacement_function(counted, shape, shape, wrap=True)
    assert len(calls) == shape[0] * shape[1] == weight.table.size and weight.kind == snn_amd.network.WEIGHT_DISPLACEMENT
    by_rule = snn_amd.Lattice(0)
    by_rule.populate(snn_amd.IzhikevichNeuron(), *shape)
    by_rule.connect(ConnectionRule.all_to_all(wrap=True), weight)
    assert by_rule.rule_held
    twin = closure_lattice(shape, fn)
    assert by_rule.get_weight((0, 0), (shape[0] - 1, 0)) == twin.get_weight((0, 0), (shape[0] - 1, 0))
    assert by_rule.get_incoming_connections((1, 0)) == twin.get_incoming_connections((1, 0))
    assert by_rule.rule_held, "single lookups must not build the matrices"
    assert np.array_equal(by_rule.connections, twin.connections) and twin.connections.all()
    assert np.array_equal(parity.bits(by_rule.weights), parity.bits(twin.weights))
    assert len(np.unique(twin.weights)) > 2


def test_displacement_function_none_is_no_edge_and_unwrapped_tables():
    shape = (3, 4)

    def fn(a, b):
        d = (b[0] - a[0], b[1] - a[1])
        return None if d == (0, 0) or abs(d[1]) == 3 else 10.0 * d[0] + d[1]
    weight = WeightRule.from_displacement_function(fn, shape, (2, 5))
    assert weight.table.shape == (4, 8) and np.isnan(weight.table).sum() == 1 + 2 * 4
    on, w = snn_amd.network.rule_pairs(ConnectionRule.all_to_all(), weight, shape, (2, 5))
    for i, j in itertools.product(range(12), range(10)):
        a, b = (i // 4, i % 4), (j // 5, j % 5)
        want = fn(a, b)
        assert on[i, j] == (want is not None) and w[i, j] == np.float32(0.0 if want is None else want)
    lat = snn_amd.Lattice(0)
    lat.populate(snn_amd.IzhikevichNeuron(), 3, 4)
    lat.connect(ConnectionRule.chebyshev(1), WeightRule.from_displacement_function(fn, shape, shape))
    twin = closure_lattice(shape, lambda a, b: 0.0)
    twin.connect(lambda a, b: max(abs(a[0] - b[0]), abs(a[1] - b[1])) <= 1 and fn(a, b) is not None, fn)
    assert lat.get_weight((1, 1), (1, 1)) == 0.0 and lat.get_outgoing_connections((1, 1)) == twin.get_outgoing_connections((1, 1))
    assert np.array_equal(lat.connections, twin.connections) and np.array_equal(parity.bits(lat.weights), parity.bits(twin.weights))


def test_python_errors():
    with pytest.raises(ValueError, match="wrap"):
        ConnectionRule.all_to_all(wrap=3)
    with pytest.raises(ValueError, match="2-D"):
        WeightRule.displacement(np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="infinite"):
        WeightRule.displacement(np.array([[1.0, np.inf]], np.float32))
    with pytest.raises(ValueError, match="table goes with"):
        WeightRule(snn_amd.network.WEIGHT_CONSTANT, 1.0, table=np.zeros((1, 1), np.float32))
    with pytest.raises(ValueError, match="unknown weight rule"):
        WeightRule(3, 1.0)
    table = np.zeros((5, 5), np.float32)
    with pytest.raises(ValueError, match="wrap"):                      # the table's wrap is its rule's
        snn_amd.network.rule_pairs(ConnectionRule.all_to_all(), WeightRule.displacement(table, wrap=True), (5, 5), (5, 5))
    with pytest.raises(ValueError, match="wrap"):
        snn_amd.network.rule_pairs(ConnectionRule.chebyshev(1, wrap=(True, False)), WeightRule.displacement(table, wrap=True), (5, 5), (5, 5))
    lat = snn_amd.Lattice(0)
    lat.populate(snn_amd.IzhikevichNeuron(), 5, 5)
    with pytest.raises(ValueError, match="wrap"):
        lat.connect(ConnectionRule.all_to_all(), WeightRule.displacement(table, wrap=True))
    with pytest.raises(ValueError, match="does not fit"):               # a table for other grids
        WeightRule.displacement(table, wrap=True).values((5, 5), (6, 6))
    with pytest.raises(ValueError, match="does not fit"):
        WeightRule.displacement(table).values((5, 5), (5, 5))
    with pytest.raises(TypeError):
        lat.connect(lambda a, b: True, WeightRule.displacement(table))
