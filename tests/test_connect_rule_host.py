"""Host twin of snn_connect_by_rule (no GPU): ConnectionRule.mask / WeightRule.values against the per-pair restatement of the
header's formulas (connect_rule_cases), and the builders' connect(...) taking the records in place of the two closures."""
import itertools

import numpy as np
import pytest

import snn_amd
from snn_amd import ConnectionRule, WeightRule
import connect_rule_cases as cases
import parity

SHAPES = [((3, 5), (3, 5)), ((3, 5), (5, 7)), ((2, 3), (5, 7)), ((1, 1), (1, 1))]
RULES = [(cases.ALL, 0), (cases.CHEBYSHEV, 1), (cases.EUCLIDEAN, 5), (cases.SAME_POSITION, 0)]


@pytest.mark.parametrize("pre_shape,post_shape", SHAPES)
def test_mask_and_values_equal_the_per_pair_loop(pre_shape, post_shape):
    for (kind, extent), self_edges, probability, weight_kind in itertools.product(RULES, (True, False), (0.0, 0.37, 1.0), (0, 1)):
        rule = ConnectionRule(kind, extent=extent, self_edges=self_edges, probability=probability, seed=7)
        weight = WeightRule.constant(0.75) if weight_kind == cases.CONSTANT else WeightRule.uniform(-0.5, 1.5, seed=9)
        on, w = cases.expected_for(rule, weight, pre_shape, post_shape)
        what = f"{rule!r} {weight!r}"
        mask, values = rule.mask(pre_shape, post_shape), weight.values(pre_shape, post_shape)
        assert mask.dtype == bool and mask.shape == on.shape and values.dtype == np.float32 and values.shape == on.shape
        assert np.array_equal(mask, on), what
        assert np.array_equal(parity.bits(np.where(mask, values, np.float32(0))), parity.bits(w)), what
        if kind != cases.SAME_POSITION and 0 < probability < 1 and on.size > 1:
            assert 0 < on.sum() < on.size, what              # the draw thins, it does not empty


def test_constructors_and_refusals():
    r = ConnectionRule.chebyshev(2, self_edges=False)
    assert (r.kind, r.extent, r.self_edges, r.probability, r.seed) == (cases.CHEBYSHEV, 2, False, 1.0, 0)
    assert ConnectionRule.euclidean(5).kind == cases.EUCLIDEAN and ConnectionRule.euclidean(5).extent == 5
    assert ConnectionRule.all_to_all().kind == cases.ALL and ConnectionRule.same_position().kind == cases.SAME_POSITION
    w = WeightRule.uniform(0.5, 1.5, 3)
    assert (w.kind, w.lo, w.hi, w.seed) == (cases.UNIFORM, 0.5, 1.5, 3) and WeightRule.constant(2.0).lo == 2.0
    with pytest.raises(ValueError):
        ConnectionRule(9)
    with pytest.raises(ValueError):
        ConnectionRule.all_to_all(probability=float("nan"))
    with pytest.raises(ValueError):
        WeightRule.constant(float("inf"))
    with pytest.raises(ValueError):
        WeightRule.uniform(0.0, float("nan"))
    with pytest.raises(ValueError):
        WeightRule.uniform(-3e38, 3e38)                      # hi - lo overflows: weights would be infinite or NaN
    assert WeightRule.constant(3e38).lo == 3e38
    from snn_amd import lixirnet
    assert lixirnet.ConnectionRule is ConnectionRule and lixirnet.WeightRule is WeightRule


def closures(rule, weight, n_post):
    """the rule and the weight as the reference's two closures on positions (pre_cols / post_cols bound by the caller)"""
    def make(pre_cols, post_cols):
        def idx(a, b):
            return (a[0] * pre_cols + a[1]) * n_post + b[0] * post_cols + b[1]

        def cond(a, b):
            dr, dc = abs(a[0] - b[0]), abs(a[1] - b[1])
            on = {cases.ALL: True, cases.CHEBYSHEV: max(dr, dc) <= rule.extent, cases.EUCLIDEAN: dr * dr + dc * dc <= rule.extent,
                  cases.SAME_POSITION: a == b}[rule.kind]
            if not rule.self_edges:
                on = on and a != b
            if 0 < rule.probability < 1:
                on = on and cases._u24(rule.seed, idx(a, b)) < np.float32(rule.probability)
            return bool(on)

        def logic(a, b):
            if weight.kind == cases.CONSTANT:
                return np.float32(weight.lo)
            return np.float32(weight.lo) + (np.float32(weight.hi) - np.float32(weight.lo)) * cases._u24(weight.seed, idx(a, b))
        return cond, logic
    return make


PAIRS = [(ConnectionRule.chebyshev(1, self_edges=False), WeightRule.constant(0.5)),
         (ConnectionRule.euclidean(5, probability=0.37, seed=3), WeightRule.uniform(0.5, 1.5, seed=4)),
         (ConnectionRule.all_to_all(self_edges=False), None),
         (ConnectionRule.same_position(), WeightRule.constant(2.0))]


@pytest.mark.parametrize("cls", [snn_amd.Lattice, snn_amd.RewardModulatedLattice])
@pytest.mark.parametrize("rule,weight", PAIRS)
def test_lattice_connect_takes_the_records(cls, rule, weight):
    by_rule, by_closure = cls(), cls()
    for l in (by_rule, by_closure):
        l.populate(snn_amd.IzhikevichNeuron(), 3, 5)
        l.connect(lambda a, b: True, lambda a, b: 9.0)             # whatever was there is replaced, pair by pair
    by_rule.connect(rule, weight)
    cond, logic = closures(rule, weight or WeightRule.constant(1.0), 15)(5, 5)
    by_closure.connect(cond, logic)
    assert np.array_equal(by_rule.connections, by_closure.connections) and by_rule.connections.dtype == by_closure.connections.dtype
    assert np.array_equal(parity.bits(by_rule.weights), parity.bits(by_closure.weights))
    assert by_rule.connections.sum() > 0
    if cls is snn_amd.RewardModulatedLattice:
        assert np.array_equal(by_rule.traces, by_closure.traces)
    on, w = cases.expected_for(rule, weight or WeightRule.constant(1.0), (3, 5), (3, 5))
    assert np.array_equal(by_rule.connections != 0, on) and np.array_equal(parity.bits(by_rule.weights), parity.bits(w))


def build_network():
    net = snn_amd.LatticeNetwork()
    for id, (rows, cols) in {0: (3, 5), 1: (5, 7)}.items():
        l = snn_amd.Lattice(id)
        l.populate(snn_amd.IzhikevichNeuron(), rows, cols)
        net.add_lattice(l)
    st = snn_amd.SpikeTrainLattice(2)
    st.populate(snn_amd.RateSpikeTrain(), 2, 3)
    net.add_spike_train_lattice(st)
    return net


def test_network_connect_takes_the_records():
    shapes = {0: (3, 5), 1: (5, 7), 2: (2, 3)}
    by_rule, by_closure = build_network(), build_network()
    plan = [(0, 1, PAIRS[1]), (2, 1, PAIRS[3]), (1, 0, PAIRS[0]), (0, 1, PAIRS[0]), (1, 1, PAIRS[2])]   # (0 -> 1 twice: edges go away too)
    for pre, post, (rule, weight) in plan:
        by_rule.connect(pre, post, rule, weight)
        cond, logic = closures(rule, weight or WeightRule.constant(1.0), shapes[post][0] * shapes[post][1])(shapes[pre][1], shapes[post][1])
        by_closure.connect(pre, post, cond, logic)
    assert by_rule.connecting_nodes == by_closure.connecting_nodes
    assert list(by_rule.connecting) == list(by_closure.connecting) and len(by_rule.connecting) > 0
    assert all(np.float32(by_rule.connecting[k]) == np.float32(by_closure.connecting[k]) for k in by_rule.connecting)
    for id in (0, 1):
        assert np.array_equal(by_rule.lattices[id].connections, by_closure.lattices[id].connections)
        assert np.array_equal(parity.bits(by_rule.lattices[id].weights), parity.bits(by_closure.lattices[id].weights))
    assert by_rule.lattices[1].connections.sum() == 35 * 34
    by_rule.connect_internally(0, ConnectionRule.all_to_all(), WeightRule.constant(3.0))
    assert by_rule.lattices[0].connections.all() and (by_rule.lattices[0].weights == 3.0).all()
    with pytest.raises(KeyError):
        by_rule.connect(0, 2, ConnectionRule.all_to_all())          # a spike-train lattice is never postsynaptic


def test_closures_still_work_and_do_not_mix_with_records():
    l = snn_amd.Lattice()
    l.populate(snn_amd.IzhikevichNeuron(), 2, 2)
    l.connect(lambda a, b: a != b, lambda a, b: 0.25 * (a[0] + b[1] + 1))
    assert l.connections.sum() == 12 and l.get_weight((0, 0), (1, 1)) == 0.5 and l.get_weight((1, 1), (1, 1)) == 0.0
    l.connect(lambda a, b: a == b)
    assert l.connections.sum() == 4 and l.get_weight((1, 0), (1, 0)) == 1.0
    with pytest.raises(TypeError):
        l.connect(ConnectionRule.all_to_all(), lambda a, b: 1.0)
    with pytest.raises(TypeError):
        l.connect(lambda a, b: True, WeightRule.constant(1.0))
    assert l.connections.sum() == 4
