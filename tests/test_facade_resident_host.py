"""Rule-held lattices on the host (no GPU): a lattice whose graph was last set by a ConnectionRule / WeightRule record holds no
N x N matrix until one is asked for -- populate, connect, deep copies and the point / row / column queries stay O(N) --, the twins
evaluate single rows and columns of the pair grid, and records and closures mix as they always have."""
import copy
import tracemalloc

import numpy as np
import pytest

import connect_rule_cases as cases
from snn_amd import ConnectionRule, WeightRule
from snn_amd.lattice import IzhikevichNeuron, IzhikevichNeuronLattice

RULES = [ConnectionRule.all_to_all(), ConnectionRule.all_to_all(self_edges=False), ConnectionRule.chebyshev(1, self_edges=False),
         ConnectionRule.chebyshev(2), ConnectionRule.euclidean(5, probability=0.37, seed=21), ConnectionRule.same_position(),
         ConnectionRule.all_to_all(probability=0.0), ConnectionRule.chebyshev(2, probability=0.6, seed=31)]
WEIGHTS = [WeightRule.constant(0.25), WeightRule.uniform(0.5, 1.5, seed=22)]


def test_a_rule_built_lattice_of_9216_neurons_stays_far_below_one_matrix():
    """96 x 96: one N x N float32 matrix is 324 MiB.  populate, connect by record, a deep copy, 100 get_weight and 10 incoming /
    outgoing queries peak below 81 MiB, a quarter of one matrix (two grids of 9 216 Izhikevich neurons trace 15 MiB live / 23 MiB
    peak; the code before this test allocated 648 MiB in populate alone)."""
    side = 96
    rule, weight = ConnectionRule.chebyshev(2, self_edges=False), WeightRule.uniform(0.5, 1.5, seed=3)
    rng = np.random.default_rng(5)
    pairs = [((int(a), int(b)), (int(c), int(d))) for a, b, c, d in rng.integers(0, side, (70, 4))]
    pairs += [((r, c), (r + 1, c + 2)) for r, c in rng.integers(0, side - 2, (30, 2)).tolist()]         # pairs the rule connects
    places = [(0, 0), (0, side - 1), (side - 1, 0), (side - 1, side - 1), (1, 1)] + [(int(a), int(b)) for a, b in rng.integers(0, side, (5, 2))]
    tracemalloc.start()
    try:
        lattice = IzhikevichNeuronLattice(0)
        lattice.populate(IzhikevichNeuron(), side, side)
        lattice.connect(rule, weight)
        twin = copy.deepcopy(lattice)
        got_w = [twin.get_weight(a, b) for a, b in pairs]
        got_in = [twin.get_incoming_connections(p) for p in places]
        got_out = [twin.get_outgoing_connections(p) for p in places]
        peak = tracemalloc.get_traced_memory()[1]
    finally:
        tracemalloc.stop()
    print(f"peak traced memory {peak / 2 ** 20:.1f} MiB")
    assert peak < 81 * 2 ** 20, f"peak {peak / 2 ** 20:.1f} MiB: an N x N array was built"
    assert lattice.rule_held and twin.rule_held
    with pytest.raises(KeyError):
        twin.get_weight((0, 0), (side, 0))
    with pytest.raises(KeyError):
        twin.get_incoming_connections((-1, 0))
    # a separate step, after the measurement: the same lattice's matrices (reading them materialises)
    w, c = lattice.weights, lattice.connections
    assert not lattice.rule_held and w.shape == c.shape == (side * side, side * side) and w.dtype == np.float32 and c.dtype == np.uint32
    index = lambda p: p[0] * side + p[1]
    assert sum(1 for a, b in pairs if c[index(a), index(b)]) >= 30
    for (a, b), g in zip(pairs, got_w):
        assert g == (float(w[index(a), index(b)]) if c[index(a), index(b)] else 0.0) and isinstance(g, float)
        assert g == lattice.get_weight(a, b)
    for p, gi, go in zip(places, got_in, got_out):
        assert gi == {(i // side, i % side) for i in np.nonzero(c[:, index(p)])[0]} == lattice.get_incoming_connections(p)
        assert go == {(j // side, j % side) for j in np.nonzero(c[index(p)])[0]} == lattice.get_outgoing_connections(p)
        assert 8 <= len(gi) <= 24 and 8 <= len(go) <= 24


@pytest.mark.parametrize("rule", RULES, ids=repr)
def test_twins_on_chosen_rows_and_columns_are_slices_of_the_full_twins(rule):
    pre, post = (5, 7), (3, 5)
    rows, cols = np.array([34, 0, 7, 7, 19]), np.array([14, 3, 0])
    full = rule.mask(pre, post)
    assert np.array_equal(full, cases.expected_for(rule, WEIGHTS[0], pre, post)[0])
    assert np.array_equal(rule.mask(pre, post, pre_index=rows), full[rows])
    assert np.array_equal(rule.mask(pre, post, post_index=cols), full[:, cols])
    assert np.array_equal(rule.mask(pre, post, rows, cols), full[np.ix_(rows, cols)])
    assert rule.mask(pre, post, [], cols).shape == (0, 3)
    for weight in WEIGHTS:
        values = weight.values(pre, post)
        assert np.array_equal(weight.values(pre, post, pre_index=rows).view(np.uint32), values[rows].view(np.uint32))
        assert np.array_equal(weight.values(pre, post, post_index=cols).view(np.uint32), values[:, cols].view(np.uint32))
        assert np.array_equal(weight.values(pre, post, rows, cols).view(np.uint32), values[np.ix_(rows, cols)].view(np.uint32))
    with pytest.raises(IndexError):
        rule.mask(pre, post, pre_index=[35])
    with pytest.raises(IndexError):
        WEIGHTS[1].values(pre, post, post_index=[-1])


def by_hand(shape, rule, weight):
    on, w = cases.expected_for(rule, weight, shape, shape)
    return np.where(on, w, np.float32(0)).astype(np.float32), on.astype(np.uint32)


def by_closure(shape, condition, weight_of):
    n = shape[0] * shape[1]
    w, c = np.zeros((n, n), np.float32), np.zeros((n, n), np.uint32)
    for i in range(n):
        for j in range(n):
            a, b = (i // shape[1], i % shape[1]), (j // shape[1], j % shape[1])
            if condition(a, b):
                c[i, j], w[i, j] = 1, weight_of(a, b)
    return w, c


def test_records_and_closures_in_either_order():
    shape = (4, 5)
    rule, weight = ConnectionRule.chebyshev(1, self_edges=False), WeightRule.uniform(0.5, 1.5, seed=9)
    condition, weight_of = (lambda a, b: a[0] == b[0] and a != b), (lambda a, b: 1.0 + a[1] + b[1] / 8.0)
    # a record, then closures: the closures replace every pair
    l = IzhikevichNeuronLattice(3)
    l.populate(IzhikevichNeuron(), *shape)
    assert l.rule_held and l.get_weight((0, 0), (0, 1)) == 0.0 and l.get_outgoing_connections((1, 1)) == set()
    l.connect(rule, weight)
    assert l.rule_held
    l.connect(condition, weight_of)
    assert not l.rule_held
    w, c = by_closure(shape, condition, weight_of)
    assert np.array_equal(l.connections, c) and np.array_equal(l.weights.view(np.uint32), w.view(np.uint32))
    # closures, then a record: the record replaces every pair, and the lattice is rule-held again
    l.connect(rule, weight)
    assert l.rule_held
    w, c = by_hand(shape, rule, weight)
    assert l.get_weight((1, 1), (2, 2)) == float(w[6, 12]) != 0.0
    assert np.array_equal(l.connections, c) and np.array_equal(l.weights.view(np.uint32), w.view(np.uint32))
    assert l.weights.dtype == np.float32 and l.connections.dtype == np.uint32 and np.array_equal(l.get_weights(), w)
    # a populated lattice that was never connected: the empty matrices, as always
    e = IzhikevichNeuronLattice(4)
    e.populate(IzhikevichNeuron(), 2, 3)
    assert e.weights.shape == e.connections.shape == (6, 6) and not e.weights.any() and not e.connections.any()
    # a deep copy of a materialised lattice carries its matrices, not a reference to them
    k = copy.deepcopy(l)
    k.weights[0, 1] = 77.0
    assert l.weights[0, 1] != 77.0 and k._device is None
