"""Ring and torus attractors stated as ConnectionRule / WeightRule records through the Lixirnet-style classes: a head-direction
ring (three 12x1 lattices and two rate cells, connected among each other with the three weight forms of connect_spec_cases) and
a 6x6 torus.  The rule-built network holds no N x N host matrix after from_network, answers get_weight / get_incoming_connections
as its closure-built twin does, and steps to the same voltage history, bit for bit."""
import numpy as np
import pytest

import connect_spec_cases as cases
import parity

pytestmark = pytest.mark.gpu

RING = (12, 1)
SHIFT_RIGHT, SHIFT_LEFT, HD, CELLS = 0, 1, 2, 3


def ring_network(ln, by_rule):
    forms = cases.attractor_forms(RING)
    neuron = ln.IzhikevichNeuron(gap_conductance=10.0)
    init = np.random.default_rng(5).uniform(-65, 30, (3,) + RING).astype(np.float32)
    lattices = []
    for id in (SHIFT_RIGHT, SHIFT_LEFT, HD):
        l = ln.IzhikevichNeuronLattice(id)
        l.populate(neuron, *RING)
        l.apply_given_position(lambda pos, n, id=id: setattr(n, "current_voltage", float(init[id][pos])))
        l.update_grid_history = True
        lattices.append(l)
    cells = ln.RateSpikeTrainLattice(CELLS)
    cells.populate(ln.RateSpikeTrain(rate=1.5), 1, 2)
    net = ln.IzhikevichNeuronNetwork.generate_network(lattices, [cells])
    everything = lambda a, b: True
    left = cases.shift(RING, -20.0)
    plan = [(HD, HD, forms["bump"]), (CELLS, SHIFT_RIGHT, lambda a, b: 10.0), (SHIFT_RIGHT, HD, forms["shift"]), (SHIFT_LEFT, HD, left),
            (HD, SHIFT_RIGHT, forms["scaled_bump"]), (HD, SHIFT_LEFT, forms["scaled_bump"])]
    for pre, post, fn in plan:
        if not by_rule:
            net.connect(pre, post, everything, fn)
        elif pre == CELLS:
            net.connect(pre, post, ln.ConnectionRule.all_to_all(), ln.WeightRule.constant(10.0))
        else:
            net.connect(pre, post, ln.ConnectionRule.all_to_all(wrap=True), ln.WeightRule.from_displacement_function(fn, RING, RING, wrap=True))
    net.electrical_synapse = True
    net.chemical_synapse = False
    return net


def test_head_direction_ring_by_rules(snn):
    ln = snn
    a, b = ring_network(ln, True), ring_network(ln, False)
    ga, gb = ln.IzhikevichNeuronNetworkGPU.from_network(a), ln.IzhikevichNeuronNetworkGPU.from_network(b)
    ga.run_lattices(0)                                           # (the handle exists from here on)
    assert all(l.rule_held for l in ga.network.lattices.values()), "a rule-built lattice must not hold host matrices"
    hd_a, hd_b = ga.network.lattices[HD], gb.network.lattices[HD]
    for pre, post in [((0, 0), (11, 0)), ((11, 0), (0, 0)), ((3, 0), (9, 0)), ((5, 0), (5, 0))]:
        assert np.float32(hd_a.get_weight(pre, post)) == np.float32(hd_b.get_weight(pre, post)) != 0
        for ids in ((SHIFT_RIGHT, HD), (SHIFT_LEFT, HD), (HD, SHIFT_RIGHT), (HD, SHIFT_LEFT)):
            x, y = ln.GraphPosition(ids[0], pre), ln.GraphPosition(ids[1], post)
            assert np.float32(ga.network.get_weight(x, y)) == np.float32(gb.network.get_weight(x, y))
    assert np.float32(ga.network.get_weight(ln.GraphPosition(SHIFT_RIGHT, (0, 0)), ln.GraphPosition(HD, (1, 0)))) == \
        -np.float32(ga.network.get_weight(ln.GraphPosition(SHIFT_LEFT, (0, 0)), ln.GraphPosition(HD, (1, 0)))) != 0
    assert hd_a.get_incoming_connections((0, 0)) == hd_b.get_incoming_connections((0, 0)) == {(r, 0) for r in range(12)}
    assert hd_a.get_outgoing_connections((11, 0)) == hd_b.get_outgoing_connections((11, 0))
    assert hd_a.rule_held, "single rows and columns come from the device, not from a matrix"
    ga.run_lattices(50)
    gb.run_lattices(50)
    for id in (SHIFT_RIGHT, SHIFT_LEFT, HD):
        ha, hb = ga.history(id), gb.history(id)
        assert ha.shape == (50,) + RING and np.array_equal(parity.bits(ha), parity.bits(hb)), f"voltage history of lattice {id}"
    assert len(np.unique(ga.history(HD)[-1])) > 1
    assert all(l.rule_held for l in ga.network.lattices.values())
    # the matrix, once asked for, is the closure's
    assert np.array_equal(parity.bits(hd_a.weights), parity.bits(hd_b.weights)) and np.array_equal(hd_a.connections, hd_b.connections)
    ga.close()
    gb.close()


def test_torus_by_rules(snn):
    ln = snn
    shape = (6, 6)
    fn = cases.attractor_forms(shape)["bump"]
    init = np.random.default_rng(6).uniform(-65, 30, shape).astype(np.float32)
    nets = []
    for by_rule in (True, False):
        l = ln.IzhikevichNeuronLattice(0)
        l.populate(ln.IzhikevichNeuron(gap_conductance=10.0), *shape)
        l.apply_given_position(lambda pos, n: setattr(n, "current_voltage", float(init[pos])))
        l.update_grid_history = True
        if by_rule:                                              # a radius on the torus, the table inside it; no self edges
            l.connect(ln.ConnectionRule.chebyshev(2, self_edges=False, wrap=True), ln.WeightRule.from_displacement_function(fn, shape, shape, wrap=True))
        else:
            ring = cases.ring_distance
            l.connect(lambda a, b: a != b and max(ring(6, a[0], b[0]), ring(6, a[1], b[1])) <= 2, fn)
        nets.append(ln.IzhikevichNeuronNetwork.generate_network([l], []))
    ga, gb = (ln.IzhikevichNeuronNetworkGPU.from_network(n) for n in nets)
    ga.run_lattices(0)
    la, lb = ga.network.lattices[0], gb.network.lattices[0]
    assert la.rule_held
    for pre, post in [((0, 0), (5, 5)), ((0, 0), (4, 4)), ((0, 0), (3, 3)), ((5, 0), (0, 5)), ((2, 2), (2, 2))]:
        assert np.float32(la.get_weight(pre, post)) == np.float32(lb.get_weight(pre, post))
    assert la.get_weight((0, 0), (3, 3)) == 0.0 and la.get_weight((0, 0), (4, 4)) != 0.0
    assert la.get_incoming_connections((0, 0)) == lb.get_incoming_connections((0, 0)) and len(la.get_incoming_connections((0, 0))) == 24
    assert la.get_outgoing_connections((5, 5)) == lb.get_outgoing_connections((5, 5))
    assert la.rule_held
    ga.run_lattices(50)
    gb.run_lattices(50)
    assert np.array_equal(parity.bits(ga.history(0)), parity.bits(gb.history(0))) and ga.history(0).shape == (50, 6, 6)
    assert la.rule_held
    ga.close()
    gb.close()
