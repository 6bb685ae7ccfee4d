"""Rule-held lattices through the GPU classes: a network built with ConnectionRule / WeightRule records behaves, in everything the
classes let one observe, exactly as the same network built with the equivalent closures (the existing code path is the reference)
-- while its lattices hold no matrix on the host: the graph goes up as one device call per lattice plus one edit for the edges
between lattices, queries are answered by the device (right under plasticity), and weights come home only when the device copy
goes away and they may differ from the rule."""
import copy

import numpy as np
import pytest

from snn_amd import ConnectionRule, WeightRule

pytestmark = pytest.mark.gpu

SHAPE = (5, 7)
E1, I1, C1 = 1, 2, 0


def build(ln, records):
    """two 5x7 Izhikevich lattices connected all to all but for x == y (weights 5 and 3), a rate spike-train lattice, position to
    position edges between them (5, -3, 5); STDP on in the first lattice; grid histories on"""
    neuron = ln.IzhikevichNeuron(gap_conductance=0.05, c_m=25.0)      # loosely coupled: neurons fire one after the other
    rng = np.random.default_rng(8)
    v1, v2 = (rng.uniform(neuron.c, neuron.v_th, SHAPE).astype(np.float32) for _ in range(2))
    rates = rng.uniform(0.0, 100.0, SHAPE).astype(np.float32)
    train = ln.RateSpikeTrainLattice(C1)
    train.populate(ln.RateSpikeTrain(rate=100.0), *SHAPE)
    train.apply_given_position(lambda pos, n: setattr(n, "step", float(rates[pos])))
    train.update_grid_history = True
    lattices = []
    for id, v, weight in ((E1, v1, 5.0), (I1, v2, 3.0)):
        l = ln.IzhikevichNeuronLattice(id)
        l.populate(neuron, *SHAPE)
        l.apply_given_position(lambda pos, n, v=v: setattr(n, "current_voltage", float(v[pos])))
        if records:
            l.connect(ConnectionRule.all_to_all(self_edges=False), WeightRule.constant(weight))
        else:
            l.connect(lambda x, y: x != y, lambda x, y, weight=weight: weight)
        l.update_grid_history = True
        lattices.append(l)
    lattices[0].do_plasticity = True
    net = ln.IzhikevichNeuronNetwork.generate_network(lattices, [train])
    for pre, post, weight in ((E1, I1, 5.0), (I1, E1, -3.0), (C1, E1, 5.0)):
        if records:
            net.connect(pre, post, ConnectionRule.same_position(), WeightRule.constant(weight))
        else:
            net.connect(pre, post, lambda x, y: x == y, lambda x, y, weight=weight: weight)
    net.electrical_synapse, net.chemical_synapse = True, False
    return net


def state(lattice):
    cells = [c for row in lattice.cell_grid for c in row]
    return ([c.current_voltage for c in cells], [c.last_firing_time for c in cells], [c.is_spiking for c in cells])


def test_records_and_closures_give_the_same_network(snn):
    ln = snn
    host_r, host_c = build(ln, True), build(ln, False)
    assert all(l.rule_held for l in host_r.lattices.values()) and not any(l.rule_held for l in host_c.lattices.values())
    assert host_r.connecting == host_c.connecting and host_r.connecting_nodes == host_c.connecting_nodes
    r, c = ln.IzhikevichNeuronNetworkGPU.from_network(host_r), ln.IzhikevichNeuronNetworkGPU.from_network(host_c)
    assert all(l.rule_held for l in host_r.lattices.values()), "from_network must not materialise the caller's lattices"
    for g in (r, c):
        g.run_lattices(60)
    assert all(l.rule_held for l in r.network.lattices.values()), "a run must not materialise a rule-held lattice"
    for id in (E1, I1, C1):
        assert np.array_equal(r.history(id).view(np.uint32), c.history(id).view(np.uint32)), f"history of lattice {id}"
        assert r.history(id).shape == (60,) + SHAPE
    for id in (E1, I1):
        assert state(r.get_lattice(id)) == state(c.get_lattice(id))
        assert np.array_equal(r.get_lattice(id).history.view(np.uint32), c.get_lattice(id).history.view(np.uint32))
    assert any(t is not None for t in state(c.get_lattice(E1))[1]), "neurons must have fired"
    assert state(r.get_spike_train_lattice(C1)) == state(c.get_spike_train_lattice(C1))
    assert r.network.internal_clock == c.network.internal_clock == 60
    assert list(r.network.connecting.items()) == list(c.network.connecting.items())
    assert np.array_equal(np.asarray(r.connecting_weights).view(np.uint32), np.asarray(c.connecting_weights).view(np.uint32))
    assert r.connecting_position_to_index == c.connecting_position_to_index
    # queries on the rule-held lattices are answered by the device: the plastic lattice's weights are no longer its rule's
    pos = [(a, b) for a in range(SHAPE[0]) for b in range(SHAPE[1])]
    for id in (E1, I1):
        for a, b in zip(pos, pos[3:] + pos[:3]):
            got = r.get_weight(ln.GraphPosition(id, a), ln.GraphPosition(id, b))
            assert got == c.get_weight(ln.GraphPosition(id, a), ln.GraphPosition(id, b)) and isinstance(got, float)
        assert r.get_weight(ln.GraphPosition(id, (2, 2)), ln.GraphPosition(id, (2, 2))) == 0.0
        for p in ((0, 0), (2, 3), (4, 6)):
            assert r.get_incoming_connections_within_lattice(id, p) == c.get_incoming_connections_within_lattice(id, p) == set(pos) - {p}
            assert r.get_outgoing_connections_within_lattice(id, p) == c.get_outgoing_connections_within_lattice(id, p)
        with pytest.raises(KeyError):
            r.get_weight(ln.GraphPosition(id, (0, 0)), ln.GraphPosition(id, (5, 0)))
    cw, cc = c.get_lattice(E1).weights, c.get_lattice(E1).connections
    moved = np.argwhere((cc != 0) & (cw != np.float32(5.0)))
    assert len(moved) > 0, "STDP must have changed weights of the first lattice"
    for i, j in moved[:20]:
        assert r.get_weight(ln.GraphPosition(E1, pos[i]), ln.GraphPosition(E1, pos[j])) == float(cw[i, j]) != 5.0
    assert r.get_weight(ln.GraphPosition(C1, (1, 1)), ln.GraphPosition(E1, (1, 1))) == c.get_weight(ln.GraphPosition(C1, (1, 1)), ln.GraphPosition(E1, (1, 1)))
    assert all(l.rule_held for l in r.network.lattices.values()), "queries must not materialise"
    # a deep copy of a lattice whose weights live on the device brings them along, without the device
    twin = copy.deepcopy(r.get_lattice(E1))
    assert twin._device is None and not twin.rule_held
    assert np.array_equal(twin.weights.view(np.uint32), c.get_lattice(E1).weights.view(np.uint32))
    # a second run, then the device copy goes: the plastic lattice comes home, the static one stays with its rule
    for g in (r, c):
        g.run_lattices(20)
    lr, lc = r.get_lattice(I1), c.get_lattice(I1)
    r.close()
    c.close()
    assert lr.rule_held and lr._device is None
    for id in (E1, I1):
        a, b = r.get_lattice(id), c.get_lattice(id)
        assert np.array_equal(a.connections, b.connections) and np.array_equal(a.weights.view(np.uint32), b.weights.view(np.uint32)), id
        assert a.weights.dtype == np.float32 and a.connections.dtype == np.uint32
    assert (r.get_lattice(E1).weights[cc != 0] != np.float32(5.0)).any(), "the plastic lattice came home with what STDP made of its weights"
    # and the network goes on from the host copy exactly as the closure build does
    for g in (r, c):
        g.run_lattices(15)
    for id in (E1, I1):
        assert np.array_equal(r.history(id).view(np.uint32), c.history(id).view(np.uint32))
        assert np.array_equal(r.get_lattice(id).weights.view(np.uint32), c.get_lattice(id).weights.view(np.uint32))
    r.close()
    c.close()


def test_single_lattice_class_by_record(snn):
    ln = snn
    rule, weight = ConnectionRule.chebyshev(2, self_edges=False), WeightRule.uniform(0.5, 1.5, seed=3)
    on, w = rule.mask((9, 9), (9, 9)), weight.values((9, 9), (9, 9))
    rng = np.random.default_rng(2)
    v = rng.uniform(-65.0, 30.0, (9, 9)).astype(np.float32)
    a, b = ln.IzhikevichNeuronLatticeGPU(0), ln.IzhikevichNeuronLatticeGPU(0)
    for g in (a, b):
        g.populate(ln.IzhikevichNeuron(gap_conductance=10.0), 9, 9)
        g.apply_given_position(lambda pos, n: setattr(n, "current_voltage", float(v[pos])))
        g.update_grid_history = True
    a.connect(rule, weight)
    b.connect(lambda x, y: bool(on[x[0] * 9 + x[1], y[0] * 9 + y[1]]), lambda x, y: float(w[x[0] * 9 + x[1], y[0] * 9 + y[1]]))
    assert a.rule_held and not b.rule_held
    assert a.get_weight((0, 0), (1, 1)) == b.get_weight((0, 0), (1, 1)) != 0.0          # no handle yet: the twin answers
    for g in (a, b):
        g.run_lattice(30)
    assert a.rule_held, "run_lattice must not materialise"
    assert np.array_equal(a.history.view(np.uint32), b.history.view(np.uint32)) and a.history.shape == (30, 9, 9)
    for p, q in (((0, 0), (1, 1)), ((4, 4), (4, 4)), ((8, 8), (6, 7)), ((0, 0), (8, 8))):
        assert a.get_weight(p, q) == b.get_weight(p, q)
    for p in ((0, 0), (4, 4), (8, 3)):
        assert a.get_incoming_connections(p) == b.get_incoming_connections(p) and a.get_outgoing_connections(p) == b.get_outgoing_connections(p)
    assert a.get_neuron(3, 3).current_voltage == b.get_neuron(3, 3).current_voltage
    assert a.rule_held
    assert np.array_equal(a.weights.view(np.uint32), b.weights.view(np.uint32)) and not a.rule_held      # asked for: materialised
    # a closure connect on top replaces the graph as it always has
    for g in (a, b):
        g.connect(lambda x, y: x[0] == y[0] and x != y, lambda x, y: 2.0)
        g.run_lattice(10)
    assert np.array_equal(a.history.view(np.uint32), b.history.view(np.uint32))
    assert np.array_equal(a.weights.view(np.uint32), b.weights.view(np.uint32))
    a.close()
    b.close()
