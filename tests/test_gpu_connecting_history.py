"""update_connecting_graph_history through the network classes (LatticeNetwork::iterate*, neuron/mod.rs:2463-2465: the connecting
graph's weights after every step), dense and sparse, and update_graph_history of a lattice on a sparse handle -- both served by the
device's edge recorder.  Bit-exact against the oracle stepped one step at a time."""
import numpy as np
import pytest

import oracle_binding as ob
import parity
from snn_amd import ConnectionRule, WeightRule

pytestmark = pytest.mark.gpu

FIRING = [5.0, 6.0, 2.5]                # one firing period per preset spike train, in ms
WEIGHTS = [1.5, 2.0, 2.5]
STEPS = 500


def stdp_example_oracle():
    """the oracle's side of the example: the weights of the three spike train -> neuron edges after every step"""
    o = parity.make_oracle(parity.Layout([(1, 1, 1)], [(0, 3, 1)]), st_kind=ob.ST_PRESET)
    o["gap_conductance"] = 10.0
    o.set_firing_times([[t] for t in FIRING])
    o["connections"][1:, 0] = 1
    o["weights"][1:, 0] = WEIGHTS
    o["do_plasticity"] = 1
    rows = []
    for _ in range(STEPS):
        o.run(1)
        rows.append(o["weights"][1:, 0].copy())
    return np.array(rows)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_stdp_example_of_the_reference(snn, sparse):
    """backend/src/lib.rs:124-196 re-expressed: a line of preset spike trains with distinct firing periods drives one Izhikevich
    neuron with STDP; the example returns network.get_connecting_graph().history, the weight of every spike train -> neuron edge
    after every step."""
    ln = snn
    want = stdp_example_oracle()
    assert np.any(want[0] != want[-1]), "STDP must have moved a weight"
    trains = ln.PresetSpikeTrainLattice(0)
    trains.populate(ln.PresetSpikeTrain(), len(FIRING), 1)
    trains.apply_given_position(lambda pos, cell: setattr(cell, "firing_times", [FIRING[pos[0]]]))
    trains.update_grid_history = True
    lattice = ln.IzhikevichNeuronLattice(1)
    lattice.populate(ln.IzhikevichNeuron(gap_conductance=10.0), 1, 1)
    lattice.do_plasticity = True
    lattice.update_grid_history = True
    network = ln.IzhikevichNeuronNetwork.generate_network([lattice], [trains])
    network.connect(0, 1, lambda x, y: True, lambda x, y: WEIGHTS[x[0]])
    network.update_connecting_graph_history = True
    network.electrical_synapse, network.chemical_synapse = True, False
    gpu = ln.IzhikevichNeuronNetworkGPU.from_network(network, sparse=sparse)
    gpu.run_lattices(STEPS)
    history = gpu.network.connecting_graph_history
    assert len(history) == STEPS and history.weights.shape == (STEPS, 3) and history.connected.all()
    edges = [(ln.GraphPosition(0, (i, 0)), ln.GraphPosition(1, (0, 0))) for i in range(3)]
    assert set(history.edges) == set(edges)
    for t in (0, 250, STEPS - 1):
        assert set(history[t]) == set(edges)
    for i, edge in enumerate(edges):
        column = history.weights[:, history.edges.index(edge)]
        assert np.array_equal(parity.bits(column), parity.bits(want[:, i])), f"edge from spike train {i}"
        assert np.float32(history[STEPS - 1][edge]) == want[-1, i] == np.float32(gpu.network.connecting[edge])
    assert gpu.history(1).shape[0] == STEPS                      # one step axis with the grid histories
    # reset_graph_history (neuron/mod.rs:1728) clears the record
    gpu.reset_graph_history()
    assert len(gpu.network.connecting_graph_history) == 0
    gpu.run_lattices(3)
    assert len(gpu.network.connecting_graph_history) == 3
    gpu.close()


E1, E2 = 1, 2
SHAPES = {E1: (5, 6), E2: (4, 4)}
INSIDE = {E1: (ConnectionRule.chebyshev(1, self_edges=False), WeightRule.uniform(3.0, 6.0, seed=11)),
          E2: (ConnectionRule.chebyshev(1, self_edges=False), WeightRule.constant(3.0))}
BETWEEN = [(E1, E2, ConnectionRule.all_to_all(probability=0.3, seed=5), WeightRule.uniform(1.0, 2.0, seed=6)),
           (E2, E1, ConnectionRule.all_to_all(probability=0.3, seed=7), WeightRule.constant(2.0))]
RUN = 120


def voltages(id):
    return np.random.default_rng(8 + id).uniform(-65.0, 30.0, SHAPES[id]).astype(np.float32)


def two_lattices(ln, sparse):
    neuron = ln.IzhikevichNeuron(gap_conductance=0.05, c_m=25.0)      # loosely coupled: neurons fire one after the other
    lattices = []
    for id in (E1, E2):
        v = voltages(id)
        l = ln.IzhikevichNeuronLattice(id)
        l.populate(neuron, *SHAPES[id])
        l.apply_given_position(lambda pos, n, v=v: setattr(n, "current_voltage", float(v[pos])))
        l.do_plasticity = True
        lattices.append(l)
    g = ln.IzhikevichNeuronNetworkGPU.generate_network(lattices, [], sparse=sparse)
    for id, (rule, weight) in INSIDE.items():
        g.connect_internally(id, rule, weight)
    for pre, post, rule, weight in BETWEEN:
        g.connect(pre, post, rule, weight)
    g.electrical_synapse, g.chemical_synapse = True, False
    g.update_connecting_graph_history = True
    g.set_update_graph_history(E1, True)
    return g


def two_lattice_oracle():
    """the same network from the rules' host twins; returns (before [steps, n, n_neurons], after [...]) of the whole matrix"""
    o = parity.make_oracle(parity.Layout([(id, *SHAPES[id]) for id in (E1, E2)]))
    first = {E1: 0, E2: SHAPES[E1][0] * SHAPES[E1][1]}
    size = {id: SHAPES[id][0] * SHAPES[id][1] for id in SHAPES}
    o["gap_conductance"] = 0.05
    o["c_m"] = 25.0
    o["current_voltage"] = np.concatenate([voltages(E1).reshape(-1), voltages(E2).reshape(-1)])
    for pre, post, rule, weight in [(id, id, *INSIDE[id]) for id in INSIDE] + BETWEEN:
        on, w = rule.mask(SHAPES[pre], SHAPES[post]), weight.values(SHAPES[pre], SHAPES[post])
        block = (slice(first[pre], first[pre] + size[pre]), slice(first[post], first[post] + size[post]))
        o["connections"][block] = on
        o["weights"][block] = np.where(on, w, 0)
    o["do_plasticity"] = 1
    before, after = [], []
    for _ in range(RUN):
        before.append(np.where(o["connections"] != 0, o["weights"], np.float32(0)))
        o.run(1)
        after.append(np.where(o["connections"] != 0, o["weights"], np.float32(0)))
    return np.array(before), np.array(after), o["connections"] != 0, first, size


def test_sparse_network_with_a_rule_held_lattice_and_a_record_block(snn):
    ln = snn
    before, after, on, first, size = two_lattice_oracle()
    n1 = size[E1]
    assert np.any(after[0][:n1, n1:] != after[-1][:n1, n1:]) and np.any(before[0][:n1, :n1] != before[-1][:n1, :n1]), "weights must have moved"
    s, d = two_lattices(ln, True), two_lattices(ln, False)
    assert s.network.lattices[E1].rule_held and set(s.network.connecting_rules) == {(E1, E2), (E2, E1)} and not s.network.connecting
    for g in (s, d):
        g.run_lattices(RUN)
    assert s._dn.csr and not d._dn.csr
    assert s.network.lattices[E1].rule_held and set(s.network.connecting_rules) == {(E1, E2), (E2, E1)}, \
        "recording keeps the rule-held pieces on the device"

    def index(gp):
        return first[gp.id] + gp.pos[0] * SHAPES[gp.id][1] + gp.pos[1]

    # the connecting graph: every edge between the lattices, after the step's weight updates
    cross = on.copy()
    cross[:n1, :n1] = cross[n1:, n1:] = False
    for g in (s, d):
        h = g.network.connecting_graph_history
        assert len(h) == RUN and h.connected.all() and len(h.edges) == cross.sum() == h.weights.shape[1]
        pre, post = np.array([index(a) for a, _ in h.edges]), np.array([index(b) for _, b in h.edges])
        assert cross[pre, post].all() and len(set(zip(pre.tolist(), post.tolist()))) == len(h.edges)
        assert np.array_equal(parity.bits(h.weights), parity.bits(after[:, pre, post]))
        a, b = h.edges[5]
        assert np.float32(h[RUN - 1][(a, b)]) == after[-1, index(a), index(b)]
    # lattice E1's own graph: before the step's weight updates (a lattice inside a network)
    h = s.graph_history(E1)
    want = before[:, :n1, :n1]
    assert len(h) == RUN and h.size == n1 and len(h.edges) == on[:n1, :n1].sum() and h.connected.all()
    assert np.array_equal(parity.bits(h.dense()), parity.bits(want))
    dense = d.graph_history(E1)
    for t in (0, 1, RUN // 2, RUN - 1):
        assert np.array_equal(parity.bits(h.dense()[t]), parity.bits(dense[t]))
    p, q = h.edges[3]
    assert np.float32(h[RUN - 1][(p, q)]) == want[-1, p, q]
    assert np.array_equal(parity.bits(s.network.lattices[E1].weights_history), parity.bits(d.network.lattices[E1].weights_history))
    # closing brings the plastic pieces home by the existing rules: both ran with plasticity, so they are materialised
    s.close()
    d.close()
    assert not s.network.lattices[E1].rule_held and not s.network.connecting_rules
    assert np.array_equal(parity.bits(s.network.lattices[E1].weights), parity.bits(d.network.lattices[E1].weights))


def test_single_lattice_class_on_a_sparse_handle_records_its_graph(snn):
    """LatticeGPU(sparse=True) with update_graph_history: the lattice's stored edges after the step's weight updates (a lone
    Lattice, neuron/mod.rs:904-910), equal to the [steps, n, n] snapshots of the dense class"""
    ln = snn
    rule, weight = ConnectionRule.chebyshev(2, self_edges=False), WeightRule.uniform(3.0, 6.0, seed=3)
    v = np.random.default_rng(2).uniform(-65.0, 30.0, (9, 9)).astype(np.float32)
    a, b = ln.IzhikevichNeuronLatticeGPU(0, sparse=True), ln.IzhikevichNeuronLatticeGPU(0)
    for g in (a, b):
        g.populate(ln.IzhikevichNeuron(gap_conductance=0.05, c_m=25.0), 9, 9)
        g.apply_given_position(lambda pos, n: setattr(n, "current_voltage", float(v[pos])))
        g.connect(rule, weight)
        g.do_plasticity = True
        g.update_graph_history = True
        g.run_lattice(80)
    assert a._net._dn.csr and not b._net._dn.csr
    h, want = a.graph_history, b.graph_history
    assert len(h) == 80 and want.shape == (80, 81, 81) and h.connected.all() and len(h.edges) == rule.mask((9, 9), (9, 9)).sum()
    assert np.array_equal(parity.bits(h.dense()), parity.bits(want))
    assert np.any(parity.bits(want[0]) != parity.bits(want[-1])), "weights must have moved"
    a.close()
    b.close()
