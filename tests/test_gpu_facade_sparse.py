"""The network classes on a sparse handle: LatticeNetworkGPU(sparse=True) / LatticeGPU(sparse=True) against the dense default, which
is the trusted path -- grid histories bit for bit with and without STDP, the same answers to get_weight / incoming / outgoing inside
lattices and across them, a mixed network (closures, records, dict edges) uploaded through the host-CSR-then-merge route to the
same graph, and record blocks that come home with the device's weights after a plastic run."""
import numpy as np
import pytest

from snn_amd import ConnectionRule, WeightRule

pytestmark = pytest.mark.gpu

SHAPE = (9, 11)
E1, E2, P0 = 1, 2, 0
INSIDE = {E1: (ConnectionRule.euclidean(8, self_edges=False), WeightRule.uniform(3.0, 6.0, seed=11)),
          E2: (ConnectionRule.chebyshev(2, self_edges=False), WeightRule.constant(3.0))}
BETWEEN = [(E1, E2, ConnectionRule.same_position(), WeightRule.constant(5.0)),
           (E2, E1, ConnectionRule.all_to_all(probability=0.15, seed=5), WeightRule.uniform(-1.0, 2.0, seed=6)),     # thinned, uniform
           (P0, E1, ConnectionRule.same_position(), WeightRule.constant(5.0))]
POSITIONS = [(0, 0), (4, 5), (8, 10), (3, 0), (0, 7)]


def lattices(ln, plastic):
    neuron = ln.IzhikevichNeuron(gap_conductance=0.05, c_m=25.0)      # loosely coupled: neurons fire one after the other
    rng = np.random.default_rng(8)
    out = []
    for id in (E1, E2):
        v = rng.uniform(neuron.c, neuron.v_th, SHAPE).astype(np.float32)
        l = ln.IzhikevichNeuronLattice(id)
        l.populate(neuron, *SHAPE)
        l.apply_given_position(lambda pos, n, v=v: setattr(n, "current_voltage", float(v[pos])))
        l.update_grid_history = True
        l.do_plasticity = plastic
        out.append(l)
    train = ln.PoissonNeuronLattice(P0)
    train.populate(ln.PoissonNeuron(chance_of_firing=0.05), *SHAPE)
    train.apply_given_position(lambda pos, n: setattr(n, "seed", 1 + pos[0] * SHAPE[1] + pos[1]))
    train.update_grid_history = True
    return out, [train]


def by_records(ln, sparse, plastic):
    """the whole network by records, built through the GPU class"""
    neurons, trains = lattices(ln, plastic)
    g = ln.IzhikevichNeuronNetworkGPU.generate_network(neurons, trains, sparse=sparse)
    for id, (rule, weight) in INSIDE.items():
        g.connect_internally(id, rule, weight)
    for pre, post, rule, weight in BETWEEN:
        g.connect(pre, post, rule, weight)
    g.electrical_synapse, g.chemical_synapse = True, False
    return g


def gp(ln, id, pos):
    return ln.GraphPosition(id, pos)


def assert_same_queries(ln, s, d):
    for id in (E1, E2):
        for a in POSITIONS:
            for b in POSITIONS + [(a[0], (a[1] + 1) % SHAPE[1]), ((a[0] + 2) % SHAPE[0], a[1])]:
                got = s.get_weight(gp(ln, id, a), gp(ln, id, b))
                assert isinstance(got, float) and got == d.get_weight(gp(ln, id, a), gp(ln, id, b)), (id, a, b)
            assert s.get_incoming_connections_within_lattice(id, a) == d.get_incoming_connections_within_lattice(id, a)
            assert s.get_outgoing_connections_within_lattice(id, a) == d.get_outgoing_connections_within_lattice(id, a)
            assert s.get_incoming_connectings_across_lattices(id, a) == d.get_incoming_connectings_across_lattices(id, a), (id, a)
            assert s.get_outgoing_connectings_across_lattices(id, a) == d.get_outgoing_connectings_across_lattices(id, a), (id, a)
    for pre, post, _, _ in BETWEEN:
        for a in POSITIONS:
            for b in POSITIONS:
                assert s.get_weight(gp(ln, pre, a), gp(ln, post, b)) == d.get_weight(gp(ln, pre, a), gp(ln, post, b)), (pre, a, post, b)
    assert len(s.get_incoming_connectings_across_lattices(E1, (4, 5))) > 2, "the thinned block and the cells both reach this neuron"
    assert s.get_weight(gp(ln, E1, (4, 5)), gp(ln, E2, (4, 5))) == 5.0 and s.get_weight(gp(ln, E1, (4, 5)), gp(ln, E2, (4, 6))) == 0.0


@pytest.mark.parametrize("plastic", [False, True], ids=["static", "stdp"])
def test_sparse_and_dense_networks_run_alike(snn, plastic):
    ln = snn
    s, d = by_records(ln, True, plastic), by_records(ln, False, plastic)
    assert s.network.hold_connecting_rules and set(s.network.connecting_rules) == {(a, b) for a, b, _, _ in BETWEEN}
    assert not s.network.connecting and len(d.network.connecting) > 0 and not d.network.connecting_rules
    assert_same_queries(ln, s, d)                                   # no handle yet: the records' twins answer
    for g in (s, d):
        g.run_lattices(50)
    assert s._dn.csr and not d._dn.csr
    assert all(l.rule_held for l in s.network.lattices.values()) and len(s.network.connecting_rules) == 3 and not s.network.connecting, \
        "a run keeps the rule-held pieces on the device"
    for id in (E1, E2, P0):
        assert s.history(id).shape == (50,) + SHAPE
        assert np.array_equal(s.history(id).view(np.uint32), d.history(id).view(np.uint32)), f"history of lattice {id}"
    fired = [c.last_firing_time for row in d.get_lattice(E1).cell_grid for c in row]
    assert any(t is not None for t in fired), "neurons must have fired"
    assert_same_queries(ln, s, d)                                   # the device answers, right under plasticity
    if plastic:
        rule_w = INSIDE[E2][1].lo
        moved = [(a, b) for a in POSITIONS for b in d.get_outgoing_connections_within_lattice(E2, a)
                 if d.get_weight(gp(ln, E2, a), gp(ln, E2, b)) != rule_w]
        assert moved, "STDP must have changed weights"
        assert all(s.get_weight(gp(ln, E2, a), gp(ln, E2, b)) == d.get_weight(gp(ln, E2, a), gp(ln, E2, b)) for a, b in moved)
    for g in (s, d):
        g.run_lattices(10)
    for id in (E1, E2, P0):
        assert np.array_equal(s.history(id).view(np.uint32), d.history(id).view(np.uint32))
    s.close()
    d.close()


def test_record_blocks_come_home_with_the_device_weights_after_a_plastic_run(snn):
    ln = snn
    s, d = by_records(ln, True, True), by_records(ln, False, True)
    for g in (s, d):
        g.set_do_plasticity(E2, False)                               # E1 plastic, E2 static
        g.connect(P0, E2, ConnectionRule.same_position(), WeightRule.constant(2.0))       # a block neither end of which is plastic
    for g in (s, d):
        g.run_lattices(50)
    s.close()
    d.close()
    net, want = s.network, d.network
    # blocks into and out of the plastic lattice became dict blocks with what STDP made of them (its rule moves the weights of both);
    # the block between two static lattices is still its record
    assert set(net.connecting_rules) == {(P0, E2)}
    blocks = {(E2, E1), (P0, E1), (E1, E2)}
    expected = {k: v for k, v in want.connecting.items() if (k[0].id, k[1].id) in blocks}
    assert set(net.connecting) == set(expected) and len(expected) > 0
    assert all(np.float32(net.connecting[k]) == np.float32(v) for k, v in expected.items())
    rule_on, rule_w = BETWEEN[1][2].mask(SHAPE, SHAPE), BETWEEN[1][3].values(SHAPE, SHAPE)
    cols = SHAPE[1]
    changed = sum(np.float32(v) != rule_w[k[0].pos[0] * cols + k[0].pos[1], k[1].pos[0] * cols + k[1].pos[1]]
                  for k, v in net.connecting.items() if k[0].id == E2)
    assert changed > 0 and rule_on.sum() == sum(k[0].id == E2 for k in net.connecting), "the structure is the rule's, the weights are the device's"
    a, b = net.lattices[E1], want.lattices[E1]
    assert not a.rule_held and np.array_equal(a.connections, b.connections) and np.array_equal(a.weights.view(np.uint32), b.weights.view(np.uint32))
    assert net.lattices[E2].rule_held
    # ... and the network goes on from the host copy (host CSR first, then the merge of the records) as the dense one does
    for g in (s, d):
        g.run_lattices(10)
    for id in (E1, E2, P0):
        assert np.array_equal(s.history(id).view(np.uint32), d.history(id).view(np.uint32))
    s.close()
    d.close()


def test_a_mixed_network_uploads_to_the_same_graph(snn):
    ln = snn
    on, w = INSIDE[E1][0].mask(SHAPE, SHAPE), INSIDE[E1][1].values(SHAPE, SHAPE)
    cols = SHAPE[1]

    def mixed(sparse):
        neurons, trains = lattices(ln, False)
        g = ln.IzhikevichNeuronNetworkGPU.generate_network(neurons, trains, sparse=sparse)
        g.connect_internally(E1, lambda x, y: bool(on[x[0] * cols + x[1], y[0] * cols + y[1]]),
                             lambda x, y: float(w[x[0] * cols + x[1], y[0] * cols + y[1]]))            # closures: materialised
        g.connect_internally(E2, *INSIDE[E2])                                                             # a record: rule-held
        g.connect(E1, E2, lambda x, y: x[0] == y[0] and abs(x[1] - y[1]) <= 1, lambda x, y: 0.5 + 0.25 * y[1])    # dict edges
        g.connect(E2, E1, *BETWEEN[1][2:])                                                                # a record block (sparse) / dict (dense)
        g.connect(P0, E1, *BETWEEN[2][2:])
        return g

    s, d = mixed(True), mixed(False)
    assert not s.network.lattices[E1].rule_held and s.network.lattices[E2].rule_held
    assert s.network.connecting and set(s.network.connecting_rules) == {(E2, E1), (P0, E1)}
    sd, dd = s._ensure(), d._ensure()
    assert sd.csr and not dd.csr and sd.n_tot == dd.n_tot == 3 * SHAPE[0] * SHAPE[1]
    pre, post = np.meshgrid(np.arange(sd.n_tot, dtype=np.uint32), np.arange(sd.n_neurons, dtype=np.uint32), indexing="ij")
    ws, cs = sd.graph_lookup(pre.reshape(-1), post.reshape(-1))
    wd, cd = dd.graph_lookup(pre.reshape(-1), post.reshape(-1))
    assert np.array_equal(cs, cd) and np.array_equal(ws.view(np.uint32), wd.view(np.uint32)) and cs.sum() > 1000
    for g in (s, d):
        g.run_lattices(20)
    for id in (E1, E2, P0):
        assert np.array_equal(s.history(id).view(np.uint32), d.history(id).view(np.uint32))
    # the download on a sparse handle: the materialised lattice's block from the CSR arrays, the dict through one lookup
    a, b = s.get_lattice(E1), d.get_lattice(E1)
    assert np.array_equal(a.connections, b.connections) and np.array_equal(a.weights.view(np.uint32), b.weights.view(np.uint32))
    shared = [k for k in s.network.connecting]
    assert shared and all(np.float32(s.network.connecting[k]) == np.float32(d.network.connecting[k]) for k in shared)
    s.close()
    d.close()


def test_single_lattice_class_on_a_sparse_handle(snn):
    ln = snn
    rule, weight = ConnectionRule.chebyshev(2, self_edges=False), WeightRule.uniform(0.5, 1.5, seed=3)
    v = np.random.default_rng(2).uniform(-65.0, 30.0, (9, 9)).astype(np.float32)
    a, b = ln.IzhikevichNeuronLatticeGPU(0, sparse=True), ln.IzhikevichNeuronLatticeGPU(0)
    for g in (a, b):
        g.populate(ln.IzhikevichNeuron(gap_conductance=10.0), 9, 9)
        g.apply_given_position(lambda pos, n: setattr(n, "current_voltage", float(v[pos])))
        g.update_grid_history = True
        g.connect(rule, weight)
        g.run_lattice(30)
    assert a._net._dn.csr and not b._net._dn.csr and a.rule_held
    assert np.array_equal(a.history.view(np.uint32), b.history.view(np.uint32)) and a.history.shape == (30, 9, 9)
    for p, q in (((0, 0), (1, 1)), ((4, 4), (4, 4)), ((8, 8), (6, 7)), ((0, 0), (8, 8))):
        assert a.get_weight(p, q) == b.get_weight(p, q)
    for p in ((0, 0), (4, 4), (8, 3)):
        assert a.get_incoming_connections(p) == b.get_incoming_connections(p) and a.get_outgoing_connections(p) == b.get_outgoing_connections(p)
    assert np.array_equal(a.weights.view(np.uint32), b.weights.view(np.uint32)) and not a.rule_held      # asked for: from the CSR arrays
    for g in (a, b):
        g.run_lattice(10)                                                                                  # a materialised lattice: host CSR
    assert np.array_equal(a.history.view(np.uint32), b.history.view(np.uint32))
    a.close()
    b.close()
