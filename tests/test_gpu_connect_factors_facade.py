"""The associative-memory network of the reference's pipelines through the network classes, by records: a 6x6 excitatory lattice
connected with WeightRule.hopfield of three fixture patterns, a 3x3 inhibitory lattice that reaches it with WeightRule.per_post, a
Bernoulli record back and a same-position Poisson lattice -- against the same network connected with the reference's two
closures reading the fixture's matrices.  Dense and sparse handles, chemical synapses, 200 steps: histories, get_weight and the
incoming / outgoing lists agree, and the excitatory lattice is still rule-held afterwards."""
import numpy as np
import pytest

import connect_factors_cases as cases

pytestmark = pytest.mark.gpu

EXC, INH, TRAIN = 1, 2, 0
SHAPE, SMALL = (6, 6), (3, 3)
A, B, SCALAR = 0.3, 0.7, 1.7 / 3


def matrices():
    """the fixture's patterns on 36 cells, the reference's own get_weights matrix for them and its weights_ie table (inhibitory: negated)"""
    xi, _, _, _, w = cases.case("facade")
    return xi, w, np.ascontiguousarray(cases.data()["ie_table"][:6, :6]) * -4.0


def network(ln, by_rule, sparse):
    xi, w, w_ie = matrices()
    ampa = ln.IonotropicNeurotransmitterType.AMPA
    receptors = ln.Ionotropic()
    receptors.insert(ampa, ln.AMPAReceptor(g=3.0))
    neuron = ln.IzhikevichNeuron(gap_conductance=0.05, c_m=25.0)
    neuron.set_synaptic_neurotransmitters({ampa: ln.ApproximateNeurotransmitter()})
    neuron.set_receptors(receptors)
    rng = np.random.default_rng(9)
    neurons = []
    for id, shape in ((EXC, SHAPE), (INH, SMALL)):
        v = rng.uniform(neuron.c, neuron.v_th, shape).astype(np.float32)
        l = ln.IzhikevichNeuronLattice(id)
        l.populate(neuron, *shape)
        l.apply_given_position(lambda pos, n, v=v: setattr(n, "current_voltage", float(v[pos])))
        l.update_grid_history = True
        neurons.append(l)
    st = ln.PoissonNeuron(chance_of_firing=0.05)
    st.set_synaptic_neurotransmitters({ampa: ln.ApproximateNeurotransmitter()})
    train = ln.PoissonNeuronLattice(TRAIN)
    train.populate(st, *SHAPE)
    train.apply_given_position(lambda pos, n: setattr(n, "seed", 1 + pos[0] * SHAPE[1] + pos[1]))
    train.update_grid_history = True
    g = ln.IzhikevichNeuronNetworkGPU.generate_network(neurons, [train], sparse=sparse)
    i = lambda pos: pos[0] * SHAPE[1] + pos[1]
    back = ln.ConnectionRule.all_to_all(probability=0.4, seed=17)
    if by_rule:
        g.connect_internally(EXC, ln.ConnectionRule.all_to_all(self_edges=False), ln.WeightRule.hopfield(xi, a=A, b=B, scalar=SCALAR))
        g.connect(INH, EXC, ln.ConnectionRule.all_to_all(), ln.WeightRule.per_post(w_ie))
    else:
        g.connect_internally(EXC, lambda x, y: w[i(x)][i(y)] != 0, lambda x, y: w[i(x)][i(y)])
        g.connect(INH, EXC, lambda x, y: True, lambda x, y: w_ie[y])
    g.connect(EXC, INH, back, ln.WeightRule.constant(2.0))
    g.connect(TRAIN, EXC, ln.ConnectionRule.same_position(), ln.WeightRule.constant(5.0))
    g.electrical_synapse, g.chemical_synapse = True, True
    return g


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_hopfield_network_by_records_runs_as_its_closure_twin(snn, sparse):
    ln = snn
    a, b = network(ln, True, sparse), network(ln, False, sparse)
    for g in (a, b):
        g.run_lattices(200)
    assert a._dn.csr == b._dn.csr == sparse
    for id, shape in ((EXC, SHAPE), (INH, SMALL), (TRAIN, SHAPE)):
        ha, hb = a.history(id), b.history(id)
        assert ha.shape == (200,) + shape and np.array_equal(ha.view(np.uint32), hb.view(np.uint32)), f"history of lattice {id}"
    fired = [c.last_firing_time for row in b.get_lattice(EXC).cell_grid for c in row]
    assert any(t is not None for t in fired), "neurons must have fired"
    gp = ln.GraphPosition
    positions = [(0, 0), (2, 3), (5, 5), (4, 1)]
    xi, w, w_ie = matrices()
    for x in positions:
        for y in positions:
            got = a.get_weight(gp(EXC, x), gp(EXC, y))
            assert got == b.get_weight(gp(EXC, x), gp(EXC, y)) == float(np.float32(w[x[0] * 6 + x[1], y[0] * 6 + y[1]])), (x, y)
        for z in [(0, 0), (1, 2), (2, 2)]:
            assert a.get_weight(gp(INH, z), gp(EXC, x)) == b.get_weight(gp(INH, z), gp(EXC, x)) == float(np.float32(w_ie[x])), (z, x)
        assert a.get_incoming_connections_within_lattice(EXC, x) == b.get_incoming_connections_within_lattice(EXC, x)
        assert a.get_outgoing_connections_within_lattice(EXC, x) == b.get_outgoing_connections_within_lattice(EXC, x)
        assert a.get_incoming_connectings_across_lattices(EXC, x) == b.get_incoming_connectings_across_lattices(EXC, x)
        assert a.get_outgoing_connectings_across_lattices(EXC, x) == b.get_outgoing_connectings_across_lattices(EXC, x)
    assert len(a.get_incoming_connections_within_lattice(EXC, (2, 3))) > 0
    assert a.network.lattices[EXC].rule_held and not b.network.lattices[EXC].rule_held
    a.close()
    b.close()
