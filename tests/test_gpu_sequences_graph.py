"""Random sequences of C-ABI calls that write, record and read the GRAPH between runs -- snn_graph_edit, snn_graph_csr_edit,
snn_graph_csr_edit_structure, the connect-by-rule calls of both graph forms, wholesale writes with a new mask, the four lookups
and line reads, edge-weight and graph histories, a checkpoint round trip -- interleaved with the runs, writes, switches and
toggles of test_gpu_sequences.py, on one handle against the same sequence on the oracle.  The generator, its ops and what is out
of scope: tests/sequence_graph_ops.py; the conditions it meets: tests/test_sequences_graph_plan.py.
SNN_RANDOM_SEEDS_SEQUENCES_GRAPH=n widens the sweep (the suite keeps the usable seeds of range(60))."""
import os

import numpy as np
import pytest

import oracle_binding as ob
import parity
import sequence_graph_ops as ops

pytestmark = pytest.mark.gpu

SEEDS = ops.seeds(int(os.environ.get("SNN_RANDOM_SEEDS_SEQUENCES_GRAPH", "60")))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_graph_call_sequence(snn, seed):
    """state, clock, graph weights and (sparse handles) graph structure equal the oracle's at the end of the sequence, every read
    and record on the way; a mismatch carries the log of ops"""
    ops.play(snn, seed)


def test_graph_history_switched_on_again_after_the_capacity_grew(snn):
    """Found by seed 103 of a wider sweep: lattice 0's graph history recorded ONE step and was switched off, another lattice's
    history then grew the handle's common history capacity, and lattice 0's history -- switched on again -- recorded 20 rows into
    the buffer it had kept from the one-step record, which the capacity check took for large enough.  The record is the oracle's."""
    net = parity.make_oracle(parity.Layout([(0, 4, 5), (3, 3, 7)]))
    net["current_voltage"] = ob.uniform_array(5, net.n_neurons, -65.0, 30.0)
    net["gap_conductance"] = 10.0
    net.fill_graph(6, 0.5, 1.5)
    net["do_plasticity"] = 1
    dn = parity.device_from_oracle(snn, net)
    ranges = net.layout.ranges()
    for lattice, steps in ((0, 1), (3, 30), (0, 20)):
        first, count, _ = ranges[lattice]
        dn.set_graph_history(lattice, 1)
        dn.run(steps)
        want = []
        for _ in range(steps):
            net.run(1)
            want.append(ops.sample_block(net, first, count))
        got = dn.graph_history(lattice)
        assert got.shape == (steps, count, count) and np.array_equal(parity.bits(got), parity.bits(np.array(want)))
        dn.set_graph_history(lattice, 0)
    parity.assert_state_equal(net, parity.pull_state(dn, net))
    dn.close()
