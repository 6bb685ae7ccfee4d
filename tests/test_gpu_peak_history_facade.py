"""The voltage-peak record through the lattice classes, dense and sparse: peaks(id) and peak_counts(id, window) against the two
expressions of the reference's experiments (interface_gpu/experiments/hd_model.py) evaluated over `history` -- the voltage history
the same object recorded --, and the settings across a re-upload of the device copy."""
import numpy as np
import pytest

from snn_amd import ConnectionRule, WeightRule

scipy_signal = pytest.importorskip("scipy.signal")
pytestmark = pytest.mark.gpu

FORMS = [pytest.param(False, id="dense"), pytest.param(True, id="sparse")]
STEPS, WINDOW = 300, 120
E1, E2 = 1, 2
SHAPES = {E1: (9, 9), E2: (5, 7)}
THRESHOLDS = {E1: 20.0, E2: -40.0}


def find_peaks_above_threshold(series, threshold):
    """as the experiments define it"""
    found, _ = scipy_signal.find_peaks(np.array(series))
    return [index for index in found if series[index] > threshold]


def experiments_readout(data, n, threshold, first_window):
    """(peaks, counts) of hd_model.py:43-47, 98-100: data[t] is the flattened grid of step t"""
    found = [find_peaks_above_threshold([j[i] for j in data], threshold) for i in range(n)]
    return found, [len([j for j in found[i] if j >= first_window]) for i in range(n)]


def voltages(shape, seed):
    return np.random.default_rng(seed).uniform(-65.0, 30.0, shape).astype(np.float32)


def check(peaks, counts, history, threshold, window):
    steps, rows, cols = history.shape
    data = [history[t].reshape(-1).tolist() for t in range(steps)]
    want_peaks, want_counts = experiments_readout(data, rows * cols, threshold, window)
    assert len(peaks) == rows * cols and all(list(a) == [int(j) for j in b] for a, b in zip(peaks, want_peaks))
    assert counts.shape == (rows, cols) and counts.reshape(-1).tolist() == want_counts
    return sum(len(p) for p in want_peaks)


@pytest.mark.parametrize("sparse", FORMS)
def test_lattice_class(snn, sparse):
    ln = snn
    v = voltages((9, 9), 2)
    g = ln.IzhikevichNeuronLatticeGPU(0, sparse=sparse)
    g.populate(ln.IzhikevichNeuron(gap_conductance=10.0), 9, 9)
    g.apply_given_position(lambda pos, n: setattr(n, "current_voltage", float(v[pos])))
    g.update_grid_history = True
    g.connect(ConnectionRule.chebyshev(2, self_edges=False), WeightRule.uniform(0.5, 1.5, seed=3))
    assert g.peaks() == [[] for _ in range(81)] and not g.peak_counts().any()          # nothing has run
    g.set_peak_history()                              # the experiments' threshold, 20
    g.run_lattice(STEPS)
    assert g.history.shape == (STEPS, 9, 9)
    assert check(g.peaks(), g.peak_counts(WINDOW), g.history, 20.0, WINDOW) > 0
    check(g.peaks(), g.peak_counts(), g.history, 20.0, 0)
    # a builder call drops the device copy: the setting is applied to the fresh handle, and the record starts with it
    g.set_dt(0.1)
    assert g._net is None
    g.run_lattice(40)
    assert g.history.shape == (40, 9, 9)
    check(g.peaks(), g.peak_counts(7), g.history, 20.0, 7)
    g.set_peak_history(-40.0)                         # a new threshold restarts the record of the handle
    g.run_lattice(60)
    assert g.history.shape == (60, 9, 9)
    assert check(g.peaks(), g.peak_counts(7), g.history, -40.0, 7) > 0
    g.set_peak_history(enable=False)
    with pytest.raises(snn.SnnError):
        g.peaks()
    g.close()


def network(ln, sparse):
    lattices = []
    for id in (E1, E2):
        v = voltages(SHAPES[id], 8 + id)
        l = ln.IzhikevichNeuronLattice(id)
        l.populate(ln.IzhikevichNeuron(gap_conductance=10.0), *SHAPES[id])
        l.apply_given_position(lambda pos, n, v=v: setattr(n, "current_voltage", float(v[pos])))
        l.update_grid_history = True
        lattices.append(l)
    g = ln.IzhikevichNeuronNetworkGPU.generate_network(lattices, [], sparse=sparse)
    for id in (E1, E2):
        g.connect_internally(id, ConnectionRule.chebyshev(2, self_edges=False), WeightRule.uniform(0.5, 1.5, seed=11 + id))
    g.connect(E1, E2, ConnectionRule.all_to_all(probability=0.3, seed=5), WeightRule.uniform(0.5, 1.5, seed=6))
    g.connect(E2, E1, ConnectionRule.all_to_all(probability=0.3, seed=7), WeightRule.constant(1.0))
    g.electrical_synapse, g.chemical_synapse = True, False
    return g


@pytest.mark.parametrize("sparse", FORMS)
def test_network_class(snn, sparse):
    g = network(snn, sparse)
    for id in (E1, E2):
        g.set_peak_history(id, THRESHOLDS[id])
    g.run_lattices(STEPS)
    total = 0
    for id in (E1, E2):
        assert g.history(id).shape == (STEPS, *SHAPES[id])
        total += check(g.peaks(id), g.peak_counts(id, WINDOW), g.history(id), THRESHOLDS[id], WINDOW)
        check(g.peaks(id), g.peak_counts(id), g.history(id), THRESHOLDS[id], 0)
    assert total > 0
    # the settings survive a re-upload: a builder call drops the handle, the next run records on the fresh one
    g.set_dt(0.1)
    assert g._dn is None
    g.run_lattices(50)
    for id in (E1, E2):
        assert g.history(id).shape == (50, *SHAPES[id])
        check(g.peaks(id), g.peak_counts(id, 10), g.history(id), THRESHOLDS[id], 10)
    g.set_peak_history(E2, enable=False)              # one lattice's record off: the other goes on, from a fresh step axis
    g.run_lattices(30)
    check(g.peaks(E1), g.peak_counts(E1, 3), g.history(E1), THRESHOLDS[E1], 3)
    with pytest.raises(snn.SnnError):
        g.peaks(E2)
    with pytest.raises(KeyError):
        g.set_peak_history(77)
    g.close()
