"""The voltage-peak totals through the lattice classes: a head-direction ring built like the reference's hd_model.py (three 60 x 1
Izhikevich lattices, two rate cells, electrical synapses, dt = 1), totals from sample 1 on in windows of 100 steps -- row k - 1
of peak_totals(2) against the experiment's own expression for firing_rates[100 k], evaluated with tests/peaks_ref.py over the
voltage history the same object recorded; the single-lattice class; the settings across a fresh handle."""
import numpy as np
import pytest

import connect_spec_cases as cases
import peaks_ref

pytestmark = pytest.mark.gpu

N, STEPS, WINDOW = 60, 400, 100
RING = (N, 1)
SHIFT_RIGHT, SHIFT_LEFT, HD, CELLS = 0, 1, 2, 3
PEAK_THRESHOLD = 20


def firing_rates(history, threshold, window):
    """hd_model.py:96-125 over history [steps, rows, cols]: {i: [count per neuron]} for i = 0, window, 2 window, ..."""
    iterations = history.shape[0]
    data = [i.flatten() for i in np.array(history)]
    peaks = [peaks_ref.peaks([j[i] for j in data], threshold) for i in range(len(data[0]))]
    rates = {}
    for i in range(0, iterations, window):
        rates[i] = {}
        for n, peak_array in enumerate(peaks):
            rates[i][n] = len([j for j in peak_array if j <= i and j > i - window])
    return rates, peaks


def head_direction_network(ln):
    forms = cases.attractor_forms(RING)
    init = np.random.default_rng(5).uniform(-65, 30, (3,) + RING).astype(np.float32)
    lattices = []
    for id in (SHIFT_RIGHT, SHIFT_LEFT, HD):
        l = ln.IzhikevichNeuronLattice(id)
        l.populate(ln.IzhikevichNeuron(gap_conductance=10.0), *RING)
        l.apply_given_position(lambda pos, n, id=id: setattr(n, "current_voltage", float(init[id][pos])))
        l.update_grid_history = True
        lattices.append(l)
    cells = ln.RateSpikeTrainLattice(CELLS)
    cells.populate(ln.RateSpikeTrain(rate=1.5), 2, 1)
    g = ln.IzhikevichNeuronNetworkGPU.generate_network(lattices, [cells])
    everything = lambda a, b: True
    g.connect_internally(HD, everything, forms["bump"])
    g.connect(CELLS, SHIFT_RIGHT, everything, lambda a, b: 10.0)
    g.connect(SHIFT_RIGHT, HD, everything, forms["shift"])
    g.connect(SHIFT_LEFT, HD, everything, cases.shift(RING, -20.0))
    g.connect(HD, SHIFT_RIGHT, everything, forms["scaled_bump"])
    g.connect(HD, SHIFT_LEFT, everything, forms["scaled_bump"])
    g.set_dt(1)
    g.electrical_synapse, g.chemical_synapse = True, False
    return g


def check_windows(totals, history, threshold, window):
    """rows of the totals against the experiment's dictionary; returns the number of peaks counted"""
    rates, peaks = firing_rates(history, threshold, window)
    n_windows = totals.shape[0]
    assert totals.shape == (n_windows,) + history.shape[1:] and totals.dtype == np.uint32
    for k in range(1, n_windows + 1):
        if k * window in rates:
            assert totals[k - 1].reshape(-1).tolist() == list(rates[k * window].values()), k
        else:                                                   # a window the run has not finished: what it holds so far
            want = [len([j for j in p if (k - 1) * window < j <= k * window]) for p in peaks]
            assert totals[k - 1].reshape(-1).tolist() == want, k
    return int(totals.sum())


def test_network_class_counts_the_experiments_firing_rates(snn):
    g = head_direction_network(snn)
    with pytest.raises(KeyError):
        g.set_peak_totals(77)
    with pytest.raises(ValueError):
        g.set_peak_totals(HD, PEAK_THRESHOLD, window=0, n_windows=2)
    g.set_peak_totals(HD, PEAK_THRESHOLD, origin=1, window=WINDOW, n_windows=4)
    assert g.peak_totals(HD).shape == (4,) + RING and not g.peak_totals(HD).any()       # nothing has run
    g.run_lattices(STEPS)
    assert g._dn.stat("persistent_run_launches") > 0, "the totals ride inside the one-launch run"
    history = g.history(HD)
    assert history.shape == (STEPS,) + RING
    assert check_windows(g.peak_totals(HD), history, PEAK_THRESHOLD, WINDOW) > 0
    with pytest.raises(ValueError):
        g.peak_totals(SHIFT_LEFT)                               # off for that lattice
    # a builder call drops the handle: the setting is applied to the fresh one, which counts from its own first step
    g.set_dt(0.5)
    assert g._dn is None
    g.run_lattices(150)
    assert g.history(HD).shape == (150,) + RING
    check_windows(g.peak_totals(HD), g.history(HD), PEAK_THRESHOLD, WINDOW)
    # a second lattice, the pipelines' shape: everything from a first window on
    g.set_peak_totals(SHIFT_RIGHT, -40.0, origin=30)
    g.reset_history()
    g.run_lattices(120)
    check_windows(g.peak_totals(HD), g.history(HD), PEAK_THRESHOLD, WINDOW)
    data = g.history(SHIFT_RIGHT).reshape(120, -1)
    want = [len([j for j in peaks_ref.peaks(data[:, i], -40.0) if j >= 30]) for i in range(N)]      # pipeline_setup.py:230
    assert g.peak_totals(SHIFT_RIGHT).shape == (1,) + RING and g.peak_totals(SHIFT_RIGHT).reshape(-1).tolist() == want
    g.set_peak_totals(HD, enable=False)
    with pytest.raises(ValueError):
        g.peak_totals(HD)
    g.close()


def test_lattice_class(snn):
    ln = snn
    v = np.random.default_rng(2).uniform(-65.0, 30.0, (9, 9)).astype(np.float32)
    g = ln.IzhikevichNeuronLatticeGPU(0)
    g.populate(ln.IzhikevichNeuron(gap_conductance=10.0), 9, 9)
    g.apply_given_position(lambda pos, n: setattr(n, "current_voltage", float(v[pos])))
    g.update_grid_history = True
    g.connect(ln.ConnectionRule.chebyshev(2, self_edges=False), ln.WeightRule.uniform(0.5, 1.5, seed=3))
    with pytest.raises(ValueError):
        g.peak_totals()                                         # off
    g.set_peak_totals(PEAK_THRESHOLD, origin=1, window=50, n_windows=6)
    assert g.peak_totals().shape == (6, 9, 9) and not g.peak_totals().any()
    g.run_lattice(300)
    assert g.history.shape == (300, 9, 9)
    assert check_windows(g.peak_totals(), g.history, PEAK_THRESHOLD, 50) > 0
    g.set_dt(0.1)                                               # a fresh handle: the setting is kept
    assert g._net is None
    g.run_lattice(80)
    check_windows(g.peak_totals(), g.history, PEAK_THRESHOLD, 50)
    g.close()
