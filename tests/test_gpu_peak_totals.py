"""The voltage-peak totals (snn_set_peak_totals / snn_get_peak_totals / snn_peak_totals_steps) through the C ABI: per neuron and
window the number of peaks, counted where the neuron is updated, in EVERY step form -- the one-launch run included.  The expected
value is always the numpy twin of the peak record (tests/peaks_ref.py) over the voltage history THE SAME HANDLE recorded (history
on, stride 1, started with the totals), bucketed by tests/peak_totals_ref.py: integer for integer, no tolerance.  The network,
the helpers and the forced series are those of test_gpu_peak_history.py."""
import numpy as np
import pytest

import oracle_binding as ob
import parity
import peak_totals_ref
import peaks_ref
from test_gpu_peak_history import (BAD_ARG, BAD_STATE, DIM_MISMATCH, IDS, LATTICES, NAN_NEURONS, THRESHOLD, code_of, force,
                                   forced_series, handle, patterns)
from test_gpu_persistent_run import build as build_run, build_chemical, build_with_cells
from test_gpu_persistent_stdp import build as build_stdp

pytestmark = pytest.mark.gpu

# 400 steps: 13 of them fall beyond the last bucket, and some peaks before the origin
WINDOWS = {0: (THRESHOLD[0], 37, 50, 7), 3: (THRESHOLD[3], 37, 50, 7)}
OPEN = {0: (THRESHOLD[0], 37, 0, 1), 3: (THRESHOLD[3], 37, 0, 1)}


def switch_on(dn, settings):
    for id, (threshold, origin, window, n_windows) in settings.items():
        dn.set_peak_totals(id, threshold, origin, window, n_windows)


def twin(dn, settings):
    """id -> uint32[n_windows, count] from the handle's own voltage history, which must cover the totals' samples"""
    steps = dn.history_steps()
    assert dn.peak_totals_steps() == steps, (dn.peak_totals_steps(), steps)
    out = {}
    for id, (threshold, origin, window, n_windows) in settings.items():
        raster = peaks_ref.peak_raster(dn.voltage_history(id).reshape(steps, -1), threshold)
        out[id] = peak_totals_ref.bucket(raster, origin, window, n_windows)
    return out


def assert_totals(dn, settings):
    """the handle's totals against the twin; returns them"""
    want, got = twin(dn, settings), {id: dn.peak_totals(id) for id in settings}
    for id in settings:
        assert got[id].shape == want[id].shape and got[id].dtype == np.uint32
        assert np.array_equal(got[id], want[id]), (id, np.argwhere(got[id] != want[id])[:8].tolist())
    return got


def totals_handle(snn, settings=WINDOWS, options=(), **kw):
    """test_gpu_peak_history.handle (260 warm-up steps, voltage history on) with the totals switched on in place of the record"""
    dn = handle(snn, peaks=False, **kw)
    for name, value in options:
        dn.set_option(name, value)
    switch_on(dn, settings)
    return dn


# ---- 1. natural runs over every step form ----------------------------------------------------------------------------------------
STEP_FORMS = [pytest.param((), {}, id="default"), pytest.param((("persistent_run", 0),), {}, id="one-launch-step"),
              pytest.param((("fused_step", 0),), {}, id="two-kernel"), pytest.param((), {"csr": True}, id="csr"),
              pytest.param((), {"csr": True, "shard": (0, 1)}, id="csr-single-shard")]


@pytest.fixture(scope="module")
def natural(snn):
    """the default form's totals of both settings (what every other form must give) and the facts about the input"""
    out = {}
    for name, settings in (("windows", WINDOWS), ("open", OPEN)):
        dn = totals_handle(snn, settings)
        before = dn.stat("persistent_run_launches")
        dn.run(400)
        assert dn.stat("persistent_run_launches") > before and dn.stat("steps_dense_one_launch") == 0, "the totals must ride inside the one-launch run"
        out[name] = assert_totals(dn, settings)
        if name == "windows":
            steps = dn.history_steps()
            rasters = {id: peaks_ref.peak_raster(dn.voltage_history(id).reshape(steps, -1), WINDOWS[id][0]) for id in IDS}
            spikes = {id: dn.spike_history(id).reshape(steps, -1).sum(axis=0) for id in IDS}
            out["facts"] = {"counted": sum(int(out[name][id].sum()) for id in IDS), "before origin": sum(int(rasters[id][:37].sum()) for id in IDS),
                            "buckets": int(sum(out[name][id].sum(axis=1) for id in IDS).astype(bool).sum()),
                            "differ from spikes": any(np.any(rasters[id].sum(axis=0) != spikes[id]) for id in IDS)}
        dn.close()
    return out


def test_inputs_are_not_vacuous(natural):
    facts = natural["facts"]
    assert facts["counted"] >= 50 and facts["before origin"] >= 1 and facts["buckets"] >= 2 and facts["differ from spikes"], facts


@pytest.mark.parametrize("options, kw", STEP_FORMS)
@pytest.mark.parametrize("name, settings", [("windows", WINDOWS), ("open", OPEN)])
def test_natural_runs_over_every_step_form(snn, natural, name, settings, options, kw):
    dn = totals_handle(snn, settings, options, **kw)
    before = {k: dn.stat(k) for k in ("persistent_run_launches", "steps_dense_one_launch", "steps_two_kernel", "steps_sparse_one_launch")}
    dn.run(400)
    took = {k: dn.stat(k) - v for k, v in before.items()}
    if kw.get("csr"):
        assert took["persistent_run_launches"] == 0
    elif options == ():
        assert took["persistent_run_launches"] > 0 and took["steps_dense_one_launch"] == 0
    elif options[0][0] == "persistent_run":
        assert took["persistent_run_launches"] == 0 and took["steps_dense_one_launch"] > 0
    else:
        assert took["steps_two_kernel"] == 400
    got = assert_totals(dn, settings)
    for id in IDS:
        assert np.array_equal(got[id], natural[name][id]), id
    dn.close()


# ---- 2. the variants of the one-launch run ---------------------------------------------------------------------------------------
def without_plasticity(net):
    net["do_plasticity"] = 0
    return net


def variant_net(name):
    """(oracle net, neuron lattice id, (threshold, origin, window, n_windows), run calls); weakly coupled networks (the builder of
    test_gpu_persistent_stdp.py) where the strongly coupled ones fall silent"""
    if name == "lif-registers":        # (a leaky integrate-and-fire series peaks just above v_reset = -75: some above, some below)
        return without_plasticity(build_stdp(ob.LIF, [(3, 13, 12)], 7)), 3, (-74.95, 5, 30, 5), (150, 50)
    if name == "izhikevich-alone":
        return without_plasticity(build_stdp(ob.IZHIKEVICH, [(3, 8, 8)], 2)), 3, (0.0, 5, 30, 5), (150, 50)
    if name == "hodgkin-huxley-generic":
        return without_plasticity(build_stdp(ob.HH, [(3, 8, 9)], 1, drive=(-75, -40))), 3, (-40.0, 5, 100, 6), (400, 200)
    if name == "cells":
        return build_with_cells(ob.IZHIKEVICH, [(0, 9, 9)], [(5, 2, 2)], ob.ST_RATE, 61), 0, (20.0, 5, 30, 5), (150, 50)
    if name == "lend":
        return build_chemical(ob.IZHIKEVICH, 16, 16, 62, (0,), 0, 0, True), 3, (20.0, 5, 30, 5), (150, 50)
    if name == "chem":
        return build_chemical(ob.IZHIKEVICH, 15, 20, 63, (0,), 0, 0, True), 3, (20.0, 5, 30, 5), (150, 50)
    if name == "stdp":
        return build_stdp(ob.IZHIKEVICH, [(3, 12, 12)], 2), 3, (20.0, 5, 30, 5), (150, 50)
    assert name == "two-row-groups"
    return build_run(ob.IZHIKEVICH, 25, 44, 41, density=0.5), 3, (20.0, 5, 30, 5), (40,)


VARIANTS = ["lif-registers", "izhikevich-alone", "hodgkin-huxley-generic", "cells", "lend", "chem", "stdp", "two-row-groups"]


@pytest.mark.parametrize("name", VARIANTS)
def test_the_runs_variants(snn, name):
    net, id, setting, calls = variant_net(name)
    settings = {id: setting}
    got = []
    for persistent in (1, 0):
        dn = parity.device_from_oracle(snn, net)
        dn.set_option("persistent_run", persistent)
        dn.set_history(voltage=True, spikes=False)
        switch_on(dn, settings)
        for k in calls:
            dn.run(k)
        assert (dn.stat("persistent_run_launches") == len(calls)) if persistent else (dn.stat("persistent_run_launches") == 0)
        if name == "stdp" and persistent:
            assert dn.stat("persistent_run_stdp_steps") == sum(calls)
        got.append(assert_totals(dn, settings)[id])
        dn.close()
    assert np.array_equal(got[0], got[1])
    assert got[0].sum() > 0, "no peak was counted: the case shows nothing"


# ---- 3. teacher-forced series across launches ------------------------------------------------------------------------------------
FORCED = {0: (20.0, 5, 4, 3), 3: (25.0, 10, 40, 4)}          # lattice 0: buckets [5, 9) [9, 13) [13, 17); lattice 3: [10, 170)
# per forced value the steps of a run call that follow it with the voltage unchanged (dt = 0): calls of >= 4 steps are one launch
EXTRA = [0] * 20 + [4] + [0] * 5 + [6] + [0] * 4 + [70] + [0] * 10 + [4, 6] + [0] * 10
LONG = EXTRA.index(70)                                       # the forced value that is held for 71 samples ...
LONG_START = LONG + sum(EXTRA[:LONG])                        # ... from this sample index on


def forced_values():
    """[len(EXTRA), 116] values, one per forced step; sample index of value j: START[j]"""
    x = forced_series()[:len(EXTRA)].copy()                  # random levels, NaN after a rise in the first 8 samples of three neurons
    x[:20, 0] = [0, 10, 25, 25, 10, 28, 28, 28, 0, 20, 0, 25, 0, 0, 0, 0, 0, 0, 0, 0]    # plateaus of 2 and 3; 20 = the threshold
    x[:20, 2] = [0, 0, 0, 0, 0, 28, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]            # a peak at exactly the origin
    x[:20, 3] = [0, 0, 0, 0, 0, 0, 0, 0, 28, 0, 0, 0, 28, 0, 0, 0, 0, 0, 0, 0]           # origin + window - 1, origin + 2 window - 1
    x[:20, 4] = [0, 0, 0, 0, 0, 0, 0, 0, 0, 28, 0, 0, 0, 28, 0, 0, 0, 28, 0, 0]          # origin + window, + 2 window, + 3 window (dropped)
    x[:, 1] = 0
    x[:, 99] = 0
    x[LONG, 1] = x[LONG, 99] = 28                            # a plateau of 71: the rise in one launch, 70 samples in the next, the fall in a third
    x[-2:, 7] = [28, 28]                                     # plateaus still open at the last step, one per lattice
    x[-3, 7] = 0
    x[-3:, 100] = [0, 28, 28]
    return x


def force_and_hold(dn, row, extra):
    force(dn, row)
    if extra:
        dn.run(extra)


def test_teacher_forced_series_across_launches(snn):
    x = forced_values()
    thresholds = {id: FORCED[id][0] for id in IDS}
    dn = handle(snn, threshold=thresholds, peaks=False, silent=NAN_NEURONS, spikes=False, warm=0)
    for id, rows, cols in LATTICES:
        dn.set_attr(id, "dt", np.zeros(rows * cols, np.float32))
    switch_on(dn, FORCED)
    for row, extra in zip(x, EXTRA):
        force_and_hold(dn, row, extra)
    assert dn.stat("persistent_run_launches") == sum(1 for e in EXTRA if e >= 4)
    total = len(EXTRA) + sum(EXTRA)
    assert dn.history_steps() == total
    history = np.concatenate([dn.voltage_history(id).reshape(total, -1) for id in IDS], axis=1)
    assert np.array_equal(history, np.repeat(x, 1 + np.array(EXTRA), axis=0), equal_nan=True), "the recorded history is not the chosen series"
    seen = patterns(history, thresholds)
    raster0 = peaks_ref.peak_raster(history[:, :81], thresholds[0])
    origin, window, n_windows = FORCED[0][1:]
    seen["peak at the origin"] = bool(raster0[origin].any() and not raster0[origin - 1, 2])
    seen["both sides of a bucket edge"] = bool(raster0[origin + window - 1, 3] and raster0[origin + window, 4])
    seen["peak past the last bucket"] = bool(raster0[origin + window * n_windows, 4])
    long = history[LONG_START - 1:LONG_START + 72, 1]
    seen["rise and fall in different launches"] = bool(long[0] < long[1] and np.all(long[1:72] == long[1]) and long[72] < long[1])
    assert all(seen.values()), seen
    before = assert_totals(dn, FORCED)
    assert sum(int(before[id].sum()) for id in IDS) >= 50
    assert before[0][:, 2].tolist() == [1, 0, 0] and before[0][:, 3].tolist() == [1, 1, 0] and before[0][:, 4].tolist() == [0, 1, 1]
    assert before[0][:, 0].tolist() == [1, 1, 0]             # 28 at index 6 and 25 at 11; 25 at index 2 is before the origin; 20 is not above 20
    assert before[3][:, 99 - 81].sum() == 1                  # the plateau of 71
    # one more step ends the open plateaus: lattice 3's is counted in its bucket, lattice 0's lies past the last bucket
    force(dn, np.zeros(116, np.float32))
    after = assert_totals(dn, FORCED)
    assert after[3][:, 100 - 81].sum() == before[3][:, 100 - 81].sum() + 1
    assert after[3][(total - 2 - 10) // 40, 100 - 81] == before[3][(total - 2 - 10) // 40, 100 - 81] + 1
    assert np.array_equal(after[0][:, 7], before[0][:, 7])
    dn.close()


# ---- 4. split invariance ---------------------------------------------------------------------------------------------------------
def test_split_invariance_and_chunks(snn):
    results = []
    for runs, chunk in (((300,), 0), ((1,) * 300, 0), ((7, 293), 0), ((300,), 16)):
        dn = totals_handle(snn, options=(("run_resident_chunk_steps", chunk),) if chunk else ())
        launches = dn.stat("persistent_run_launches")
        for k in runs:
            dn.run(k)
        if chunk:
            assert dn.stat("persistent_run_launches") - launches == 19          # 18 chunks of 16 and one of 12
        results.append(assert_totals(dn, WINDOWS))
        dn.close()
    assert sum(int(results[0][id].sum()) for id in IDS) >= 30
    for other in results[1:]:
        assert all(np.array_equal(results[0][id], other[id]) for id in IDS)


# ---- 5. exact once ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault, chunk", [(37, 0), (40, 16)])
def test_a_run_that_gives_up_counts_once(snn, fault, chunk):
    """the launch ends normally (test hook: a workgroup withholds its voltages, the readers give up), the chunk is rolled back and
    repeated per step: its peaks must not be counted twice, those of the chunks before it not lost"""
    options = [("run_resident_fault_step", fault), ("run_resident_spin_limit", 20000)] + ([("run_resident_chunk_steps", chunk)] if chunk else [])
    dn = totals_handle(snn, options=options)
    dn.run(400)
    assert dn.stat("persistent_run_fallbacks") == 1
    got = assert_totals(dn, WINDOWS)
    assert sum(int(got[id].sum()) for id in IDS) >= 50
    dn.close()


def test_both_passes_of_verify_count_once(snn, natural):
    dn = totals_handle(snn, options=(("verify", 1),))
    dn.run(200)
    dn.run(200)
    assert dn.stat("verify_runs") >= 1 and dn.stat("verify_mismatches") == 0, dn.verify_report()
    got = assert_totals(dn, WINDOWS)
    assert all(np.array_equal(got[id], natural["windows"][id]) for id in IDS)
    dn.close()


@pytest.mark.parametrize("csr", [False, True])
def test_checkpoint(snn, natural, csr):
    dn = totals_handle(snn, csr=csr)
    dn.run(170)
    dn.checkpoint()
    dn.run(230)
    first = assert_totals(dn, WINDOWS)
    dn.restore_checkpoint()
    assert dn.peak_totals_steps() == 170
    early = assert_totals(dn, WINDOWS)
    dn.run(230)
    second = assert_totals(dn, WINDOWS)
    for id in IDS:
        assert np.array_equal(first[id], natural["windows"][id]) and np.array_equal(second[id], first[id])
        assert np.all(early[id] <= first[id]) and early[id].sum() < first[id].sum()
    dn.close()


# ---- 6. restarts and independence ------------------------------------------------------------------------------------------------
def test_restarts(snn):
    dn = totals_handle(snn)
    dn.run(150)
    assert dn.peak_totals_steps() == 150 and sum(int(dn.peak_totals(id).sum()) for id in IDS) > 0
    dn.reset_history()
    assert dn.peak_totals_steps() == 0 and all(not dn.peak_totals(id).any() for id in IDS)
    dn.run(150)
    held = assert_totals(dn, WINDOWS)
    assert sum(int(held[id].sum()) for id in IDS) > 0
    # a call that changes nothing restarts nothing; a new threshold of one lattice restarts both
    switch_on(dn, WINDOWS)
    assert dn.peak_totals_steps() == 150 and all(np.array_equal(dn.peak_totals(id), held[id]) for id in IDS)
    dn.set_peak_totals(3, -35.0, *WINDOWS[3][1:])
    assert dn.peak_totals_steps() == 0 and all(not dn.peak_totals(id).any() for id in IDS)
    dn.close()
    # a plateau across the reset is not counted: rise and first plateau sample before it, the fall after it
    dn = handle(snn, peaks=False, spikes=False, warm=0)
    for id, rows, cols in LATTICES:
        dn.set_attr(id, "dt", np.zeros(rows * cols, np.float32))
    switch_on(dn, {id: (20.0, 0, 0, 1) for id in IDS})
    for v in (0.0, 28.0, 28.0):
        force(dn, np.full(116, v, np.float32))
    dn.reset_history()
    for v in (28.0, 0.0, 28.0, 0.0):
        force(dn, np.full(116, v, np.float32))
    assert dn.peak_totals_steps() == 4
    for id in IDS:
        assert np.all(dn.peak_totals(id) == 1)               # the peak at index 2 alone
    dn.close()


def test_other_records_do_not_restart_the_totals(snn):
    """the raster record of the same handle shares the axis of snn_history_steps and restarts with it; the totals go on"""
    dn = totals_handle(snn, OPEN)
    for id in IDS:
        dn.set_peak_history(id, THRESHOLD[id])               # (restarts the history axis: 0 rows, as the totals' 0 samples)
    dn.run(120)
    raster = {id: dn.peak_raster(id) for id in IDS}
    got = assert_totals(dn, OPEN)                            # started together, same thresholds: the bucketed raster is the totals
    for id in IDS:
        assert np.array_equal(peak_totals_ref.bucket(raster[id], *OPEN[id][1:]), got[id])
    dn.set_reduced_history(average_voltage=True)
    assert dn.history_steps() == 0 and dn.peak_totals_steps() == 120
    assert all(np.array_equal(dn.peak_totals(id), got[id]) for id in IDS)
    dn.run(80)
    assert dn.history_steps() == 80 and dn.peak_totals_steps() == 200
    later = {id: dn.peak_totals(id) for id in IDS}
    assert all(np.all(later[id] >= got[id]) for id in IDS) and sum(int(later[id].sum() - got[id].sum()) for id in IDS) > 0
    dn.close()


def test_totals_of_one_lattice_alone(snn, natural):
    dn = totals_handle(snn, {3: WINDOWS[3]})
    dn.run(400)
    assert code_of(snn, lambda: dn.peak_totals(0)) == BAD_STATE
    assert np.array_equal(assert_totals(dn, {3: WINDOWS[3]})[3], natural["windows"][3])
    dn.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_errors(snn):
    L = snn._lib.load()
    net = parity.make_oracle(parity.Layout([(0, 3, 3)], [(5, 2, 2)]), st_kind=ob.ST_RATE)
    dn = parity.device_from_oracle(snn, net)
    assert code_of(snn, lambda: dn.set_peak_totals(5, 20.0)) == BAD_ARG          # a spike-train lattice
    assert code_of(snn, lambda: dn.set_peak_totals(9, 20.0)) == BAD_ARG          # no such lattice
    dn.close()
    raw = snn.DeviceNetwork()
    raw.add_lattice(0, 4, 4)
    assert code_of(snn, lambda: raw.set_peak_totals(0, 20.0)) == BAD_STATE       # not finalized
    raw.finalize(1, 2)
    assert code_of(snn, lambda: raw.set_peak_totals(0, 20.0)) == BAD_STATE       # one of several shards
    raw.close()
    dn = handle(snn, peaks=False)
    assert code_of(snn, lambda: dn.set_peak_totals(0, float("nan"))) == BAD_ARG
    assert code_of(snn, lambda: dn.set_peak_totals(0, 20.0, 0, 10, 0)) == BAD_ARG
    assert code_of(snn, lambda: dn.set_peak_totals(0, 20.0, 0, 0, 2)) == BAD_ARG
    assert code_of(snn, lambda: dn.peak_totals(0)) == BAD_STATE                  # totals off
    assert dn.peak_totals_steps() == 0
    dn.set_peak_totals(0, float("-inf"), 3, 10, 4)                               # allowed: keeps every peak
    assert code_of(snn, lambda: dn.peak_totals(3)) == BAD_STATE                  # ... of lattice 0 only
    dn.run(60)
    assert_totals(dn, {0: (-np.inf, 3, 10, 4)})
    out = np.zeros(5 * 82, np.uint32)
    assert L.snn_get_peak_totals(dn._h, 0, out.ctypes.data_as(snn._lib.u32p), 5, 81) == DIM_MISMATCH
    assert L.snn_get_peak_totals(dn._h, 0, out.ctypes.data_as(snn._lib.u32p), 4, 80) == DIM_MISMATCH
    assert L.snn_get_peak_totals(dn._h, 0, None, 4, 81) == BAD_ARG
    assert L.snn_peak_totals_steps(dn._h, None) == BAD_ARG
    assert not out.any()
    dn.set_peak_totals(0, 0.0, enable=False)
    assert code_of(snn, lambda: dn.peak_totals(0)) == BAD_STATE
    dn.close()
