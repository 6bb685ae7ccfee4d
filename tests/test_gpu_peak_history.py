"""The voltage-peak record (snn_set_peak_history / snn_get_peak_raster / snn_get_peak_counts / snn_get_peaks) through the C ABI.
The expected result is always the numpy twin (tests/peaks_ref.py, held to scipy.signal.find_peaks by test_peaks_ref_host.py)
applied to the voltage history THE SAME HANDLE recorded: integer for integer, no tolerance.  One network throughout: a 9 x 9
lattice (81 neurons: crosses a raster word) and a 5 x 7 lattice (starts at bit 17 of word 1), 116 neurons, Izhikevich with gap
junctions from random voltages, one Hodgkin-Huxley case.  With seed 2 the Izhikevich network starts to fire around step 270, so
a handle is stepped 260 times before its records are switched on (WARM): the 400 steps after that hold 228 voltage peaks, and 28
neurons have another number of them than of spikes."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import parity
import peaks_ref

pytestmark = pytest.mark.gpu

LATTICES = [(0, 9, 9), (3, 5, 7)]
IDS = (0, 3)
THRESHOLD = {0: 20.0, 3: -40.0}                 # the experiments' 20 on one lattice, another value on the other
DIM_MISMATCH, BAD_ARG, BAD_STATE = 10, 11, 12   # snn_status of include/snn_amd.h
FORMS = [pytest.param(False, id="dense"), pytest.param(True, id="csr")]
WARM = 260


def build(model=ob.IZHIKEVICH, seed=2, silent=()):
    """fill_graph with 40 % of the connections cleared, as test_gpu_edge_history.build; `silent`: neurons without outgoing edges"""
    net = parity.make_oracle(parity.Layout(LATTICES), model=model)
    net["current_voltage"] = ob.uniform_array(seed, net.n_neurons, -65.0, 30.0)
    net["gap_conductance"] = 10.0
    net.fill_graph(seed + 1, 0.5, 1.5)
    rng = np.random.default_rng(seed)
    net["connections"][rng.random(net["connections"].shape) < 0.4] = 0
    for q in silent:
        net["connections"][q, :] = 0
    return net


def handle(snn, csr=False, model=ob.IZHIKEVICH, seed=2, threshold=THRESHOLD, peaks=True, shard=None, silent=(), spikes=True, warm=WARM):
    net = build(model, seed, silent)
    dn = parity.device_from_oracle(snn, net, csr=csr, shard=shard)
    dn.run(warm)                                   # (no record is on yet: switching them on below starts the step axis)
    dn.set_history(voltage=True, spikes=spikes)
    for id in IDS if peaks else ():
        dn.set_peak_history(id, threshold[id])
    return dn


def assert_record(dn, threshold=THRESHOLD, first_steps=(0, 137)):
    """raster, counts and lists of every lattice against the twin over the handle's own voltage history; returns the total"""
    steps = dn.history_steps()
    total = 0
    for id in IDS:
        history = dn.voltage_history(id).reshape(steps, -1)
        want = peaks_ref.peak_raster(history, threshold[id])
        got = dn.peak_raster(id)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (id, np.argwhere(got != want)[:8].tolist())
        for first in tuple(first_steps) + (steps,):
            assert np.array_equal(dn.peak_counts(id, first), peaks_ref.peak_counts(want, first)), (id, first)
            lists, ref = dn.peaks(id, first), peaks_ref.peak_lists(want, first)
            assert len(lists) == len(ref) and all(np.array_equal(a, b) for a, b in zip(lists, ref)), (id, first)
        total += int(want.sum())
    return total


@pytest.mark.parametrize("model, csr", [pytest.param(ob.IZHIKEVICH, False, id="izhikevich-dense"),
                                        pytest.param(ob.IZHIKEVICH, True, id="izhikevich-csr"),
                                        pytest.param(ob.HH, False, id="hodgkin-huxley-dense")])
def test_natural_run(snn, model, csr):
    """400 steps; Hodgkin-Huxley (seed 3, threshold -40 on both lattices): 174 peaks without a single reset or spike"""
    hh = model == ob.HH
    threshold = {0: -40.0, 3: -40.0} if hh else THRESHOLD
    dn = handle(snn, csr, model, seed=3 if hh else 2, threshold=threshold, warm=0 if hh else WARM)
    dn.run(400)
    assert dn.history_steps() == 400
    assert assert_record(dn, threshold) >= 50
    # the record is of VOLTAGE peaks: some neuron has another number of them than of is_spiking flags
    differ = any(np.any(dn.peak_counts(id) != dn.spike_history(id).reshape(400, -1).sum(axis=0)) for id in IDS)
    assert differ, "the test could pass on the spike raster"
    dn.close()


def test_single_shard_handle_is_covered(snn):
    """a handle finalized as shard 0 of 1 takes the calls (one of several shards refuses them: test_errors) and records what the
    unsharded handle records"""
    one, whole = handle(snn, shard=(0, 1)), handle(snn)
    one.run(200)
    whole.run(200)
    v = one.voltage_history(0)
    assert one.history_steps() == 200 and assert_record(one) > 0, (one.history_steps(), float(v.min()), float(v.max()))
    for id in IDS:
        assert np.array_equal(one.peak_raster(id), whole.peak_raster(id))
    one.close()
    whole.close()


# ---- teacher-forced series ----------------------------------------------------------------------------------------------------
FORCED_THRESHOLD = {0: 20.0, 3: 25.0}
LEVELS = np.array([-70.0, -50.0, 0.0, 20.0, 25.0, 28.0], np.float32)       # below v_th = 30: no reset rewrites a sample
NAN_NEURONS = (5, 40, 90)                       # (their outgoing edges are cleared: a NaN voltage reaches nobody's input sum)
T_FORCED = 90


def forced_series():
    """[T_FORCED, 116]: random levels, and in chosen columns the cases the issue names"""
    rng = np.random.default_rng(21)
    x = LEVELS[rng.integers(0, LEVELS.size, (T_FORCED, 116))]
    nan = np.float32(np.nan)
    x[:12, 0] = [0, 10, 25, 25, 10, 28, 28, 28, 0, 20, 0, 25]          # plateaus of 2 and 3, a peak equal to the threshold (lattice 0)
    x[:, 1] = 0
    x[3:70, 1] = 28                                                      # a plateau of 67 samples
    for q in NAN_NEURONS:
        x[:8, q] = [0, 28, nan, 0, 28, nan, nan, 28]                    # NaN after a rise, a rise out of NaN
    x[-3:, 7] = [0, 28, 28]                                              # plateaus still open at the last step, one per lattice
    x[-4:, 100] = [0, 28, 28, 28]
    return x


def patterns(history, thresholds):
    """which of the named cases the RECORDED history holds (run lengths read off the columns themselves)"""
    seen = {"plateau of 2": False, "plateau of 3": False, "plateau of 64+": False, "nan": bool(np.isnan(history).any()),
            "peak equal to its threshold": False, "open plateau at the end": False, "rise, flat, fall": False}
    first = 0
    for (id, rows, cols) in LATTICES:
        for q in range(first, first + rows * cols):
            x, thr = history[:, q], np.float32(thresholds[id])
            t = 1
            while t < x.size:
                if x[t] > x[t - 1]:
                    r = t
                    while r + 1 < x.size and x[r + 1] == x[t]:
                        r += 1
                    if r + 1 == x.size:
                        seen["open plateau at the end"] |= bool(r > t and x[t] > thr)
                    elif x[r + 1] < x[t]:
                        n = r - t + 1
                        seen["plateau of 2"] |= n == 2
                        seen["plateau of 3"] |= n == 3
                        seen["plateau of 64+"] |= n >= 64
                        seen["rise, flat, fall"] |= n >= 2
                        seen["peak equal to its threshold"] |= bool(x[t] == thr)
                    t = r + 1
                else:
                    t += 1
        first += rows * cols
    return seen


def force(dn, row):
    """one step whose recorded sample is `row`: dt is 0, so the update leaves the voltage it finds (and a NaN voltage would
    stay in the recovery variable: it is written too)"""
    first = 0
    for (id, rows, cols) in LATTICES:
        n = rows * cols
        dn.set_attr(id, "current_voltage", row[first:first + n])
        dn.set_attr(id, "w_value", np.zeros(n, np.float32))
        first += n
    dn.run(1)


@pytest.mark.parametrize("csr", FORMS)
def test_teacher_forced_series(snn, csr):
    x = forced_series()
    dn = handle(snn, csr, threshold=FORCED_THRESHOLD, silent=NAN_NEURONS, spikes=False, warm=0)
    for id, rows, cols in LATTICES:
        dn.set_attr(id, "dt", np.zeros(rows * cols, np.float32))
    for row in x:
        force(dn, row)
    history = np.concatenate([dn.voltage_history(id).reshape(T_FORCED, -1) for id in IDS], axis=1)
    seen = patterns(history, FORCED_THRESHOLD)
    assert all(seen.values()), seen
    assert np.array_equal(history, x, equal_nan=True), "the recorded history is not the chosen series"
    assert assert_record(dn, FORCED_THRESHOLD, first_steps=(0, 37)) >= 50
    before = {id: dn.peak_raster(id) for id in IDS}
    assert not before[0][-3:, 7].any() and not before[3][-4:, 100 - 81].any()        # the open plateaus are not reported yet
    # one more step ends them: their peaks appear at the right PAST index
    force(dn, np.zeros(116, np.float32))
    after = {id: dn.peak_raster(id) for id in IDS}
    assert after[0][T_FORCED - 2, 7] and after[0][:, 7].sum() == before[0][:, 7].sum() + 1          # (88 + 89) // 2
    assert after[3][T_FORCED - 2, 100 - 81] and after[3][:, 100 - 81].sum() == before[3][:, 100 - 81].sum() + 1   # (87 + 89) // 2
    assert_record(dn, FORCED_THRESHOLD, first_steps=(0, T_FORCED - 2))
    dn.close()


# ---- the record through run calls, strides, restarts, checkpoints -----------------------------------------------------------------
@pytest.mark.parametrize("csr", FORMS)
def test_split_invariance_and_regrowth(snn, csr):
    rasters = []
    for runs in ((300,), (1,) * 300, (7, 293)):
        dn = handle(snn, csr)
        for k in runs:
            dn.run(k)
        rasters.append([dn.peak_raster(id) for id in IDS])
        if len(runs) == 300:
            assert dn.stat("history_regrows") > 1, "the record must have been regrown with rows in it"
            assert_record(dn)
        dn.close()
    assert sum(int(r.sum()) for r in rasters[0]) >= 30
    for other in rasters[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(rasters[0], other))


@pytest.mark.parametrize("csr", FORMS)
def test_stride(snn, csr):
    dn = handle(snn, csr)
    dn.set_history_stride(3)
    dn.run(200)
    dn.run(200)
    assert dn.history_steps() == 134
    assert assert_record(dn, first_steps=(0, 45)) > 0
    dn.close()


def test_restart(snn):
    dn = handle(snn)
    dn.run(150)
    dn.reset_history()
    dn.run(150)
    assert dn.history_steps() == 150
    assert assert_record(dn) > 0                        # (the twin never reports sample 0: the first sample after the reset is no peak)
    dn.set_reduced_history(average_voltage=True)        # another record switched on: the shared cursor restarts
    assert dn.history_steps() == 0
    assert all(not dn.peak_counts(id).any() and dn.peak_raster(id).shape[0] == 0 for id in IDS)
    dn.run(100)
    assert dn.history_steps() == 100
    assert_record(dn, first_steps=(0, 50))
    dn.close()
    # a plateau across the reset is not counted: rise and first plateau sample before it, the fall after it
    dn = handle(snn, threshold=FORCED_THRESHOLD, spikes=False, warm=0)
    for id, rows, cols in LATTICES:
        dn.set_attr(id, "dt", np.zeros(rows * cols, np.float32))
    for v in (0.0, 28.0, 28.0):
        force(dn, np.full(116, v, np.float32))
    dn.reset_history()
    for v in (28.0, 0.0, 28.0, 0.0):
        force(dn, np.full(116, v, np.float32))
    for id in IDS:
        raster = dn.peak_raster(id)
        assert raster.shape[0] == 4 and not raster[:2].any() and raster[2].all() and not raster[3].any()
    assert_record(dn, FORCED_THRESHOLD, first_steps=(0, 2))
    dn.close()


@pytest.mark.parametrize("csr", FORMS)
def test_checkpoint(snn, csr):
    whole = handle(snn, csr)
    whole.run(250)
    want = [whole.peak_raster(id) for id in IDS]
    whole.close()
    dn = handle(snn, csr)
    dn.run(120)
    dn.checkpoint()
    dn.run(130)
    first = [dn.peak_raster(id) for id in IDS]
    dn.restore_checkpoint()
    assert dn.history_steps() == 120
    early = [dn.peak_raster(id) for id in IDS]
    dn.run(130)
    second = [dn.peak_raster(id) for id in IDS]
    for w, a, b, e in zip(want, first, second, early):
        assert np.array_equal(a, w) and np.array_equal(b, w)
        assert e.sum() <= w[:120].sum() and not (e & ~w[:120]).any()       # the rows of the checkpoint, without what later steps found
    assert_record(dn)
    dn.close()


def test_fast_paths(snn):
    """with a record on the one-launch run is not taken and the state is, bit for bit, that of the same run without a record;
    switched off again, the one-launch run is back"""
    net = build()
    off, on = handle(snn, peaks=False, warm=0), handle(snn, warm=0)
    off.run(200)
    on.run(200)
    assert off.stat("persistent_run_launches") > 0, "this network must be eligible for the one-launch run"
    assert on.stat("persistent_run_launches") == 0 and on.stat("persistent_run_steps") == 0
    a, b = parity.pull_state(off, net), parity.pull_state(on, net)
    assert set(a) == set(b) and all(np.array_equal(parity.bits(a[k]), parity.bits(b[k])) for k in a)
    for id in IDS:
        assert np.array_equal(parity.bits(off.voltage_history(id)), parity.bits(on.voltage_history(id)))
        assert np.array_equal(off.spike_history(id), on.spike_history(id))
    for id in IDS:
        on.set_peak_history(id, 0.0, enable=False)
    on.run(50)
    off.run(50)
    assert on.stat("persistent_run_launches") > 0
    a, b = parity.pull_state(off, net), parity.pull_state(on, net)
    assert all(np.array_equal(parity.bits(a[k]), parity.bits(b[k])) for k in a)
    off.close()
    on.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def code_of(snn, call):
    with pytest.raises(snn.SnnError) as e:
        call()
    assert str(e.value).split(":", 1)[1].strip()
    return e.value.code


def test_errors(snn):
    L = snn._lib.load()
    # a spike-train lattice
    net = parity.make_oracle(parity.Layout([(0, 3, 3)], [(5, 2, 2)]), st_kind=ob.ST_RATE)
    dn = parity.device_from_oracle(snn, net)
    assert code_of(snn, lambda: dn.set_peak_history(5, 20.0)) == BAD_ARG
    assert code_of(snn, lambda: dn.set_peak_history(9, 20.0)) == BAD_ARG          # no such lattice
    dn.close()
    # a handle that is not finalized; one of several shards
    raw = snn.DeviceNetwork()
    raw.add_lattice(0, 4, 4)
    assert code_of(snn, lambda: raw.set_peak_history(0, 20.0)) == BAD_STATE
    raw.finalize(1, 2)
    assert code_of(snn, lambda: raw.set_peak_history(0, 20.0)) == BAD_STATE
    raw.close()
    dn = handle(snn, peaks=False)
    assert code_of(snn, lambda: dn.set_peak_history(0, float("nan"))) == BAD_ARG
    for getter in (dn.peak_raster, dn.peak_counts, dn.peaks):                      # record off
        assert code_of(snn, lambda: getter(0)) == BAD_STATE
    dn.set_peak_history(0, float("-inf"))                                          # allowed: keeps every peak
    assert code_of(snn, lambda: dn.peaks(3)) == BAD_STATE                          # ... of lattice 0 only
    dn.run(60)
    steps = dn.history_steps()
    want = peaks_ref.peak_raster(dn.voltage_history(0).reshape(steps, -1), -np.inf)
    assert want.sum() > 0 and np.array_equal(dn.peak_raster(0), want)
    same = dn.history_steps()
    dn.set_peak_history(0, float("-inf"))                                          # nothing changes: no restart
    assert dn.history_steps() == same
    out8, out32 = np.zeros(steps * 81 + 81, np.uint8), np.zeros(82, np.uint32)
    assert L.snn_get_peak_raster(dn._h, 0, out8.ctypes.data_as(snn._lib.u8p), steps + 1) == DIM_MISMATCH
    assert L.snn_get_peak_counts(dn._h, 0, 0, out32.ctypes.data_as(snn._lib.u32p), 80) == DIM_MISMATCH
    # a capacity too small for snn_get_peaks: the total is reported, nothing partial is written
    total = C.c_uint64()
    ptr, lists = np.full(82, 77, np.uint64), np.full(int(want.sum()), 77, np.uint32)
    assert L.snn_get_peaks(dn._h, 0, 0, ptr.ctypes.data_as(snn._lib.u64p), lists.ctypes.data_as(snn._lib.u32p), lists.size - 1,
                           C.byref(total)) == 0
    assert total.value == want.sum() and np.all(ptr == 77) and np.all(lists == 77)
    assert L.snn_get_peaks(dn._h, 0, 0, ptr.ctypes.data_as(snn._lib.u64p), lists.ctypes.data_as(snn._lib.u32p), lists.size,
                           C.byref(total)) == 0
    assert ptr[0] == 0 and ptr[81] == want.sum() and np.array_equal(np.diff(ptr.astype(np.int64)), want.sum(axis=0))
    assert L.snn_get_peaks(dn._h, 0, 0, ptr.ctypes.data_as(snn._lib.u64p), lists.ctypes.data_as(snn._lib.u32p), lists.size, None) == BAD_ARG
    dn.set_peak_history(0, 5.0)                                                    # a new threshold restarts the record
    assert dn.history_steps() == 0
    dn.close()


# ---- allocation failures, in the pattern of test_gpu_alloc_failures_graph_query.py -------------------------------------------------
def arm(snn, n):
    seen = C.c_uint64()
    snn._lib.check(snn._lib.load().snn_debug_fail_alloc_at(int(n), C.byref(seen)))
    return int(seen.value)


def rasters(dn):
    return [dn.peak_raster(id) for id in IDS]


ALLOC_CALLS = {
    # (handle as the call finds it, the call, what must hold after a FAILED call)
    "set_peak_history": (lambda snn: handle(snn, peaks=False), lambda dn: dn.set_peak_history(3, -40.0)),
    "run_that_regrows": (lambda snn: handle(snn), lambda dn: dn.run(400)),
    "peaks": (lambda snn: handle(snn), lambda dn: dn.peaks(0, 5)),
}


@pytest.mark.parametrize("name", list(ALLOC_CALLS))
def test_every_allocation_of_a_call_may_fail(snn, name):
    make, call = ALLOC_CALLS[name]

    def fresh():
        dn = make(snn)
        dn.run(40)
        return dn

    def after_success(dn, got):
        """the state every successful execution of the call must reach"""
        if name == "set_peak_history":
            assert dn.history_steps() == 0                 # switched on: the record restarted
            dn.run(60)
            steps = dn.history_steps()
            want = peaks_ref.peak_raster(dn.voltage_history(3).reshape(steps, -1), -40.0)
            assert np.array_equal(dn.peak_raster(3), want)
        elif name == "run_that_regrows":
            assert dn.history_steps() == 440 and dn.stat("history_regrows") >= 2
            assert_record(dn)
        else:
            steps = dn.history_steps()
            want = peaks_ref.peak_lists(peaks_ref.peak_raster(dn.voltage_history(0).reshape(steps, -1), THRESHOLD[0]), 5)
            assert all(np.array_equal(a, b) for a, b in zip(got, want))

    try:
        dn = fresh()
        before = arm(snn, 0)
        got = call(dn)
        total = arm(snn, 0) - before
        after_success(dn, got)
        dn.close()
        assert total >= 3, f"only {total} allocations counted in {name}: is the hook wired to the allocators?"
        failed = 0
        for n in range(1, total + 1):
            dn = fresh()
            try:
                held = None if name == "set_peak_history" else rasters(dn)
                arm(snn, n)
                try:
                    call(dn)
                except snn.SnnError as e:
                    arm(snn, 0)
                    assert e.code in (3, 4, 5, 6, 8) and str(e).split(":", 1)[1].strip(), (name, n, total, str(e))
                else:
                    arm(snn, 0)
                    continue
                failed += 1
                # the handle and its record are as they were ...
                assert dn.history_steps() == 40, (name, n)
                if held is None:
                    assert code_of(snn, lambda: dn.peak_raster(3)) == BAD_STATE
                else:
                    assert all(np.array_equal(a, b) for a, b in zip(rasters(dn), held)), (name, n)
                    assert_record(dn, first_steps=(0, 11))
                after_success(dn, call(dn))                # ... and the same call now succeeds
            finally:
                arm(snn, 0)
                dn.close()
        assert failed == total, (name, failed, total)
    finally:
        arm(snn, 0)
