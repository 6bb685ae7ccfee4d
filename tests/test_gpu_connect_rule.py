"""snn_connect_by_rule on the device: every block against the per-pair restatement of the header's formulas
(connect_rule_cases), everything outside the block left alone, the handle's derived state refreshed (run parity), shard
handles, reward-modulated handles, the refusals and the C++ mirror.  All comparisons go through get_graph_rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import parity
import connect_rule_cases as cases
from snn_amd import ConnectionRule, WeightRule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the ragged network: neuron lattices 3x5 and 5x7 (first = 15, no multiple of 4), a 2x3 spike-train lattice; ld = 64 > n_loc = 50
RAGGED = parity.Layout([(0, 3, 5), (1, 5, 7)], [(2, 2, 3)])
PLAN = [(0, 0, ConnectionRule.chebyshev(1, self_edges=False), WeightRule.constant(0.5)),
        (0, 1, ConnectionRule.euclidean(5, probability=0.37, seed=21), WeightRule.uniform(0.5, 1.5, seed=22)),
        (1, 1, ConnectionRule.all_to_all(self_edges=False), WeightRule.constant(0.25)),
        (2, 1, ConnectionRule.same_position(), WeightRule.constant(2.0))]


def geometry(layout):
    """id -> (first global index, (rows, cols))"""
    rng = layout.ranges()
    out = {}
    for i, r, c in layout.lattices:
        out[i] = (rng[i][0], (r, c))
    for i, r, c in layout.st_lattices:
        out[i] = (layout.n_neurons + rng[i][0], (r, c))
    return out


def handle(snn, layout, shard=None, csr=False, finalize=True):
    dn = snn.DeviceNetwork(model=snn.IZHIKEVICH, spike_train=snn.ST_RATE if layout.st_lattices else snn.ST_NONE)
    for i, r, c in layout.lattices:
        dn.add_lattice(i, r, c)
    for i, r, c in layout.st_lattices:
        dn.add_spike_train_lattice(i, r, c)
    if finalize:
        dn.finalize(*(shard or ()), csr=csr)
    return dn


def pattern(layout):
    """a recognisable graph over the whole matrix: every weight names its place, about four edges in five present"""
    n_tot, nn = layout.n_neurons + layout.n_cells, layout.n_neurons
    p, q = np.arange(n_tot)[:, None], np.arange(nn)[None, :]
    c = ((p * 7 + q * 3) % 5 != 0).astype(np.uint32)
    w = (np.float32(100.0) + p.astype(np.float32) + q.astype(np.float32) / np.float32(256.0)).astype(np.float32)
    return np.where(c != 0, w, np.float32(0)), c


def apply_host(w, c, layout, plan):
    """the plan's blocks written into host rows [n_tot, n_neurons] from the per-pair expectation"""
    geo = geometry(layout)
    for pre, post, rule, weight in plan:
        (f0, s0), (f1, s1) = geo[pre], geo[post]
        on, ww = cases.expected_for(rule, weight, s0, s1)
        w[f0:f0 + on.shape[0], f1:f1 + on.shape[1]] = ww
        c[f0:f0 + on.shape[0], f1:f1 + on.shape[1]] = on
    return w, c


def assert_rows(dn, w, c, cols=slice(None), what=""):
    gw, gc = dn.get_graph_rows(0, dn.n_tot)
    assert np.array_equal(gc[:, cols], c[:, cols]), f"connections differ {what}: {np.argwhere(gc[:, cols] != c[:, cols])[:4].tolist()}"
    bad = np.argwhere(parity.bits(gw[:, cols]) != parity.bits(w[:, cols]))
    assert len(bad) == 0, f"weights differ {what} at {bad[:4].tolist()}"


def test_ragged_network_blocks_and_everything_outside_them(snn):
    dn = handle(snn, RAGGED)
    w, c = pattern(RAGGED)
    dn.set_graph_rows(0, w, c)
    assert_rows(dn, w, c, what="after the upload of the pattern")
    for k, (pre, post, rule, weight) in enumerate(PLAN):
        dn.connect_by_rule(pre, post, rule, weight)
        apply_host(w, c, RAGGED, PLAN[k:k + 1])
        # the block as the per-pair loop has it; every entry outside the blocks written so far still the pattern
        assert_rows(dn, w, c, what=f"after connecting {pre} -> {post}")
    untouched, _ = pattern(RAGGED)
    assert np.array_equal(w[15:50, 0:15], untouched[15:50, 0:15]) and np.array_equal(w[50:, 0:15], untouched[50:, 0:15])
    dn.close()


def test_all_to_all_uniform_equals_the_bench_generator(snn):
    lay = parity.Layout([(0, 9, 9)])
    a, b = handle(snn, lay), handle(snn, lay)
    a.connect_by_rule(0, 0, ConnectionRule.all_to_all(self_edges=False), WeightRule.uniform(0.5, 1.5, seed=1234))
    b.fill_graph_synthetic(1234, 0.5, 1.5, False)
    wa, ca = a.get_graph_rows(0, 81)
    wb, cb = b.get_graph_rows(0, 81)
    assert ca.sum() == 81 * 80 and np.array_equal(ca, cb) and np.array_equal(wa.view(np.uint32), wb.view(np.uint32))
    on, w = cases.expected_block((9, 9), (9, 9), cases.ALL, self_edges=False, weight_kind=cases.UNIFORM, lo=0.5, hi=1.5, weight_seed=1234)
    assert np.array_equal(ca != 0, on) and np.array_equal(wa.view(np.uint32), w.view(np.uint32))
    a.close()
    b.close()


def test_extremes(snn):
    dn = handle(snn, RAGGED)
    w, c = pattern(RAGGED)
    dn.set_graph_rows(0, w, c)
    weight = WeightRule.uniform(-1.0, 1.0, seed=5)

    def rows_after(pre, post, rule):
        dn.connect_by_rule(pre, post, rule, weight)
        apply_host(w, c, RAGGED, [(pre, post, rule, weight)])
        assert_rows(dn, w, c, what=f"after {rule!r} on {pre} -> {post}")
        return dn.get_graph_rows(0, dn.n_tot)

    # extent 0 with self edges is position to position
    w0, c0 = rows_after(0, 1, ConnectionRule.chebyshev(0))
    w1, c1 = rows_after(0, 1, ConnectionRule.same_position())
    assert c0[0:15, 15:50].sum() == 15 and np.array_equal(c0, c1) and np.array_equal(w0.view(np.uint32), w1.view(np.uint32))
    w0, c0 = rows_after(2, 1, ConnectionRule.euclidean(0))
    assert c0[50:56, 15:50].sum() == 6 and np.array_equal(c0[50:56, 15:50] != 0, cases.expected_block((2, 3), (5, 7), cases.SAME_POSITION)[0])
    # an extent no smaller than both dimensions is everything
    w0, c0 = rows_after(1, 1, ConnectionRule.chebyshev(7, self_edges=False))
    w1, c1 = rows_after(1, 1, ConnectionRule.all_to_all(self_edges=False))
    assert c0[15:50, 15:50].sum() == 35 * 34 and np.array_equal(c0, c1) and np.array_equal(w0.view(np.uint32), w1.view(np.uint32))
    w0, c0 = rows_after(1, 1, ConnectionRule.euclidean(6 * 6 + 4 * 4))
    assert c0[15:50, 15:50].all()
    # probability 0 clears a connected block, probability 1 draws nothing
    w0, c0 = rows_after(1, 1, ConnectionRule.all_to_all(probability=0.0, seed=3))
    assert not c0[15:50, 15:50].any() and c0[0:15, 15:50].sum() == 15
    w0, c0 = rows_after(1, 1, ConnectionRule.all_to_all(probability=1.0, seed=3))
    w1, c1 = rows_after(1, 1, ConnectionRule.all_to_all())
    assert c0[15:50, 15:50].all() and np.array_equal(c0, c1) and np.array_equal(w0.view(np.uint32), w1.view(np.uint32))
    dn.close()


def ragged_oracle():
    """the ragged network with state that makes it fire: both synapse kinds on, rate spike trains that fire within 20 steps"""
    net = parity.make_oracle(RAGGED, st_kind=ob.ST_RATE, electrical=True, chemical=True)
    nn, nc = net.n_neurons, net.n_cells
    net["current_voltage"] = ob.uniform_array(6, nn, -65.0, 30.0)
    net["gap_conductance"] = 10.0
    net["nt_flags"][:, 0] = 1
    net["rc_flags"][:, 0] = 1
    net["rc_g"][:, 0] = 3.0
    net["st_nt_flags"][:, 0] = 1
    net["st_rate"] = ob.uniform_array(7, nc, 0.3, 1.5)
    net["weights"][...] = 0
    net["connections"][...] = 0
    return net


def twin_graph(net, plan):
    """the plan's blocks into the oracle's matrices from the records' host twins (mask / values)"""
    geo = geometry(RAGGED)
    for pre, post, rule, weight in plan:
        (f0, s0), (f1, s1) = geo[pre], geo[post]
        on = rule.mask(s0, s1)
        net["connections"][f0:f0 + on.shape[0], f1:f1 + on.shape[1]] = on
        net["weights"][f0:f0 + on.shape[0], f1:f1 + on.shape[1]] = np.where(on, weight.values(s0, s1), np.float32(0))


def histories(dn, layout):
    out = []
    for i, _, _ in layout.lattices:
        out += [dn.spike_history(i), parity.bits(dn.voltage_history(i))]
    return out


def test_run_parity_of_a_graph_built_by_rule(snn):
    net = ragged_oracle()
    a = parity.device_from_oracle(snn, net)                  # no edge at all ...
    for pre, post, rule, weight in PLAN:
        a.connect_by_rule(pre, post, rule, weight)           # ... then the graph, on the device
    twin_graph(net, PLAN)
    b = parity.device_from_oracle(snn, net)                  # the same graph uploaded from the host twin
    parity.assert_graph_equal(net, a)
    parity.assert_graph_equal(net, b)
    for dn in (a, b):
        dn.set_history(voltage=True, spikes=True)
        dn.run(20)
    net.run(20, voltage_history=True, spike_history=True)
    rng = RAGGED.ranges()
    for dn in (a, b):
        for i, _, _ in RAGGED.lattices:
            first, count, _ = rng[i]
            assert np.array_equal(dn.spike_history(i), net.spike_history[:, first:first + count]), f"raster of lattice {i}"
            assert np.array_equal(parity.bits(dn.voltage_history(i)), parity.bits(net.voltage_history[:, first:first + count]))
        parity.assert_state_equal(net, parity.pull_state(dn, net))          # last_firing_time among it
        parity.assert_graph_equal(net, dn)
    assert all(np.array_equal(x, y) for x, y in zip(histories(a, RAGGED), histories(b, RAGGED)))
    assert net["st_last_firing_time"].max() > 0, "the spike trains must have fired"
    a.close()
    b.close()


def test_rule_after_a_run(snn):
    net = ragged_oracle()
    twin_graph(net, PLAN)
    a, b = parity.device_from_oracle(snn, net), parity.device_from_oracle(snn, net)
    for dn in (a, b):
        dn.set_history(voltage=True, spikes=True)
        dn.run(5)
    edit = (0, 1, ConnectionRule.chebyshev(2, probability=0.6, seed=31), WeightRule.uniform(1.0, 3.0, seed=32))
    a.connect_by_rule(*edit)
    w, c = b.get_graph_rows(0, b.n_tot)
    before = c.copy()
    apply_host(w, c, RAGGED, [edit])
    assert not np.array_equal(before, c)
    b.set_graph_rows(0, w, c)
    assert_rows(a, w, c, what="after the edit by rule")
    for dn in (a, b):
        dn.run(5)
    assert a.clock == b.clock == 10
    assert all(np.array_equal(x, y) for x, y in zip(histories(a, RAGGED), histories(b, RAGGED)))
    sa, sb = parity.pull_state(a, net), parity.pull_state(b, net)
    for name in sa:
        assert np.array_equal(parity.bits(sa[name]), parity.bits(sb[name])), name
    assert_rows(a, *b.get_graph_rows(0, b.n_tot), what="after the second run")
    a.close()
    b.close()


# two lattices whose neurons both shards own a part of: 191 neurons, stride 128 -- lattice 1 (first = 81) straddles the cut at 128
SPLIT = parity.Layout([(0, 9, 9), (1, 10, 11)], [(2, 2, 3)])
SPLIT_PLAN = [(0, 0, ConnectionRule.chebyshev(1, self_edges=False), WeightRule.constant(0.5)),
              (0, 1, ConnectionRule.euclidean(5, probability=0.37, seed=21), WeightRule.uniform(0.5, 1.5, seed=22)),
              (1, 1, ConnectionRule.all_to_all(self_edges=False), WeightRule.constant(0.25)),
              (2, 1, ConnectionRule.same_position(), WeightRule.constant(2.0))]


@pytest.mark.parametrize("layout,plan", [(RAGGED, PLAN), (SPLIT, SPLIT_PLAN)], ids=["ragged", "split"])
def test_shard_handles_write_the_columns_they_own(snn, layout, plan):
    whole = handle(snn, layout)
    shards = [handle(snn, layout, shard=(k, 2)) for k in range(2)]
    w, c = pattern(layout)
    for dn in [whole] + shards:
        dn.set_graph_rows(0, w, c)
        for pre, post, rule, weight in plan:
            dn.connect_by_rule(pre, post, rule, weight)
    apply_host(w, c, layout, plan)
    assert_rows(whole, w, c, what="on the unsharded handle")
    gw, gc = whole.get_graph_rows(0, whole.n_tot)
    owned = 0
    for k, dn in enumerate(shards):
        cols = slice(dn.post_begin, dn.post_end)
        owned += dn.post_end - dn.post_begin
        assert_rows(dn, gw, gc, cols=cols, what=f"on shard {k} (columns {dn.post_begin}..{dn.post_end})")
    assert owned == layout.n_neurons
    if layout is SPLIT:
        assert (shards[0].post_end, shards[1].post_begin) == (128, 128)
    for dn in [whole] + shards:
        dn.close()


def test_reward_modulated_handle_restarts_the_traces_of_the_block(snn):
    dn = handle(snn, RAGGED)
    w, c = pattern(RAGGED)
    dn.set_graph_rows(0, w, c)
    dn.set_reward_modulator(1, do_modulation=True)
    n_tot, nn = dn.n_tot, dn.n_neurons
    t = (np.float32(1.0) + np.arange(n_tot * nn, dtype=np.float32).reshape(n_tot, nn) / np.float32(4096.0)).astype(np.float32)
    dn.set_trace_rows(0, t)
    dn.set_pending_rows(0, -t)
    dn.set_counter_rows(0, np.ones((n_tot, nn), np.uint8))
    dn.connect_by_rule(0, 1, ConnectionRule.chebyshev(1), WeightRule.constant(1.0))
    want = t.copy()
    want[0:15, 15:50] = 0
    assert np.array_equal(dn.get_trace_rows(0, n_tot).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dn.get_pending_rows(0, n_tot).view(np.uint32), (-want).view(np.uint32) * (want != 0))
    counters = np.ones((n_tot, nn), np.uint8)
    counters[0:15, 15:50] = 0
    assert np.array_equal(dn.get_counter_rows(0, n_tot), counters)
    apply_host(w, c, RAGGED, [(0, 1, ConnectionRule.chebyshev(1), WeightRule.constant(1.0))])
    assert_rows(dn, w, c)
    dn.close()


def test_refusals_leave_the_graph_alone(snn):
    BAD_ARG, BAD_STATE = 11, 12
    dn = handle(snn, RAGGED)
    L, h = dn._L, dn._h
    w, c = pattern(RAGGED)
    dn.set_graph_rows(0, w, c)
    ok = dict(pre=0, post=1, rule=cases.CHEBYSHEV, extent=1, self_edges=1, probability=1.0, edge_seed=0, weight_rule=cases.UNIFORM,
              lo=0.5, hi=1.5, weight_seed=0)

    def call(handle_, **change):
        a = dict(ok, **change)
        code = L.snn_connect_by_rule(handle_, a["pre"], a["post"], a["rule"], a["extent"], a["self_edges"], a["probability"], a["edge_seed"],
                                     a["weight_rule"], a["lo"], a["hi"], a["weight_seed"])
        return code, (L.snn_last_error() or b"").decode()

    code, msg = call(None)
    assert code == BAD_ARG and "null" in msg
    for change, name in [(dict(pre=9), "pre_id"), (dict(post=9), "post_id"), (dict(post=2), "post_id"), (dict(rule=4), "rule"),
                         (dict(weight_rule=2), "weight_rule"), (dict(lo=float("nan")), "w_lo"), (dict(lo=float("inf")), "w_lo"),
                         (dict(hi=float("-inf")), "w_hi"), (dict(hi=float("nan")), "w_hi"), (dict(probability=float("nan")), "probability"),
                         (dict(lo=-3e38, hi=3e38), "w_hi - w_lo")]:
        code, msg = call(h, **change)
        assert code == BAD_ARG and name in msg, (change, code, msg)
    assert "spike-train" in call(h, post=2)[1]
    assert_rows(dn, w, c, what="after the refused calls")
    # the accepted call, for contrast, does change it
    assert call(h)[0] == 0
    assert not np.array_equal(dn.get_graph_rows(0, dn.n_tot)[1], c)
    dn.close()

    raw = handle(snn, RAGGED, finalize=False)
    code, msg = call(raw._h)
    assert code == BAD_STATE and "finalized" in msg
    raw.close()

    sparse = handle(snn, RAGGED, csr=True)
    row_ptr, pre_index, weights = np.arange(51, dtype=np.uint64), np.arange(50, dtype=np.uint32)[::-1].copy(), np.full(50, 0.5, np.float32)
    sparse.set_graph_csr(row_ptr, pre_index, weights)
    code, msg = call(sparse._h)
    assert code == BAD_STATE and "dense handles only" in msg
    assert np.array_equal(sparse.get_graph_csr(), weights)
    with pytest.raises(snn.SnnError) as e:
        sparse.connect_by_rule(0, 1, ConnectionRule.all_to_all())
    assert e.value.code == BAD_STATE
    sparse.close()


def fnv1a(data):
    h = 0xcbf29ce484222325
    for byte in data:
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_mirror_connects_by_rule(tmp_path, snn):
    from snn_amd import _lib
    exe = tmp_path / "connect_rule_test"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "connect_rule_test.cpp"),
                    "-L" + libdir, "-lsnn_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    on, w = cases.expected_block((4, 4), (4, 4), cases.EUCLIDEAN, extent=2, self_edges=False, probability=0.75, edge_seed=11,
                                 weight_kind=cases.UNIFORM, lo=0.25, hi=1.75, weight_seed=5)
    assert 0 < on.sum() < 16 * 8
    want = fnv1a(w.astype("<f4").tobytes() + on.astype("<u4").tobytes())
    assert r.stdout.split() == ["digest", f"{want:016x}", "edges", str(int(on.sum()))], r.stdout
