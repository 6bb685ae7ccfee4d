"""The Graph trait on a dense handle -- snn_graph_lookup / snn_graph_edit / snn_graph_incoming / snn_graph_outgoing -- held, element
for element and bit for bit, to what snn_get_graph_rows returns at the same moment: ragged and long networks (a last quad group
with one real row, padding columns, lattices that start off a multiple of 4, lines longer than one pass of the workgroup), edits
that reach the stepper, deferred plasticity updates, reward-modulated handles, shard handles and the refusals."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle_binding as ob
import parity
from snn_amd import ConnectionRule, WeightRule, _lib

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_STATE = 11, 12
# neuron lattices 3x5 and 5x7 (first = 15, no multiple of 4), a 2x3 spike-train lattice; ld = 64 > n_loc = 50
RAGGED = parity.Layout([(0, 3, 5), (1, 5, 7)], [(2, 2, 3)])
# 1 675 neurons, n_tot = 1 681 = 1 mod 4 and no multiple of 64 or 256: lines of several passes, one real row in the last quad group
LONG = parity.Layout([(0, 40, 41), (1, 5, 7)], [(2, 2, 3)])


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


def long_pattern():
    w, c = pattern(LONG)
    w, c = w.copy(), c.copy()
    c[1680, :] = 1                       # the last row -- the one real row of the last quad group -- fully connected
    w[1680, :] = np.float32(7.0) + np.arange(LONG.n_neurons, dtype=np.float32)
    c[:, 1639] = 0                       # and a column without an edge
    w[:, 1639] = 0
    return w, c


@pytest.fixture(scope="module")
def ragged(snn):
    dn = handle(snn, RAGGED)
    dn.set_graph_rows(0, *pattern(RAGGED))
    yield dn
    dn.close()


@pytest.fixture(scope="module")
def long(snn):
    dn = handle(snn, LONG)
    dn.set_graph_rows(0, *long_pattern())
    yield dn
    dn.close()


def all_pairs(dn):
    pre, post = np.meshgrid(np.arange(dn.n_tot, dtype=np.uint32), np.arange(dn.n_neurons, dtype=np.uint32), indexing="ij")
    return pre.reshape(-1), post.reshape(-1)


def digest(dn):
    w, c = dn.get_graph_rows(0, dn.n_tot)
    return hashlib.sha256(w.tobytes() + c.tobytes()).hexdigest()


def assert_column(dn, q, gw, gc):
    index, weights = dn.graph_incoming(q)
    want = np.nonzero(gc[:, q])[0]
    assert index.dtype == np.uint32 and weights.dtype == np.float32
    assert np.array_equal(index, want), f"incoming({q}): {index[:8]} ... against {want[:8]} ..."
    col = gw[:, q]
    assert np.array_equal(weights.view(np.uint32), col[want].view(np.uint32)), f"weights of incoming({q})"


def assert_row(dn, p, gw, gc, cols=(0, None)):
    index, weights = dn.graph_outgoing(p)
    lo, hi = cols[0], gc.shape[1] if cols[1] is None else cols[1]
    want = np.nonzero(gc[p, lo:hi])[0] + lo
    assert np.array_equal(index, want), f"outgoing({p}): {index[:8]} ... against {want[:8]} ..."
    assert np.array_equal(weights.view(np.uint32), gw[p, want].view(np.uint32)), f"weights of outgoing({p})"


# ---- 1. lookups, columns and rows against get_graph_rows -------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ragged", "long"])
def test_lookup_of_every_pair_equals_the_rows(request, which):
    dn = request.getfixturevalue(which)
    gw, gc = dn.get_graph_rows(0, dn.n_tot)
    w, on = dn.graph_lookup(*all_pairs(dn))              # (long: 2.8 million pairs, three hops of the staging lists)
    assert on.dtype == bool and w.dtype == np.float32
    assert np.array_equal(on.reshape(gc.shape), gc != 0)
    assert np.array_equal(w.reshape(gw.shape).view(np.uint32), gw.view(np.uint32))
    assert not w[~on].view(np.uint32).any(), "an absent edge reads +0.0"
    want_w, want_c = pattern(RAGGED) if which == "ragged" else long_pattern()
    assert np.array_equal(gc, want_c) and np.array_equal(gw.view(np.uint32), want_w.view(np.uint32))


def test_incoming_and_outgoing_on_the_ragged_network(ragged):
    gw, gc = ragged.get_graph_rows(0, ragged.n_tot)
    for q in range(ragged.n_neurons):
        assert_column(ragged, q, gw, gc)
    for p in range(ragged.n_tot):
        assert_row(ragged, p, gw, gc)


def test_incoming_and_outgoing_on_the_long_network(long):
    gw, gc = long.get_graph_rows(0, long.n_tot)
    assert np.delete(gc[1680], 1639).all() and long.n_tot == 1681 and long.n_neurons == 1675
    for q in (0, 14, 15, 1639, 1640, 1674):
        assert_column(long, q, gw, gc)
        index, _ = long.graph_incoming(q)
        assert (q == 1639) == (index.size == 0) and (index.size == 0 or index[-1] == 1680)
    assert long.graph_incoming(0)[0].size > 1024, "more candidates than one pass of the workgroup covers"
    for p in (0, 3, 4, 1674, 1675, 1680):
        assert_row(long, p, gw, gc)
    assert long.graph_outgoing(1680)[0].size == 1674                           # (column 1639 has no edge)


# ---- 2. the two-call idiom ----------------------------------------------------------------------------------------------------
def test_capacity_below_the_count_writes_nothing(ragged, long):
    L = ragged._L
    for dn, fn, which in [(ragged, L.snn_graph_incoming, 17), (ragged, L.snn_graph_outgoing, 52), (long, L.snn_graph_incoming, 3),
                          (long, L.snn_graph_outgoing, 1680)]:
        n = C.c_uint64(12345)
        assert fn(dn._h, which, None, None, 0, C.byref(n)) == 0 and 0 < n.value < 12345
        count = int(n.value)
        index, w = np.full(count + 2, 0xABCDABCD, np.uint32), np.full(count + 2, -77.0, np.float32)
        n = C.c_uint64(0)
        assert fn(dn._h, which, index.ctypes.data_as(_lib.u32p), w.ctypes.data_as(_lib.f32p), count - 1, C.byref(n)) == 0
        assert n.value == count and (index == 0xABCDABCD).all() and (w == -77.0).all(), "capacity < count: the lists stay untouched"
        assert fn(dn._h, which, index.ctypes.data_as(_lib.u32p), w.ctypes.data_as(_lib.f32p), count, C.byref(n)) == 0
        assert n.value == count and (index[:count] != 0xABCDABCD).all() and (index[count:] == 0xABCDABCD).all() and (w[count:] == -77.0).all()
        assert (np.diff(index[:count].astype(np.int64)) > 0).all()
    n = C.c_uint64(99)
    assert L.snn_graph_incoming(long._h, 1639, None, None, 0, C.byref(n)) == 0 and n.value == 0
    n = C.c_uint64(99)
    assert L.snn_graph_incoming(long._h, 1639, None, None, 50, C.byref(n)) == 0 and n.value == 0, "no edge: null lists are fine"
    index, w = long.graph_incoming(1639)
    assert index.size == 0 and w.size == 0


# ---- 3. edits -----------------------------------------------------------------------------------------------------------------
def boundary_pairs():
    """pairs on both sides of every block boundary of RAGGED: rows 14|15, 49|50, 55 (last), columns 14|15, 49 (last)"""
    return [(p, q) for p in (0, 13, 14, 15, 16, 48, 49, 50, 51, 55) for q in (0, 14, 15, 16, 48, 49)]


def test_edit_of_500_pairs_changes_those_and_nothing_else(snn):
    dn = handle(snn, RAGGED)
    w, c = pattern(RAGGED)
    w, c = w.copy(), c.copy()
    dn.set_graph_rows(0, w, c)
    rng = np.random.default_rng(11)
    flat = rng.choice(56 * 50, 500 - len(boundary_pairs()), replace=False)
    pairs = boundary_pairs() + [(int(k) // 50, int(k) % 50) for k in flat]
    pairs = list(dict.fromkeys(pairs))
    while len(pairs) < 500:
        k = int(rng.integers(0, 56 * 50))
        if (k // 50, k % 50) not in pairs:
            pairs.append((k // 50, k % 50))
    order = rng.permutation(500)
    pre, post = np.array(pairs, np.uint32)[order].T
    some = rng.random(500) < 0.6
    values = rng.uniform(-3.0, 3.0, 500).astype(np.float32)
    values[~some & (rng.random(500) < 0.5)] = np.nan          # a NaN weight of a None pair is not looked at
    dn.graph_edit(pre, post, values, some)
    c[pre, post] = some
    w[pre, post] = np.where(some, values, np.float32(0))
    gw, gc = dn.get_graph_rows(0, dn.n_tot)
    assert np.array_equal(gc, c) and np.array_equal(gw.view(np.uint32), w.view(np.uint32))
    assert 0 < some.sum() < 500 and (pattern(RAGGED)[1][pre, post] != some).any()
    # a pair listed three times with different values, among others, in both orders of Some / None: the last one wins
    pre = np.array([7, 20, 7, 55, 20, 7, 3], np.uint32)
    post = np.array([30, 2, 30, 49, 2, 30, 3], np.uint32)
    values = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], np.float32)
    some = np.array([1, 1, 0, 1, 0, 1, 1], bool)
    dn.graph_edit(pre, post, values, some)
    for p, q, v, s in zip(pre, post, values, some):            # applied one after another
        c[p, q], w[p, q] = s, (v if s else 0)
    assert w[7, 30] == 6.0 and c[20, 2] == 0 and w[20, 2] == 0
    gw, gc = dn.get_graph_rows(0, dn.n_tot)
    assert np.array_equal(gc, c) and np.array_equal(gw.view(np.uint32), w.view(np.uint32))
    # connected=None: every pair Some; a scalar weight
    dn.graph_edit([20, 7], [2, 30], 0.125)
    c[[20, 7], [2, 30]], w[[20, 7], [2, 30]] = 1, 0.125
    gw, gc = dn.get_graph_rows(0, dn.n_tot)
    assert np.array_equal(gc, c) and np.array_equal(gw.view(np.uint32), w.view(np.uint32))
    dn.close()


# ---- 4. edits reach the stepper -------------------------------------------------------------------------------------------------
def test_edits_reach_the_stepper(snn):
    rule, weight = ConnectionRule.chebyshev(2, self_edges=False), WeightRule.uniform(0.5, 1.5, seed=2)
    on = rule.mask((9, 9), (9, 9))

    def oracle():
        net = parity.make_oracle(parity.Layout([(0, 9, 9)]), model=ob.IZHIKEVICH, electrical=True, chemical=False)
        net["current_voltage"] = ob.uniform_array(1, 81, -65.0, 30.0)
        net["gap_conductance"] = 1.0                          # (loose enough that neurons fire before and after the edit)
        net["connections"][...] = on
        net["weights"][...] = np.where(on, weight.values((9, 9), (9, 9)), np.float32(0))
        return net

    net, unedited = oracle(), oracle()
    dn = parity.device_from_oracle(snn, net)
    dn.connect_by_rule(0, 0, rule, weight)                    # the graph by rule, on the device
    dn.set_history(voltage=True, spikes=True)
    dn.run(20)                                                # the 24-bit image of W and the counts exist now
    net.run(20, voltage_history=True, spike_history=True)
    v0, s0 = net.voltage_history.copy(), net.spike_history.copy()
    unedited.run(20)
    unedited.run(30, voltage_history=True)
    rng = np.random.default_rng(3)
    present, absent = np.argwhere(on), np.argwhere(~on)
    removed = present[rng.choice(len(present), 10, replace=False)]
    reweighted = present[rng.choice(len(present), 10, replace=False)]
    added = absent[rng.choice(len(absent), 10, replace=False)]
    pre = np.concatenate([removed[:, 0], reweighted[:, 0], added[:, 0]]).astype(np.uint32)
    post = np.concatenate([removed[:, 1], reweighted[:, 1], added[:, 1]]).astype(np.uint32)
    some = np.array([0] * 10 + [1] * 20, bool)
    values = rng.uniform(2.0, 6.0, 30).astype(np.float32)
    dn.graph_edit(pre, post, values, some)
    for p, q, v, s in zip(pre, post, values, some):
        net["connections"][p, q], net["weights"][p, q] = s, (v if s else 0)
    parity.assert_graph_equal(net, dn)
    dn.run(30)
    net.run(30, voltage_history=True, spike_history=True)
    want_v, want_s = np.concatenate([v0, net.voltage_history]), np.concatenate([s0, net.spike_history])
    assert np.array_equal(dn.spike_history(0), want_s), "raster differs from the oracle's run on the edited graph"
    assert np.array_equal(parity.bits(dn.voltage_history(0)), parity.bits(want_v))
    assert want_s[:20].sum() > 0 and want_s[20:].sum() > 0, "neurons must fire before and after the edit"
    assert not np.array_equal(unedited.voltage_history, net.voltage_history), "the edit must matter to the voltages"
    parity.assert_state_equal(net, parity.pull_state(dn, net))
    dn.close()


# ---- 5. deferred updates --------------------------------------------------------------------------------------------------------
def stdp_oracle():
    lay = parity.Layout([(0, 4, 4), (1, 4, 4)])
    net = parity.make_oracle(lay, model=ob.IZHIKEVICH, electrical=True, chemical=False)
    net["current_voltage"] = ob.uniform_array(4, 32, 0.0, 29.9)            # close to the threshold: several fire in either run
    net["gap_conductance"] = ob.uniform_array(9, 32, 0.2, 1.0)         # weak coupling: the neurons fire one after the other
    net.fill_graph(7, 0.5, 2.5, with_diagonal=False)
    net["connections"][np.random.default_rng(2).random(net["connections"].shape) >= 0.8] = 0
    net["weights"][...] *= net["connections"]
    net["do_plasticity"][:] = 1
    return net


def test_lookups_see_deferred_updates_and_edits_survive_them(snn):
    net = stdp_oracle()
    a, b, c = (parity.device_from_oracle(snn, net) for _ in range(3))
    before = a.get_graph_rows(0, 32)[0].copy()
    for dn in (a, b, c):
        dn.run(40)
    # the first getter after the run: the lookup (handle a), the column lists (handle b) -- then the rows
    w, on = a.graph_lookup(*all_pairs(a))
    gw, gc = a.get_graph_rows(0, 32)
    assert np.array_equal(w.reshape(32, 32).view(np.uint32), gw.view(np.uint32)) and np.array_equal(on.reshape(32, 32), gc != 0)
    assert not np.array_equal(gw.view(np.uint32), before.view(np.uint32)), "the run must have changed weights (STDP)"
    columns = [b.graph_incoming(q) for q in range(32)]
    bw, bc = b.get_graph_rows(0, 32)
    assert np.array_equal(bw.view(np.uint32), gw.view(np.uint32))
    for q, (index, weights) in enumerate(columns):
        assert np.array_equal(index, np.nonzero(bc[:, q])[0]) and np.array_equal(weights.view(np.uint32), bw[index, q].view(np.uint32))
    # an edit right after a run (handle c: the edit is its first call) against the same weights set through rows (handle a)
    p, q = (int(x) for x in np.argwhere(gc != 0)[5])
    c.graph_edit([p, 3], [q, 3], [4.5, 1.25])
    gw[p, q], gw[3, 3], gc[3, 3] = 4.5, 1.25, 1
    a.set_graph_rows(0, gw, gc)
    for dn in (a, c):
        dn.run(20)
    wa, ca = a.get_graph_rows(0, 32)
    wc, cc = c.get_graph_rows(0, 32)
    assert np.array_equal(ca, cc) and np.array_equal(wa.view(np.uint32), wc.view(np.uint32))
    assert not np.array_equal(wa.view(np.uint32), gw.view(np.uint32)), "the second run must have changed weights too"
    for dn in (a, b, c):
        dn.close()


# ---- 6. reward-modulated handles ------------------------------------------------------------------------------------------------
def test_reward_modulated_handle_restarts_the_traces_of_edited_pairs(snn):
    dn = handle(snn, RAGGED)
    w, c = pattern(RAGGED)
    dn.set_graph_rows(0, w, c)
    dn.set_reward_modulator(1, do_modulation=True)
    n_tot, nn = dn.n_tot, dn.n_neurons
    t = (np.float32(1.0) + np.arange(n_tot * nn, dtype=np.float32).reshape(n_tot, nn) / np.float32(4096.0)).astype(np.float32)
    dn.set_trace_rows(0, t)
    dn.set_pending_rows(0, -t)
    dn.set_counter_rows(0, np.ones((n_tot, nn), np.uint8))
    pre, post = np.array(boundary_pairs(), np.uint32).T
    some = np.arange(pre.size) % 3 != 0
    dn.graph_edit(pre, post, np.full(pre.size, 0.75, np.float32), some)
    want = t.copy()
    want[pre, post] = 0
    assert np.array_equal(dn.get_trace_rows(0, n_tot).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dn.get_pending_rows(0, n_tot).view(np.uint32), (-want).view(np.uint32) * (want != 0))
    counters = np.ones((n_tot, nn), np.uint8)
    counters[pre, post] = 0
    assert np.array_equal(dn.get_counter_rows(0, n_tot), counters)
    dn.close()


# ---- 7. shard handles -----------------------------------------------------------------------------------------------------------
def test_shard_handles_answer_for_the_columns_they_own(snn, long):
    gw, gc = long.get_graph_rows(0, long.n_tot)
    shards = [handle(snn, LONG, shard=(k, 2)) for k in range(2)]
    owned = 0
    for k, dn in enumerate(shards):
        dn.set_graph_rows(0, *long_pattern())
        b, e = dn.post_begin, dn.post_end
        owned += e - b
        rows = np.array([0, 3, 4, 1674, 1675, 1680] * 2, np.uint32)
        cols = np.array([b, b + 1, b + 63, e - 1, e - 2, (b + e) // 2] + [e - 1, b, e - 3, b + 5, b + 64, b + 65], np.uint32)
        w, on = dn.graph_lookup(rows, cols)
        ww, won = long.graph_lookup(rows, cols)
        assert np.array_equal(on, won) and np.array_equal(w.view(np.uint32), ww.view(np.uint32)) and np.array_equal(on, gc[rows, cols] != 0)
        for q in sorted({b, b + 1, e - 1, min(max(1639, b), e - 1), min(max(1640, b), e - 1)}):
            index, weights = dn.graph_incoming(q)
            wi, ww = long.graph_incoming(q)
            assert np.array_equal(index, wi) and np.array_equal(weights.view(np.uint32), ww.view(np.uint32)), (k, q)
        for p in (0, 4, 1675, 1680):
            assert_row(dn, p, gw, gc, cols=(b, e))                 # the owned columns only, as global indices
        other = e if k == 0 else b - 1
        for call, text in [(lambda: dn.graph_lookup([5, 6, 7], [b, other, b]), "pair 1"), (lambda: dn.graph_incoming(other), f"post {other}"),
                           (lambda: dn.graph_edit([5, 6, 7], [b, b, other], 1.0), "pair 2")]:
            with pytest.raises(snn.SnnError) as err:
                call()
            assert err.value.code == BAD_ARG and text in str(err.value) and "shard owns" in str(err.value), str(err.value)
        w2, c2 = dn.get_graph_rows(0, dn.n_tot)
        assert np.array_equal(c2[:, b:e], gc[:, b:e]) and np.array_equal(w2[:, b:e].view(np.uint32), gw[:, b:e].view(np.uint32))
    assert owned == LONG.n_neurons
    for dn in shards:
        dn.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_graph_alone(snn, ragged):
    L, h = ragged._L, ragged._h
    before = digest(ragged)
    u32 = lambda *v: np.array(v, np.uint32)
    w3, c3 = np.array([1.0, 2.0, 3.0], np.float32), np.ones(3, np.uint8)
    out_w, out_c = np.zeros(3, np.float32), np.zeros(3, np.uint8)
    ptr = lambda a: a.ctypes.data_as({np.dtype(np.uint32): _lib.u32p, np.dtype(np.float32): _lib.f32p, np.dtype(np.uint8): _lib.u8p}[a.dtype])
    msg = lambda: (L.snn_last_error() or b"").decode()
    n = C.c_uint64()

    def lookup(handle_, pre, post):
        return L.snn_graph_lookup(handle_, ptr(pre), ptr(post), pre.size, ptr(out_w), ptr(out_c))

    def edit(handle_, pre, post, w=w3, c=c3):
        return L.snn_graph_edit(handle_, ptr(pre), ptr(post), ptr(w), ptr(c), pre.size)

    ok_pre, ok_post = u32(1, 20, 55), u32(2, 30, 49)
    # indices outside the matrix: the pair is named, nothing of the call is applied
    for pre, post, text in [(u32(1, 56, 3), ok_post, "pair 1 (pre 56, post 30)"), (ok_pre, u32(2, 30, 50), "pair 2 (pre 55, post 50)"),
                            (ok_pre, u32(0xFFFFFFFF, 30, 49), "pair 0")]:
        assert lookup(h, pre, post) == BAD_ARG and text in msg(), msg()
        assert edit(h, pre, post) == BAD_ARG and text in msg(), msg()
    assert L.snn_graph_incoming(h, 50, None, None, 0, C.byref(n)) == BAD_ARG and "post 50" in msg()
    assert L.snn_graph_outgoing(h, 56, None, None, 0, C.byref(n)) == BAD_ARG and "pre 56" in msg()
    # a connected NaN in the middle of an otherwise valid edit
    assert edit(h, ok_pre, ok_post, w=np.array([1.0, np.nan, 3.0], np.float32)) == BAD_ARG and "pair 1" in msg() and "NaN" in msg()
    # null pointers with n > 0, null count; n == 0 touches nothing
    assert L.snn_graph_lookup(h, None, ptr(ok_post), 3, ptr(out_w), ptr(out_c)) == BAD_ARG and "null" in msg()
    assert L.snn_graph_lookup(h, ptr(ok_pre), ptr(ok_post), 3, ptr(out_w), None) == BAD_ARG
    assert L.snn_graph_edit(h, ptr(ok_pre), ptr(ok_post), None, ptr(c3), 3) == BAD_ARG
    assert L.snn_graph_edit(h, ptr(ok_pre), ptr(ok_post), ptr(w3), None, 3) == BAD_ARG
    assert L.snn_graph_incoming(h, 3, None, None, 0, None) == BAD_ARG
    assert L.snn_graph_lookup(None, ptr(ok_pre), ptr(ok_post), 3, ptr(out_w), ptr(out_c)) == BAD_ARG
    assert L.snn_graph_lookup(h, None, None, 0, None, None) == 0 and L.snn_graph_edit(h, None, None, None, None, 0) == 0
    count = ragged.graph_incoming(3)[0].size
    assert count and L.snn_graph_incoming(h, 3, None, None, count, C.byref(n)) == BAD_ARG and n.value == count, "room but no lists"
    assert digest(ragged) == before
    # the accepted calls, for contrast
    assert lookup(h, ok_pre, ok_post) == 0 and edit(h, ok_pre, ok_post) == 0
    assert digest(ragged) != before
    ragged.set_graph_rows(0, *pattern(RAGGED))
    assert digest(ragged) == before

    raw = handle(snn, RAGGED, finalize=False)
    for code in (lookup(raw._h, ok_pre, ok_post), edit(raw._h, ok_pre, ok_post), L.snn_graph_incoming(raw._h, 3, None, None, 0, C.byref(n)),
                 L.snn_graph_outgoing(raw._h, 3, None, None, 0, C.byref(n))):
        assert code == BAD_STATE and "finalized" in msg()
    raw.close()

    sparse = handle(snn, RAGGED, csr=True)
    row_ptr, pre_index, weights = np.arange(51, dtype=np.uint64), np.arange(50, dtype=np.uint32)[::-1].copy(), np.full(50, 0.5, np.float32)
    sparse.set_graph_csr(row_ptr, pre_index, weights)
    for code in (lookup(sparse._h, ok_pre, ok_post), edit(sparse._h, ok_pre, ok_post),
                 L.snn_graph_incoming(sparse._h, 3, None, None, 0, C.byref(n)), L.snn_graph_outgoing(sparse._h, 3, None, None, 0, C.byref(n))):
        assert code == BAD_STATE and "snn_get_graph_csr_structure" in msg() and "snn_get_graph_csr" in msg()
    assert np.array_equal(sparse.get_graph_csr(), weights)
    sparse.close()
