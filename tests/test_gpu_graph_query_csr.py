"""The Graph trait on a sparse handle -- snn_graph_csr_lookup / _edit / _incoming / _outgoing -- held, bit for bit, to the trusted
snn_graph_* calls of a dense handle that holds the same edges and to the host CSR arrays that were set.  Layouts: RAGGED (50 rows,
one partial SELL slice, a lattice starting off a multiple of 4, cells as presynaptic indices) and LONG (1 675 rows = 27 slices, the
last with 11 rows; rows longer than 64, 256 and 1 024 entries, outgoing lists longer than one pass of a workgroup; a neuron without
an incoming edge, a source without an outgoing one, a row of exactly one entry, rows of 63 / 64 / 65 entries so that padding sits
beside real entries).  No tolerance anywhere."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle_binding as ob
import parity
import test_gpu_graph_query as dense_tests
from test_gpu_connect_rule_csr import csr_of
from snn_amd import ConnectionRule, WeightRule, _lib

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_STATE = 11, 12
RAGGED, LONG = dense_tests.RAGGED, dense_tests.LONG
handle, all_pairs = dense_tests.handle, dense_tests.all_pairs
NO_SOURCE, NO_INCOMING, ONE_ENTRY = 1677, 1639, 7
SHORT_ROWS = {q: (63, 64, 65)[k % 3] for k, q in enumerate([192, 193, 194] + list(range(1664, 1675)))}


def long_graph():
    w, c = dense_tests.pattern(LONG)
    w, c = w.copy(), c.copy()
    c[NO_SOURCE, :] = 0                                # a source (a spike-train cell) without an outgoing edge
    c[:, NO_INCOMING] = 0                              # a neuron without an incoming edge
    c[:, ONE_ENTRY] = 0
    c[1680, ONE_ENTRY] = 1                             # a row of exactly one entry: the last source
    for q, length in SHORT_ROWS.items():               # three rows of a long slice, and the whole last slice (11 rows, width 65)
        c[np.nonzero(c[:, q])[0][length:], q] = 0
    w = np.where(c != 0, w, np.float32(0))
    w[1680, ONE_ENTRY] = np.float32(7.5)
    return w, c


GRAPHS = {"ragged": (RAGGED, lambda: dense_tests.pattern(RAGGED)), "long": (LONG, long_graph)}


class Twin:
    """a sparse handle and a dense one that hold the same edges, and those edges on the host"""

    def __init__(self, snn, which, shard=None):
        layout, graph = GRAPHS[which]
        self.w, self.c = graph()
        self.sparse = handle(snn, layout, csr=True, shard=shard)
        self.csr = csr_of(self.w, self.c, self.sparse.owned)
        self.sparse.set_graph_csr(*self.csr)
        self.dense = None
        if shard is None:
            self.dense = handle(snn, layout)
            self.dense.set_graph_rows(0, self.w, self.c)

    def close(self):
        self.sparse.close()
        if self.dense is not None:
            self.dense.close()


@pytest.fixture(scope="module")
def ragged(snn):
    t = Twin(snn, "ragged")
    yield t
    t.close()


@pytest.fixture(scope="module")
def long(snn):
    t = Twin(snn, "long")
    yield t
    t.close()


def digest(dn):
    rp, pi = dn.graph_csr_structure()
    return hashlib.sha256(rp.tobytes() + pi.tobytes() + dn.get_graph_csr().tobytes()).hexdigest()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def edge_pairs(csr, posts):
    """(pre, post) of every stored edge, in the edge order of get_graph_csr"""
    rp, pi, _ = csr
    return pi.astype(np.uint32), np.repeat(np.asarray(posts, np.uint32), np.diff(rp.astype(np.int64)))


# ---- 1. lookups -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ragged", "long"])
def test_lookup_of_every_pair_equals_the_dense_handle(request, which):
    t = request.getfixturevalue(which)
    pre, post = all_pairs(t.sparse)                    # (long: 2.8 million pairs, three hops of the staging lists)
    assert which == "ragged" or pre.size > 2 * (1 << 20)
    w, on = t.sparse.graph_lookup(pre, post)
    dw, don = t.dense.graph_lookup(pre, post)
    assert on.dtype == bool and w.dtype == np.float32
    assert np.array_equal(on, don) and same_bits(w, dw)
    assert np.array_equal(on.reshape(t.c.shape), t.c != 0) and same_bits(w.reshape(t.w.shape), t.w)
    assert not w[~on].view(np.uint32).any(), "an absent edge reads +0.0"
    # unsorted, with repeats
    rng = np.random.default_rng(5)
    pick = rng.integers(0, pre.size, 5000)
    pick[100:200] = pick[0:100]
    w, on = t.sparse.graph_lookup(pre[pick], post[pick])
    dw, don = t.dense.graph_lookup(pre[pick], post[pick])
    assert np.array_equal(on, don) and same_bits(w, dw) and on.any() and not on.all()


def test_the_long_graph_has_the_shapes_it_is_meant_to_have(long):
    lengths = (long.c != 0).sum(axis=0)
    assert lengths[NO_INCOMING] == 0 and lengths[ONE_ENTRY] == 1 and not long.c[NO_SOURCE].any()
    assert all(lengths[q] == n for q, n in SHORT_ROWS.items()) and lengths[1664:].max() == 65 and lengths[195] > 1024
    assert lengths.max() > 1024 and (long.c != 0).sum(axis=1).max() > 1024 and long.sparse.n_neurons == 1675 == 26 * 64 + 11


# ---- 2. incoming and outgoing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ragged", "long"])
def test_incoming_and_outgoing_of_every_line_equal_the_dense_handle(request, which):
    t = request.getfixturevalue(which)
    for q in range(t.sparse.n_neurons):
        index, weights = t.sparse.graph_incoming(q)
        di, dw = t.dense.graph_incoming(q)
        assert index.dtype == np.uint32 and weights.dtype == np.float32
        assert np.array_equal(index, di) and same_bits(weights, dw), f"incoming({q})"
        assert np.array_equal(index, np.nonzero(t.c[:, q])[0]) and same_bits(weights, t.w[index, q])
    for p in range(t.sparse.n_tot):
        index, weights = t.sparse.graph_outgoing(p)
        di, dw = t.dense.graph_outgoing(p)
        assert index.dtype == np.uint32 and np.array_equal(index, di) and same_bits(weights, dw), f"outgoing({p})"
        assert np.array_equal(index, np.nonzero(t.c[p])[0]) and same_bits(weights, t.w[p, index])


def test_capacity_below_the_count_writes_nothing(ragged, long):
    L = ragged.sparse._L
    for dn, fn, which in [(ragged.sparse, L.snn_graph_csr_incoming, 17), (ragged.sparse, L.snn_graph_csr_outgoing, 52),
                          (long.sparse, L.snn_graph_csr_incoming, 3), (long.sparse, L.snn_graph_csr_outgoing, 1680),
                          (long.sparse, L.snn_graph_csr_incoming, 193)]:
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
        assert fn(dn._h, which, None, None, count, C.byref(n)) == BAD_ARG and n.value == count, "room but no lists"
    for fn, which in [(L.snn_graph_csr_incoming, NO_INCOMING), (L.snn_graph_csr_outgoing, NO_SOURCE)]:
        for capacity in (0, 50):
            n = C.c_uint64(99)
            assert fn(long.sparse._h, which, None, None, capacity, C.byref(n)) == 0 and n.value == 0, "no edge: null lists are fine"
    index, w = long.sparse.graph_incoming(NO_INCOMING)
    assert index.size == 0 and w.size == 0


# ---- 3. edits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ragged", "long"])
def test_edit_of_stored_edges_changes_those_and_nothing_else(snn, which):
    layout, graph = GRAPHS[which]
    w, c = graph()
    dn = handle(snn, layout, csr=True)
    csr = csr_of(w, c, dn.owned)
    dn.set_graph_csr(*csr)
    structure = dn.graph_csr_structure()
    pre, post = edge_pairs(csr, dn.owned)
    rng = np.random.default_rng(11)
    edges = rng.choice(pre.size, 400, replace=False)
    edges = np.concatenate([edges, edges[:50], edges[10:30]])[rng.permutation(470)]          # shuffled, with pairs listed 2 and 3 times
    values = rng.uniform(-3.0, 3.0, edges.size).astype(np.float32)
    absent = np.argwhere(c == 0)[rng.choice((c == 0).sum(), 30, replace=False)]             # "stay absent", scattered among them
    at = np.sort(rng.choice(edges.size, 30, replace=False))
    p = np.insert(pre[edges], at, absent[:, 0].astype(np.uint32))
    q = np.insert(post[edges], at, absent[:, 1].astype(np.uint32))
    v = np.insert(values, at, np.float32(np.nan))                                           # (the weight of a None pair is not looked at)
    on = np.insert(np.ones(edges.size, bool), at, False)
    dn.graph_edit(p, q, v, on)
    want = csr[2].copy()
    for e, value in zip(edges, values):                                                      # applied one after another
        want[e] = value
    assert same_bits(dn.get_graph_csr(), want) and (want != csr[2]).sum() == 400
    for x, y in zip(dn.graph_csr_structure(), structure):
        assert np.array_equal(x, y)
    # strictly ascending pairs take the path without the sort; a scalar weight, connected=None
    asc = np.unique(edges[:100])
    asc = asc[np.lexsort((post[asc], pre[asc]))]
    dn.graph_edit(pre[asc], post[asc], 0.125)
    want[asc] = 0.125
    assert same_bits(dn.get_graph_csr(), want)
    lw, lon = dn.graph_lookup(pre[asc], post[asc])
    assert lon.all() and (lw == 0.125).all()
    dn.close()


def test_edit_refusals_name_the_pair_and_leave_the_graph_alone(snn, ragged):
    dn, L = ragged.sparse, ragged.sparse._L
    before = digest(dn)
    pre, post = edge_pairs(ragged.csr, dn.owned)
    absent = np.argwhere(ragged.c == 0).astype(np.uint32)
    ok_p, ok_q = pre[[3, 40, 900]], post[[3, 40, 900]]
    w3 = np.array([1.0, 2.0, 3.0], np.float32)

    def refused(p, q, w, on, *texts, code=BAD_ARG):
        with pytest.raises(snn.SnnError) as err:
            dn.graph_edit(p, q, w, on)
        assert err.value.code == code and all(t in str(err.value) for t in texts), str(err.value)
        assert digest(dn) == before

    a = absent[5]
    refused([ok_p[0], a[0], ok_p[2]], [ok_q[0], a[1], ok_q[2]], w3, [1, 1, 1], f"pair 1 (pre {a[0]}, post {a[1]})", "structure of a sparse graph is fixed",
            "snn_connect_by_rules_csr", "snn_set_graph_csr")
    refused(ok_p, ok_q, w3, [1, 1, 0], f"pair 2 (pre {ok_p[2]}, post {ok_q[2]})", "structure of a sparse graph is fixed")
    # of two offending pairs the first in the call is named, wherever the pairs sort; a later valid occurrence does not heal it
    refused([ok_p[2], ok_p[1], ok_p[0], ok_p[1]], [ok_q[2], ok_q[1], ok_q[0], ok_q[1]], 1.0, [1, 0, 0, 1], f"pair 1 (pre {ok_p[1]}, post {ok_q[1]})")
    refused(ok_p, ok_q, [1.0, np.nan, 3.0], [1, 1, 1], "pair 1", "NaN")
    refused([1, 56, 3], ok_q, w3, [1, 1, 1], f"pair 1 (pre 56, post {ok_q[1]})")
    refused(ok_p, [2, 30, 50], w3, [1, 1, 1], f"pair 2 (pre {ok_p[2]}, post 50)")
    u32 = lambda *v: np.array(v, np.uint32)
    ptr = lambda x: x.ctypes.data_as({np.dtype(np.uint32): _lib.u32p, np.dtype(np.float32): _lib.f32p, np.dtype(np.uint8): _lib.u8p}[x.dtype])
    c3, out_w, out_c = np.ones(3, np.uint8), np.zeros(3, np.float32), np.zeros(3, np.uint8)
    msg = lambda: (L.snn_last_error() or b"").decode()
    assert L.snn_graph_csr_lookup(dn._h, ptr(u32(1, 56, 3)), ptr(ok_q), 3, ptr(out_w), ptr(out_c)) == BAD_ARG and "pair 1 (pre 56" in msg()
    assert L.snn_graph_csr_lookup(dn._h, None, ptr(ok_q), 3, ptr(out_w), ptr(out_c)) == BAD_ARG and "null" in msg()
    assert L.snn_graph_csr_lookup(dn._h, ptr(ok_p), ptr(ok_q), 3, ptr(out_w), None) == BAD_ARG
    assert L.snn_graph_csr_edit(dn._h, ptr(ok_p), ptr(ok_q), None, ptr(c3), 3) == BAD_ARG
    assert L.snn_graph_csr_edit(dn._h, ptr(ok_p), ptr(ok_q), ptr(w3), None, 3) == BAD_ARG
    assert L.snn_graph_csr_lookup(None, ptr(ok_p), ptr(ok_q), 3, ptr(out_w), ptr(out_c)) == BAD_ARG
    assert L.snn_graph_csr_lookup(dn._h, None, None, 0, None, None) == 0 and L.snn_graph_csr_edit(dn._h, None, None, None, None, 0) == 0
    n = C.c_uint64()
    assert L.snn_graph_csr_incoming(dn._h, 50, None, None, 0, C.byref(n)) == BAD_ARG and "post 50" in msg()
    assert L.snn_graph_csr_outgoing(dn._h, 56, None, None, 0, C.byref(n)) == BAD_ARG and "pre 56" in msg()
    assert L.snn_graph_csr_incoming(dn._h, 3, None, None, 0, None) == BAD_ARG
    assert digest(dn) == before
    # "stay absent" alone is accepted and changes nothing; so is an accepted edit of the three edges, for contrast
    dn.graph_edit(absent[:20, 0], absent[:20, 1], 5.0, np.zeros(20, bool))
    assert digest(dn) == before
    dn.graph_edit(ok_p, ok_q, w3)
    assert digest(dn) != before
    dn.graph_edit(ok_p, ok_q, ragged.csr[2][[3, 40, 900]])
    assert digest(dn) == before


# ---- 4. edits reach the stepper through the step image ------------------------------------------------------------------------------
def test_edits_reach_the_stepper_through_the_step_image(snn):
    rule, weight = ConnectionRule.chebyshev(2, self_edges=False), WeightRule.uniform(0.5, 1.5, seed=2)
    on = rule.mask((9, 9), (9, 9))
    net = parity.make_oracle(parity.Layout([(0, 9, 9)]), model=ob.IZHIKEVICH, electrical=True, chemical=False)
    net["current_voltage"] = ob.uniform_array(1, 81, -65.0, 30.0)
    net["gap_conductance"] = 1.0
    net["connections"][...] = on
    net["weights"][...] = np.where(on, weight.values((9, 9), (9, 9)), np.float32(0))
    edited, fresh, unedited = (parity.device_from_oracle(snn, net, csr=True) for _ in range(3))
    dense = parity.device_from_oracle(snn, net)
    csr = parity.csr_for_posts(net, edited.owned)
    pre, post = edge_pairs(csr, edited.owned)
    handles = (edited, fresh, unedited, dense)
    for dn in handles:
        dn.set_history(voltage=True)
        dn.run(5)                                                 # the step image is packed now
    packed = edited.stat("steps_sparse_image")
    assert packed > 0
    rng = np.random.default_rng(3)
    edges = rng.choice(pre.size, 40, replace=False)
    values = rng.uniform(2.0, 6.0, 40).astype(np.float32)
    edited.graph_edit(pre[edges], post[edges], values)
    dense.graph_edit(pre[edges], post[edges], values)
    w = csr[2].copy()
    w[edges] = values
    fresh.set_graph_csr(csr[0], csr[1], w)
    for dn in handles:
        dn.run(20)
    assert edited.stat("steps_sparse_image") > packed, "the image path is the one under test"
    v = edited.voltage_history(0)
    assert v.shape[0] == 25
    assert np.array_equal(parity.bits(v), parity.bits(fresh.voltage_history(0))), "against set_graph_csr with the edited weights"
    assert np.array_equal(parity.bits(v), parity.bits(dense.voltage_history(0))), "against the dense handle edited the same way"
    assert not np.array_equal(parity.bits(v), parity.bits(unedited.voltage_history(0))), "the edit must matter to the voltages"
    assert np.array_equal(parity.bits(v[:5]), parity.bits(unedited.voltage_history(0)[:5]))
    for dn in handles:
        dn.close()


# ---- 5. deferred updates ---------------------------------------------------------------------------------------------------------
def test_queries_see_deferred_updates_and_edits_survive_them(snn):
    net = dense_tests.stdp_oracle()
    a, b, c = (parity.device_from_oracle(snn, net, csr=True) for _ in range(3))
    d = parity.device_from_oracle(snn, net)
    csr = parity.csr_for_posts(net, a.owned)
    pre, post = edge_pairs(csr, a.owned)
    before = a.get_graph_csr().copy()
    for dn in (a, b, c, d):
        dn.run(40)
    # the first getter after the run: the lookup (handle a), the row lists (handle b) -- then the weights
    w, on = a.graph_lookup(pre, post)
    now = a.get_graph_csr()
    assert on.all() and same_bits(w, now)
    assert not same_bits(now, before), "the run must have changed weights (STDP)"
    rows = [b.graph_incoming(q) for q in range(32)]
    assert same_bits(b.get_graph_csr(), now)
    for q, (index, weights) in enumerate(rows):
        lo, hi = int(csr[0][q]), int(csr[0][q + 1])
        assert np.array_equal(index, csr[1][lo:hi]) and same_bits(weights, now[lo:hi]), q
    # an edit right after a run (handle c: the edit is its first call) survives the next steps' updates as on the dense handle
    c.graph_edit(pre[[5, 77]], post[[5, 77]], [4.5, 1.25])
    d.graph_edit(pre[[5, 77]], post[[5, 77]], [4.5, 1.25])
    for dn in (c, d):
        dn.run(20)
    dw, _ = d.graph_lookup(pre, post)
    after = c.get_graph_csr()
    assert same_bits(after, dw)
    edited = now.copy()
    edited[[5, 77]] = [4.5, 1.25]
    assert not same_bits(after, edited), "the second run must have changed weights too"
    for dn in (a, b, c, d):
        dn.close()


# ---- 6. handle forms -----------------------------------------------------------------------------------------------------------
def test_reward_modulated_handle_restarts_the_traces_of_edited_edges(snn):
    dn = handle(snn, RAGGED, csr=True)
    w, c = dense_tests.pattern(RAGGED)
    csr = csr_of(w, c, dn.owned)
    dn.set_graph_csr(*csr)
    dn.set_reward_modulator(1, do_modulation=True)
    pre, post = edge_pairs(csr, dn.owned)
    t = (np.float32(1.0) + np.arange(pre.size, dtype=np.float32) / np.float32(4096.0)).astype(np.float32)
    dn.set_traces_csr(t)
    edges = np.random.default_rng(8).choice(pre.size, 60, replace=False)
    dn.graph_edit(pre[edges], post[edges], 0.75)
    want = t.copy()
    want[edges] = 0
    assert same_bits(dn.get_traces_csr(), want)
    weights = csr[2].copy()
    weights[edges] = 0.75
    assert same_bits(dn.get_graph_csr(), weights)
    dn.close()


def test_contiguous_shards_answer_for_the_rows_they_own(snn, long):
    shards = [Twin(snn, "long", shard=(k, 3)) for k in range(3)]
    out = {p: [] for p in (0, 4, 1675, NO_SOURCE, 1680)}
    owned = 0
    for k, t in enumerate(shards):
        dn = t.sparse
        b, e = dn.post_begin, dn.post_end
        owned += e - b
        rows = np.array([0, 3, 4, 1674, 1675, 1680] * 2, np.uint32)
        cols = np.array([b, b + 1, b + 63, e - 1, e - 2, (b + e) // 2] + [e - 1, b, e - 3, b + 5, b + 64, b + 65], np.uint32)
        w, on = dn.graph_lookup(rows, cols)
        ww, won = long.dense.graph_lookup(rows, cols)
        assert np.array_equal(on, won) and same_bits(w, ww)
        for q in sorted({b, b + 1, e - 1, min(max(NO_INCOMING, b), e - 1), min(max(ONE_ENTRY, b), e - 1), min(max(193, b), e - 1)}):
            index, weights = dn.graph_incoming(q)
            wi, ww = long.dense.graph_incoming(q)
            assert np.array_equal(index, wi) and same_bits(weights, ww), (k, q)
        for p in out:
            index, weights = dn.graph_outgoing(p)
            assert index.size == 0 or (b <= index[0] and index[-1] < e), "the owned rows only, as global indices"
            out[p].append((index, weights))
        other = e if k == 0 else b - 1
        for call, text in [(lambda: dn.graph_lookup([5, 6, 7], [b, other, b]), "pair 1"), (lambda: dn.graph_incoming(other), f"post {other}"),
                           (lambda: dn.graph_edit([5, 6, 7], [b, b, other], 1.0), "pair 2")]:
            with pytest.raises(snn.SnnError) as err:
                call()
            assert err.value.code == BAD_ARG and text in str(err.value) and "shard owns" in str(err.value), str(err.value)
        # an edit of owned edges, read back through the shard
        pre, post = edge_pairs(t.csr, dn.owned)
        dn.graph_edit(pre[[0, -1]], post[[0, -1]], [9.0, -9.0])
        weights = t.csr[2].copy()
        weights[[0, -1]] = [9.0, -9.0]
        assert same_bits(dn.get_graph_csr(), weights)
        dn.graph_edit(pre[[0, -1]], post[[0, -1]], t.csr[2][[0, -1]])
    assert owned == LONG.n_neurons
    for p, parts in out.items():
        index, weights = long.sparse.graph_outgoing(p)
        assert np.array_equal(np.concatenate([x for x, _ in parts]), index) and same_bits(np.concatenate([y for _, y in parts]), weights), p
    for t in shards:
        t.close()


def test_handles_the_calls_do_not_cover_and_the_empty_graph(snn, ragged):
    L = ragged.sparse._L
    u32 = lambda *v: np.array(v, np.uint32)
    ptr = lambda x: x.ctypes.data_as({np.dtype(np.uint32): _lib.u32p, np.dtype(np.float32): _lib.f32p, np.dtype(np.uint8): _lib.u8p}[x.dtype])
    p3, q3, w3, c3 = u32(1, 20, 55), u32(2, 30, 49), np.array([1.0, 2.0, 3.0], np.float32), np.ones(3, np.uint8)
    out_w, out_c, n = np.zeros(3, np.float32), np.zeros(3, np.uint8), C.c_uint64()
    msg = lambda: (L.snn_last_error() or b"").decode()

    def four(h):
        return (L.snn_graph_csr_lookup(h, ptr(p3), ptr(q3), 3, ptr(out_w), ptr(out_c)), msg(),
                L.snn_graph_csr_edit(h, ptr(p3), ptr(q3), ptr(w3), ptr(c3), 3), msg(),
                L.snn_graph_csr_incoming(h, 3, None, None, 0, C.byref(n)), msg(),
                L.snn_graph_csr_outgoing(h, 3, None, None, 0, C.byref(n)), msg())

    before = dense_tests.digest(ragged.dense)
    answers = four(ragged.dense._h)
    assert answers[0::2] == (BAD_STATE,) * 4 and all("dense" in m and "snn_graph_lookup" in m and "snn_graph_edit" in m for m in answers[1::2])
    assert dense_tests.digest(ragged.dense) == before

    by_lattice = handle(snn, RAGGED, finalize=False)
    by_lattice.finalize(0, 2, csr=True, by_lattice=True)
    answers = four(by_lattice._h)
    assert answers[0::2] == (BAD_STATE,) * 4 and all("not covered" in m for m in answers[1::2]), answers
    by_lattice.close()

    raw = handle(snn, RAGGED, finalize=False)
    answers = four(raw._h)
    assert answers[0::2] == (BAD_STATE,) * 4 and all("finalized" in m for m in answers[1::2])
    raw.close()

    empty = handle(snn, RAGGED, csr=True)                  # a sparse handle that holds no graph yet
    w, on = empty.graph_lookup(*all_pairs(empty))
    assert not on.any() and not w.view(np.uint32).any()
    assert all(empty.graph_incoming(q)[0].size == 0 for q in (0, 49)) and all(empty.graph_outgoing(p)[0].size == 0 for p in (0, 55))
    empty.graph_edit(p3, q3, w3, np.zeros(3, bool))
    with pytest.raises(snn.SnnError) as err:
        empty.graph_edit(p3, q3, w3, [0, 1, 1])
    assert err.value.code == BAD_ARG and "pair 1 (pre 20, post 30)" in str(err.value) and "fixed" in str(err.value)
    empty.close()
