"""snn_graph_csr_edit_structure: edit_weight(pre, post, Option<f32>) on a sparse handle WITH the structure -- Some(w) on an absent
pair connects it, None on a stored edge removes it -- merged on the device and held, bit for bit, to expectations that do not
touch the new kernels: the edits applied one after another to the host matrices in numpy and taken in CSR order, and the trusted
snn_graph_edit of a dense handle that holds the same edges.  Layouts: RAGGED (50 rows, one partial SELL slice, cells as
presynaptic indices; here with one row emptied and one row of a single entry) and LONG (27 slices; rows of 0, 1, 63, 64, 65 and
more than 1 024 entries).  No tolerance anywhere."""

import numpy as np
import pytest

import oracle_binding as ob
import parity
import test_gpu_alloc_failures_connect_spec as model
import test_gpu_connect_rule as rule_tests
import test_gpu_connect_rule_csr as csr_tests
import test_gpu_graph_query as dense_tests
import test_gpu_graph_query_csr as query_tests
from snn_amd import ConnectionRule, WeightRule, _lib

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_STATE = 11, 12
RAGGED, LONG = dense_tests.RAGGED, dense_tests.LONG
handle, pattern, all_pairs = dense_tests.handle, dense_tests.pattern, dense_tests.all_pairs
long_graph, edge_pairs, same_bits = query_tests.long_graph, query_tests.edge_pairs, query_tests.same_bits
csr_of, assert_csr, read, patterned = csr_tests.csr_of, csr_tests.assert_csr, csr_tests.read, csr_tests.patterned


def ragged_graph():
    """pattern(RAGGED) with a row without an incoming edge and a row of exactly one entry (a cell)"""
    w, c = pattern(RAGGED)
    w, c = w.copy(), c.copy()
    c[:, 3] = 0
    c[:, 4] = 0
    c[52, 4] = 1
    w = np.where(c != 0, w, np.float32(0))
    w[52, 4] = np.float32(7.5)
    return w, c


GRAPHS = {"ragged": (RAGGED, ragged_graph), "long": (LONG, long_graph)}


def apply_edits(w, c, p, q, v, on):
    """edit_weight, one pair after another, on host matrices [n_tot, n_neurons]"""
    w, c = w.copy(), c.copy()
    for a, b, x, o in zip(p, q, v, on):
        c[a, b] = 1 if o else 0
        w[a, b] = x if o else np.float32(0)
    return w, c


def shuffled_call(c, rng, posts=None):
    """One call with everything a structural edit can meet, over the rows `posts` (None: all); returns (pre, post, weights,
    connected) shuffled, with repeats, and the set of kinds it contains.  Weights name the position in the call."""
    n_tot, nn = c.shape
    rows = np.arange(nn) if posts is None else np.asarray(posts)
    lengths = (c != 0).sum(axis=0)
    edits, ordered, kinds = [], [], set()             # (pre, post, connected); (i, j): edit i must stay before edit j

    def stored(q):
        return np.nonzero(c[:, q])[0]

    def absent(q):
        return np.nonzero(c[:, q] == 0)[0]

    def add(kind, p, q, on):
        edits.append((int(p), int(q), bool(on)))
        kinds.add(kind)
        return len(edits) - 1

    used = set()

    def take(candidates, kind):
        for q in candidates:
            if int(q) not in used:
                used.add(int(q))
                return int(q)
        return None

    q = take(rows[lengths[rows] == 0], "empty")
    if q is not None:
        add("insert into the row without incoming edges", 5, q, True)
    q = take(rows[lengths[rows] == 1], "one")
    if q is not None:
        add("remove the only entry", stored(q)[0], q, False)
    q = take([r for r in rows if lengths[r] > 2 and c[0, r] == 0 and c[n_tot - 1, r] == 0], "ends")
    if q is not None:
        add("insert before the first entry", 0, q, True)
        add("insert after the last entry, a cell", n_tot - 1, q, True)
    q = take(rows[lengths[rows] == 64], "64")
    if q is not None:
        add("insert into a 64-entry row", absent(q)[3], q, True)
    q = take(rows[lengths[rows] == 65], "65")
    if q is not None:
        add("remove from a 65-entry row", stored(q)[40], q, False)
    first_slice = [r for r in rows if r < 64 and r not in used]
    if first_slice:                                    # the widest row of the first slice grows: every later slice_ptr moves
        q = take([max(first_slice, key=lambda r: lengths[r])], "widest")
        add("insert into the widest row of slice 0", absent(q)[0], q, True)
    q = take([r for r in rows if 2 < lengths[r] < 100], "all")
    if q is not None:
        for p in stored(q):
            add("remove every entry of a row", p, q, False)
    q = take(sorted(rows, key=lambda r: -lengths[r]), "long")                 # (the longest row no other kind has taken)
    many = 70 if lengths[q] > 1024 else 6
    for p in rng.choice(absent(q), min(many, absent(q).size), replace=False):
        add(f"{many} inserts into one row", p, q, True)
    for p in rng.choice(stored(q), many, replace=False):
        add(f"{many} removes from one row", p, q, False)
    free = [r for r in rows if r not in used and 4 < lengths[r] < n_tot - 4]
    for k in range(120):                               # reweights and "stay absent", scattered over other rows
        q = free[int(rng.integers(len(free)))]
        if k % 3:
            add("reweight", rng.choice(stored(q)), q, True)
        else:
            add("stay absent", rng.choice(absent(q)), q, False)
    q1, q2 = free[0], free[-1]
    for p, q, first in [(absent(q1)[1], q1, True), (stored(q1)[1], q1, True), (absent(q2)[2], q2, False), (stored(q2)[2], q2, False)]:
        i = add("connect-then-remove" if first else "remove-then-connect", p, q, first)
        j = add("connect-then-remove" if first else "remove-then-connect", p, q, not first)
        ordered.append((i, j))
    for k in rng.choice(len(edits) - 8, 30, replace=False):               # repeats: the same pair again, with another weight
        edits.append(edits[int(k)])
    index = [int(k) for k in rng.permutation(len(edits))]
    for i, j in ordered:
        a, b = index.index(i), index.index(j)
        if a > b:
            index[a], index[b] = index[b], index[a]
    p = np.array([edits[k][0] for k in index], np.uint32)
    q = np.array([edits[k][1] for k in index], np.uint32)
    on = np.array([edits[k][2] for k in index], bool)
    v = (np.float32(-1000.0) - np.arange(p.size, dtype=np.float32)).astype(np.float32)
    return p, q, v, on, kinds


def ascending_call(c, rng, posts=None):
    """strictly ascending by (pre, post), every pair once: inserts, removes and reweights"""
    n_tot, nn = c.shape
    rows = np.arange(nn) if posts is None else np.asarray(posts)
    flat = np.sort(rng.choice(n_tot * rows.size, min(300, n_tot * rows.size // 4), replace=False))
    p, q = (flat // rows.size).astype(np.uint32), rows[flat % rows.size].astype(np.uint32)
    on = rng.random(p.size) < 0.6
    v = (np.float32(5000.0) + np.arange(p.size, dtype=np.float32)).astype(np.float32)
    return p, q, v, on


def assert_equals_the_dense_twin(sparse, dense, p, q):
    pre, post = all_pairs(sparse)
    w, on = sparse.graph_lookup(pre, post)
    dw, don = dense.graph_lookup(pre, post)
    assert np.array_equal(on, don) and same_bits(w, dw)
    for b in np.unique(q):
        index, weights = sparse.graph_incoming(b)
        di, dw = dense.graph_incoming(b)
        assert np.array_equal(index, di) and same_bits(weights, dw), f"incoming({b})"
    for a in np.unique(p):
        index, weights = sparse.graph_outgoing(a)
        di, dw = dense.graph_outgoing(a)
        assert np.array_equal(index, di) and same_bits(weights, dw), f"outgoing({a})"


# ---- 1. layouts and edit lists ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ragged", "long"])
def test_three_calls_against_numpy_and_the_dense_twin(snn, which):
    layout, graph = GRAPHS[which]
    w, c = graph()
    sparse, dense, plain = handle(snn, layout, csr=True), handle(snn, layout), handle(snn, layout, csr=True)
    sparse.set_graph_csr(*csr_of(w, c, sparse.owned))
    dense.set_graph_rows(0, w, c)
    rng = np.random.default_rng(17)
    p, q, v, on, kinds = shuffled_call(c, rng)
    want_kinds = {"insert into the row without incoming edges", "remove the only entry", "insert before the first entry",
                  "insert after the last entry, a cell", "insert into the widest row of slice 0", "remove every entry of a row", "reweight",
                  "stay absent", "connect-then-remove", "remove-then-connect"}
    want_kinds |= ({"insert into a 64-entry row", "remove from a 65-entry row", "70 inserts into one row", "70 removes from one row"}
                   if which == "long" else {"6 inserts into one row", "6 removes from one row"})
    assert kinds == want_kinds, kinds ^ want_kinds
    assert (p >= layout.n_neurons).any(), "a spike-train cell as pre"
    sparse.graph_edit(p, q, v, on, structure=True)
    dense.graph_edit(p, q, v, on, structure=True)              # (the keyword changes nothing on a dense handle)
    w1, c1 = apply_edits(w, c, p, q, v, on)
    want = csr_of(w1, c1, sparse.owned)
    assert not np.array_equal(want[0], csr_of(w, c, sparse.owned)[0]) and sparse._nnz == want[1].size
    assert_csr(sparse, want, "after the shuffled call")
    assert_equals_the_dense_twin(sparse, dense, p, q)
    # strictly ascending, no pair twice
    p, q, v, on = ascending_call(c1, rng)
    sparse.graph_edit(p, q, v, on, structure=True)
    dense.graph_edit(p, q, v, on)
    w2, c2 = apply_edits(w1, c1, p, q, v, on)
    want = csr_of(w2, c2, sparse.owned)
    assert want[1].size != csr_of(w1, c1, sparse.owned)[1].size and sparse._nnz == want[1].size
    assert_csr(sparse, want, "after the ascending call")
    assert_equals_the_dense_twin(sparse, dense, p, q)
    # non-structural only: the structure stays, the weights are those snn_graph_csr_edit leaves
    plain.set_graph_csr(*want)
    structure = sparse.graph_csr_structure()
    pre, post = edge_pairs(want, sparse.owned)
    edges = rng.choice(pre.size, 200, replace=False)
    edges = np.concatenate([edges, edges[:30]])[rng.permutation(230)]
    gone = np.argwhere(c2 == 0)[rng.choice((c2 == 0).sum(), 25, replace=False)].astype(np.uint32)
    at = np.sort(rng.choice(edges.size, 25, replace=False))
    p, q = np.insert(pre[edges], at, gone[:, 0]), np.insert(post[edges], at, gone[:, 1])
    v = np.insert(rng.uniform(-3.0, 3.0, edges.size).astype(np.float32), at, np.float32(np.nan))
    on = np.insert(np.ones(edges.size, bool), at, False)
    sparse.graph_edit(p, q, v, on, structure=True)
    plain.graph_edit(p, q, v, on)
    for x, y in zip(sparse.graph_csr_structure(), structure):
        assert np.array_equal(x, y)
    assert same_bits(sparse.get_graph_csr(), plain.get_graph_csr())
    assert (sparse.get_graph_csr().view(np.uint32) != want[2].view(np.uint32)).sum() == 200
    for dn in (sparse, dense, plain):
        dn.close()


# ---- 2. a handle with no graph ---------------------------------------------------------------------------------------------------------
def test_connects_build_a_graph_from_the_empty_one(snn):
    dn = handle(snn, RAGGED, csr=True)
    w, c = pattern(RAGGED)
    p, q = np.nonzero(c[:, ::3])
    q = q * 3
    order = np.random.default_rng(2).permutation(p.size)
    p, q = p[order].astype(np.uint32), q[order].astype(np.uint32)
    dn.graph_edit(p, q, w[p, q], np.zeros(p.size, bool), structure=True)            # "stay absent" everywhere: still no graph
    assert dn._nnz == 0 and dn.graph_csr_structure()[1].size == 0
    dn.graph_edit(p, q, w[p, q], structure=True)
    c0 = np.zeros_like(c)
    c0[:, ::3] = c[:, ::3]
    assert_csr(dn, csr_of(np.where(c0 != 0, w, np.float32(0)), c0, dn.owned), "on a handle that held no graph")
    assert dn._nnz == p.size
    dn.run(3)
    dn.close()


# ---- 3. the stepper --------------------------------------------------------------------------------------------------------------------
def test_structural_edits_reach_the_stepper_through_the_step_image(snn):
    rule, weight = ConnectionRule.chebyshev(2, self_edges=False), WeightRule.uniform(0.5, 1.5, seed=2)
    on = rule.mask((9, 9), (9, 9))
    net = parity.make_oracle(parity.Layout([(0, 9, 9)]), model=ob.IZHIKEVICH, electrical=True, chemical=False)
    net["current_voltage"] = ob.uniform_array(1, 81, -65.0, 30.0)
    net["gap_conductance"] = 1.0
    net["connections"][...] = on
    net["weights"][...] = np.where(on, weight.values((9, 9), (9, 9)), np.float32(0))
    edited, fresh, unedited = (parity.device_from_oracle(snn, net, csr=True) for _ in range(3))
    for dn in (edited, fresh, unedited):
        dn.set_history(voltage=True)
        dn.run(5)                                                 # the step image is packed now
    net.run(5)
    packed = edited.stat("steps_sparse_image")
    assert packed > 0
    c = np.array(net["connections"], np.uint32)
    rng = np.random.default_rng(3)
    cut = [np.array([(a, b) for a in np.nonzero(c[:, b])[0]]) for b in (0, 40, 77)]          # every edge into three neurons
    some = np.argwhere(c != 0)[rng.choice(int((c != 0).sum()), 30, replace=False)]
    far = np.argwhere(c == 0)
    far = far[np.abs(far[:, 0] - far[:, 1]) > 30]
    far = far[rng.choice(far.shape[0], 40, replace=False)]                                   # long-range edges
    pairs = np.concatenate(cut + [some, far])
    kinds = np.concatenate([np.zeros(pairs.shape[0] - 40, bool), np.ones(40, bool)])
    order = rng.permutation(pairs.shape[0])
    p, q, kinds = pairs[order, 0].astype(np.uint32), pairs[order, 1].astype(np.uint32), kinds[order]
    v = rng.uniform(2.0, 6.0, p.size).astype(np.float32)
    edited.graph_edit(p, q, v, kinds, structure=True)
    w1, c1 = apply_edits(np.array(net["weights"], np.float32), c, p, q, v, kinds)
    want = csr_of(w1, c1, edited.owned)
    assert_csr(edited, want, "after the structural edit")
    fresh.set_graph_csr(*want)
    net["connections"][...] = c1
    net["weights"][...] = w1
    for dn in (edited, fresh, unedited):
        dn.run(30)
    net.run(30)
    assert edited.stat("steps_sparse_image") > packed, "the image path is the one under test"
    v_edited = edited.voltage_history(0)
    assert v_edited.shape[0] == 35
    assert np.array_equal(parity.bits(v_edited), parity.bits(fresh.voltage_history(0))), "against set_graph_csr with the expected CSR"
    assert not np.array_equal(parity.bits(v_edited), parity.bits(unedited.voltage_history(0))), "the edit must matter to the voltages"
    for dn in (edited, fresh):
        parity.assert_state_equal(net, parity.pull_state(dn, net))
        parity.assert_graph_equal(net, dn)
    for dn in (edited, fresh, unedited):
        dn.close()


def test_kept_edges_keep_plastic_weights_and_the_run_goes_on(snn):
    net = csr_tests.firing_oracle(RAGGED, chemical=False, plastic=True)
    rule_tests.twin_graph(net, rule_tests.PLAN)
    dn = parity.device_from_oracle(snn, net, csr=True)
    uploaded = dn.get_graph_csr()
    dn.run(csr_tests.STDP_STEPS)
    net.run(csr_tests.STDP_STEPS)
    rp, pi, now = read(dn)
    assert (now.view(np.uint32) != uploaded.view(np.uint32)).any(), "STDP must have moved a weight for this test to mean anything"
    parity.assert_graph_equal(net, dn)
    w, c = csr_tests.dense_of(rp, pi, now, dn.n_tot, dn.n_neurons, dn.owned)
    rng = np.random.default_rng(9)
    stored, gone = np.argwhere(c != 0), np.argwhere(c == 0)
    removed = stored[rng.choice(stored.shape[0], 40, replace=False)]
    added = gone[rng.choice(gone.shape[0], 40, replace=False)]
    pairs = np.concatenate([removed, added])
    order = rng.permutation(80)
    p, q = pairs[order, 0].astype(np.uint32), pairs[order, 1].astype(np.uint32)
    on = (np.arange(80) >= 40)[order]
    v = rng.uniform(0.5, 1.5, 80).astype(np.float32)
    dn.graph_edit(p, q, v, on, structure=True)
    w1, c1 = apply_edits(w, c, p, q, v, on)
    want = csr_of(w1, c1, dn.owned)
    assert_csr(dn, want, "after the structural edit")           # kept edges: the weights from before the edit, bit for bit
    pre1, post1 = edge_pairs(want, dn.owned)
    kept = c[pre1, post1] != 0
    assert kept.sum() == now.size - 40 and same_bits(want[2][kept], w[pre1[kept], post1[kept]])
    net["connections"][...] = c1
    net["weights"][...] = w1
    dn.run(100)
    net.run(100)
    parity.assert_state_equal(net, parity.pull_state(dn, net))
    parity.assert_graph_equal(net, dn)
    assert not same_bits(dn.get_graph_csr(), want[2]), "the second run must have changed weights too"
    dn.close()


# ---- 4. per-edge state -----------------------------------------------------------------------------------------------------------------
def test_kept_edges_keep_traces_dw_and_counters(snn):
    dn, w, c = patterned(snn, RAGGED)
    dn.set_reward_modulator(1, do_modulation=True)
    dn.set_connection_kind(0, 1, 1)
    before = csr_of(w, c, dn.owned)
    pre, post = edge_pairs(before, dn.owned)
    t = (np.float32(1.0) + np.arange(pre.size, dtype=np.float32) / np.float32(4096.0)).astype(np.float32)
    counters = (np.arange(pre.size) % 3 != 0).astype(np.uint8)
    dn.set_traces_csr(t)
    dn.set_pending_csr(-t)
    dn.set_counters_csr(counters)
    rng = np.random.default_rng(12)
    stored, gone = np.argwhere(c != 0), np.argwhere(c == 0)
    pairs = np.concatenate([stored[rng.choice(stored.shape[0], 90, replace=False)], gone[rng.choice(gone.shape[0], 50, replace=False)]])
    on = np.concatenate([np.zeros(45, bool), np.ones(45, bool), np.ones(30, bool), np.zeros(20, bool)])    # remove, reweight, insert, stay absent
    order = rng.permutation(140)
    p, q, on = pairs[order, 0].astype(np.uint32), pairs[order, 1].astype(np.uint32), on[order]
    dn.graph_edit(p, q, 0.75, on, structure=True)
    w1, c1 = apply_edits(w, c, p, q, np.full(140, 0.75, np.float32), on)
    want = csr_of(w1, c1, dn.owned)
    assert_csr(dn, want)
    assert dn._nnz == want[1].size == pre.size - 45 + 30
    old_edge = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(pre, post))}
    written = {(int(a), int(b)) for a, b, o in zip(p, q, on) if o}
    pre1, post1 = edge_pairs(want, dn.owned)
    source = np.array([-1 if (int(a), int(b)) in written else old_edge[(int(a), int(b))] for a, b in zip(pre1, post1)])
    assert (source < 0).sum() == 75
    for got, plane in ((dn.get_traces_csr(), t), (dn.get_pending_csr(), -t), (dn.get_counters_csr(), counters)):
        assert got.size == dn._nnz
        assert same_bits(got, np.where(source >= 0, plane[source], 0).astype(plane.dtype))
    dn.run(3)
    dn.close()


# ---- 5. contiguous shards --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ragged", "long"])
def test_contiguous_shards_edit_the_rows_they_own(snn, which):
    layout, graph = GRAPHS[which]
    w, c = graph()
    owned = 0
    for k in range(3):
        dn = handle(snn, layout, csr=True, shard=(k, 3))
        dn.set_graph_csr(*csr_of(w, c, dn.owned))
        b, e = dn.post_begin, dn.post_end
        owned += e - b
        if e == b:                                         # (RAGGED is one slice: the other two shards own no row, and no pair)
            with pytest.raises(snn.SnnError) as err:
                dn.graph_edit([5], [0], 1.0, structure=True)
            assert err.value.code == BAD_ARG and "pair 0 (pre 5, post 0)" in str(err.value) and "shard owns" in str(err.value)
            dn.close()
            continue
        p, q, v, on, _ = shuffled_call(c, np.random.default_rng(30 + k), posts=dn.owned)
        assert q.min() >= b and q.max() < e
        other = b - 1 if b else e                          # (a shard that owns every row: the first index that is no neuron)
        why = "shard owns" if other < layout.n_neurons else "n_neurons"
        before = read(dn)
        with pytest.raises(snn.SnnError) as err:
            dn.graph_edit(np.append(p[:9], 5), np.append(q[:9], other), np.append(v[:9], 1.0), np.append(on[:9], True), structure=True)
        assert err.value.code == BAD_ARG and f"pair 9 (pre 5, post {other})" in str(err.value) and why in str(err.value)
        assert_csr(dn, before, "after the refused call")
        dn.graph_edit(p, q, v, on, structure=True)
        w1, c1 = apply_edits(w, c, p, q, v, on)
        twin = handle(snn, layout, csr=True, shard=(k, 3))
        twin.set_graph_csr(*csr_of(w1, c1, twin.owned))
        for x, y in zip(read(dn), read(twin)):
            assert same_bits(x, y), f"shard {k} of 3 (rows {b}..{e})"
        for peer in range(3):
            assert np.array_equal(dn.halo_needs(peer), twin.halo_needs(peer)), (k, peer)
        dn.close()
        twin.close()
    assert owned == layout.n_neurons


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_graph_alone(snn):
    dn, w, c = patterned(snn, RAGGED)
    L = dn._L
    before = query_tests.digest(dn)
    pre, post = edge_pairs(csr_of(w, c, dn.owned), dn.owned)
    gone = np.argwhere(c == 0).astype(np.uint32)
    ok_p, ok_q = np.array([pre[3], gone[5, 0], pre[900]], np.uint32), np.array([post[3], gone[5, 1], post[900]], np.uint32)
    w3, on3 = np.array([1.0, 2.0, 3.0], np.float32), np.array([1, 1, 0], np.uint8)
    ptr = lambda x: x.ctypes.data_as({np.dtype(np.uint32): _lib.u32p, np.dtype(np.float32): _lib.f32p, np.dtype(np.uint8): _lib.u8p}[x.dtype])
    msg = lambda: (L.snn_last_error() or b"").decode()

    def refused(p, q, v, on, *texts, code=BAD_ARG):
        with pytest.raises(snn.SnnError) as err:
            dn.graph_edit(p, q, v, on, structure=True)
        assert err.value.code == code and all(t in str(err.value) for t in texts), str(err.value)
        assert query_tests.digest(dn) == before

    refused(ok_p, ok_q, [1.0, np.nan, 3.0], [1, 1, 0], f"pair 1 (pre {ok_p[1]}, post {ok_q[1]})", "NaN")
    refused([1, 56, 3], ok_q, w3, [0, 0, 0], f"pair 1 (pre 56, post {ok_q[1]})", "n_tot")
    refused(ok_p, [2, 30, 50], w3, on3, f"pair 2 (pre {ok_p[2]}, post 50)")
    for args in [(None, ptr(ok_q), ptr(w3), ptr(on3)), (ptr(ok_p), None, ptr(w3), ptr(on3)), (ptr(ok_p), ptr(ok_q), None, ptr(on3)),
                 (ptr(ok_p), ptr(ok_q), ptr(w3), None)]:
        assert L.snn_graph_csr_edit_structure(dn._h, *args, 3) == BAD_ARG and "null" in msg()
        assert query_tests.digest(dn) == before
    assert L.snn_graph_csr_edit_structure(None, ptr(ok_p), ptr(ok_q), ptr(w3), ptr(on3), 3) == BAD_ARG
    assert L.snn_graph_csr_edit_structure(dn._h, None, None, None, None, 0) == 0
    dn.graph_edit(ok_p, ok_q, w3, [1, 0, 1], structure=True)         # accepted, for contrast: two weights, one "stay absent"
    assert query_tests.digest(dn) != before
    stored_w = csr_of(w, c, dn.owned)[2]                             # (the weight of a pair that is not connected is not looked at)
    dn.graph_edit(ok_p, ok_q, [stored_w[3], np.nan, stored_w[900]], [1, 0, 1], structure=True)
    assert query_tests.digest(dn) == before
    # the call that refuses to change a structure still does
    for on, text in (([1, 1, 1], "cannot connect"), ([1, 0, 0], "cannot remove")):
        with pytest.raises(snn.SnnError) as err:
            dn.graph_edit(ok_p, ok_q, w3, on)
        assert err.value.code == BAD_ARG and text in str(err.value) and "structure of a sparse graph is fixed" in str(err.value)
        assert query_tests.digest(dn) == before
    dn.close()

    dense = handle(snn, RAGGED)
    dense.set_graph_rows(0, w, c)
    was = dense_tests.digest(dense)
    assert L.snn_graph_csr_edit_structure(dense._h, ptr(ok_p), ptr(ok_q), ptr(w3), ptr(on3), 3) == BAD_STATE and "dense" in msg()
    assert dense_tests.digest(dense) == was
    dense.graph_edit(ok_p, ok_q, w3, on3, structure=True)            # accepted: a dense edit, structural as ever
    gw, gc = dense.get_graph_rows(0, dense.n_tot)
    assert gc[ok_p[1], ok_q[1]] == 1 and gc[ok_p[2], ok_q[2]] == 0 and gw[ok_p[1], ok_q[1]] == 2.0
    dense.close()

    slab = handle(snn, RAGGED, finalize=False)
    slab.finalize(0, 2, csr=True, by_lattice=True)
    slab.set_graph_csr(*csr_of(w, c, slab.owned))
    assert L.snn_graph_csr_edit_structure(slab._h, ptr(ok_p), ptr(ok_q), ptr(w3), ptr(on3), 3) == BAD_STATE and "not covered" in msg()
    assert_csr(slab, csr_of(w, c, slab.owned), "on the by-lattice shard after the refusal")
    slab.close()

    raw = handle(snn, RAGGED, finalize=False)
    assert L.snn_graph_csr_edit_structure(raw._h, ptr(ok_p), ptr(ok_q), ptr(w3), ptr(on3), 3) == BAD_STATE and "finalized" in msg()
    raw.close()


# ---- 7. allocation failures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structural", [True, False], ids=["structural", "weights_only"])
def test_every_allocation_of_a_call_may_fail(snn, structural):
    w, c = pattern(RAGGED)
    rng = np.random.default_rng(4)
    if structural:
        p, q, v, on, _ = shuffled_call(c, rng)
    else:
        stored, gone = np.argwhere(c != 0), np.argwhere(c == 0)
        pairs = np.concatenate([stored[rng.choice(stored.shape[0], 150, replace=False)], gone[rng.choice(gone.shape[0], 20, replace=False)]])
        order = rng.permutation(170)
        p, q, on = pairs[order, 0].astype(np.uint32), pairs[order, 1].astype(np.uint32), (np.arange(170) < 150)[order]
        v = rng.uniform(-2.0, 2.0, 170).astype(np.float32)
    failed, total, messages = model.walk(snn, lambda: patterned(snn, RAGGED)[0], lambda dn: dn.graph_edit(p, q, v, on, structure=True), read,
                                         20 if structural else 10)
    assert failed == total, (failed, total, messages)
    dn = patterned(snn, RAGGED)[0]
    dn.graph_edit(p, q, v, on, structure=True)
    assert_csr(dn, csr_of(*apply_edits(w, c, p, q, v, on), dn.owned), "after the walk")
    dn.close()
