"""snn_connect_by_rules_csr: the sparse graph merged on the device, record by record, against expectations that do not touch the
new kernels -- the per-pair restatement of the header's formulas (connect_rule_cases.expected_for) patched into a dense host
matrix and taken in CSR order, synthetic.c5_csr, and the dense snn_connect_by_rule.  Layouts are the smallest at which the cut
points (a first lattice that starts on no multiple of 4, a spike-train pre lattice), the multi-round rank (a pre lattice of 289:
five ballot rounds with a ragged tail) and the slice padding (370 rows: six SELL slices, the last ragged) can each go wrong."""
import ctypes as C

import numpy as np
import pytest

import connect_rule_cases as cases
import oracle_binding as ob
import parity
import test_gpu_connect_rule as dense_tests          # its layouts and helpers (pattern, apply_host, geometry, handle)
from snn_amd import ConnectionRule, WeightRule, _lib, synthetic

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_STATE, DIM_MISMATCH = 11, 12, 10
RAGGED = dense_tests.RAGGED                                                       # 3x5, 5x7 neurons, 2x3 Rate cells: one slice
WIDE = parity.Layout([(0, 17, 17), (1, 9, 9)], [(2, 3, 3)])                       # 370 rows, 6 slices; 289 = 4 * 64 + 33 candidates
# all four rules, with and without thinning, with and without self edges, constant and uniform weights, a spike-train pre
# lattice, and a later record for a pair an earlier one wrote
# (block 1 -> 0 of RAGGED and block 2 -> 0 of WIDE are written by no record: they must keep the uploaded pattern)
RAGGED_PLAN = dense_tests.PLAN + [
    (2, 0, ConnectionRule.all_to_all(probability=0.5, seed=3), WeightRule.uniform(-1.0, 1.0, seed=4)),
    (1, 1, ConnectionRule.chebyshev(2, self_edges=False, probability=0.8, seed=5), WeightRule.uniform(2.0, 3.0, seed=6))]
WIDE_PLAN = [(0, 0, ConnectionRule.all_to_all(self_edges=False), WeightRule.constant(0.25)),            # 5 rounds per row
             (0, 1, ConnectionRule.euclidean(8, probability=0.6, seed=4), WeightRule.uniform(0.5, 1.5, seed=14)),
             (1, 0, ConnectionRule.all_to_all(probability=0.3, seed=9), WeightRule.constant(2.5)),
             (2, 1, ConnectionRule.same_position(), WeightRule.uniform(1.0, 2.0, seed=15)),
             (1, 1, ConnectionRule.chebyshev(3, self_edges=False), WeightRule.constant(0.75))]


def csr_of(w, c, posts):
    """CSR rows `posts` of a dense host graph [n_tot, n_neurons]: ascending presynaptic index per row"""
    on = c[:, posts].T != 0
    row_ptr = np.concatenate([[0], np.cumsum(on.sum(axis=1))]).astype(np.uint64)
    return row_ptr, np.nonzero(on)[1].astype(np.uint32), np.ascontiguousarray(w[:, posts].T[on], dtype=np.float32)


def dense_of(row_ptr, pre_index, weights, n_tot, n_neurons, posts):
    w, c = np.zeros((n_tot, n_neurons), np.float32), np.zeros((n_tot, n_neurons), np.uint32)
    cols = np.repeat(np.asarray(posts, np.int64), np.diff(row_ptr.astype(np.int64)))
    w[pre_index, cols] = weights
    c[pre_index, cols] = 1
    return w, c


def read(dn):
    rp, pi = dn.graph_csr_structure()
    return rp, pi, dn.get_graph_csr()


def assert_csr(dn, want, what=""):
    rp, pi, w = read(dn)
    assert np.array_equal(rp, want[0]), f"row_ptr differs {what}: first at row {np.argwhere(rp != want[0])[:1].tolist()}"
    assert np.array_equal(pi, want[1]), f"pre_index differs {what}: first at edge {np.argwhere(pi != want[1])[:1].tolist()}"
    assert np.array_equal(w.view(np.uint32), want[2].view(np.uint32)), f"weights differ {what}: {np.argwhere(w.view(np.uint32) != want[2].view(np.uint32))[:4].tolist()}"


def patterned(snn, layout, shard=None):
    dn = dense_tests.handle(snn, layout, shard=shard, csr=True)
    w, c = dense_tests.pattern(layout)
    dn.set_graph_csr(*csr_of(w, c, dn.owned))
    return dn, w, c


@pytest.mark.parametrize("layout,plan", [(RAGGED, RAGGED_PLAN), (WIDE, WIDE_PLAN)], ids=["ragged", "wide"])
def test_block_by_block_and_as_one_batch(snn, layout, plan):
    one, w, c = patterned(snn, layout)
    batch, _, _ = patterned(snn, layout)
    assert_csr(one, csr_of(w, c, one.owned), "after the upload of the pattern")
    for k, record in enumerate(plan):
        one.connect_sparse([record])
        dense_tests.apply_host(w, c, layout, [record])
        # the block as the per-pair loop has it; every entry outside the blocks written so far still the pattern
        assert_csr(one, csr_of(w, c, one.owned), f"after record {k}: {record[0]} -> {record[1]}")
    batch.connect_sparse(plan)
    for x, y in zip(read(one), read(batch)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "the batch and the sequence of calls differ"
    untouched, cu = dense_tests.pattern(layout)
    written = np.zeros(c.shape, bool)
    geo = dense_tests.geometry(layout)
    for pre, post, _, _ in plan:
        (f0, s0), (f1, s1) = geo[pre], geo[post]
        written[f0:f0 + s0[0] * s0[1], f1:f1 + s1[0] * s1[1]] = True
    assert (~written).any() and np.array_equal(w[~written], untouched[~written]) and np.array_equal(c[~written], cu[~written])
    one.close()
    batch.close()


def firing_oracle(layout, chemical, plastic=False):
    """both lattices fire within a few steps: gap junctions on, Rate cells, optionally AMPA and STDP"""
    net = parity.make_oracle(layout, st_kind=ob.ST_RATE, electrical=True, chemical=chemical)
    net["current_voltage"] = ob.uniform_array(6, net.n_neurons, -65.0, 30.0)
    net["gap_conductance"] = 10.0
    if chemical:
        net["nt_flags"][:, 0] = 1
        net["rc_flags"][:, 0] = 1
        net["rc_g"][:, 0] = 3.0
        net["st_nt_flags"][:, 0] = 1
    net["st_rate"] = ob.uniform_array(7, net.n_cells, 0.3, 1.5)
    net["weights"][...] = 0
    net["connections"][...] = 0
    if plastic:
        net["do_plasticity"][...] = 1
    return net


STDP_STEPS = 300          # (dt = 0.1: pairs of spikes close enough for STDP take a few hundred steps)


def test_kept_weights_are_the_current_ones(snn):
    net = firing_oracle(RAGGED, chemical=False, plastic=True)
    dense_tests.twin_graph(net, dense_tests.PLAN)
    dn = parity.device_from_oracle(snn, net, csr=True)
    uploaded = dn.get_graph_csr()
    dn.run(STDP_STEPS)
    rp, pi, now = read(dn)
    w, c = dense_of(rp, pi, now, dn.n_tot, dn.n_neurons, dn.owned)
    edit = (2, 0, ConnectionRule.chebyshev(1), WeightRule.constant(7.0))          # a block that held no edge: every old edge is kept
    moved = now.view(np.uint32) != uploaded.view(np.uint32)
    assert moved.any(), "STDP must have moved a weight for this test to mean anything"
    dn.connect_sparse([edit])
    dense_tests.apply_host(w, c, RAGGED, [edit])
    assert_csr(dn, csr_of(w, c, dn.owned), "after connecting another block")
    rp2, pi2, w2 = read(dn)
    posts = np.repeat(dn.owned, np.diff(rp2.astype(np.int64)))
    kept = ~((pi2 >= RAGGED.n_neurons) & (posts < 15))                              # (the new edges: cells into lattice 0)
    assert kept.sum() == now.size and np.array_equal(w2[kept].view(np.uint32), now.view(np.uint32))
    assert not np.array_equal(w2[kept].view(np.uint32), uploaded.view(np.uint32))
    dn.close()


@pytest.mark.parametrize("chemical", [False, True], ids=["gap", "gap_ampa"])
def test_dense_and_sparse_agree(snn, chemical):
    net = firing_oracle(RAGGED, chemical)
    a = parity.device_from_oracle(snn, net)                           # dense, no edge
    b = parity.device_from_oracle(snn, net, csr=True)                 # sparse, the empty graph
    for pre, post, rule, weight in dense_tests.PLAN:
        a.connect_by_rule(pre, post, rule, weight)
    b.connect_sparse(dense_tests.PLAN)
    dense_tests.twin_graph(net, dense_tests.PLAN)
    wa, ca = a.get_graph_rows(0, a.n_tot)
    wb, cb = dense_of(*read(b), b.n_tot, b.n_neurons, b.owned)
    assert ca.sum() > 0 and np.array_equal(ca, cb) and np.array_equal(parity.bits(wa), parity.bits(wb))
    for dn in (a, b):
        dn.set_history(voltage=True, spikes=True)
        dn.run(50)
    net.run(50, voltage_history=True, spike_history=True)
    for dn in (a, b):
        parity.assert_state_equal(net, parity.pull_state(dn, net))
        parity.assert_graph_equal(net, dn)
    assert all(np.array_equal(x, y) for x, y in zip(dense_tests.histories(a, RAGGED), dense_tests.histories(b, RAGGED)))
    assert net["last_firing_time"].max() > 0 and net["st_last_firing_time"].max() > 0, "the network must have fired"
    a.close()
    b.close()


def c5_handle(snn, side):
    """BASELINE configs[4] at `side`, the state of bench.py's C5, without a graph"""
    m = side * side
    dn = snn.DeviceNetwork(model=snn.IZHIKEVICH, spike_train=snn.ST_POISSON)
    for k in range(4):
        dn.add_lattice(k, side, side)
        dn.add_spike_train_lattice(4 + k, side, side)
    dn.finalize(csr=True)
    for k in range(4):
        dn.set_attr(k, "gap_conductance", np.full(m, 10.0, np.float32))
        dn.set_attr(k, "current_voltage", synthetic.uniform(6, m, -65.0, 30.0, offset=k * m))
        dn.set_attr(4 + k, "chance_of_firing", np.full(m, 0.01, np.float32))
        dn.set_attr(4 + k, "seed", np.arange(k * m + 1, (k + 1) * m + 1, dtype=np.uint32))
    return dn


C5_PLAN = ([(k, k, ConnectionRule.euclidean(4, self_edges=False), None) for k in range(4)] +
           [(k, (k + 1) % 4, ConnectionRule.same_position(), None) for k in range(4)] +
           [(4 + k, k, ConnectionRule.same_position(), None) for k in range(4)])


@pytest.mark.parametrize("side", [9, 64])
def test_c5_by_twelve_rules(snn, side):
    a, b = c5_handle(snn, side), c5_handle(snn, side)
    want = synthetic.c5_csr(side)
    a.connect_sparse(C5_PLAN)
    b.set_graph_csr(*want)
    assert_csr(a, want, "against synthetic.c5_csr")
    for dn in (a, b):
        dn.run(20)
        assert dn.stat("steps_sparse_image") > 0, "the step image must be in use"
    assert a.stat("steps_sparse_image") == b.stat("steps_sparse_image")
    for k in range(4):
        for name, dtype in (("current_voltage", np.float32), ("last_firing_time", np.int32), ("is_spiking", np.uint32)):
            assert np.array_equal(a.get_attr(k, name, dtype).view(np.uint32), b.get_attr(k, name, dtype).view(np.uint32)), (k, name)
    a.close()
    b.close()


def test_edges_of_the_domain(snn):
    dn, w, c = patterned(snn, RAGGED)

    def after(*record):
        dn.connect_sparse([record])                                                    # (weight None: every edge weighs 1)
        dense_tests.apply_host(w, c, RAGGED, [record[:3] + (record[3] or WeightRule.constant(1.0),)])
        assert_csr(dn, csr_of(w, c, dn.owned), f"after {record[2]!r} on {record[0]} -> {record[1]}")

    assert c[15:50, 15:50].any()
    after(1, 1, ConnectionRule.all_to_all(probability=0.0, seed=3), None)              # probability <= 0 empties a block that had edges
    assert not c[15:50, 15:50].any()
    after(1, 1, ConnectionRule.all_to_all(probability=-1.0), None)
    after(0, 1, ConnectionRule.same_position(self_edges=False), None)                 # a == b and a != b: no edge
    assert not c[0:15, 15:50].any()
    after(1, 1, ConnectionRule.euclidean(6 * 6 + 4 * 4), WeightRule.constant(0.0))      # the window covers the grid; Some(0.0) is stored
    assert c[15:50, 15:50].all() and not w[15:50, 15:50].any()
    after(1, 1, ConnectionRule.euclidean(2 ** 32 - 1, self_edges=False), WeightRule.uniform(1.0, 2.0, seed=1))
    after(1, 0, ConnectionRule.chebyshev(2 ** 32 - 1), None)                           # post grid smaller than the pre grid, and the other way round
    after(0, 1, ConnectionRule.chebyshev(1), None)
    after(2, 1, ConnectionRule.euclidean(1), None)
    # a later record for the same pair wins
    first, last = (0, 0, ConnectionRule.all_to_all(), WeightRule.constant(4.0)), (0, 0, ConnectionRule.chebyshev(1, self_edges=False), WeightRule.constant(5.0))
    dn.connect_sparse([first, last])
    dense_tests.apply_host(w, c, RAGGED, [last])
    assert_csr(dn, csr_of(w, c, dn.owned), "after two records for one pair")
    # a call that leaves nothing: every block of the layout emptied
    nothing = ConnectionRule.all_to_all(probability=0.0)
    dn.connect_sparse([(pre, post, nothing, None) for pre in (0, 1, 2) for post in (0, 1)])
    rp, pi, ww = read(dn)
    assert dn._nnz == 0 and pi.size == 0 and ww.size == 0 and not rp.any() and rp.size == 51
    dn.run(3)
    dn.connect_sparse([(0, 1, ConnectionRule.same_position(), None)])                  # ... and from nothing again
    assert dn._nnz == 15
    dn.close()
    # a handle with no graph set connects from the empty graph
    fresh = dense_tests.handle(snn, RAGGED, csr=True)
    rp, pi = fresh.graph_csr_structure()
    assert rp.size == 51 and not rp.any() and pi.size == 0
    fresh.connect_sparse(dense_tests.PLAN)
    w0, c0 = np.zeros_like(w), np.zeros_like(c)
    dense_tests.apply_host(w0, c0, RAGGED, dense_tests.PLAN)
    assert_csr(fresh, csr_of(w0, c0, fresh.owned), "on a handle that held no graph")
    fresh.close()


@pytest.mark.parametrize("layout,plan,n_shards", [(WIDE, WIDE_PLAN, 2), (WIDE, WIDE_PLAN, 3), (RAGGED, RAGGED_PLAN, 2)],
                         ids=["wide-2", "wide-3", "ragged-2-one-empty"])
def test_contiguous_shards_write_the_rows_they_own(snn, layout, plan, n_shards):
    whole, w, c = patterned(snn, layout)
    whole.connect_sparse(plan)
    dense_tests.apply_host(w, c, layout, plan)
    assert_csr(whole, csr_of(w, c, whole.owned), "on the unsharded handle")
    owned = 0
    for k in range(n_shards):
        dn, _, _ = patterned(snn, layout, shard=(k, n_shards))
        dn.connect_sparse(plan)
        assert_csr(dn, csr_of(w, c, dn.owned), f"on shard {k} of {n_shards} (rows {dn.post_begin}..{dn.post_end})")
        owned += dn.owned.size
        twin = dense_tests.handle(snn, layout, shard=(k, n_shards), csr=True)
        twin.set_graph_csr(*csr_of(w, c, twin.owned))
        for peer in range(n_shards):
            assert np.array_equal(dn.halo_needs(peer), twin.halo_needs(peer)), (k, peer)
        dn.close()
        twin.close()
    assert owned == layout.n_neurons
    whole.close()


def raw_call(L, handle, records, n=None):
    arr = (_lib.ConnectRecord * max(len(records), 1))(*records)
    code = L.snn_connect_by_rules_csr(handle, arr if records or n is None else None, len(records) if n is None else n)
    return code, (L.snn_last_error() or b"").decode()


def record(**change):
    f = dict(pre_id=0, post_id=1, rule=cases.CHEBYSHEV, extent=1, self_edges=1, probability=1.0, edge_seed=0, weight_rule=cases.UNIFORM,
             w_lo=0.5, w_hi=1.5, weight_seed=0)
    f.update(change)
    return _lib.ConnectRecord(**f)


def test_refusals_are_all_or_nothing(snn):
    net = firing_oracle(RAGGED, chemical=False)
    dense_tests.twin_graph(net, dense_tests.PLAN)
    dn, control = parity.device_from_oracle(snn, net, csr=True), parity.device_from_oracle(snn, net, csr=True)
    L = dn._L
    before = read(dn)

    def unchanged(what):
        assert_csr(dn, before, what)

    assert raw_call(L, None, [record()])[0] == BAD_ARG
    code, msg = raw_call(L, dn._h, [], n=0)
    assert code == 0
    unchanged("after an empty call")
    code = L.snn_connect_by_rules_csr(dn._h, None, 0)
    assert code == 0
    code = L.snn_connect_by_rules_csr(dn._h, None, 2)
    assert code == BAD_ARG and "records" in L.snn_last_error().decode()
    unchanged("after null records")
    bad = [(dict(pre_id=9), "pre_id"), (dict(post_id=9), "post_id"), (dict(post_id=2), "post_id"), (dict(rule=4), "rule"),
           (dict(weight_rule=2), "weight_rule"), (dict(w_lo=float("nan")), "w_lo"), (dict(w_lo=float("inf")), "w_lo"),
           (dict(w_hi=float("-inf")), "w_hi"), (dict(w_hi=float("nan")), "w_hi"), (dict(probability=float("nan")), "probability"),
           (dict(w_lo=-3e38, w_hi=3e38), "w_hi - w_lo")]
    for change, name in bad:
        code, msg = raw_call(L, dn._h, [record(**change)])
        assert code == BAD_ARG and name in msg and "record 0" in msg, (change, code, msg)
        unchanged(f"after a record with a bad {name}")
    assert "spike-train" in raw_call(L, dn._h, [record(post_id=2)])[1]
    # a batch whose third record is invalid: the two valid ones before it change nothing either
    code, msg = raw_call(L, dn._h, [record(), record(pre_id=1, post_id=0), record(rule=7), record()])
    assert code == BAD_ARG and "record 2" in msg and "rule" in msg, msg
    unchanged("after a batch whose third record is invalid")
    with pytest.raises(TypeError):
        dn.connect_sparse([(0, 1, "all", None)])
    unchanged("after a plan that is not made of rules")
    for h in (dn, control):
        h.run(10)
    sa, sb = parity.pull_state(dn, net), parity.pull_state(control, net)
    for name in sa:
        assert np.array_equal(parity.bits(sa[name]), parity.bits(sb[name])), name
    # the accepted call, for contrast, does change it
    assert raw_call(L, dn._h, [record()])[0] == 0
    assert not np.array_equal(dn.graph_csr_structure()[1], before[1])
    dn.close()
    control.close()

    dense = dense_tests.handle(snn, RAGGED)
    code, msg = raw_call(L, dense._h, [record()])
    assert code == BAD_STATE and "with snn_connect_by_rule" in msg, msg
    with pytest.raises(snn.SnnError) as e:
        dense.connect_sparse([(0, 1, ConnectionRule.all_to_all(), None)])
    assert e.value.code == BAD_STATE
    nnz = C.c_uint64(7)
    assert L.snn_graph_csr_nnz(dense._h, C.byref(nnz)) == BAD_STATE
    dense.close()

    raw = dense_tests.handle(snn, RAGGED, csr=True, finalize=False)
    raw._check(L.snn_network_use_csr(raw._h, 1))
    code, msg = raw_call(L, raw._h, [record()])
    assert code == BAD_STATE and "finalized" in msg
    raw.close()

    slab = dense_tests.handle(snn, RAGGED, finalize=False)
    slab.finalize(0, 2, csr=True, by_lattice=True)
    w, c = dense_tests.pattern(RAGGED)
    slab.set_graph_csr(*csr_of(w, c, slab.owned))
    code, msg = raw_call(L, slab._h, [record()])
    assert code == BAD_STATE and "not covered" in msg and "by lattice" in msg
    assert_csr(slab, csr_of(w, c, slab.owned), "on the by-lattice shard after the refusal")      # (the getters do cover it)
    slab.close()


def test_structure_getter_checks_the_count(snn):
    dn, w, c = patterned(snn, RAGGED)
    L = dn._L
    nnz = C.c_uint64()
    assert L.snn_graph_csr_nnz(dn._h, C.byref(nnz)) == 0 and nnz.value == int(c[:, :].sum()) == dn._nnz
    rp, pi = np.zeros(51, np.uint64), np.zeros(nnz.value + 1, np.uint32)
    assert L.snn_get_graph_csr_structure(dn._h, rp.ctypes.data_as(_lib.u64p), pi.ctypes.data_as(_lib.u32p), nnz.value + 1) == DIM_MISMATCH
    assert L.snn_get_graph_csr_structure(dn._h, rp.ctypes.data_as(_lib.u64p), pi.ctypes.data_as(_lib.u32p), nnz.value - 1) == DIM_MISMATCH
    assert L.snn_get_graph_csr_structure(dn._h, None, pi.ctypes.data_as(_lib.u32p), nnz.value) == BAD_ARG
    assert L.snn_graph_csr_nnz(dn._h, None) == BAD_ARG
    dn.close()


def test_the_edge_total_is_counted_in_64_bits(snn):
    """256x256 neurons connected all-to-all are 2^32 stored edges: the counting pass alone runs (65 536 rows x 1 024 rounds, no
    weight, no draw), the total does not fit 32 bits, and the call is refused before anything of that size is allocated"""
    lay = parity.Layout([(0, 256, 256), (1, 2, 2)])
    dn = dense_tests.handle(snn, lay, csr=True)
    dn.connect_sparse([(1, 0, ConnectionRule.same_position(), None)])
    before = read(dn)
    assert before[1].size == 4
    with pytest.raises(snn.SnnError) as e:
        dn.connect_sparse([(1, 1, ConnectionRule.all_to_all(), None), (0, 0, ConnectionRule.all_to_all(), None)])
    assert e.value.code == DIM_MISMATCH and "record 1" in str(e.value) and str(2 ** 32 + 20) in str(e.value), str(e.value)
    assert_csr(dn, before, "after the refused call")
    dn.close()


def test_reward_modulated_handle_restarts_traces_dw_and_counters(snn):
    dn, w, c = patterned(snn, RAGGED)
    dn.set_reward_modulator(1, do_modulation=True)
    dn.set_connection_kind(0, 1, 1)
    n0 = dn._nnz
    t = (np.float32(1.0) + np.arange(n0, dtype=np.float32) / np.float32(4096.0)).astype(np.float32)
    dn.set_traces_csr(t)
    dn.set_pending_csr(-t)
    dn.set_counters_csr(np.ones(n0, np.uint8))
    assert np.array_equal(dn.get_traces_csr(), t) and dn.get_counters_csr().all()
    edit = (0, 1, ConnectionRule.chebyshev(1), WeightRule.constant(1.0))
    dn.connect_sparse([edit])
    dense_tests.apply_host(w, c, RAGGED, [edit])
    want = csr_of(w, c, dn.owned)
    assert_csr(dn, want)
    assert dn._nnz == want[1].size != n0
    for got in (dn.get_traces_csr(), dn.get_pending_csr(), dn.get_counters_csr()):
        assert got.size == dn._nnz and not got.any()
    dn.close()
