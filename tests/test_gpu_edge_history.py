"""GPU parity for the edge-weight history (snn_set_edge_history / snn_get_edge_history): the weights of a caller-chosen list of
(pre, post) pairs per recorded step, on dense and sparse handles.  Bit-exact against the oracle stepped one step at a time, its
`weights` / `connections` read after (order 1) or before (order 2) each step -- the scheme of
test_gpu_reduced_history.py::test_graph_history.  One small network throughout: lattices 9 x 10 and 17 x 17 plus a 2 x 3 Rate
spike-train lattice (379 neurons: two SELL-64 slices of lattice 0 with a ragged second, more than one 256-row chunk, cells as pre)."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import parity

pytestmark = pytest.mark.gpu

MAIN = ([(0, 9, 10), (3, 17, 17)], [(5, 2, 3)])
SMALL = ([(0, 6, 7), (3, 5, 5)], [])           # eligible for the one-launch step and the one-launch run
# With the voltages, rates and weights of test_gpu_reduced_history.build this network is slow to fire (most seeds: no spike within
# the 250 steps of test 1).  Seed 157 is the first of 1 .. 400 whose large AND small network both spike more than ten times in them,
# from step 235 on, so that weights of both orders move inside the record; it stays fixed.
SEED = 157
DIM_MISMATCH, BAD_ARG, BAD_STATE = 10, 11, 12   # snn_status of include/snn_amd.h


def build(shape=MAIN, seed=SEED, reward=False):
    """as test_gpu_reduced_history.build: fill_graph, 40 % of the connections cleared, plasticity on"""
    lattices, st = shape
    lay = parity.Layout(lattices, st)
    net = parity.make_oracle(lay, st_kind=ob.ST_RATE if st else ob.ST_NONE)
    net["current_voltage"] = ob.uniform_array(seed, net.n_neurons, -65.0, 30.0)
    net["gap_conductance"] = 10.0
    if st:
        net["st_rate"] = ob.uniform_array(seed + 3, net.n_cells, 1.0, 5.0)
    net.fill_graph(seed + 1, 0.5, 1.5)
    rng = np.random.default_rng(seed)
    net["connections"][rng.random(net["connections"].shape) < 0.4] = 0
    if reward:                                  # rm_* as in test_graph_history
        net["rm_do_modulation"][0] = 1
        net["rm_tau_c"][0] = 0.05
        net["rm_a_plus"][0] = 0.01
        net["rm_a_minus"][0] = 0.01
        net["rm_dopamine"][0] = 0.02
    else:
        net["do_plasticity"] = 1
    return net


def mixed_list(net, seed=SEED):
    """The list of test 1, as (pre, post, when, parts): all cell -> lattice-0 edges and 50 random lattice-3 -> lattice-0 edges
    with when = 1, all internal edges of lattice 0 with when = 2, 20 absent pairs (alternating orders), three pairs listed twice.
    `parts` names the column ranges."""
    rng = np.random.default_rng(seed + 100)
    conn = net["connections"]
    nn = net.n_neurons
    r = net.layout.ranges()
    f0, c0, _ = r[0]
    f3, c3, _ = r[3]
    pre, post, when, parts = [], [], [], {}

    def add(name, p, q, w):
        at = sum(x.size for x in pre)
        pre.append(np.asarray(p, np.int64))
        post.append(np.asarray(q, np.int64))
        when.append(np.broadcast_to(np.asarray(w, np.uint8), pre[-1].shape).copy())
        parts[name] = slice(at, at + pre[-1].size)

    i, j = np.nonzero(conn[nn:, f0:f0 + c0])
    add("cells", i + nn, j + f0, 1)
    i, j = np.nonzero(conn[f3:f3 + c3, f0:f0 + c0])
    pick = rng.choice(i.size, 50, replace=False)
    add("cross", i[pick] + f3, j[pick] + f0, 1)
    i, j = np.nonzero(conn[f0:f0 + c0, f0:f0 + c0])
    add("internal", i + f0, j + f0, 2)
    i, j = np.nonzero(conn[:, :] == 0)
    pick = rng.choice(i.size, 20, replace=False)
    add("absent", i[pick], j[pick], np.arange(20) % 2 + 1)
    add("twice", pre[1][:3], post[1][:3], 1)
    return np.concatenate(pre), np.concatenate(post), np.concatenate(when), parts


def sample(net, pre, post):
    on = net["connections"][pre, post] != 0
    return np.where(on, net["weights"][pre, post], np.float32(0)).astype(np.float32), on


def oracle_record(net, pre, post, when, runs, every, between=None):
    """Steps the oracle one step at a time through `runs` (step counts); `between(k)` is called after run k.  Returns
    (weights [rows, n], connected [rows, n], voltages of lattice 0 [rows, count]) of the recorded steps: every `every`-th."""
    ws, cs, vs, t = [], [], [], 0
    first, count, _ = net.layout.ranges()[0]
    for k, steps in enumerate(runs):
        for _ in range(steps):
            rec = t % every == 0
            if rec:
                w2, c2 = sample(net, pre, post)
            net.run(1)
            if rec:
                w1, c1 = sample(net, pre, post)
                ws.append(np.where(when == 2, w2, w1))
                cs.append(np.where(when == 2, c2, c1))
                vs.append(net["current_voltage"][first:first + count].copy())
            t += 1
        if between is not None and k + 1 < len(runs):
            between(k)
    return np.array(ws), np.array(cs), np.array(vs)


RUNS, EVERY = (100, 1, 149), 3


@functools.lru_cache(maxsize=None)
def reference(shape_key, reward=False):
    """the oracle's record of the mixed list (test 1's runs and stride), computed once per network"""
    shape = MAIN if shape_key == "main" else SMALL
    net = build(shape, reward=reward)
    pre, post, when, parts = mixed_list(net)
    if reward:
        when = np.ones_like(when)
    w, c, v = oracle_record(net, pre, post, when, RUNS, EVERY)
    for a in (w, c, v):
        a.setflags(write=False)
    return pre, post, when, parts, w, c, v, net


def run_device(snn, shape, csr, pre, post, when, runs=RUNS, every=EVERY, prepare=None, reward=False):
    net = build(shape, reward=reward)
    dn = parity.device_from_oracle(snn, net, csr=csr)
    if reward:
        dn.set_reward_modulator(0, dopamine=0.02, tau_c=0.05, a_plus=0.01, a_minus=0.01)
    if prepare is not None:
        prepare(dn)
    dn.set_history(voltage=True, spikes=False)
    dn.set_history_stride(every)
    dn.set_edge_history(pre, post, when)
    for steps in runs:
        dn.run(steps)
    return dn


def assert_record(dn, w, c):
    got_w, got_c = dn.edge_history()
    assert dn.history_steps() == w.shape[0] and got_w.shape == w.shape and got_c.shape == c.shape
    print("edge history: rows", w.shape[0], "pairs", w.shape[1], "weight mismatches", int((parity.bits(got_w) != parity.bits(w)).sum()),
          "flag mismatches", int((got_c != c).sum()))
    assert np.array_equal(got_c, c), "connected flags differ from the oracle"
    assert np.array_equal(parity.bits(got_w), parity.bits(w)), "recorded weights differ from the oracle"


@pytest.mark.parametrize("csr", [False, True])
def test_mixed_list(snn, csr):
    """Orders 1 and 2 in one list, cells as pre, absent pairs, pairs listed twice, stride 3 over runs of 100 + 1 + 149 steps; the
    row axis is the voltage history's."""
    pre, post, when, parts, w, c, v, _ = reference("main")
    # the input, against the oracle alone: weights must have moved, and some pair is absent throughout
    internal, absent = parts["internal"], parts["absent"]
    cross = slice(parts["cells"].start, parts["cross"].stop)      # order 1, across lattices: cells -> lattice 0, lattice 3 -> lattice 0
    assert np.all(when[cross] == 1) and np.all(when[internal] == 2)
    assert np.any(parity.bits(w[0, cross]) != parity.bits(w[-1, cross])), "no order-1 cross-lattice weight moved"
    assert np.any(parity.bits(w[0, internal]) != parity.bits(w[-1, internal])), "no order-2 weight moved"
    assert np.any(~c[:, absent].any(axis=0)) and np.all(w[:, absent][:, ~c[:, absent].any(axis=0)] == 0)
    assert c[:, parts["cells"]].all() and parts["cells"].stop > 0
    dn = run_device(snn, MAIN, csr, pre, post, when)
    assert dn.history_steps() == len(range(0, sum(RUNS), EVERY))
    assert_record(dn, w, c)
    assert np.array_equal(parity.bits(dn.voltage_history(0)), parity.bits(v))
    dn.close()


@pytest.mark.parametrize("form", ["small-dense", "small-sparse", "defer_stdp"])
def test_every_step_form(snn, form):
    """The list on a 6 x 7 + 5 x 5 electrical network (the one-launch step; the one-launch run while no list is installed) and on
    a dense handle with the option defer_stdp SET: the oracle's record, and the neuron state the run leaves is the oracle's too.
    At 379 neurons the matrix is not streamed, so stdp_deferral_applies() is false and nothing is deferred with or without a
    list: the case shows that the option does no harm.  The flush of a pending update by set_edge_history, and deferral standing
    back while a list is installed, are tested where deferral applies: test_gpu_streamed_walk.py::test_plastic_walk."""
    key, shape = ("main", MAIN) if form == "defer_stdp" else ("small", SMALL)
    pre, post, when, parts, w, c, v, net = reference(key)
    dn = run_device(snn, shape, form == "small-sparse", pre, post, when,
                    prepare=(lambda d: d.set_option("defer_stdp", 1)) if form == "defer_stdp" else None)
    assert_record(dn, w, c)
    assert dn.stat("persistent_run_launches") == 0          # every step passes step_end's two snapshot points
    if form == "small-dense":
        assert dn.stat("steps_dense_one_launch") > 0         # (the one-launch step is what records here)
    parity.assert_state_equal(net, parity.pull_state(dn, net))
    parity.assert_graph_equal(net, dn)
    dn.close()


@pytest.mark.parametrize("csr", [False, True])
def test_edits_during_the_record(snn, csr):
    """Between two runs: two recorded pairs reweighted with graph_edit; one recorded edge removed and one recorded absent pair
    connected (on the sparse handle with structure=True: a commit, after which every pair finds its entry again).  The rows before
    and after are the oracle's with the same edits applied to its matrices; the other columns go on undisturbed."""
    net = build()
    pre, post, when, parts = mixed_list(net)
    cells, internal, absent = parts["cells"], parts["internal"], parts["absent"]
    reweigh = [cells.start, parts["cross"].start + 5]
    gone, fresh = internal.start + 7, absent.start + 2
    runs = (240, 20)                            # (the network fires from step 235 on: the edited weights move after the edit)

    def edit_oracle(_):
        for k, value in zip(reweigh, (0.25, 1.75)):
            net["weights"][pre[k], post[k]] = value
        net["connections"][pre[gone], post[gone]] = 0
        net["connections"][pre[fresh], post[fresh]] = 1
        net["weights"][pre[fresh], post[fresh]] = 0.75

    assert net["connections"][pre[gone], post[gone]] != 0 and net["connections"][pre[fresh], post[fresh]] == 0
    w, c, _ = oracle_record(net, pre, post, when, runs, 1, between=edit_oracle)
    assert c[:240, gone].all() and not c[240:, gone].any() and not c[:240, fresh].any() and c[240:, fresh].all()
    assert np.any(parity.bits(w[240]) != parity.bits(w[-1])), "weights must have moved after the edit"
    dev = build()
    dn = parity.device_from_oracle(snn, dev, csr=csr)
    dn.set_edge_history(pre, post, when)
    dn.run(runs[0])
    dn.graph_edit(pre[reweigh], post[reweigh], [0.25, 1.75])
    dn.graph_edit([pre[gone], pre[fresh]], [post[gone], post[fresh]], [0.0, 0.75], connected=[0, 1], structure=True)
    dn.run(runs[1])
    assert_record(dn, w, c)
    dn.close()


@pytest.mark.parametrize("csr", [False, True])
def test_reward_modulated_lattice(snn, csr):
    """lattice 0 reward-modulated (its weight update then a standalone pass), every pair recorded after the step's updates"""
    pre, post, when, parts, w, c, _, _ = reference("main", reward=True)
    assert np.any(parity.bits(w[0, parts["internal"]]) != parity.bits(w[-1, parts["internal"]])), "weights must have moved"
    dn = run_device(snn, MAIN, csr, pre, post, when, reward=True)
    assert_record(dn, w, c)
    dn.close()


@pytest.mark.parametrize("csr", [False, True])
def test_contract(snn, csr):
    net = build()
    pre, post, when, _ = mixed_list(net)
    dn = parity.device_from_oracle(snn, net, csr=csr)
    n_tot, nn = dn.n_tot, dn.n_neurons
    with pytest.raises(snn.SnnError) as e:
        dn.edge_history()                                   # no list installed
    assert e.value.code == BAD_STATE
    dn.set_edge_history(pre, post, when)
    assert dn.edge_history_count() == pre.size
    dn.run(7)
    before = dn.edge_history()
    # refused calls name the pair's position and leave the list and its record as they were
    for bad_pre, bad_post, bad_when, k, words in ((pre[:4], post[:4], [1, 2, 3, 1], 2, "when is 3"),
                                                  (np.r_[pre[:3], n_tot], np.r_[post[:3], 0], 1, 3, "pre is not below n_tot"),
                                                  (np.r_[pre[:1], 0], np.r_[post[:1], nn], 2, 1, "post is not below n_neurons")):
        with pytest.raises(snn.SnnError) as e:
            dn.set_edge_history(bad_pre, bad_post, bad_when)
        assert e.value.code == BAD_ARG and f"pair {k} (pre " in str(e.value) and words in str(e.value), str(e.value)
    assert dn.history_steps() == 7 and dn.edge_history_count() == pre.size
    after = dn.edge_history()
    assert np.array_equal(parity.bits(before[0]), parity.bits(after[0])) and np.array_equal(before[1], after[1])
    # a wrong step count
    w = np.zeros((8, pre.size), np.float32)
    code = dn._L.snn_get_edge_history(dn._h, w.ctypes.data_as(snn._lib.f32p), None, 8)
    assert code == DIM_MISMATCH and b"mismatch" in dn._L.snn_last_error()
    # reset_history zeroes the step count, the list stays
    dn.reset_history()
    assert dn.history_steps() == 0 and dn.edge_history()[0].shape == (0, pre.size)
    dn.run(5)
    assert dn.history_steps() == 5
    # replacing the list restarts the record
    dn.set_edge_history(pre[:10], post[:10], 1)
    assert dn.history_steps() == 0 and dn.edge_history_count() == 10
    dn.run(2)
    assert dn.edge_history()[0].shape == (2, 10)
    # n = 0 switches off
    dn.set_edge_history([], [])
    assert dn.edge_history_count() == 0 and dn.history_steps() == 0
    with pytest.raises(snn.SnnError):
        dn.edge_history()
    dn.run(3)                                               # nothing is recorded any more
    assert dn.history_steps() == 0
    dn.close()
    # shard handles of any kind are refused, and the message says so
    shard = parity.device_from_oracle(snn, build(), shard=(0, 2), csr=csr)
    with pytest.raises(snn.SnnError) as e:
        shard.set_edge_history(pre[:4], np.minimum(post[:4], shard.post_end - 1), 1)
    assert e.value.code == BAD_STATE and "shard" in str(e.value), str(e.value)
    shard.close()


def test_sparse_handle_without_a_graph_records_absent_until_one_is_set(snn):
    """No graph yet: every pair reads absent.  snn_set_graph_csr commits a structure, every pair finds its entry, and the record
    goes on (static weights: the rows after the commit are the graph's own values)."""
    net = build()
    net["do_plasticity"] = 0
    pre, post, when, parts = mixed_list(net)
    dn = snn.DeviceNetwork(model=net.model, spike_train=net.st_kind)
    for i, r, c in net.layout.lattices:
        dn.add_lattice(i, r, c)
    for i, r, c in net.layout.st_lattices:
        dn.add_spike_train_lattice(i, r, c)
    dn.finalize(csr=True)
    parity.push_state(dn, net)
    dn.set_synapses(True, False)
    dn.set_edge_history(pre, post, when)
    dn.run(3)
    w, c = dn.edge_history()
    assert w.shape == (3, pre.size) and not c.any() and not w.any()
    dn.set_graph_csr(*parity.csr_for_posts(net, dn.owned))
    dn.run(2)
    w, c = dn.edge_history()
    want_w, want_c = sample(net, pre, post)
    assert dn.history_steps() == 5 and not c[:3].any() and not w[:3].any()
    for t in (3, 4):
        assert np.array_equal(c[t], want_c) and np.array_equal(parity.bits(w[t]), parity.bits(want_w))
    assert want_c.sum() > 5000 and (~want_c).sum() >= 20
    dn.close()
