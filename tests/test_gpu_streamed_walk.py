"""Two scripted walks at the smallest STREAMED size (the network of test_gpu_dense_w24.py: 1 x 4099 Izhikevich neurons plus 2 x 3
spike-train cells, 65 MiB of dense matrix, gap junctions, present weights U[0.5, 1.5)), ONE handle per walk: what small sequences
cannot reach -- the 24-bit image of W under every writer of weights, STDP riding on the input pass, the flush of a deferred update
before a graph call or a change of step form.

A STATION is one write on both sides, 4 steps on both sides, assert_state_equal and a check of the pass the handle reads:
input_kernel_bytes() == 3 * n_tot * n_neurons (the image) exactly when, by the oracle and the flags alone, electrical synapses
are on and chemical off, no lattice is plastic, there is no modulator, connection kind or weight record, and the unsigned span of
the bit patterns of the oracle's present weights is <= 0xFFFFFE (or no edge is present); otherwise != 3 * n.  For every WRITING
station the oracle alone first shows that the write matters: a clone stepped without it ends with other voltage bits, so a stale
image cannot pass.  Each walk is first taken on the oracle alone (`device=False`): the expected list and the conditions on it are
asserted before a handle exists.  The static walk is two tests, stations 1 - 9 and 10 - 14, each on a handle of its own, so that
no case runs longer than a few seconds.  The conditions count the stations of both halves: the plan test (no GPU) asserts them
on the oracle alone, each GPU test takes its own half on the oracle first -- every sensitivity check -- and holds the device walk
to that list.

The reference of the connect_by_rule stations is the package's own host twin of the two records, snn_amd.network.rule_pairs --
independent of the device kernel, not of the package: the plain-loop restatements of connect_spec_cases.py would take minutes
at 4099 x 4099 pairs.  What makes that sound is tests/test_connect_spec_host.py, which holds rule_pairs to the plain loops."""
import functools
import os

import numpy as np
import pytest

import checkpoint
import parity
from test_gpu_dense_w24 import CELLS, ROW, static_net
from test_gpu_sequences import _Absent

STEPS = 4
F = np.float32


def span_ok(net):
    present = net["connections"] != 0
    if not present.any():
        return True
    b = net["weights"].view(np.uint32)
    return int(np.where(present, b, np.uint32(0)).max()) - int(np.where(present, b, np.uint32(0xFFFFFFFF)).min()) <= 0xFFFFFE


def weights_move(net):
    return bool(net["do_plasticity"].any() or net["rm_do_modulation"].any() or net["conn_kind"].any())


def image_expected(net, record, span):
    return bool(net.electrical and not net.chemical and not weights_move(net) and not record and span)


def handle(snn, net):
    old = os.environ.get("SNN_AMD_W24")
    os.environ["SNN_AMD_W24"] = "1"
    try:
        return parity.device_from_oracle(snn, net)
    finally:
        if old is None:
            del os.environ["SNN_AMD_W24"]
        else:
            os.environ["SNN_AMD_W24"] = old


class Walk:
    """one handle (or none: device=False) and its oracle through the stations; `visited` is the expected list"""

    def __init__(self, snn, net, device):
        self.snn, self.net, self.device = snn, net, device
        self.dn = handle(snn, net) if device else _Absent()
        self.n = net.n_tot * net.n_neurons
        self.record = False                 # a weight record (edge list, graph history) is installed
        self.live = None                    # the image is expected live, after the last station
        self.span = None                    # span_ok of the oracle's weights (taken again after whatever may have moved a weight)
        self.visited = []                   # (name, writing, entered live, left live, sensitive)

    def run(self, steps=STEPS):
        self.dn.run(steps)
        self.net.run(steps)

    def compare(self, name):
        if not self.device:
            return
        try:
            parity.assert_state_equal(self.net, parity.pull_state(self.dn, self.net))
        except AssertionError as e:
            raise AssertionError(f"station {name}: {e}") from e
        got = self.dn.input_kernel_bytes()
        assert (got == 3 * self.n) == self.live, f"station {name}: input pass reads {got} bytes, 3 n = {3 * self.n}, image expected: {self.live}"

    def station(self, name, write, writing=True, run=None, ghost=None):
        """`write(dn, net)` on both sides, then the steps (`run(walk)`, by default 4 of them); `ghost()`: the oracle WITHOUT the
        write, by default a clone of the oracle as it stands"""
        entered, sensitive, moving = self.live, None, weights_move(self.net)
        ghost = (ghost() if ghost else checkpoint.clone(self.net)) if writing else None
        write(self.dn, self.net)
        (run or Walk.run)(self)
        if writing:
            ghost.run(STEPS)
            sensitive = not np.array_equal(parity.bits(ghost["current_voltage"]), parity.bits(self.net["current_voltage"]))
            assert sensitive, f"station {name}: the write does not change the voltages of the {STEPS} steps after it"
        if writing or moving or self.span is None:
            self.span = span_ok(self.net)
        self.live = image_expected(self.net, self.record, self.span)
        self.visited.append((name, writing, entered, self.live, sensitive))
        self.compare(name)


def edges(net, rng, count, present=True, rows=None):
    """`count` random pairs that are stored edges (present) or absent pairs; `rows`: among these presynaptic rows only"""
    conn = net["connections"] if rows is None else net["connections"][rows]
    p, q = np.nonzero((conn != 0) == present)
    pick = rng.choice(p.size, count, replace=False)
    return (p[pick] if rows is None else np.asarray(rows)[p[pick]]), q[pick]


def edit(pre, post, w, on=None):
    on = np.ones(len(pre), np.uint8) if on is None else np.asarray(on, np.uint8)
    w = np.asarray(w, np.float32)

    def write(dn, net):
        net["connections"][pre, post] = on
        net["weights"][pre, post] = np.where(on != 0, w, F(0))
        dn.graph_edit(pre, post, w, connected=on)
    return write


_blocks = {}


def connect(pre_id, post_id, rule, weight):
    """connect_by_rule on both sides; the oracle's block from the host twins of the two records (network.rule_pairs, which
    test_connect_spec_host.py holds to the plain loops -- those would take minutes at 4099 x 4099 pairs), computed once"""
    def write(dn, net):
        from snn_amd.network import rule_pairs
        shapes = {i: (r, c) for i, r, c in net.layout.lattices + net.layout.st_lattices}
        ranges = net.layout.ranges()
        p0 = ranges[pre_id][0] + (net.n_neurons if ranges[pre_id][2] else 0)
        q0 = ranges[post_id][0]
        key = (pre_id, post_id, repr(rule), repr(weight), None if weight.table is None else weight.table.tobytes())
        if key not in _blocks:
            _blocks[key] = rule_pairs(rule, weight, shapes[pre_id], shapes[post_id])
        on, w = _blocks[key]
        net["connections"][p0:p0 + on.shape[0], q0:q0 + on.shape[1]] = on
        net["weights"][p0:p0 + on.shape[0], q0:q0 + on.shape[1]] = w
        dn.connect_by_rule(pre_id, post_id, rule, weight)
    return write


def restore_oracle(net, snap):
    for name, a in snap.arr.items():
        net.arr[name][...] = a
    net.clock = snap.clock


def pair_list(net, rng, stored, absent, cells):
    sp, sq = edges(net, rng, stored)
    ap, aq = edges(net, rng, absent, present=False)
    cp, cq = rng.integers(net.n_neurons, net.n_tot, cells), rng.integers(0, net.n_neurons, cells)
    pre, post = np.r_[sp, ap, cp, sp[:1]], np.r_[sq, aq, cq, sq[:1]]
    return pre, post, rng.integers(1, 3, pre.size).astype(np.uint8)


def oracle_rows(net, pre, post, when, steps):
    """the oracle stepped one step at a time: the record of (pre, post, when) at stride 1"""
    from sequence_graph_ops import sample_pairs
    ws, cs = [], []
    for _ in range(steps):
        w2, c2 = sample_pairs(net, pre, post)
        net.run(1)
        w1, c1 = sample_pairs(net, pre, post)
        ws.append(np.where(when == 2, w2, w1))
        cs.append(np.where(when == 2, c2, c1))
    return np.array(ws), np.array(cs)


def assert_record(walk, name, want):
    if walk.device:
        got_w, got_c = walk.dn.edge_history()
        assert np.array_equal(got_c, want[1]) and np.array_equal(parity.bits(got_w), parity.bits(want[0])), f"station {name}: the edge record differs from the oracle's"


# ---- the static walk -----------------------------------------------------------------------------------------------------------
def static_walk_writers(snn, device):
    """stations 1 - 9: every call that writes weights, the image live on entry"""
    import snn_amd
    net = static_net(ROW, CELLS, 21)
    net.n_threads = 8
    nn, n_tot = net.n_neurons, net.n_tot
    rng = np.random.default_rng(2100)
    walk = Walk(snn, net, device)
    dn = walk.dn
    uniform = lambda k: rng.uniform(0.5, 1.5, k).astype(np.float32)          # noqa: E731 (inside the span of the present weights)
    walk.station("1 baseline", lambda dn, net: None, writing=False)
    assert walk.live
    sp, sq = edges(net, rng, 70)
    ap, aq = edges(net, rng, 20, present=False)
    walk.station("2 graph_edit inside the span", edit(np.r_[sp, ap], np.r_[sq, aq], uniform(90), np.r_[np.ones(50), np.zeros(20), np.ones(20)]))
    p, q = edges(net, rng, 1)
    old = net["weights"][p, q].copy()
    walk.station("3 one weight 4.0", edit(p, q, [4.0]))
    walk.station("4 the same edge back", edit(p, q, old))
    walk.station("5 connect_by_rule inside lattice 0", connect(0, 0, snn_amd.ConnectionRule.chebyshev(300, self_edges=False),
                                                                snn_amd.WeightRule.uniform(0.5, 1.5, seed=77)))
    table = rng.uniform(0.5, 1.5, snn_amd.WeightRule.table_shape(CELLS[0][1:], ROW[0][1:])).astype(np.float32)
    table[rng.random(table.shape) < 0.2] = np.nan
    walk.station("6 connect_by_rule cells -> lattice 0", connect(3, 0, snn_amd.ConnectionRule.all_to_all(), snn_amd.WeightRule.displacement(table)))

    def synthetic(dn, net):
        net.fill_graph(4242, 0.5, 1.5)
        dn.fill_graph_synthetic(4242, 0.5, 1.5)
    walk.station("7 fill_graph_synthetic", synthetic)

    def dense(dn, net):
        c = rng.random((n_tot, n_tot), dtype=np.float32) < 0.75
        w = (rng.random((n_tot, n_tot), dtype=np.float32) + F(1.0)) * c     # U[1, 2): the base moves
        net["connections"][...] = c[:, :nn]
        net["weights"][...] = w[:, :nn]
        dn.set_graph_dense(w, c.astype(np.uint32))
    walk.station("8 set_graph_dense", dense)

    # 9: a checkpoint, a weight edit and a run; the restore, and the run again without the edit
    sp, sq = edges(net, rng, 50)
    snap = []

    def checkpoint_and_edit(dn, net):
        dn.checkpoint()
        snap.append(checkpoint.clone(net))
        edit(sp, sq, rng.uniform(1.0, 2.0, 50))(dn, net)
    walk.station("9a checkpoint, weight edit", checkpoint_and_edit)

    def restore(dn, net):
        dn.restore_checkpoint()
        restore_oracle(net, snap.pop())

    def restored_but_edited():
        """what a restore that left the edited weights behind (a stale image) would step on"""
        ghost = checkpoint.clone(snap[0])
        ghost["weights"][sp, sq] = net["weights"][sp, sq]
        return ghost
    walk.station("9b restore_checkpoint", restore, ghost=restored_but_edited)
    assert walk.live
    dn.close()
    return walk.visited


def static_walk_forms(snn, device):
    """stations 10 - 14: what changes the step form around the image, and last the reward modulator"""
    net = static_net(ROW, CELLS, 23)
    net.n_threads = 8
    n_tot = net.n_tot
    rng = np.random.default_rng(2300)
    walk = Walk(snn, net, device)
    dn = walk.dn
    walk.station("baseline", lambda dn, net: None, writing=False)
    assert walk.live

    # 10: an edge list (static weights: every row is the graph's own values), then removed
    pre, post, when = pair_list(net, rng, 150, 40, 9)
    want = []

    def install(dn, net):
        dn.set_edge_history(pre, post, when)
        walk.record = True

    def recorded_run(walk):
        walk.dn.run(STEPS)
        want.append(oracle_rows(walk.net, pre, post, when, STEPS))
    walk.station("10a set_edge_history", install, writing=False, run=recorded_run)
    assert pre.size == 200 and not walk.live
    assert_record(walk, "10a", want[0])

    def remove(dn, net):
        dn.set_edge_history([], [])
        walk.record = False
    walk.station("10b edge list removed", remove, writing=False)
    assert walk.live

    def history(value):
        def write(dn, net):
            dn.set_graph_history(0, value)
            walk.record = bool(value)
        return write
    walk.station("11a set_graph_history(0, 1)", history(1), writing=False)
    walk.station("11b graph history off", history(0), writing=False)

    def synapses(el, ch):
        def write(dn, net):
            dn.set_synapses(el, ch)
            net.electrical, net.chemical = el, ch
        return write
    walk.station("12a set_synapses(True, True)", synapses(True, True))
    walk.station("12b set_synapses(True, False)", synapses(True, False))
    for shape in (1, 2):
        walk.station(f"13 input_shape {shape}", lambda dn, net, shape=shape: dn.set_option("input_shape", shape), writing=False)
        assert walk.live

    # 14, last: a reward modulator on lattice 0 and two run_with_reward steps (rm_* as in test_gpu_edge_history.build)
    net["current_voltage"][::89] = F(35.0)                  # spikes in the two steps: traces, and weights that move
    dn.set_attr(0, "current_voltage", net["current_voltage"])

    def modulator(dn, net):
        net["rm_do_modulation"][0] = 1
        net["rm_tau_c"][0], net["rm_a_plus"][0], net["rm_a_minus"][0], net["rm_dopamine"][0] = 0.05, 0.01, 0.01, 0.02
        dn.set_reward_modulator(0, dopamine=0.02, tau_c=0.05, a_plus=0.01, a_minus=0.01)

    def rewarded(walk):
        for r in (0.02, -0.01):
            walk.dn.run_with_reward(r)
        walk.net.run(2, rewards=[0.02, -0.01])
        walk.dn.run(STEPS - 2)
        walk.net.run(STEPS - 2)
    walk.station("14 set_reward_modulator", modulator, run=rewarded)
    if device:
        parity.assert_graph_equal(net, dn)
        assert np.array_equal(parity.bits(dn.get_trace_rows(0, n_tot)), parity.bits(net["traces"])), "station 14: traces differ from the oracle's"
        assert np.array_equal(parity.bits(np.array([dn.dopamine(0)], np.float32)), parity.bits(net["rm_dopamine"][:1]))
    assert net["traces"].any(), "station 14: no trace moved"
    dn.close()
    return walk.visited


def assert_static_conditions(visited):
    """over the stations of both halves"""
    writing = [v for v in visited if v[1]]
    assert sum(1 for v in writing if v[2]) >= 8, "writing stations entered with the image live"
    assert sum(1 for v in writing if v[3]) >= 8, "writing stations that leave the image live"
    assert sum(1 for v in writing if not v[3]) >= 3, "writing stations that leave the handle off the image"
    assert all(v[4] for v in writing), "every writing station passes its sensitivity check"


@functools.lru_cache(maxsize=None)
def static_plan(half):
    """one half of the static walk on the oracle alone: its expected list (every writing station's sensitivity asserted on the way)"""
    return half(None, device=False)


HALVES = pytest.mark.parametrize("half", [static_walk_writers, static_walk_forms], ids=["weight_writers", "step_forms"])


@HALVES
def test_static_walk_plan(half):
    """the oracle alone (no GPU): every writing station of the half passes its sensitivity check"""
    assert all(v[4] for v in static_plan(half) if v[1])


def test_static_walk_plan_meets_its_conditions():
    assert_static_conditions(static_plan(static_walk_writers) + static_plan(static_walk_forms))


@pytest.mark.gpu
@HALVES
def test_static_walk(snn, half):
    plan = static_plan(half)                    # (before a handle exists)
    assert half(snn, device=True) == plan


# ---- the plastic walk ----------------------------------------------------------------------------------------------------------
A_PLUS = A_MINUS = 0.01       # small enough for the moved weights to stay inside one 24-bit span of [0.5, 1.5) (checked on the oracle)


def plastic_walk(snn, device):
    import snn_amd
    net = static_net(ROW, CELLS, 22)
    net.n_threads = 8
    net["stdp_a_plus"], net["stdp_a_minus"] = A_PLUS, A_MINUS
    rng = np.random.default_rng(2200)
    w0 = parity.bits(net["weights"]).copy()
    walk = Walk(snn, net, device)
    dn = walk.dn
    dn.set_option("defer_stdp", 1)
    deferred = lambda: dn.stat("stdp_deferred_steps") if device else 0          # noqa: E731

    def plasticity(on):
        def write(dn, net):
            net["do_plasticity"] = int(on)
            dn.set_plasticity(0, float(net["stdp_a_plus"][0]), float(net["stdp_a_minus"][0]), float(net["stdp_tau_plus"][0]),
                              float(net["stdp_tau_minus"][0]), float(net["stdp_dt"][0]), on)
        return write

    def kick(walk, steps):
        """every 89th neuron to 35 mV, then `steps` steps: the last step before a station's write has spikes, so the update it
        leaves pending moves weights; returns the oracle's weight bits before that last step"""
        net["current_voltage"][::89] = F(35.0)
        dn.set_attr(0, "current_voltage", net["current_voltage"])
        if steps > 1:
            walk.run(steps - 1)
            net["current_voltage"][::89] = F(35.0)
            dn.set_attr(0, "current_voltage", net["current_voltage"])
        before = parity.bits(net["weights"]).copy()
        walk.run(1)
        return before

    def moved_edges(before, count):
        p, q = np.nonzero((before != parity.bits(net["weights"])) & (net["connections"] != 0))
        assert p.size >= count, f"the last step moved {p.size} weights"
        pick = rng.choice(p.size, count, replace=False)
        return p[pick], q[pick]

    walk.station("P1 plasticity on", plasticity(True), writing=False, run=lambda w: kick(w, 6))
    assert not walk.live
    count = deferred()
    assert not device or count > 0, "P1: no step deferred its STDP update"
    # P2: the edit lands on weights the pending update moves -- flushed first, then edited: the edit wins.  (P1's comparison read
    # attributes, and every getter applies a pending update: the update that is pending HERE is the one this kick leaves, and
    # between the kick and the graph_edit nothing reads the handle -- snn_get_stat does not flush)
    p, q = moved_edges(kick(walk, 2), 40)
    walk.station("P2 graph_edit with an update pending", edit(p, q, rng.uniform(0.5, 1.5, 40)))
    assert not device or deferred() > count, "P2: no step deferred its STDP update"
    count = deferred()
    if device:
        parity.assert_graph_equal(net, dn)
    # P3: a run that leaves an update pending, then connect_by_rule on the block
    kick(walk, 2)
    walk.station("P3 connect_by_rule with an update pending", connect(0, 0, snn_amd.ConnectionRule.chebyshev(300, self_edges=False),
                                                                       snn_amd.WeightRule.uniform(0.5, 1.5, seed=78)))
    assert not device or deferred() > count, "P3: no step deferred its STDP update"
    if device:
        parity.assert_graph_equal(net, dn)
    # P4: the same, then an edge list of both orders over weights the pending update moves
    p, q = moved_edges(kick(walk, 2), 60)
    pre, post, when = pair_list(net, rng, 100, 30, 9)
    pre, post, when = np.r_[p, pre], np.r_[q, post], np.r_[np.tile([1, 2], 30).astype(np.uint8), when]
    want = []

    def install(dn, net):
        dn.set_edge_history(pre, post, when)
        walk.record = True

    def recorded_run(walk):
        walk.dn.run(STEPS)
        want.append(oracle_rows(walk.net, pre, post, when, STEPS))
    count = deferred()
    walk.station("P4 set_edge_history with an update pending", install, writing=False, run=recorded_run)
    assert_record(walk, "P4", want[0])
    assert deferred() == count, "P4: a step deferred its update while the edge list was installed"

    def remove(dn, net):
        dn.set_edge_history([], [])
        walk.record = False
    walk.station("P5 edge list removed", remove, writing=False, run=lambda w: kick(w, STEPS))
    assert not device or deferred() > count, "P5: deferral did not resume"
    assert span_ok(net), "the moved weights must still be encodable (A_PLUS, A_MINUS)"
    assert np.any(parity.bits(net["weights"]) != w0), "plasticity moved no weight"
    walk.station("P6 plasticity off", plasticity(False), writing=False)
    assert walk.live
    if device:
        parity.assert_graph_equal(net, dn)
    dn.close()
    return walk.visited


def test_plastic_walk_plan():
    """the oracle alone (no GPU): spikes where the walk needs them, weights that move and stay encodable"""
    visited = plastic_walk(None, device=False)
    assert [v[3] for v in visited] == [False] * 5 + [True]


@pytest.mark.gpu
def test_plastic_walk(snn):
    visited = plastic_walk(snn, device=True)
    assert [v[3] for v in visited] == [False] * 5 + [True]
