"""Random call sequences that know the graph calls (test infrastructure; the device side is tests/test_gpu_sequences_graph.py,
the conditions on the generator are asserted on the CPU by tests/test_sequences_graph_plan.py).

The networks are those of test_gpu_randomized.draw(1000 + seed) under test_gpu_sequences.usable (no reward sequence, no BCM
kind), the graph form is plan["csr"], the generator stream is default_rng(500_000 + seed).  Kept from test_gpu_sequences.play, with
their meaning unchanged: run, voltage write, switch flip, plasticity toggle, synapse-kind toggle, reset_timing, and the
checkpoint.Tracker split (seed % 3 != 1: compared at every run-call boundary; the others only at the end, so that pending deferred
updates survive between calls).  New, each applied to the device AND to the oracle's `connections` / `weights` matrices:

  1 weight edit       graph_edit on 1 .. 40 stored edges (cells as pre among them), a few pairs repeated (the last occurrence wins);
                      sparse handles also get absent pairs with connected = 0 (no-ops)
  2 structural edit   absent pairs connected, stored edges removed, Some(0.0) written; graph_edit on dense handles,
                      graph_edit(..., structure=True) on sparse ones; sometimes connect-then-remove / remove-then-connect of one pair
  3 connect by rule   a random block (pre == post and spike-train lattices as pre allowed), the four rule kinds, random extent,
                      self_edges, probability in {1, 0.5, 0}, wrap flags; constant, uniform or displacement-table weights (NaN
                      entries); connect_by_rule on dense handles, connect_sparse with 1 .. 3 records on sparse ones (sometimes two
                      records for one block: the later wins).  Expected blocks: the plain loops of connect_rule_cases.py /
                      connect_spec_cases.py -- never ConnectionRule.mask or WeightRule.values
  4 wholesale write   a new mask: set_graph_rows for a band of rows (dense), set_graph_csr with a new structure (sparse)
  5 reads             graph_lookup on present and absent pairs, one graph_incoming and one graph_outgoing line, bit for bit; on
                      sparse handles graph_csr_structure() against parity.csr_for_posts
  6 edge history      a list of up to 60 pairs (stored, absent, cells as pre, one pair twice, orders 1 and 2 mixed), stride from
                      {1, 2, 3}, 1 .. 3 run calls with at most one weight or structural edit between them; the record equals the
                      oracle's, stepped one step at a time; the list is then removed, or with probability 1/3 left installed
  7 graph history     dense handles: set_graph_history(id, 1 or 2) on one lattice, a few steps, the oracle's sampled block
  8 checkpoint        checkpoint(), a weight-only edit, k steps, restore_checkpoint(), k steps: the state is that of an oracle clone
                      taken at the checkpoint and run k steps without the edit (weight-only: a restore after a structural call on a
                      sparse handle is refused by contract)

`Record` is the host model of the record axis: installing, replacing or removing the list, set_history_stride with another
stride, reset_history and switching a graph history on or off restart the record; while something records, rows are stored at
ticks 0, every, 2 * every ... since the restart; restore_checkpoint puts the cursor back where checkpoint() saw it.

A writing op that leaves `connections` and `weights` bit-identical is VOID and logged as such.

Out of scope: shard handles, reward-modulated and BCM networks -- their per-edge traces (trace, dw, counter) differ between the
dense and the sparse connect calls (the dense call restarts those of its block, the sparse one those of the whole graph) and
would need an oracle model of their own.

Measured by test_sequences_graph_plan.py on the oracle alone over the usable seeds of range(60) (the test compares a fresh
count with MEASURED below, which restates these numbers, so they cannot go stale): 24 sequences, 8 on dense and 16 on sparse
handles.  Sequences that hold op 1 .. 8: 21, 21, 18, 11, 12, 23, 8 (every dense one), 15; times drawn on dense handles: 11, 15,
9, 9, 4, 14, 17, 7; on sparse handles: 32, 30, 21, 9, 13, 38, - , 18 (op 1 counts its draws inside a static stretch).  185 writing
op instances (those inside ops 6 and 8 included), none of them void.  24 sequences hold a structural op that changes a column's
incoming-edge count and is followed by a run step with a synapse kind on; 7 sparse sequences leave an edge list installed across
a later structural op that changes the structure and is followed by a run; 12 connect_sparse calls hold two records for one
block.
"""
import collections

import numpy as np

import checkpoint
import connect_rule_cases
import connect_spec_cases
import parity
from test_gpu_randomized import SWITCHES, draw, make_handle
from test_gpu_sequences import _Absent, usable

# what the plan test measured (seeds usable of range(60)); the test asserts that a fresh measurement equals this
MEASURED = dict(sequences=24, dense=8, sparse=16, writes=185, voids=0, structural_then_run=24, list_across_structural=7,
                repeated_blocks=12,
                sequences_with={1: 21, 2: 21, 3: 18, 4: 11, 5: 12, 6: 23, 7: 8, 8: 15},
                dense_times={1: 11, 2: 15, 3: 9, 4: 9, 5: 4, 6: 14, 7: 17, 8: 7},
                sparse_times={1: 32, 2: 30, 3: 21, 4: 9, 5: 13, 6: 38, 7: 0, 8: 18})

F = np.float32
NEW_OPS = {1: "weight edit", 2: "structural edit", 3: "connect by rule", 4: "wholesale write", 5: "reads", 6: "edge history",
           7: "graph history", 8: "checkpoint"}
# draw weights of the op table: the kept ops first (run three times as likely as the others), then the new ones
# (only 8 of the kept networks are dense and a graph history needs one: op 7 weighs what puts it into every one of them)
KEPT_OPS = ["run"] * 3 + ["voltage", "switch", "plasticity", "synapses", "reset_timing"]
# "static": op 1 inside a stretch of kept ops that puts the handle on its static step forms (see static_stretch)
OP_TABLE = {False: KEPT_OPS + [1, "static"] + [2] * 3 + [3] * 3 + [4] * 2 + [5] * 2 + [6] * 5 + [7] * 6 + [8] * 2,
            True: KEPT_OPS + [1, "static", "static"] + [2] * 3 + [3] * 3 + [4] * 2 + [5] * 2 + [6] * 5 + [8] * 2}


class Record:
    """host model of the record axis (see the module docstring)"""

    def __init__(self):
        self.pairs = None               # (pre, post, when) of the installed edge list
        self.whist = None               # (lattice id, order) of the graph history that is on
        self.every = 1
        self.restart()

    def restart(self):
        self.tick, self.w, self.c, self.g = 0, [], [], []

    def active(self):
        return self.pairs is not None or self.whist is not None

    def mark(self):
        return self.tick, len(self.w), len(self.g)

    def rewind(self, mark):
        self.tick = mark[0]
        del self.w[mark[1]:], self.c[mark[1]:], self.g[mark[2]:]


def sample_pairs(net, pre, post):
    on = net["connections"][pre, post] != 0
    return np.where(on, net["weights"][pre, post], F(0)).astype(np.float32), on


def sample_block(net, first, count):
    return np.where(net["connections"][first:first + count, first:first + count] != 0,
                    net["weights"][first:first + count, first:first + count], F(0)).astype(np.float32)


def play(snn, seed, device=True):
    """One random sequence (a function of the seed alone) on a device handle and on the oracle; device=False replays it on the
    oracle alone.  Returns (log, info): info holds what the plan test asserts on."""
    net, plan = draw(1000 + seed)
    rng = np.random.default_rng(500_000 + seed)
    csr = bool(plan["csr"])
    dn = make_handle(snn, net, plan) if device else _Absent()
    nn, n_tot = net.n_neurons, net.n_tot
    ranges = net.layout.ranges()
    shapes = {i: (r, c) for i, r, c in net.layout.lattices + net.layout.st_lattices}
    lattices = [i for i, _, _ in net.layout.lattices]
    sources = lattices + [i for i, _, _ in net.layout.st_lattices]
    conn, wts = net["connections"], net["weights"]
    lo, hi = float(net["current_voltage"].min()) - 1.0, float(net["current_voltage"].max()) + 1.0
    log = []
    info = dict(csr=csr, kinds=collections.Counter(), writes=0, voids=0, structural_then_run=False, list_across_structural=False,
                repeated_blocks=0)
    rec = Record()
    real_run = net.run
    state = dict(structural_pending=False, list_structural_pending=False, top_level_list=False)

    def first_of(i):
        first, count, is_st = ranges[i]
        return (nn + first if is_st else first), count

    def oracle_run(k, **kw):
        if k and (net.electrical or net.chemical):
            info["structural_then_run"] |= state["structural_pending"]
            info["list_across_structural"] |= state["list_structural_pending"]
        if not rec.active():
            return real_run(k, **kw)
        for _ in range(k):
            now = rec.tick % rec.every == 0
            if now and rec.pairs is not None:
                w2, c2 = sample_pairs(net, rec.pairs[0], rec.pairs[1])
            if now and rec.whist is not None and rec.whist[1] == 2:
                rec.g.append(sample_block(net, *first_of(rec.whist[0])))
            real_run(1)
            if now and rec.pairs is not None:
                w1, c1 = sample_pairs(net, rec.pairs[0], rec.pairs[1])
                rec.w.append(np.where(rec.pairs[2] == 2, w2, w1))
                rec.c.append(np.where(rec.pairs[2] == 2, c2, c1))
            if now and rec.whist is not None and rec.whist[1] == 1:
                rec.g.append(sample_block(net, *first_of(rec.whist[0])))
            rec.tick += 1
    net.run = oracle_run
    tr = checkpoint.Tracker(snn, dn, net, plan, f"graph-sequence-{seed}", log=log, enabled=device and seed % 3 != 1)

    def run_both(k, tracked=True):
        if tracked and tr.enabled:
            tr.run(k)
        else:
            dn.run(k)
            net.run(k)

    def check_record():
        """the device's record(s) against the model's"""
        if not device:
            return
        if rec.pairs is not None:
            got_w, got_c = dn.edge_history()
            want_w = np.array(rec.w, np.float32).reshape(len(rec.w), rec.pairs[0].size)
            want_c = np.array(rec.c, bool).reshape(len(rec.c), rec.pairs[0].size)
            assert dn.history_steps() == len(rec.w) and got_w.shape == want_w.shape, f"record axis: {dn.history_steps()} rows, model {len(rec.w)}"
            assert np.array_equal(got_c, want_c), "edge history: connected flags differ from the oracle"
            assert np.array_equal(parity.bits(got_w), parity.bits(want_w)), "edge history: recorded weights differ from the oracle"
        if rec.whist is not None:
            first, count = first_of(rec.whist[0])
            got = dn.graph_history(rec.whist[0])
            want = np.array(rec.g, np.float32).reshape(len(rec.g), count, count)
            assert got.shape == want.shape and np.array_equal(parity.bits(got), parity.bits(want)), "graph history differs from the oracle"

    # ---- the writing ops: each returns its log entry; `written` wraps them with the void / structure bookkeeping --------------
    def written(kind, apply, top_level):
        before_c, before_w = conn.copy(), parity.bits(wts).copy()
        entry = apply()
        void = np.array_equal(before_c, conn) and np.array_equal(before_w, parity.bits(wts))
        info["writes"] += 1
        info["voids"] += int(void)
        if kind in (2, 3, 4) and top_level and np.any(before_c.sum(axis=0, dtype=np.int64) != conn.sum(axis=0, dtype=np.int64)):
            state["structural_pending"] = True
        if kind in (2, 3, 4) and top_level and csr and state["top_level_list"] and rec.pairs is not None and np.any(before_c != conn):
            state["list_structural_pending"] = True
        log.append(entry + (("VOID",) if void else ()))

    def edit_both(pre, post, w, on, structure):
        """the pairs applied one after another to the oracle's matrices, in one call to the device"""
        for p, q, x, c in zip(pre, post, w, on):
            conn[p, q] = 1 if c else 0
            wts[p, q] = x if c else F(0)
        dn.graph_edit(pre, post, w, connected=on, structure=structure)

    def weight_edit():
        sp, sq = np.nonzero(conn)
        m = int(rng.integers(1, 41))
        if sp.size == 0:
            return ("weight edit", 0)
        pick = rng.integers(0, sp.size, m)
        pre, post = sp[pick], sq[pick]
        again = rng.integers(0, m, int(rng.integers(1, 4)))                  # a few pairs once more, with another weight
        pre, post = np.r_[pre, pre[again]], np.r_[post, post[again]]
        on = np.ones(pre.size, np.uint8)
        if csr:                                                               # absent pairs with connected = 0: no-ops
            ap, aq = np.nonzero(conn == 0)
            if ap.size:
                pick = rng.integers(0, ap.size, int(rng.integers(1, 6)))
                at = rng.integers(0, pre.size + 1)
                pre, post = np.insert(pre, at, ap[pick]), np.insert(post, at, aq[pick])
                on = np.insert(on, at, np.zeros(pick.size, np.uint8))
        w = rng.uniform(-0.5, 2.0, pre.size).astype(np.float32)
        edit_both(pre, post, w, on, structure=False)
        return ("weight edit", int(pre.size))

    def structural_edit():
        ap, aq = np.nonzero(conn == 0)
        sp, sq = np.nonzero(conn)
        pre, post, on = [], [], []

        def add(p, q, c):
            pre.append(int(p))
            post.append(int(q))
            on.append(c)
        for k in (rng.integers(0, ap.size, int(rng.integers(1, 9))) if ap.size else ()):
            add(ap[k], aq[k], 1)                                              # connect
        for k in (rng.integers(0, sp.size, int(rng.integers(1, 9))) if sp.size else ()):
            add(sp[k], sq[k], 0)                                              # remove
        twice = int(rng.integers(0, 3))                                       # 1: connect then remove one pair, 2: the reverse
        if twice:
            p, q = int(rng.integers(0, n_tot)), int(rng.integers(0, nn))
            add(p, q, 2 - twice)
            add(p, q, twice - 1)
        order = rng.permutation(len(pre)) if not twice else np.r_[rng.permutation(len(pre) - 2), len(pre) - 2, len(pre) - 1]
        pre, post, on = np.array(pre)[order], np.array(post)[order], np.array(on, np.uint8)[order]
        w = rng.uniform(-0.5, 2.0, pre.size).astype(np.float32)
        w[rng.random(pre.size) < 0.2] = F(0)                                  # Some(0.0) is an edge
        edit_both(pre, post, w, on, structure=True)
        return ("structural edit", int(pre.size), twice)

    def one_rule(block=None):
        """a random record: (pre id, post id, fields of the rule and of the weight)"""
        pre_id, post_id = block or (int(rng.choice(sources)), int(rng.choice(lattices)))
        kind = int(rng.integers(0, 4))
        extent = int(rng.integers(0, 9 if kind == connect_spec_cases.EUCLIDEAN else 4))
        wrap = int(rng.integers(0, 4))
        rule = dict(kind=kind, extent=extent, self_edges=bool(rng.integers(0, 2)), probability=float(rng.choice([1.0, 0.5, 0.0])),
                    seed=int(rng.integers(0, 2**40)), wrap=wrap)
        wk = int(rng.integers(0, 3))
        weight = dict(kind=wk, lo=float(F(rng.uniform(-0.5, 1.0))), hi=float(F(rng.uniform(1.0, 2.0))), seed=int(rng.integers(0, 2**40)), table=None)
        if wk == connect_spec_cases.DISPLACEMENT:
            t = rng.uniform(-0.5, 2.0, connect_spec_cases.table_shape(shapes[pre_id], shapes[post_id], wrap)).astype(np.float32)
            t[rng.random(t.shape) < 0.15] = np.nan
            weight["table"] = t
        return pre_id, post_id, rule, weight

    def expected(pre_id, post_id, rule, weight):
        if rule["wrap"] == 0 and weight["kind"] != connect_spec_cases.DISPLACEMENT:
            return connect_rule_cases.expected_block(shapes[pre_id], shapes[post_id], rule["kind"], rule["extent"], rule["self_edges"],
                                                     rule["probability"], rule["seed"], weight["kind"], weight["lo"], weight["hi"], weight["seed"])
        return connect_spec_cases.expected_block(shapes[pre_id], shapes[post_id], rule["kind"], rule["extent"], rule["self_edges"],
                                                 rule["probability"], rule["seed"], weight["kind"], weight["lo"], weight["hi"], weight["seed"],
                                                 rule["wrap"], weight["table"])

    def device_rule(rule, weight):
        wrap = (bool(rule["wrap"] & 1), bool(rule["wrap"] & 2))
        r = snn.ConnectionRule(rule["kind"], rule["extent"], rule["self_edges"], rule["probability"], rule["seed"], wrap=wrap)
        if weight["kind"] == connect_spec_cases.DISPLACEMENT:
            return r, snn.WeightRule.displacement(weight["table"], wrap=wrap)
        return r, snn.WeightRule(weight["kind"], weight["lo"], weight["hi"], weight["seed"])

    def connect_rule():
        records = [one_rule()]
        if csr:
            for _ in range(int(rng.integers(0, 3))):
                records.append(one_rule(records[0][:2] if rng.integers(0, 2) else None))      # (the same block again: the later wins)
        info["repeated_blocks"] += int(len({r[:2] for r in records}) < len(records))      # two records for one block in this call
        for pre_id, post_id, rule, weight in records:
            on, w = expected(pre_id, post_id, rule, weight)
            (p0, pn), (q0, qn) = first_of(pre_id), first_of(post_id)
            conn[p0:p0 + pn, q0:q0 + qn] = on
            wts[p0:p0 + pn, q0:q0 + qn] = w
        if device and csr:
            dn.connect_sparse([(p, q) + device_rule(r, w) for p, q, r, w in records])
        elif device:
            dn.connect_by_rule(records[0][0], records[0][1], *device_rule(*records[0][2:]))
        return ("connect by rule",) + tuple((p, q, r["kind"], r["extent"], r["probability"], r["wrap"], w["kind"]) for p, q, r, w in records)

    def wholesale():
        density = float(rng.choice([0.1, 0.4, 0.9]))
        if csr:
            b, e = 0, n_tot
        else:
            b = int(rng.integers(0, n_tot))
            e = int(rng.integers(b + 1, n_tot + 1))
        conn[b:e] = rng.random((e - b, nn)) < density
        wts[b:e] = rng.uniform(-0.5, 2.0, (e - b, nn)).astype(np.float32) * conn[b:e]
        if device and csr:
            dn.set_graph_csr(*parity.csr_for_posts(net, dn.owned))
        elif device:
            dn.set_graph_rows(b, wts[b:e], conn[b:e].astype(np.uint32))
        return ("wholesale write", b, e, density)

    WRITERS = {1: weight_edit, 2: structural_edit, 3: connect_rule, 4: wholesale}

    def reads():
        m = int(rng.integers(1, 31))
        pre, post = rng.integers(0, n_tot, m), rng.integers(0, nn, m)
        sp, sq = np.nonzero(conn)
        if sp.size:
            pick = rng.integers(0, sp.size, int(rng.integers(1, 11)))
            pre, post = np.r_[pre, sp[pick]], np.r_[post, sq[pick]]
        q, p = int(rng.integers(0, nn)), int(rng.integers(0, n_tot))
        if device:
            want_w, want_c = sample_pairs(net, pre, post)
            got_w, got_c = dn.graph_lookup(pre, post)
            assert np.array_equal(got_c, want_c) and np.array_equal(parity.bits(got_w), parity.bits(want_w)), "graph_lookup differs from the oracle"
            for (index, w), line, lw in ((dn.graph_incoming(q), conn[:, q], wts[:, q]), (dn.graph_outgoing(p), conn[p], wts[p])):
                want = np.nonzero(line)[0]
                assert np.array_equal(index, want) and np.array_equal(parity.bits(w), parity.bits(np.ascontiguousarray(lw[want]))), \
                    "a graph line differs from the oracle"
            if csr:
                rp, pi = dn.graph_csr_structure()
                want_rp, want_pi, _ = parity.csr_for_posts(net, dn.owned)
                assert np.array_equal(rp, want_rp) and np.array_equal(pi, want_pi), "graph_csr_structure differs from the oracle"
        log.append(("reads", int(pre.size), q, p))

    def edge_history():
        check_record()                                                        # (a list left installed is about to be replaced)
        pre, post = [], []
        sp, sq = np.nonzero(conn)
        if sp.size:
            pick = rng.integers(0, sp.size, int(rng.integers(1, 26)))
            pre.extend(sp[pick])
            post.extend(sq[pick])
        ap, aq = np.nonzero(conn == 0)
        if ap.size:
            pick = rng.integers(0, ap.size, int(rng.integers(1, 16)))
            pre.extend(ap[pick])
            post.extend(aq[pick])
        if n_tot > nn:
            m = int(rng.integers(1, 11))
            pre.extend(rng.integers(nn, n_tot, m))
            post.extend(rng.integers(0, nn, m))
        pre.append(pre[0])                                                    # one pair listed twice
        post.append(post[0])
        pre, post = np.array(pre, np.int64), np.array(post, np.int64)
        when = rng.integers(1, 3, pre.size).astype(np.uint8)
        every = int(rng.choice([1, 2, 3]))
        dn.set_history_stride(every)
        dn.set_edge_history(pre, post, when)
        rec.pairs, rec.every = (pre, post, when), every
        rec.restart()
        state["top_level_list"] = False
        runs = [int(rng.integers(1, 26)) for _ in range(int(rng.integers(1, 4)))]
        between = int(rng.integers(0, 3)) if len(runs) > 1 else 0              # 0 nothing, 1 a weight edit, 2 a structural edit
        at = int(rng.integers(0, len(runs) - 1)) if between else -1
        log.append(("edge history", int(pre.size), every, tuple(runs), between))
        for k, steps in enumerate(runs):
            run_both(steps)
            if k == at:
                written(between, WRITERS[between], top_level=False)
        check_record()
        if rng.integers(0, 3) == 0:
            state["top_level_list"] = True                                    # left installed for the following ops
            log.append(("edge list stays",))
        else:
            remove_list()

    def remove_list():
        dn.set_edge_history([], [])
        dn.set_history_stride(1)
        rec.pairs, rec.every = None, 1
        rec.restart()
        state["top_level_list"] = False

    def graph_history():
        i, order, k = int(rng.choice(lattices)), int(rng.integers(1, 3)), int(rng.integers(1, 11))
        dn.reset_history()
        dn.set_graph_history(i, order)
        rec.whist = (i, order)
        rec.restart()
        run_both(k, tracked=False)
        check_record()
        dn.set_graph_history(i, 0)
        rec.whist = None
        rec.restart()
        log.append(("graph history", i, order, k))

    def checkpoint_round_trip():
        k = int(rng.integers(1, 21))
        dn.checkpoint()
        snap, mark = checkpoint.clone(net), rec.mark()
        written(1, weight_edit, top_level=False)
        run_both(k, tracked=False)
        dn.restore_checkpoint()
        rec.rewind(mark)
        for name, a in snap.arr.items():
            net.arr[name][...] = a                                            # (in place: `conn` and `wts` stay the oracle's arrays)
        net.clock = snap.clock
        run_both(k, tracked=False)
        if tr.enabled:
            parity.assert_state_equal(net, parity.pull_state(dn, net))
            parity.assert_graph_equal(net, dn)
        log.append(("checkpoint", k))

    def static_stretch():
        """Kept ops chosen, not drawn, around a weight edit: plasticity off everywhere, gap junctions only, the one-launch step
        allowed, a run, the edit, a run, a comparison.  A sparse handle then steps from its step image before AND after the edit
        (a random sequence hardly ever stands there when op 1 comes): an in-place edit that left the image's records behind shows."""
        for slot, (i, _, _) in enumerate(net.layout.lattices):
            dn.set_plasticity(i, float(net["stdp_a_plus"][slot]), float(net["stdp_a_minus"][slot]), float(net["stdp_tau_plus"][slot]),
                              float(net["stdp_tau_minus"][slot]), float(net["stdp_dt"][slot]), False)
            net["do_plasticity"][slot] = 0
            log.append(("plasticity", i, False))
        dn.set_synapses(True, False)
        net.electrical, net.chemical = True, False
        log.append(("synapses", True, False))
        dn.set_option("fused_step", 1)
        tr.options["fused_step"] = 1
        log.append(("switch", "fused_step", 1))
        k = [int(rng.integers(1, 20)), int(rng.integers(1, 20))]
        run_both(k[0])
        log.append(("run", k[0]))
        written(1, weight_edit, top_level=True)
        run_both(k[1])
        log.append(("run", k[1]))
        if device:
            parity.assert_state_equal(net, parity.pull_state(dn, net))
            parity.assert_graph_equal(net, dn)

    # ---- the sequence ------------------------------------------------------------------------------------------------------------
    try:
        table = OP_TABLE[csr]
        for _ in range(int(rng.integers(10, 19))):
            op = table[int(rng.integers(0, len(table)))]
            if op in NEW_OPS or op == "static":
                info["kinds"][1 if op == "static" else op] += 1
            if op == "run":
                k = int(rng.integers(1, 50))
                run_both(k)
                log.append(("run", k))
            elif op == "voltage":
                i = int(rng.choice(lattices))
                first, count, _ = ranges[i]
                v = rng.uniform(lo, hi, count).astype(np.float32)
                dn.set_attr(i, "current_voltage", v)
                net["current_voltage"][first:first + count] = v
                log.append(("voltage", i))
            elif op == "switch":
                name = str(rng.choice(list(SWITCHES)))
                value = int(rng.choice(SWITCHES[name]))
                dn.set_option(name, value)
                tr.options[name] = value
                log.append(("switch", name, value))
            elif op == "plasticity":
                slot = int(rng.integers(0, len(net.layout.lattices)))
                i = net.layout.lattices[slot][0]
                on = bool(rng.integers(0, 2))
                dn.set_plasticity(i, float(net["stdp_a_plus"][slot]), float(net["stdp_a_minus"][slot]), float(net["stdp_tau_plus"][slot]),
                                  float(net["stdp_tau_minus"][slot]), float(net["stdp_dt"][slot]), on)
                net["do_plasticity"][slot] = int(on)
                log.append(("plasticity", i, on))
            elif op == "synapses":
                el, ch = [(True, False), (True, True), (False, True)][int(rng.integers(0, 3))]
                dn.set_synapses(el, ch)
                net.electrical, net.chemical = el, ch
                log.append(("synapses", el, ch))
            elif op == "reset_timing":
                dn.reset_timing()
                net.clock = 0                                    # neuron/mod.rs:405-420, 1710-1717
                net["last_firing_time"][...] = -1
                if net.n_cells:
                    net["st_last_firing_time"][...] = -1
                    net["st_clock"][...] = 0
                log.append(("reset_timing",))
            elif op == "static":
                static_stretch()
            elif op in WRITERS:
                written(op, WRITERS[op], top_level=True)
            elif op == 5:
                reads()
            elif op == 6:
                edge_history()
            elif op == 7:
                graph_history()
            elif op == 8:
                checkpoint_round_trip()
        run_both(5)
        if device:
            check_record()
            parity.assert_state_equal(net, parity.pull_state(dn, net))
            parity.assert_graph_equal(net, dn)
            assert dn.clock == net.clock
            if csr:
                rp, pi = dn.graph_csr_structure()
                want_rp, want_pi, _ = parity.csr_for_posts(net, dn.owned)
                assert np.array_equal(rp, want_rp) and np.array_equal(pi, want_pi), "graph structure differs from the oracle"
    except Exception as e:                      # noqa: BLE001 (a refused call is a finding like a mismatch: both carry the log)
        dn.close()
        raise AssertionError(f"{type(e).__name__}: {e}; sequence: {log}") from e
    dn.close()
    return log, info


def measure(seeds):
    """the counts the plan test asserts on, over the oracle-only replays of `seeds`"""
    out = dict(sequences=0, dense=0, sparse=0, writes=0, voids=0, structural_then_run=0, list_across_structural=0, repeated_blocks=0,
               sequences_with={k: 0 for k in NEW_OPS}, dense_times={k: 0 for k in NEW_OPS}, sparse_times={k: 0 for k in NEW_OPS})
    for seed in seeds:
        _, info = play(None, seed, device=False)
        form = "sparse" if info["csr"] else "dense"
        out["sequences"] += 1
        out[form] += 1
        out["writes"] += info["writes"]
        out["voids"] += info["voids"]
        out["structural_then_run"] += int(info["structural_then_run"])
        out["list_across_structural"] += int(info["list_across_structural"])
        out["repeated_blocks"] += info["repeated_blocks"]
        for k, n in info["kinds"].items():
            out["sequences_with"][k] += 1
            out[form + "_times"][k] += n
    return out


def seeds(limit):
    return [s for s in range(limit) if usable(s)]
