#!/usr/bin/env python3
"""snn_connect_by_rules_csr at BASELINE configs[4] full size (4 x 512^2 Izhikevich neurons + 4 x 512^2 Poisson cells, CSR), one
process, median of 5 with the range:

(a) the twelve-record call on a handle that holds the empty graph (reset, untimed, before every run).  The library has no phase
    timer (and gets no statistic for this), so the split is taken from outside: `commit` is snn_set_graph_csr on the very arrays
    the call produced -- the same code the call ends in -- and `build_and_download` is the call minus that commit.  The download
    moves 12 B per edge + 4 B per row through the handle's page-locked stage; it is not separated from the kernels here.
(b) the route without the call: synthetic.c5_csr(512) in numpy, then snn_set_graph_csr; (a).build_and_download against
    (b).numpy_build is the comparison that matters, the commit being the same code in both.
(c) two 128x128 lattices connected SNN_RULE_ALL with probability 0.001 and uniform weights on a sparse handle: every pair is
    visited twice (count, fill), 2 x 268 M draws for ~268 k edges.
(d) the structure and weights of (a) against c5_csr(512), and bench.py's 105 steps (warm-up 5 + 5 x 20) from its C5 initial state
    on the rule-built handle and on a handle set through snn_set_graph_csr: the sha256 of the state table bench.py hashes.

Writes profiles/connect_rule_csr.json and prints it.  Usage: measure_connect_rule_csr.py [side]"""
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import snn_amd  # noqa: E402
from snn_amd import ConnectionRule, WeightRule, synthetic  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 512
m = side * side
PLAN = ([(k, k, ConnectionRule.euclidean(4, self_edges=False), None) for k in range(4)] +
        [(k, (k + 1) % 4, ConnectionRule.same_position(), None) for k in range(4)] +
        [(4 + k, k, ConnectionRule.same_position(), None) for k in range(4)])


def c5_handle():
    """bench.py's C5 (build_config) without its graph"""
    dn = snn_amd.DeviceNetwork(model=snn_amd.IZHIKEVICH, spike_train=snn_amd.ST_POISSON)
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


def timed(call, before=None, repeats=5):
    runs = []
    for _ in range(repeats):
        if before:
            before()
        t0 = time.perf_counter()
        call()
        runs.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}


def state_sha(dn):
    cols = []
    for name, dtype in (("current_voltage", np.float32), ("last_firing_time", np.int32), ("is_spiking", np.uint32)):
        cols.append(np.concatenate([dn.get_attr(k, name, dtype=dtype) for k in range(4)]).view(np.uint32))
    cols.append(np.concatenate([dn.spike_counts(k) for k in range(4)]).astype(np.uint32))
    return hashlib.sha256(np.stack(cols).tobytes()).hexdigest()


def bench_steps(dn):
    dn.set_reduced_history(False, False, True)
    dn.run(5)
    for _ in range(5):
        dn.run(20)
    return state_sha(dn)


out = {"workload": f"4 x ({side}x{side}) Izhikevich lattices + 4 Poisson lattices, CSR, {4 * m} rows"}
empty = (np.zeros(4 * m + 1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32))
rule = c5_handle()
rule.connect_sparse(PLAN)                                     # (first touch: page-locked stage, code objects)
call = timed(lambda: rule.connect_sparse(PLAN), before=lambda: rule.set_graph_csr(*empty))
rp, pi = rule.graph_csr_structure()
w = rule.get_graph_csr()
commit = timed(lambda: rule.set_graph_csr(rp, pi, w), before=lambda: rule.set_graph_csr(*empty))
out["a_rule_route"] = {"edges": int(pi.size), "call": call, "commit": commit,
                       "build_and_download_ms": call["median_ms"] - commit["median_ms"],
                       "download_bytes": int(pi.size) * 8 + (4 * m + 1) * 4}
numpy_build = timed(lambda: synthetic.c5_csr(side))
want = synthetic.c5_csr(side)
host = c5_handle()
host.set_graph_csr(*want)
out["b_host_route"] = {"numpy_build": numpy_build, "set_graph_csr": timed(lambda: host.set_graph_csr(*want), before=lambda: host.set_graph_csr(*empty))}
out["b_host_route"]["total_ms"] = numpy_build["median_ms"] + out["b_host_route"]["set_graph_csr"]["median_ms"]
out["rule_build_and_download_over_numpy_build"] = out["a_rule_route"]["build_and_download_ms"] / numpy_build["median_ms"]
out["rule_call_over_host_route"] = call["median_ms"] / out["b_host_route"]["total_ms"]

pair = snn_amd.DeviceNetwork(model=snn_amd.IZHIKEVICH)
pair.add_lattice(0, 128, 128)
pair.add_lattice(1, 128, 128)
pair.finalize(csr=True)
thin = [(0, 1, ConnectionRule.all_to_all(probability=0.001, seed=1), WeightRule.uniform(0.5, 1.5, seed=2))]
pair.connect_sparse(thin)
out["c_all_pairs_thinned"] = {"pairs": 128 ** 4, "edges": pair._nnz, "call": timed(lambda: pair.connect_sparse(thin), before=lambda: pair.set_graph_csr(np.zeros(2 * 128 * 128 + 1, np.uint64), empty[1], empty[2]))}
pair.close()

out["d_structure_equals_c5_csr"] = bool(np.array_equal(rp, want[0]) and np.array_equal(pi, want[1]) and np.array_equal(w.view(np.uint32), want[2].view(np.uint32)))
out["d_state_after_steps"] = 105
rule.set_graph_csr(*empty)
rule.connect_sparse(PLAN)                                     # (the steps below run on the graph the CALL committed)
out["d_state_sha256_rule_route"] = bench_steps(rule)
out["d_state_sha256_host_route"] = bench_steps(host)
out["d_states_equal"] = out["d_state_sha256_rule_route"] == out["d_state_sha256_host_route"]
out["d_steps_sparse_image"] = [int(rule.stat("steps_sparse_image")), int(host.stat("steps_sparse_image"))]
rule.close()
host.close()
text = json.dumps(out)
if side == 512:
    with open(os.path.join(ROOT, "profiles", "connect_rule_csr.json"), "w") as f:
        f.write(text + "\n")
print(text)
