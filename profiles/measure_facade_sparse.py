#!/usr/bin/env python3
"""BASELINE configs[4] at full size -- four 512x512 Izhikevich lattices and four 512x512 Poisson lattices, 14.6 M edges, the one
config whose dense form cannot exist -- built and stepped THROUGH THE NETWORK CLASS a user of the reference writes against:
IzhikevichNeuronNetworkGPU(sparse=True), populate / apply_*_given_position / add_lattice / connect with the twelve records of
profiles/measure_connect_rule_csr.py's PLAN, run_lattices.  Every lattice stays rule-held and every block between lattices stays
a record: no matrix, no dict entry per edge and no CSR array on the host.

Initial state goes through the facade only: gap_conductance and chance_of_firing ride on the populate prototypes, voltages and
seeds are set cell by cell with apply_given_position (the facade has no bulk setter).  The graph and the state table are READ
through the handle the facade owns (network._dn: graph_csr_structure / get_graph_csr / get_attr / spike_counts), after the runs.

Two conditions, not measurements: the graph equals synthetic.c5_csr(512) bit for bit, and the state digest after bench.py's
5 + 5 x 20 steps from its C5 initial state equals d_state_sha256_rule_route of profiles/connect_rule_csr.json.  The times and the
peak resident set are measured, with no bar fixed in advance; the direct route (DeviceNetwork.connect_sparse on a handle filled by
set_attr) runs first in a child process of its own and is written beside them with the ratios.

One run, no retries, under its own time limit.  Writes profiles/facade_sparse_c5.json and prints it.
Usage: measure_facade_sparse.py [side]"""
import hashlib
import json
import os
import resource
import signal
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import snn_amd  # noqa: E402
from snn_amd import ConnectionRule, synthetic  # noqa: E402

direct = "--direct" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
side = int(args[0]) if args else 512
m = side * side
TIME_LIMIT_S = 900
PLAN = ([(k, k, ConnectionRule.euclidean(4, self_edges=False), None) for k in range(4)] +
        [(k, (k + 1) % 4, ConnectionRule.same_position(), None) for k in range(4)] +
        [(4 + k, k, ConnectionRule.same_position(), None) for k in range(4)])
phases = {}


def timed(name, call):
    t0 = time.perf_counter()
    out = call()
    phases[name] = phases.get(name, 0.0) + time.perf_counter() - t0
    print(f"[measure_facade_sparse{' direct' if direct else ''}] {name} {phases[name]:.2f} s", file=sys.stderr, flush=True)
    return out


def state_sha(dn):
    """the state table profiles/measure_connect_rule_csr.py hashes"""
    cols = []
    for name, dtype in (("current_voltage", np.float32), ("last_firing_time", np.int32), ("is_spiking", np.uint32)):
        cols.append(np.concatenate([dn.get_attr(k, name, dtype=dtype) for k in range(4)]).view(np.uint32))
    cols.append(np.concatenate([dn.spike_counts(k) for k in range(4)]).astype(np.uint32))
    return hashlib.sha256(np.stack(cols).tobytes()).hexdigest()


def max_rss_mb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


def direct_route():
    """the same network on a DeviceNetwork: attributes in bulk, the graph by connect_sparse, bench.py's steps"""
    def handle():
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
    start = time.perf_counter()
    dn = timed("handle_and_state_s", handle)
    timed("connect_s", lambda: dn.connect_sparse(PLAN))
    dn.set_reduced_history(False, False, True)
    timed("run_s", lambda: dn.run(5))
    for _ in range(5):
        timed("run_s", lambda: dn.run(20))
    # (run() returns once the steps are queued: one small read waits for them, as every run_lattices of the facade ends in reads)
    timed("run_s", lambda: dn.get_attr(0, "is_spiking", dtype=np.uint32))
    total = time.perf_counter() - start
    sha = state_sha(dn)
    edges = int(dn._nnz)
    dn.close()
    return {**{k: round(v, 3) for k, v in phases.items()}, "total_s": round(total, 3), "edges": edges, "ru_maxrss_MB": max_rss_mb(),
            "state_sha256": sha}


signal.alarm(TIME_LIMIT_S)                          # the script's own limit: SIGALRM ends the process
if direct:
    print(json.dumps(direct_route()))
    sys.exit(0)

child = subprocess.run([sys.executable, os.path.abspath(__file__), str(side), "--direct"], stdout=subprocess.PIPE, timeout=300, check=True)
direct_result = json.loads(child.stdout.decode().strip().splitlines()[-1])

start = time.perf_counter()
ln = snn_amd
network = ln.IzhikevichNeuronNetworkGPU(sparse=True)
for k in range(4):
    lattice = ln.IzhikevichNeuronLattice(k)
    timed("populate_s", lambda: lattice.populate(ln.IzhikevichNeuron(gap_conductance=10.0), side, side))
    v0 = synthetic.uniform(6, m, -65.0, 30.0, offset=k * m)
    timed("apply_s", lambda: lattice.apply_given_position(lambda pos, cell: setattr(cell, "current_voltage", float(v0[pos[0] * side + pos[1]]))))
    timed("add_lattice_s", lambda: network.add_lattice(lattice))              # (the container owns a copy)
    del lattice
for k in range(4):
    train = ln.PoissonNeuronLattice(4 + k)
    timed("populate_s", lambda: train.populate(ln.PoissonNeuron(chance_of_firing=0.01), side, side))
    timed("apply_s", lambda: train.apply_given_position(lambda pos, cell: setattr(cell, "seed", k * m + 1 + pos[0] * side + pos[1])))
    timed("add_lattice_s", lambda: network.add_spike_train_lattice(train))
    del train
for pre, post, rule, weight in PLAN:
    timed("connect_s", lambda: network.connect(pre, post, rule, weight))
network.electrical_synapse, network.chemical_synapse = True, False
dn = timed("upload_s", network._ensure)                          # handle, neuron and cell state, ONE connect_sparse of the twelve records
network.set_reduced_history(spike_counts=True)
timed("run_s", lambda: network.run_lattices(5))
for _ in range(5):
    timed("run_s", lambda: network.run_lattices(20))
total = time.perf_counter() - start
rss_after_runs = max_rss_mb()
queries = {}
gp = ln.GraphPosition
mid = side // 2
for name, call in (("get_weight_ms", lambda: network.get_weight(gp(0, (3, 4)), gp(0, (3, 6)))),
                   ("get_weight_across_lattices_ms", lambda: network.get_weight(gp(4, (mid, mid)), gp(0, (mid, mid)))),
                   ("get_incoming_connections_ms", lambda: network.get_incoming_connections_within_lattice(0, (mid, mid))),
                   ("get_outgoing_connections_ms", lambda: network.get_outgoing_connections_within_lattice(0, (mid, mid))),
                   ("get_incoming_connectings_across_lattices_ms", lambda: network.get_incoming_connectings_across_lattices(0, (mid, mid)))):
    t0 = time.perf_counter()
    answer = call()
    queries[name] = (time.perf_counter() - t0) * 1e3
    queries[name.replace("_ms", "_answer")] = answer if isinstance(answer, float) else len(answer)
held = bool(all(l.rule_held for l in network.network.lattices.values()) and len(network.network.connecting_rules) == 8
            and not network.network.connecting)
sha = state_sha(dn)
images = int(dn.stat("steps_sparse_image"))
rp, pi = dn.graph_csr_structure()
w = dn.get_graph_csr()
want = synthetic.c5_csr(side)
graph_equal = bool(np.array_equal(rp, want[0]) and np.array_equal(pi, want[1]) and np.array_equal(w.view(np.uint32), want[2].view(np.uint32)))
network.close()
rule_route = None
reference = os.path.join(ROOT, "profiles", "connect_rule_csr.json")
if side == 512 and os.path.exists(reference):
    rule_route = json.load(open(reference))["d_state_sha256_rule_route"]
facade = {**{k: round(v, 3) for k, v in phases.items()}, "total_s": round(total, 3), "edges": int(pi.size),
          "ru_maxrss_MB_after_the_runs": rss_after_runs, **queries, "rule_held_and_records_after_the_runs": held,
          "steps_sparse_image": images, "state_sha256": sha}
out = {"workload": f"4 x ({side}x{side}) Izhikevich lattices + 4 Poisson lattices through IzhikevichNeuronNetworkGPU(sparse=True), {4 * m} rows",
       "initial_state": "facade only: populate prototypes (gap_conductance, chance_of_firing) and apply_given_position per cell "
                        "(current_voltage, seed); graph and state table read through the handle the facade owns",
       "facade": facade, "direct_connect_sparse": direct_result,
       "facade_over_direct": {"total": round(total / direct_result["total_s"], 2),
                              "connect_and_upload": round((phases["connect_s"] + phases["upload_s"]) /
                                                          (direct_result["handle_and_state_s"] + direct_result["connect_s"]), 2),
                              "run": round(phases["run_s"] / direct_result["run_s"], 2),
                              "ru_maxrss": round(rss_after_runs / direct_result["ru_maxrss_MB"], 2)},
       "graph_equals_c5_csr": graph_equal, "state_after_steps": 105,
       "d_state_sha256_rule_route": rule_route, "state_equals_rule_route": (sha == rule_route) if rule_route else None,
       "state_equals_direct_route": sha == direct_result["state_sha256"]}
text = json.dumps(out)
if side == 512:
    with open(os.path.join(ROOT, "profiles", "facade_sparse_c5.json"), "w") as f:
        f.write(text + "\n")
print(text)
