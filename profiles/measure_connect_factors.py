#!/usr/bin/env python3
"""snn_connect_by_factors at the headline size (256x256 Izhikevich lattice, 65 536 neurons, 17.18 GB matrix), one process, one
handle, median of 5 with the range (wall time of the blocking call, after one untimed call of each form):
  (a) all-to-all without self edges, UNIFORM(0.5, 1.5) through snn_connect_by_rule: the yardstick of measure_connect_rule.py;
  (b) all-to-all without self edges, WeightRule.hopfield of 8 binary patterns with drop_zero: 16 binary64 operations per element;
  (c) the same with 32 patterns.
No bar; the expectation was (b) within about 1.5 x (a).  Then, through IzhikevichNeuronLatticeGPU, the lattice connected as in (b)
runs 105 steps and the hash of its state (the table bench.py hashes) is recorded as a regression anchor.

The JSON's "kernel_stats" block is not written here: it holds the kernel durations of a separate rocprofv3 --kernel-trace --stats
run of the same three calls (its summary: profiles/connect_factors_256x256_kernel_stats.csv) and is carried over.

Writes profiles/connect_factors_256x256.json (or the path given) and prints it.
Usage: measure_connect_factors.py [rows cols [output.json]]"""
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

rows, cols = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (256, 256)
path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "connect_factors_256x256.json")
n = rows * cols
gbytes = 4.0 * n * n / 1e9
A, B = 0.3, 0.7


def patterns(p):
    return np.random.default_rng(p).integers(0, 2, (p, n)).astype(np.float64)


def timed(call, repeats=5):
    call()                                                     # (untimed: first touch, code object load)
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        runs.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}


rule = ConnectionRule.all_to_all(self_edges=False)
dn = snn_amd.DeviceNetwork(model=snn_amd.IZHIKEVICH)
dn.add_lattice(0, rows, cols)
dn.finalize()
uniform = WeightRule.uniform(0.5, 1.5, seed=2)
forms = {"all_uniform": lambda: dn._check(dn._L.snn_connect_by_rule(dn._h, 0, 0, rule.kind, rule.extent, 0, 1.0, 0, uniform.kind, uniform.lo,
                                                                    uniform.hi, uniform.seed))}
for p in (8, 32):
    weight = WeightRule.hopfield(patterns(p), a=A, b=B, scalar=1.0 / p)
    forms[f"hopfield_{p}"] = lambda weight=weight: dn.connect_by_rule(0, 0, rule, weight)
dense = {}
for name in ("all_uniform", "hopfield_8", "hopfield_32", "all_uniform"):           # (the yardstick again at the end: drift shows)
    key = name if name not in dense else name + "_again"
    dense[key] = timed(forms[name])
    dense[key]["GBps"] = gbytes / (dense[key]["median_ms"] * 1e-3)
for p in (8, 32):
    dense[f"hopfield_{p}"]["binary64_GFLOP"] = 2.0 * p * n * n / 1e9
    dense[f"hopfield_{p}"]["over_uniform"] = dense[f"hopfield_{p}"]["median_ms"] / dense["all_uniform"]["median_ms"]
# what the last factors call wrote, on one column, against the host twin (the graph now holds UNIFORM again: connect once more)
weight8 = WeightRule.hopfield(patterns(8), a=A, b=B, scalar=1.0 / 8)
dn.connect_by_rule(0, 0, rule, weight8)
j = n // 2 + 3
index, w = dn.graph_incoming(j)
on, want = snn_amd.network.rule_pairs(rule, weight8, (rows, cols), (rows, cols), None, [j])
sample = bool(np.array_equal(index, np.nonzero(on[:, 0])[0]) and np.array_equal(w.view(np.uint32), want[on[:, 0], 0].view(np.uint32)))
dn.close()

# ---- the lattice built this way, 105 steps ---------------------------------------------------------------------------------------
lattice = snn_amd.IzhikevichNeuronLatticeGPU(0)
lattice.populate(snn_amd.IzhikevichNeuron(gap_conductance=10.0), rows, cols)
v0 = synthetic.uniform(1, n, -65.0, 30.0)
lattice.apply_given_position(lambda pos, cell: setattr(cell, "current_voltage", float(v0[pos[0] * cols + pos[1]])))
lattice.connect(rule, weight8)
network = lattice._ensure()
network.set_reduced_history(spike_counts=True)
lattice.run_lattice(5)
for _ in range(5):
    lattice.run_lattice(20)
cells = [c for row in lattice.cell_grid for c in row]
table = np.stack([np.array([c.current_voltage for c in cells], np.float32).view(np.uint32),
                  np.array([-1 if c.last_firing_time is None else c.last_firing_time for c in cells], np.int32).view(np.uint32),
                  np.array([c.is_spiking for c in cells], np.uint32), network.spike_counts(0).reshape(-1).astype(np.uint32)])
sha = hashlib.sha256(table.tobytes()).hexdigest()
rule_held = bool(lattice.rule_held)
lattice.close()

out = {"workload": f"{rows}x{cols} lattice, {n} neurons, {gbytes:.2f} GB matrix; ALL without self edges; hopfield of P binary patterns "
                   f"(numpy default_rng(P)), a = {A}, b = {B}, scalar = 1 / P, drop_zero",
       "dense": dense, "expectation": "hopfield_8 within about 1.5 x all_uniform", "column_sample_equals_host_twin": sample,
       "state_after_steps": 105, "state_sha256": sha, "rule_held_after_the_runs": rule_held}
if os.path.exists(path):                                       # the kernel times of the separate kernel-stats run stay with the file
    kept = json.load(open(path)).get("kernel_stats")
    if kept:
        out["kernel_stats"] = kept
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
