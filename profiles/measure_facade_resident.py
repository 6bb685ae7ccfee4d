#!/usr/bin/env python3
"""The headline lattice (256x256 Izhikevich neurons, 65 536 of them, a 17.18 GB matrix) built and stepped THROUGH THE LATTICE CLASS
a user of the reference touches -- IzhikevichNeuronLatticeGPU: populate, apply_given_position, connect by record, run_lattice --
with the graph rule-held: no N x N array on the host at any point.

Records the wall time of each phase, the process's peak resident set (ru_maxrss), the time of one get_weight, one
get_incoming_connections and one get_outgoing_connections answered by the device, and the sha256 of the state table
profiles/measure_connect_rule.py hashes (voltage bits, last_firing_time, is_spiking, spike totals) after the bench's 5 + 5 x 20
steps, next to the digest the bench records.  VERDICT.md's bars -- under 60 s, under 2 GB of host memory, the bench's digest -- are
reported, not asserted.  Prints one JSON line.  Usage: measure_facade_resident.py [rows cols]"""
import hashlib
import json
import os
import resource
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import snn_amd  # noqa: E402
from snn_amd import ConnectionRule, WeightRule, synthetic  # noqa: E402

BENCH_STATE_SHA256 = "c91f01a99e0fbb7d7bb8672dad90b71ae6584e1667a258bc22a959e3c9371743"      # BENCH_r06.json, after 105 steps

rows, cols = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (256, 256)
n = rows * cols
phases = {}


def timed(name, call):
    t0 = time.perf_counter()
    out = call()
    phases[name] = phases.get(name, 0.0) + time.perf_counter() - t0
    return out


start = time.perf_counter()
lattice = snn_amd.IzhikevichNeuronLatticeGPU(0)
timed("populate_s", lambda: lattice.populate(snn_amd.IzhikevichNeuron(gap_conductance=10.0), rows, cols))
v0 = synthetic.uniform(1, n, -65.0, 30.0)
timed("apply_s", lambda: lattice.apply_given_position(lambda pos, cell: setattr(cell, "current_voltage", float(v0[pos[0] * cols + pos[1]]))))
timed("connect_s", lambda: lattice.connect(ConnectionRule.all_to_all(self_edges=False), WeightRule.uniform(0.5, 1.5, seed=2)))
network = timed("upload_s", lattice._ensure)                  # handle, neuron state, the graph by rule on the device
network.set_reduced_history(spike_counts=True)
timed("run_s", lambda: lattice.run_lattice(5))
for _ in range(5):
    timed("run_s", lambda: lattice.run_lattice(20))
total = time.perf_counter() - start
queries = {}
for name, call in (("get_weight_ms", lambda: lattice.get_weight((3, 4), (200, 17))),
                   ("get_incoming_connections_ms", lambda: lattice.get_incoming_connections((128, 128))),
                   ("get_outgoing_connections_ms", lambda: lattice.get_outgoing_connections((128, 128)))):
    t0 = time.perf_counter()
    answer = call()
    queries[name] = (time.perf_counter() - t0) * 1e3
    queries[name.replace("_ms", "_answer")] = answer if isinstance(answer, float) else len(answer)
cells = [c for row in lattice.cell_grid for c in row]
table = np.stack([np.array([c.current_voltage for c in cells], np.float32).view(np.uint32),
                  np.array([-1 if c.last_firing_time is None else c.last_firing_time for c in cells], np.int32).view(np.uint32),
                  np.array([c.is_spiking for c in cells], np.uint32), network.spike_counts(0).reshape(-1).astype(np.uint32)])
sha = hashlib.sha256(table.tobytes()).hexdigest()
rule_held = bool(lattice.rule_held)
lattice.close()
print(json.dumps({
    "workload": f"{rows}x{cols} lattice through IzhikevichNeuronLatticeGPU, {n} neurons, {4.0 * n * n / 1e9:.2f} GB matrix",
    **{k: round(v, 3) for k, v in phases.items()}, "total_s": round(total, 3), **queries,
    "ru_maxrss_MB": resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, "rule_held_after_the_runs": rule_held,
    "state_after_steps": 105, "state_sha256": sha,
    "bench_state_sha256": BENCH_STATE_SHA256 if (rows, cols) == (256, 256) else None,
    "state_equals_bench": (sha == BENCH_STATE_SHA256) if (rows, cols) == (256, 256) else None}))
