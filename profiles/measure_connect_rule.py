#!/usr/bin/env python3
"""snn_connect_by_rule at the headline size (256x256 Izhikevich lattice, 65 536 neurons, 17.18 GB matrix):

* the call with rule ALL / no self edges / UNIFORM(0.5, 1.5) and the bench's graph seed, next to snn_fill_graph_synthetic on the
  same handle (the same store stream with the same hash per element) -- wall time of the blocking call, median of 5 each;
* CHEBYSHEV 2 with a CONSTANT weight at the same size (almost every store is the absent-edge sentinel), median of 5;
* the bench's 105 steps (warm-up 5 + 5 x 20) from the bench's initial state on the graph built BY RULE, and the sha256 of the
  state table bench.py hashes (voltage bits, last_firing_time, is_spiking, spike totals) next to the digest the bench records
  for the generator-built graph: equal digests say the headline configuration is reachable through the call with the
  reference's meaning.

Prints one JSON line.  Usage: measure_connect_rule.py [rows cols]"""
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

BENCH_STATE_SHA256 = "c91f01a99e0fbb7d7bb8672dad90b71ae6584e1667a258bc22a959e3c9371743"      # BENCH_r06.json, after 105 steps

rows, cols = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (256, 256)
n = rows * cols
dn = snn_amd.DeviceNetwork(model=snn_amd.IZHIKEVICH)
dn.add_lattice(0, rows, cols)
dn.finalize()
dn.set_attr(0, "gap_conductance", np.full(n, 10.0, np.float32))
dn.set_attr(0, "current_voltage", synthetic.uniform(1, n, -65.0, 30.0))


def median_ms(call, repeats=5):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), times


all_uniform = (ConnectionRule.all_to_all(self_edges=False), WeightRule.uniform(0.5, 1.5, seed=2))
near_constant = (ConnectionRule.chebyshev(2, self_edges=False), WeightRule.constant(1.0))
dn.fill_graph_synthetic(2, 0.5, 1.5, with_diagonal=False)                     # (first touch of the matrix is nobody's time)
generator_ms, generator_runs = median_ms(lambda: dn.fill_graph_synthetic(2, 0.5, 1.5, with_diagonal=False))
near_ms, near_runs = median_ms(lambda: dn.connect_by_rule(0, 0, *near_constant))
rule_ms, rule_runs = median_ms(lambda: dn.connect_by_rule(0, 0, *all_uniform))     # (last: the graph the steps below run on)

dn.set_reduced_history(False, False, True)
dn.run(5)
for _ in range(5):
    dn.run(20)
table = np.stack([dn.get_attr(0, "current_voltage").view(np.uint32), dn.get_attr(0, "last_firing_time", dtype=np.int32).view(np.uint32),
                  dn.get_attr(0, "is_spiking", dtype=np.uint32), dn.spike_counts(0).astype(np.uint32)])
sha = hashlib.sha256(table.tobytes()).hexdigest()
gbytes = 4.0 * n * n / 1e9
print(json.dumps({
    "workload": f"{rows}x{cols} lattice, {n} neurons, {gbytes:.2f} GB matrix",
    "connect_by_rule_all_uniform_ms": rule_ms, "connect_by_rule_all_uniform_runs_ms": rule_runs,
    "fill_graph_synthetic_ms": generator_ms, "fill_graph_synthetic_runs_ms": generator_runs,
    "rule_over_generator": rule_ms / generator_ms,
    "connect_by_rule_all_uniform_GBps": gbytes / (rule_ms * 1e-3), "fill_graph_synthetic_GBps": gbytes / (generator_ms * 1e-3),
    "connect_by_rule_chebyshev2_constant_ms": near_ms, "connect_by_rule_chebyshev2_constant_runs_ms": near_runs,
    "connect_by_rule_chebyshev2_constant_GBps": gbytes / (near_ms * 1e-3),
    "state_after_steps": 105, "state_sha256": sha,
    "bench_state_sha256": BENCH_STATE_SHA256 if (rows, cols) == (256, 256) else None,
    "state_equals_bench": (sha == BENCH_STATE_SHA256) if (rows, cols) == (256, 256) else None}))
dn.close()
