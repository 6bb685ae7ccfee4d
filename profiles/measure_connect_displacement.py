#!/usr/bin/env python3
"""snn_connect_by_spec / snn_connect_by_specs_csr with wrap-around and a displacement table, one process, median of 5 (wall time of
the blocking call):

dense, the headline size (256x256 Izhikevich lattice, 65 536 neurons, 17.18 GB matrix), three forms that stream the same bytes:
  (a) all-to-all without self edges, UNIFORM(0.5, 1.5): the case of measure_connect_rule.py, k_connect_rule;
  (b) all-to-all on the torus with a 256x256 displacement table (a bump of the toroidal distance): k_connect_spec, one table word
      read per element written;
  (c) Chebyshev 2 on the torus with the same table: almost every store is the absent-edge sentinel, 25 table reads per column.
  The bar: (b) takes no more than 2 x (a) in the same session.
sparse, BASELINE configs[4] (4 x side^2 neurons + 4 x side^2 Poisson cells, CSR), on a handle reset to the empty graph before
every run:
  (d) the twelve-record plan of measure_connect_rule_csr.py;
  (e) the same plan with the four within-lattice records made radius rules on the torus with a side x side table.
  No bar: the host commit of snn_set_graph_csr is in both.

Writes profiles/connect_displacement_256x256.json (or the path given) and prints it.
Usage: measure_connect_displacement.py [rows cols [side [output.json]]]"""
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
side = int(sys.argv[3]) if len(sys.argv) > 3 else 512
path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "connect_displacement_256x256.json")


def bump_table(n_rows, n_cols):
    """3 exp(-2 d^2 / (10 n)) - 0.9 of the toroidal distance d, indexed by the displacement modulo the grid"""
    u, v = np.arange(n_rows)[:, None], np.arange(n_cols)[None, :]
    d2 = np.minimum(u, n_rows - u) ** 2 + np.minimum(v, n_cols - v) ** 2
    return (3.0 * np.exp(-2.0 * d2 / (10.0 * max(n_rows, n_cols))) - 0.9).astype(np.float32)


def timed(call, before=None, repeats=5):
    runs = []
    for _ in range(repeats):
        if before:
            before()
        t0 = time.perf_counter()
        call()
        runs.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}


# ---- dense ----------------------------------------------------------------------------------------------------------------------
n = rows * cols
gbytes = 4.0 * n * n / 1e9
dn = snn_amd.DeviceNetwork(model=snn_amd.IZHIKEVICH)
dn.add_lattice(0, rows, cols)
dn.finalize()
weight = WeightRule.displacement(bump_table(rows, cols), wrap=True)
forms = {"all_uniform": (ConnectionRule.all_to_all(self_edges=False), WeightRule.uniform(0.5, 1.5, seed=2)),
         "all_wrapped_table": (ConnectionRule.all_to_all(self_edges=False, wrap=True), weight),
         "chebyshev2_wrapped_table": (ConnectionRule.chebyshev(2, self_edges=False, wrap=True), weight)}
dn.fill_graph_synthetic(2, 0.5, 1.5, with_diagonal=False)                     # (first touch of the matrix is nobody's time)
dense = {}
for name, (rule, w) in forms.items():
    dense[name] = timed(lambda: dn.connect_by_rule(0, 0, rule, w))
    dense[name]["GBps"] = gbytes / (dense[name]["median_ms"] * 1e-3)
# what the table form wrote, on one row and one column, against the host twin
sample = {"row": bool(np.array_equal(dn.graph_outgoing(n // 2 + 3)[0], np.nonzero(forms["chebyshev2_wrapped_table"][0].mask((rows, cols), (rows, cols), [n // 2 + 3], None)[0])[0]))}
dn.close()
ratio = dense["all_wrapped_table"]["median_ms"] / dense["all_uniform"]["median_ms"]

# ---- sparse ---------------------------------------------------------------------------------------------------------------------
m = side * side
between = ([(k, (k + 1) % 4, ConnectionRule.same_position(), None) for k in range(4)] +
           [(4 + k, k, ConnectionRule.same_position(), None) for k in range(4)])
plain = [(k, k, ConnectionRule.euclidean(4, self_edges=False), None) for k in range(4)] + between
torus_weight = WeightRule.displacement(bump_table(side, side), wrap=True)
torus = [(k, k, ConnectionRule.euclidean(4, self_edges=False, wrap=True), torus_weight) for k in range(4)] + between
sp = snn_amd.DeviceNetwork(model=snn_amd.IZHIKEVICH, spike_train=snn_amd.ST_POISSON)
for k in range(4):
    sp.add_lattice(k, side, side)
    sp.add_spike_train_lattice(4 + k, side, side)
sp.finalize(csr=True)
empty = (np.zeros(4 * m + 1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32))
sparse = {}
for name, plan in (("twelve_records", plain), ("twelve_records_torus_table", torus)):
    sparse[name] = timed(lambda: sp.connect_sparse(plan), before=lambda: sp.set_graph_csr(*empty))
    sparse[name]["edges"] = sp._nnz
sp.close()

out = {"dense_workload": f"{rows}x{cols} lattice, {n} neurons, {gbytes:.2f} GB matrix", "dense": dense,
       "table_over_uniform": ratio, "bar": 2.0, "within_bar": bool(ratio <= 2.0), "dense_sample_equals_host_twin": sample,
       "sparse_workload": f"4 x ({side}x{side}) Izhikevich lattices + 4 Poisson lattices, CSR, {4 * m} rows", "sparse": sparse}
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
