#!/usr/bin/env python3
"""What the edge-weight recorder (snn_set_edge_history, k_edge_history) costs per step, in two cases, each in one process on one
handle, recorder off and on alternating:

 (a) BASELINE configs[4] through connect_sparse (four 512x512 Izhikevich lattices, four Poisson lattices, 14.6 M edges), STDP on
     lattice 0, recording that lattice's internal edges (every stored edge inside it, in CSR order) at stride 1 and stride 10;
 (b) BASELINE configs[3], the 81 920-neuron dense STDP network, recording 10^4 random pairs -- what is paid there is mostly the step
     form: with a list installed the weight update is not deferred into the next input pass.

ms per step is a host clock around run(), which returns after the stream has drained.  Every window is preceded by a run of the
same length on the same settings (history buffers allocated, code loaded); three repeats, the median is quoted.  The recorder's
own bytes per recorded step: 16 B per pair (8 B offset + 4 B weight read, 4 B written); `recorder_share_of_8TBs` puts the extra time
per RECORDED step against them -- an end-to-end difference, not a kernel time.
No bar is set in advance.  Writes profiles/edge_history.json and prints it.  Usage: measure_edge_history.py [a|b|ab] [side]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import snn_amd  # noqa: E402
from snn_amd import ConnectionRule, synthetic  # noqa: E402

cases = sys.argv[1] if len(sys.argv) > 1 else "ab"
side = int(sys.argv[2]) if len(sys.argv) > 2 else 512
HBM_PEAK = 8.0e12
REPEATS = 3


def window(dn, steps):
    """ms per step of run(steps), after a run of the same length that leaves every buffer in place"""
    dn.run(steps)
    dn.reset_history()
    t0 = time.perf_counter()
    dn.run(steps)
    ms = (time.perf_counter() - t0) / steps * 1e3
    rows = dn.history_steps()
    dn.reset_history()
    return ms, rows


def measure(dn, pre, post, when, settings, steps):
    """settings: [(name, stride or None for "recorder off")]; alternating, REPEATS times"""
    seen = {name: [] for name, _ in settings}
    rows = {}
    for _ in range(REPEATS):
        for name, stride in settings:
            if stride is None:
                dn.set_edge_history([], [])
                dn.set_history_stride(1)
            else:
                dn.set_history_stride(stride)
                dn.set_edge_history(pre, post, when)
            ms, rows[name] = window(dn, steps)
            seen[name].append(ms)
            print(f"[measure_edge_history] {name}: {ms:.4f} ms/step, {rows[name]} rows", file=sys.stderr, flush=True)
    out = {}
    base = statistics.median(seen[settings[0][0]])
    for name, stride in settings:
        med = statistics.median(seen[name])
        out[name] = {"ms_per_step_median": round(med, 4), "ms_per_step_all": [round(x, 4) for x in seen[name]], "rows_recorded": rows[name]}
        if stride is not None:
            extra_per_row = (med - base) * steps / max(1, rows[name])            # ms per RECORDED step
            bytes_per_row = 16 * len(pre)
            out[name].update(extra_ms_per_step=round(med - base, 4), extra_ms_per_recorded_step=round(extra_per_row, 4),
                             recorder_bytes_per_recorded_step=bytes_per_row,
                             recorder_share_of_8TBs=(round(bytes_per_row / (extra_per_row * 1e-3) / HBM_PEAK, 4) if extra_per_row > 0 else None))
    return out


def case_a():
    m = side * side
    plan = ([(k, k, ConnectionRule.euclidean(4, self_edges=False), None) for k in range(4)] +
            [(k, (k + 1) % 4, ConnectionRule.same_position(), None) for k in range(4)] +
            [(4 + k, k, ConnectionRule.same_position(), None) for k in range(4)])
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
    dn.connect_sparse(plan)
    dn.set_plasticity(0)
    rp, pi = dn.graph_csr_structure()
    post = np.repeat(dn.owned, np.diff(rp.astype(np.int64)))
    first, count = dn.lattice_range(0)
    mine = (pi >= first) & (pi < first + count) & (post >= first) & (post < first + count)
    pre, post = pi[mine], post[mine]
    steps = 2000                                # (stride 1: 2000 rows of 12.5 MB)
    out = measure(dn, pre, post, 2, [("recorder_off", None), ("stride_1", 1), ("stride_10", 10)], steps)
    # the record of the last window against the weights as they are now: order 1, one step
    dn.set_history_stride(1)
    dn.set_edge_history(pre[:100000], post[:100000], 1)
    dn.run(1)
    w, c = dn.edge_history()
    now, on = dn.graph_lookup(pre[:100000], post[:100000])
    agrees = bool(np.array_equal(w[0].view(np.uint32), now.view(np.uint32)) and c.all() and on.all())
    dn.close()
    return {"workload": f"4 x ({side}x{side}) Izhikevich + 4 Poisson lattices, sparse handle, {int(pi.size)} edges, STDP on lattice 0; "
                        f"recorded: its {int(pre.size)} internal edges in CSR order, order 2",
            "pairs": int(pre.size), "steps_per_window": steps, **out, "last_row_equals_graph_lookup": agrees}


def case_b():
    n_inh, n_exc = 128 * 128, 256 * 256
    n = n_inh + n_exc
    dn = snn_amd.DeviceNetwork(model=snn_amd.IZHIKEVICH)
    dn.add_lattice(0, 128, 128)
    dn.add_lattice(1, 256, 256)
    dn.finalize()
    for i, count in ((0, n_inh), (1, n_exc)):
        dn.set_attr(i, "gap_conductance", np.full(count, 10.0, np.float32))
    dn.set_attr(0, "current_voltage", synthetic.uniform(4, n_inh, -65.0, 30.0))
    dn.set_attr(1, "current_voltage", synthetic.uniform(4, n_exc, -65.0, 30.0, offset=n_inh))
    dn.fill_graph_synthetic(5, 0.5, 1.5, with_diagonal=False)
    dn.set_plasticity(0)
    dn.set_plasticity(1)
    rng = np.random.default_rng(7)
    pre, post = rng.integers(0, n, 10000), rng.integers(0, n, 10000)
    steps = 250
    out = measure(dn, pre, post, 1, [("recorder_off", None), ("stride_1", 1)], steps)
    dn.close()
    return {"workload": f"256x256 + 128x128 Izhikevich lattices, dense matrix ({n} neurons), STDP on both; recorded: 10^4 random pairs, order 1",
            "pairs": 10000, "steps_per_window": steps, **out,
            "note": "with a list installed the STDP update runs as standalone passes at the end of the step instead of riding on the next "
                    "input pass (defer_stdp): what differs is the step form, the recorder itself moves 160 KB per step"}


result = {"hbm_peak_bytes_per_s": HBM_PEAK}
if "a" in cases:
    result["a_sparse_c5_internal_edges"] = case_a()
if "b" in cases:
    result["b_dense_c4_random_pairs"] = case_b()
text = json.dumps(result, indent=1)
if cases == "ab" and side == 512:
    with open(os.path.join(ROOT, "profiles", "edge_history.json"), "w") as f:
        f.write(text + "\n")
print(text)
