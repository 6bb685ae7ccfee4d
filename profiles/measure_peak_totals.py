#!/usr/bin/env python3
"""What the voltage-peak totals (snn_set_peak_totals) cost per step, next to the raster record (snn_set_peak_history): one
process, one handle per size, windows of the three settings alternating -- nothing on / totals on / raster record on --, REPEATS
windows each, medians and all values.  256x256 (BASELINE configs[0]: dense, gap junctions, weights U[0.5, 1.5]) in windows of 50
steps, 16x16 in windows of 2000 steps.  No other history is on.  The totals count into 8 windows from sample 1 on, the
experiments' shape (hd_model.py).

ms per step is a host clock around run(), which returns after the stream has drained; every window follows a run of the same length
on the same settings.  The only condition is one of form: with the totals on the 16x16 handle still takes the one-launch run.
Writes profiles/peak_totals.json and prints it.
Usage: measure_peak_totals.py [side of the large lattice]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import snn_amd  # noqa: E402
from snn_amd import synthetic  # noqa: E402

large = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPEATS = 5
THRESHOLD = 20.0
CASES = ("nothing", "totals", "raster")


def note(text):
    print(f"[measure_peak_totals] {text}", file=sys.stderr, flush=True)


def handle(side):
    n = side * side
    dn = snn_amd.DeviceNetwork(model=snn_amd.IZHIKEVICH)
    dn.add_lattice(0, side, side)
    dn.finalize()
    dn.set_attr(0, "gap_conductance", np.full(n, 10.0, np.float32))
    dn.set_attr(0, "current_voltage", synthetic.uniform(1, n, -65.0, 30.0))
    dn.fill_graph_synthetic(2, 0.5, 1.5, with_diagonal=False)
    dn.set_synapses(True, False)
    return dn


def window(dn, steps):
    dn.run(steps)
    dn.reset_history()
    t0 = time.perf_counter()
    dn.run(steps)
    ms = (time.perf_counter() - t0) / steps * 1e3
    counted = int(dn.peak_totals(0).sum()) if dn.peak_totals_steps() else None
    dn.reset_history()
    return ms, counted


def step_cost(side, steps):
    dn = handle(side)
    seen = {name: [] for name in CASES}
    launches, counted = {}, None
    for _ in range(REPEATS):
        for name in CASES:
            dn.set_peak_totals(0, THRESHOLD, origin=1, window=max(1, steps // 8), n_windows=8, enable=(name == "totals"))
            dn.set_peak_history(0, THRESHOLD, enable=(name == "raster"))
            before = dn.stat("persistent_run_launches")
            ms, c = window(dn, steps)
            seen[name].append(ms)
            counted = c if name == "totals" else counted
            launches[name] = dn.stat("persistent_run_launches") - before
            note(f"{side}x{side} {name}: {ms:.4f} ms/step")
    dn.close()
    med = {name: statistics.median(seen[name]) for name in CASES}
    out = {"steps_per_window": steps, "repeats": REPEATS, "peaks_counted_in_a_window": counted}
    for name in CASES:
        out[name] = {"ms_per_step_median": round(med[name], 4), "ms_per_step_all": [round(x, 4) for x in seen[name]],
                     "one_launch_run": launches[name] > 0}
    spread = max(seen["nothing"]) - min(seen["nothing"])
    out["totals_extra_ms_per_step"] = round(med["totals"] - med["nothing"], 4)
    out["totals_over_nothing"] = round(med["totals"] / med["nothing"], 3)
    out["raster_extra_ms_per_step"] = round(med["raster"] - med["nothing"], 4)
    out["raster_over_nothing"] = round(med["raster"] / med["nothing"], 3)
    out["spread_of_nothing_ms_per_step"] = round(spread, 4)
    return out


def box():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                                       # noqa: BLE001
        return "unknown"


out = {"box": box(), "threshold": THRESHOLD,
       "step_cost": {f"{large}x{large}": step_cost(large, 50), "16x16": step_cost(16, 2000)}}
assert out["step_cost"]["16x16"]["totals"]["one_launch_run"], "with the totals on the 16x16 handle must take the one-launch run"
text = json.dumps(out)
if large == 256:
    with open(os.path.join(ROOT, "profiles", "peak_totals.json"), "w") as f:
        f.write(text + "\n")
print(text)
