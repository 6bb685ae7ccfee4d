#!/usr/bin/env python3
"""What the voltage-peak record (snn_set_peak_history, k_peak_detect) costs, and what its readout saves.  Each row is measured in
this one process, as the median of REPEATS windows, record off and on alternating on one handle:

 (a) ms per step at the 256x256 headline lattice (BASELINE configs[0]: dense, gap junctions, weights U[0.5, 1.5]) and at 16x16,
     with the record off and on.  Off, the 16x16 handle takes the one-launch run; on, it takes one launch per step plus
     k_peak_detect -- what is paid there is mostly the step form.  No other history is on in either setting.
 (b) the readout of a 64x64 lattice after 2 000 recorded steps: peaks() of the device record against what the reference's
     experiments do -- download the [T, N] voltage history, scipy.signal.find_peaks per neuron, the threshold filter --, both
     giving the same lists (checked).

ms per step is a host clock around run(), which returns after the stream has drained; every window follows a run of the same length
on the same settings.  No bar is set in advance.  Writes profiles/peak_history.json and prints it.
Usage: measure_peak_history.py [side of the large lattice]"""
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


def note(text):
    print(f"[measure_peak_history] {text}", file=sys.stderr, flush=True)


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
    dn.reset_history()
    return ms


def step_cost(side, steps):
    dn = handle(side)
    seen = {"off": [], "on": []}
    launches = {}
    for _ in range(REPEATS):
        for name in ("off", "on"):
            dn.set_peak_history(0, THRESHOLD, enable=(name == "on"))
            before = dn.stat("persistent_run_launches")
            seen[name].append(window(dn, steps))
            launches[name] = dn.stat("persistent_run_launches") - before
            note(f"{side}x{side} record {name}: {seen[name][-1]:.4f} ms/step")
    dn.close()
    off, on = statistics.median(seen["off"]), statistics.median(seen["on"])
    return {"steps_per_window": steps, "repeats": REPEATS,
            "record_off": {"ms_per_step_median": round(off, 4), "ms_per_step_all": [round(x, 4) for x in seen["off"]],
                           "one_launch_run": launches["off"] > 0},
            "record_on": {"ms_per_step_median": round(on, 4), "ms_per_step_all": [round(x, 4) for x in seen["on"]],
                          "one_launch_run": launches["on"] > 0},
            "extra_ms_per_step": round(on - off, 4), "on_over_off": round(on / off, 3)}


def readout(side, steps):
    import scipy.signal
    n = side * side
    dn = handle(side)
    dn.set_history(voltage=True, spikes=False)
    dn.set_peak_history(0, THRESHOLD)
    dn.run(steps)
    device, host = [], []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        got = dn.peaks(0)
        device.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        history = dn.voltage_history(0).reshape(steps, n)
        download = (time.perf_counter() - t0) * 1e3
        want = []
        for i in range(n):
            series = history[:, i]
            found, _ = scipy.signal.find_peaks(series)
            want.append(found[series[found] > np.float32(THRESHOLD)])
        host.append((time.perf_counter() - t0) * 1e3)
        note(f"readout {side}x{side} x {steps}: device {device[-1]:.2f} ms, history + scipy {host[-1]:.2f} ms (download {download:.2f} ms)")
    equal = len(got) == n and all(np.array_equal(a, b) for a, b in zip(got, want))
    dn.close()
    d, h = statistics.median(device), statistics.median(host)
    return {"lattice": f"{side}x{side}", "recorded_steps": steps, "repeats": REPEATS, "peaks_found": int(sum(len(p) for p in want)),
            "same_lists": bool(equal), "device_record_peaks_ms_median": round(d, 3), "device_record_peaks_ms_all": [round(x, 3) for x in device],
            "history_download_and_scipy_ms_median": round(h, 3), "history_download_and_scipy_ms_all": [round(x, 3) for x in host],
            "history_bytes": steps * n * 4, "record_bytes": steps * ((n + 255) // 256 * 256) // 8, "speedup": round(h / d, 1)}


def box():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                                       # noqa: BLE001
        return "unknown"


out = {"box": box(), "threshold": THRESHOLD,
       "step_cost": {f"{large}x{large}": step_cost(large, 50), "16x16": step_cost(16, 2000)},
       "readout": readout(64, 2000)}
text = json.dumps(out)
if large == 256:
    with open(os.path.join(ROOT, "profiles", "peak_history.json"), "w") as f:
        f.write(text + "\n")
print(text)
