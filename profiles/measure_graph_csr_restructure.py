#!/usr/bin/env python3
"""snn_graph_csr_edit_structure at BASELINE configs[4] full size (4 x 512^2 Izhikevich neurons + 4 x 512^2 Poisson cells, CSR,
14.6 M edges), one process on one MI355X: 1, 1 000 and 100 000 random structural edits (half remove a stored edge, half connect an
absent pair), median of 3 with the range.

(a) the new call.  The library prints the phases of a call to stderr when SNN_DEBUG_EDIT_TIMING is set (host clock around
    synchronised sections): resolve + merge (sort and upload of the list, resolve pass, scans, count and fill kernels), download
    (12 B per edge + 4 B per row) and the host builder (set_graph_csr_impl: SELL-64, transpose, plan, step image, uploads).  The
    call's wall time is taken from outside.
(b) the only route at the parent commit: graph_csr_structure() + get_graph_csr() (download), the edit in numpy on the nnz-sized
    arrays, set_graph_csr() (the same host builder).
Before every run the handle gets the unedited graph back (untimed).  (c) both routes end in the same graph, bit for bit.

Writes profiles/graph_csr_restructure.json and prints it.  Usage: measure_graph_csr_restructure.py [side]"""
import json
import os
import re
import statistics
import sys
import tempfile
import time

os.environ["SNN_DEBUG_EDIT_TIMING"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import snn_amd  # noqa: E402
from snn_amd import synthetic  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 512
m = side * side
REPEATS = 3
PHASES = re.compile(r"resolve\+merge ([0-9.]+) ms, download ([0-9.]+) ms, host builder ([0-9.]+) ms, carry ([0-9.]+) ms")


def c5_handle():
    dn = snn_amd.DeviceNetwork(model=snn_amd.IZHIKEVICH, spike_train=snn_amd.ST_POISSON)
    for k in range(4):
        dn.add_lattice(k, side, side)
        dn.add_spike_train_lattice(4 + k, side, side)
    dn.finalize(csr=True)
    return dn


def spread(runs):
    return {"median_ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}


def captured_stderr(call):
    """`call` with file descriptor 2 in a temporary file; returns what the library wrote there"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return f.read().decode()


def edits_for(rp, pi, n, rng):
    """n distinct pairs: every second a stored edge (removed), the others absent pairs (connected)"""
    n_rows, n_tot = rp.size - 1, 8 * m
    posts = np.repeat(np.arange(n_rows, dtype=np.uint32), np.diff(rp.astype(np.int64)))
    stored_key = posts.astype(np.uint64) * np.uint64(n_tot) + pi
    remove = rng.choice(pi.size, n // 2, replace=False)
    key = np.unique(rng.integers(0, n_rows * n_tot, 2 * n, dtype=np.uint64))
    key = key[~np.isin(key, stored_key)]
    key = key[rng.permutation(key.size)[:n - n // 2]]
    pre = np.concatenate([pi[remove], (key % np.uint64(n_tot)).astype(np.uint32)])
    post = np.concatenate([posts[remove], (key // np.uint64(n_tot)).astype(np.uint32)])
    on = np.concatenate([np.zeros(remove.size, bool), np.ones(key.size, bool)])
    order = rng.permutation(pre.size)
    return pre[order], post[order], rng.uniform(0.5, 1.5, pre.size).astype(np.float32)[order], on[order]


def numpy_edit(rp, pi, w, n_tot, pre, post, v, on):
    """the same edit on the host arrays: the route of the parent commit (distinct pairs: no order to respect)"""
    posts = np.repeat(np.arange(rp.size - 1, dtype=np.uint64), np.diff(rp.astype(np.int64)))
    key = posts * np.uint64(n_tot) + pi
    edit_key = post.astype(np.uint64) * np.uint64(n_tot) + pre
    keep = ~np.isin(key, edit_key)
    key = np.concatenate([key[keep], edit_key[on]])
    w = np.concatenate([w[keep], v[on]])
    order = np.argsort(key, kind="stable")
    key, w = key[order], w[order]
    counts = np.bincount((key // np.uint64(n_tot)).astype(np.int64), minlength=rp.size - 1)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), (key % np.uint64(n_tot)).astype(np.uint32), w


want = synthetic.c5_csr(side)
dn = c5_handle()
dn.set_graph_csr(*want)
out = {"workload": f"4 x ({side}x{side}) Izhikevich lattices + 4 Poisson lattices, CSR, {4 * m} rows, {int(want[1].size)} edges",
       "repeats": REPEATS, "edits": {}}
rng = np.random.default_rng(1)
for n in (1, 1000, 100000):
    pre, post, v, on = edits_for(want[0], want[1], n, rng)
    call, phases, old = [], {"resolve_and_merge": [], "download": [], "host_builder": [], "carry": []}, {"download": [], "numpy_edit": [], "set_graph_csr": []}
    for _ in range(REPEATS):
        dn.set_graph_csr(*want)
        t0 = time.perf_counter()
        text = captured_stderr(lambda: dn.graph_edit(pre, post, v, on, structure=True))
        call.append((time.perf_counter() - t0) * 1e3)
        found = PHASES.search(text)
        for name, value in zip(phases, found.groups()):
            phases[name].append(float(value))
    new_graph = (*dn.graph_csr_structure(), dn.get_graph_csr())
    for _ in range(REPEATS):
        dn.set_graph_csr(*want)
        t0 = time.perf_counter()
        rp, pi = dn.graph_csr_structure()
        w = dn.get_graph_csr()
        t1 = time.perf_counter()
        edited = numpy_edit(rp, pi, w, 8 * m, pre, post, v, on)
        t2 = time.perf_counter()
        dn.set_graph_csr(*edited)
        t3 = time.perf_counter()
        for name, value in zip(old, (t1 - t0, t2 - t1, t3 - t2)):
            old[name].append(value * 1e3)
    old_graph = (*dn.graph_csr_structure(), dn.get_graph_csr())
    same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(new_graph, old_graph))
    old_total = [sum(r) for r in zip(*old.values())]
    out["edits"][str(n)] = {"removes": int((~on).sum()), "connects": int(on.sum()), "edges_after": int(new_graph[1].size),
                            "a_new_call": {"wall": spread(call), **{k: spread(r) for k, r in phases.items()}},
                            "b_parent_route": {"wall": spread(old_total), **{k: spread(r) for k, r in old.items()}},
                            "c_same_graph": bool(same),
                            "new_call_over_parent_route": statistics.median(call) / statistics.median(old_total)}
dn.close()
text = json.dumps(out)
if side == 512:
    with open(os.path.join(ROOT, "profiles", "graph_csr_restructure.json"), "w") as f:
        f.write(text + "\n")
print(text)
