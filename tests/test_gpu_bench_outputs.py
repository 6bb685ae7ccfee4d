"""`bench.py --dump-outputs DIR` on the device: a plain run (--steps steps timed once, headline keys only) writes the state its
timed steps leave, and that state is the one `--full` vouches for with state_sha256 after the same number of steps."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def bench(*flags, gpus=1):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "12", "--warmup", "4",
           "--spike-fraction", "0.002", *flags]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()))
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def load(d, names):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in names}


@pytest.mark.timeout(1200)
def test_plain_run_dumps_the_state_full_checksums(tmp_path):
    small = ["--config", "c2", "--rows", "96", "--cols", "96"]
    plain = bench(*small, "--dump-outputs", str(tmp_path / "plain"))
    assert all(k in plain for k in HEADLINE) and plain["repeats"] == 1 and plain["steps"] == 12
    assert "state_sha256" not in plain and "roofline" not in plain and "cpu_baseline" not in plain
    assert plain["outputs"]["after_steps"] == 4 + 12
    state = load(tmp_path / "plain", ["voltage", "last_firing_time", "is_spiking", "spike_count"])
    assert state["voltage"].dtype == np.float32 and state["voltage"].shape == (96 * 96,)
    assert state["spike_count"].sum() > 0
    full = bench(*small, "--full", "--repeats", "1", "--no-cpu-baseline")
    assert full["state_after_steps"] == 4 + 12 and "roofline" in full
    table = np.stack([state["voltage"].view(np.uint32), state["last_firing_time"].astype(np.int32).view(np.uint32),
                      state["is_spiking"].astype(np.uint32), state["spike_count"].astype(np.uint32)])
    assert hashlib.sha256(table.tobytes()).hexdigest() == full["state_sha256"]


@pytest.mark.timeout(1200)
def test_plastic_run_dumps_the_same_weight_sample_twice(tmp_path):
    small = ["--config", "c6", "--rows", "64", "--cols", "64"]
    names = ["voltage", "last_firing_time", "is_spiking", "spike_count", "weight_rows_sample", "trace_rows_sample"]
    for d in ("a", "b"):
        line = bench(*small, "--dump-outputs", str(tmp_path / d))
        assert sorted(line["outputs"]["arrays"]) == sorted(names)
    a, b = load(tmp_path / "a", names), load(tmp_path / "b", names)
    assert a["weight_rows_sample"].shape == (32, 64 * 64) and np.isfinite(a["weight_rows_sample"]).all()
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in names)


@pytest.mark.timeout(1800)
def test_dumps_do_not_depend_on_how_the_network_is_sharded(tmp_path):
    """the gathers behind --dump-outputs: two ranks (processes on one GPU) write what one rank writes, and the sharded code
    path at world size one writes what the plain one does, the weight sample of a plastic config included"""
    state = ["voltage", "last_firing_time", "is_spiking", "spike_count"]
    c5 = ["--config", "c5", "--rows", "48"]
    bench(*c5, "--dump-outputs", str(tmp_path / "c5_one"))
    bench(*c5, "--emulate-ranks-on-one-gpu", "--dump-outputs", str(tmp_path / "c5_two"), gpus=2)
    a, b = load(tmp_path / "c5_one", state), load(tmp_path / "c5_two", state)
    assert a["spike_count"].shape == (4 * 48 * 48,) and a["spike_count"].sum() > 0
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in state)
    names = state + ["weight_rows_sample"]
    bench("--config", "c4", "--dump-outputs", str(tmp_path / "c4_plain"))
    bench("--config", "c4", "--force-sharded", "--dump-outputs", str(tmp_path / "c4_sharded"))
    a, b = load(tmp_path / "c4_plain", names), load(tmp_path / "c4_sharded", names)
    assert a["weight_rows_sample"].shape == (32, 81920)
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in names)
