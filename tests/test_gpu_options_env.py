"""The environment reaches a handle through the option table when it is created, and the statistics table answers every name:
a 16x16 Izhikevich lattice with dense gap junctions, 8 steps, each case in a fresh child process with the variables in ITS
environment (the parent's own is never edited), compared with the oracle's raster."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

from test_abi import STATISTICS

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu

CHILD = textwrap.dedent("""
    import json, os, sys
    sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.dirname(sys.argv[1]))
    import conftest                                   # OpenMP settings of the oracle
    import numpy as np
    import snn_amd
    snn_amd._lib.load()
    import oracle_binding as ob
    import parity
    net = parity.make_oracle(parity.Layout([(0, 16, 16)]), model=ob.IZHIKEVICH)
    net["gap_conductance"] = 10.0
    net["current_voltage"] = ob.uniform_array(1, net.n_neurons, 20.0, 30.0)       # close to the peak: spikes in every one of the 8 steps
    net.fill_graph(2, 0.5, 1.5)
    dn = parity.device_from_oracle(snn_amd, net)
    dn.set_history(voltage=False, spikes=True)
    dn.run(8)
    net.run(8, spike_history=True)
    stats = {}
    for name in json.loads(sys.argv[2]):
        stats[name] = dn.stat(name)                   # (raises unless snn_get_stat returned SNN_OK)
    try:
        dn.stat("no_such_statistic")
        unknown = 0
    except snn_amd.SnnError as e:
        unknown = e.code
    print(json.dumps({"raster_equal": bool(np.array_equal(dn.spike_history(0), net.spike_history)),
                      "spikes": int(net.spike_history.sum()), "stats": stats, "unknown": unknown}))
    dn.close()
""")


def run_child(tmp_path, **variables):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SNN_AMD_")}
    env.update(variables)
    p = subprocess.run([sys.executable, str(script), HERE, json.dumps(sorted(STATISTICS))], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["raster_equal"] and res["spikes"] > 0, res
    assert set(res["stats"]) == STATISTICS and res["unknown"] == 11, res            # 11: SNN_ERR_BAD_ARG
    return res["stats"]


def test_nothing_set_takes_the_one_launch_run(tmp_path):
    s = run_child(tmp_path)
    assert s["persistent_run_launches"] == 1 and s["persistent_run_steps"] == 8 and s["steps_two_kernel"] == 0, s


def test_persistent_run_switched_off_by_the_environment(tmp_path):
    s = run_child(tmp_path, SNN_AMD_PERSISTENT_RUN="0")
    assert s["persistent_run_launches"] == 0 and s["persistent_run_steps"] == 0 and s["steps_dense_one_launch"] == 8, s


def test_fused_step_and_persistent_run_switched_off_by_the_environment(tmp_path):
    s = run_child(tmp_path, SNN_AMD_FUSED_STEP="0", SNN_AMD_PERSISTENT_RUN="0")
    assert s["persistent_run_launches"] == 0 and s["steps_two_kernel"] == 8 and s["steps_dense_one_launch"] == 0, s
