"""The C++ host mirror's Graph-trait forwarders (host/snn_lattice.hpp: LatticeNetworkGPU::lookup_weight, edit_weight,
incoming_connections, outgoing_connections), driven from tests/cpp/graph_query_test.cpp the way tests/test_gpu_connect_rule_csr_cpp.py
drives the sparse ones: the program holds every query to the rows itself and prints a digest of the rows after its edits, compared
here with the per-pair expectation."""
import os
import subprocess

import numpy as np
import pytest

import connect_rule_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fnv1a(data):
    h = 0xcbf29ce484222325
    for byte in data:
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_mirror_queries_and_edits_the_device_graph(tmp_path, snn):
    from snn_amd import _lib
    exe = tmp_path / "graph_query_test"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "graph_query_test.cpp"),
                    "-L" + libdir, "-lsnn_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    on, w = cases.expected_block((4, 4), (4, 4), cases.EUCLIDEAN, extent=2, self_edges=False, probability=0.75, edge_seed=11,
                                 weight_kind=cases.UNIFORM, lo=0.25, hi=1.75, weight_seed=5)
    on, w = on.copy(), w.copy()
    assert not on[0, 0] and not on[15, 3]
    on[0, 0], w[0, 0] = True, 2.5
    on[15, 3], w[15, 3] = True, -1.0
    on[5, 5], w[5, 5] = False, 0.0
    want = fnv1a(w.astype("<f4").tobytes() + on.astype("<u4").tobytes())
    assert r.stdout.split() == ["digest", f"{want:016x}", "edges", str(int(on.sum()))], r.stdout
