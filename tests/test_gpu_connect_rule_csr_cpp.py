"""The C++ host mirror on a sparse handle (host/snn_lattice.hpp: LatticeNetworkGPU::from_network_sparse, connect_sparse,
csr_structure, csr_weights), driven from tests/cpp/connect_sparse_test.cpp the way tests/test_gpu_cpp_host.py drives the others:
the program prints a digest of the CSR arrays, compared here with the per-pair expectation."""
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


def test_cpp_mirror_connects_a_sparse_handle(tmp_path, snn):
    from snn_amd import _lib
    exe = tmp_path / "connect_sparse_test"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "connect_sparse_test.cpp"),
                    "-L" + libdir, "-lsnn_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # lattices 0 and 1 (4x4 each: 0..15, 16..31), cells 32..47
    w, c = np.zeros((48, 32), np.float32), np.zeros((48, 32), bool)
    for i in range(16):
        if i % 4 != 3:                                  # the host's edges of lattice 0: (r, c) -> (r, c + 1), weight 3
            w[i, i + 1], c[i, i + 1] = 3.0, True
    blocks = [((0, 16), (16, 32), cases.expected_block((4, 4), (4, 4), cases.EUCLIDEAN, extent=2, probability=0.75, edge_seed=11,
                                                        weight_kind=cases.UNIFORM, lo=0.25, hi=1.75, weight_seed=5)),
              ((16, 32), (16, 32), cases.expected_block((4, 4), (4, 4), cases.CHEBYSHEV, extent=1, self_edges=False, lo=0.5)),
              ((32, 48), (16, 32), cases.expected_block((4, 4), (4, 4), cases.SAME_POSITION, lo=2.0))]
    for (p0, p1), (q0, q1), (on, ww) in blocks:
        c[p0:p1, q0:q1], w[p0:p1, q0:q1] = on, ww
    on = c.T
    row_ptr = np.concatenate([[0], np.cumsum(on.sum(axis=1))]).astype("<u8")
    pre = np.nonzero(on)[1].astype("<u4")
    weights = w.T[on].astype("<f4")
    assert 12 + 16 < pre.size < 12 + 16 * 9 + 16 * 8 + 16
    want = fnv1a(row_ptr.tobytes() + pre.tobytes() + weights.tobytes())
    assert r.stdout.split() == ["digest", f"{want:016x}", "edges", str(pre.size)], r.stdout
