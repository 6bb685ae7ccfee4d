"""The C++ host mirror's spec calls (host/snn_lattice.hpp: LatticeNetworkGPU::connect(snn_connect_spec) on a dense handle,
::connect_sparse(std::vector<snn_connect_spec>) on a sparse one), driven from tests/cpp/connect_spec_test.cpp the way
tests/test_gpu_connect_rule_csr_cpp.py drives the older calls: the records of the ragged plan are written to a file from the
Python rules, the program prints digests of what it reads back, compared here with the per-pair restatement."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_connect_rule as dense_tests
import test_gpu_connect_rule_csr as csr_tests
import test_gpu_connect_spec as spec_tests

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return f"{int(np.float32(x).view(np.uint32)):x}"


def test_cpp_mirror_connects_by_spec(tmp_path, snn):
    from snn_amd import _lib
    records = tmp_path / "records.txt"
    with open(records, "w") as f:
        for pre, post, rule, weight in spec_tests.PLAN:
            table = np.zeros((0, 0), np.float32) if weight.table is None else weight.table
            f.write(f"{pre} {post} {rule.kind} {rule.extent} {int(rule.self_edges)} {bits(rule.probability)} {rule.seed} {weight.kind} "
                    f"{bits(weight.lo)} {bits(weight.hi)} {weight.seed} {rule.wrap} {table.shape[0]} {table.shape[1]}\n")
            f.write(" ".join(bits(x) for x in table.reshape(-1)) + "\n")
    exe = tmp_path / "connect_spec_test"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "connect_spec_test.cpp"),
                    "-L" + libdir, "-lsnn_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe), str(records)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    w, c = np.zeros((56, 50), np.float32), np.zeros((56, 50), np.uint32)
    spec_tests.apply_host(w, c, dense_tests.RAGGED, spec_tests.PLAN)
    dense = dense_tests.fnv1a(w.astype("<f4").tobytes() + c.astype("<u4").tobytes())
    row_ptr, pre_index, weights = csr_tests.csr_of(w, c, np.arange(50))
    sparse = dense_tests.fnv1a(row_ptr.astype("<u8").tobytes() + pre_index.astype("<u4").tobytes() + weights.astype("<f4").tobytes())
    assert 100 < pre_index.size == c.sum() < 56 * 50
    assert r.stdout.split() == ["dense", f"{dense:016x}", "edges", str(int(c.sum())), "sparse", f"{sparse:016x}", "nnz", str(pre_index.size)], r.stdout
