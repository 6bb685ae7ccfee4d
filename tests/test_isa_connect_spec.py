"""Register budget of the spec connection kernels (csrc/snn_kernels_connect.hpp: k_connect_spec; csrc/snn_kernels_connect_csr.hpp:
k_connect_csr_spec): every instantiation the dispatch can launch -- the displacement table with 4 rules x wrap x thinning x self
edges, the two distance rules on a ring with 2 weight rules x thinning x self edges; 48 dense, and 96 sparse for the counting and
the filling pass -- spills no register and uses no scratch, and the sparse ones stay within the 64 VGPRs the plain ones are held
to.  Same recipe as tests/test_isa_connect_csr.py: the kernel headers compiled alone for gfx950 with -save-temps, the
amdhsa.kernels notes read by tests/isa_metadata.py.  Only metadata fields are read."""
import itertools
import os
import subprocess

import pytest

import isa_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spiking-neural-networks_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BOOL = ("false", "true")
ALL, CHEBYSHEV, EUCLIDEAN, SAME_POSITION = range(4)
CONSTANT, UNIFORM, DISPLACEMENT = range(3)
# (rule, weight, wrap) of connect_spec_kernel / connect_csr_spec_kernel: whatever connect_spec_is_plain leaves to them
FORMS = ([(rule, DISPLACEMENT, wrap) for rule in range(4) for wrap in BOOL] +
         [(rule, weight, "true") for rule in (CHEBYSHEV, EUCLIDEAN) for weight in (CONSTANT, UNIFORM)])
DENSE = [f"snn::k_connect_spec<{rule}, {weight}, {thin}, {self_}, {wrap}>"
         for (rule, weight, wrap), thin, self_ in itertools.product(FORMS, BOOL, BOOL)]
SPARSE = [f"snn::k_connect_csr_spec<{rule}, {weight}, {thin}, {self_}, {wrap}, {fill}>"
          for (rule, weight, wrap), thin, self_, fill in itertools.product(FORMS, BOOL, BOOL, BOOL)]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_connect_spec")
    src = d / "connect_spec_only.hip"
    inst = "\n".join([f"template __global__ void {name}(const snn::ConnectSpecArgs);" for name in DENSE] +
                     [f"template __global__ void {name}(const snn::ConnectCsrSpecArgs);" for name in SPARSE])
    src.write_text(f'#include "{ROOT}/include/snn_amd.h"\n#include "snn_kernels_connect_csr.hpp"\n{inst}\n')
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only", "-Wno-unused-result",
                    "-Wno-pass-failed", "-save-temps", f"-I{CSRC}", "-o", "connect_spec.o", src.name], cwd=d, check=True, capture_output=True)
    return isa_metadata.parse(str(d / "connect_spec_only-hip-amdgcn-amd-amdhsa-gfx950.s"))


def test_every_instantiation_is_in_the_code_object(table):
    assert len(DENSE) == 48 and len(SPARSE) == 96
    missing = [n for n in DENSE + SPARSE if n not in table]
    assert not missing, (missing[:4], sorted(k for k in table if "spec" in k)[:4])


@pytest.mark.parametrize("name", DENSE + SPARSE)
def test_no_spill_and_no_scratch(table, name):
    k = table[name]
    assert k["vgpr"] > 0, k
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
    assert k["max_threads"] == 256, k


def test_sparse_vgpr_range_is_that_of_the_plain_kernels(table):
    regs = [table[n]["vgpr"] + table[n]["agpr"] for n in SPARSE]
    dense = [table[n]["vgpr"] + table[n]["agpr"] for n in DENSE]
    print("k_connect_csr_spec VGPRs:", min(regs), "..", max(regs), "k_connect_spec VGPRs:", min(dense), "..", max(dense))
    assert max(regs) <= 64, max(regs)           # at least 8 wavefronts per SIMD (512 // registers)
