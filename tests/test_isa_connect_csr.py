"""Register budget of the sparse connection-rule kernels (csrc/snn_kernels_connect_csr.hpp): every instantiation of k_connect_csr
-- 4 rules x 2 weight rules x thinning x self edges, for the counting and the filling pass, 64 in all -- and the export kernel
spill no register and use no scratch.  Same recipe as tests/test_isa_w24.py: the kernel header compiled alone for gfx950 with
-save-temps, the amdhsa.kernels notes read by tests/isa_metadata.py.  Only metadata fields are read."""
import itertools
import os
import subprocess

import pytest

import isa_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spiking-neural-networks_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BOOL = ("false", "true")
INSTANCES = [f"snn::k_connect_csr<{rule}, {weight}, {thin}, {self_}, {fill}>"
             for rule, weight, thin, self_, fill in itertools.product(range(4), range(2), BOOL, BOOL, BOOL)]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_connect_csr")
    src = d / "connect_csr_only.hip"
    inst = "\n".join(f"template __global__ void {name}(const snn::ConnectCsrArgs);" for name in INSTANCES)
    src.write_text(f'#include "{ROOT}/include/snn_amd.h"\n#include "snn_kernels_connect_csr.hpp"\n{inst}\n'
                   "namespace snn { void *keep_export() { return (void *)k_connect_csr_export; } }\n")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only", "-Wno-unused-result",
                    "-Wno-pass-failed", "-save-temps", f"-I{CSRC}", "-o", "connect_csr.o", src.name], cwd=d, check=True, capture_output=True)
    return isa_metadata.parse(str(d / "connect_csr_only-hip-amdgcn-amd-amdhsa-gfx950.s"))


def test_all_64_instantiations_and_the_export_kernel_are_in_the_code_object(table):
    assert len(INSTANCES) == 64
    missing = [n for n in INSTANCES + ["snn::k_connect_csr_export"] if n not in table]
    assert not missing, (missing[:4], sorted(k for k in table if "connect_csr" in k)[:4])


@pytest.mark.parametrize("name", INSTANCES + ["snn::k_connect_csr_export"])
def test_no_spill_and_no_scratch(table, name):
    k = table[name]
    assert k["vgpr"] > 0, k
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
    assert k["max_threads"] == 256, k


def test_vgpr_range_is_the_documented_one(table):
    """DESIGN.md section 4.13 records the range; a kernel that grows past it is worth a look before it spills"""
    regs = [table[n]["vgpr"] + table[n]["agpr"] for n in INSTANCES]
    print("k_connect_csr VGPRs:", min(regs), "..", max(regs), "export:", table["snn::k_connect_csr_export"]["vgpr"])
    assert max(regs) <= 64, max(regs)           # at least 8 wavefronts per SIMD (512 // registers)
