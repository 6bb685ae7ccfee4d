"""Register and LDS budget of the factored-weight connection kernels (csrc/snn_kernels_connect_factors.hpp: k_connect_factors,
k_connect_csr_factors): every instantiation the dispatch can launch -- 4 rules x thinning x self edges; 16 dense, and 32 sparse
for the counting and the filling pass -- spills no register and uses no scratch, and the LDS of each lets at least two workgroups
share a CU (160 KiB of LDS on gfx950).  Same recipe as tests/test_isa_connect_spec.py: the kernel header compiled alone for
gfx950 with -save-temps, the amdhsa.kernels notes read by tests/isa_metadata.py.  Only metadata fields are read.

Recorded (ROCm 7.2): k_connect_factors 88 .. 94 VGPRs (26 for position-to-position without self edges, which writes None
everywhere and sums nothing), 69 632 bytes of LDS (the 64 KiB V tile and the 4 KiB U tile): the LDS, not the registers, sets its
two workgroups per CU = two wavefronts per SIMD; k_connect_csr_factors 16 .. 54 VGPRs, 4 096 bytes."""
import itertools
import os
import subprocess

import pytest

import isa_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spiking-neural-networks_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BOOL = ("false", "true")
LDS_PER_CU = 160 * 1024
# (rule, thin, self) of connect_factors_kernel / connect_csr_factors_kernel
DENSE = [f"snn::k_connect_factors<{rule}, {thin}, {self_}>" for rule, thin, self_ in itertools.product(range(4), BOOL, BOOL)]
SPARSE = [f"snn::k_connect_csr_factors<{rule}, {thin}, {self_}, {fill}>"
          for rule, thin, self_, fill in itertools.product(range(4), BOOL, BOOL, BOOL)]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_connect_factors")
    src = d / "connect_factors_only.hip"
    inst = "\n".join([f"template __global__ void {name}(const snn::ConnectFactorsArgs);" for name in DENSE] +
                     [f"template __global__ void {name}(const snn::ConnectCsrFactorsArgs);" for name in SPARSE])
    src.write_text(f'#include "{ROOT}/include/snn_amd.h"\n#include "snn_kernels_connect_factors.hpp"\n{inst}\n')
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only", "-Wno-unused-result",
                    "-Wno-pass-failed", "-save-temps", f"-I{CSRC}", "-o", "connect_factors.o", src.name], cwd=d, check=True, capture_output=True)
    return isa_metadata.parse(str(d / "connect_factors_only-hip-amdgcn-amd-amdhsa-gfx950.s"))


def test_every_instantiation_is_in_the_code_object(table):
    assert len(DENSE) == 16 and len(SPARSE) == 32
    missing = [n for n in DENSE + SPARSE if n not in table]
    assert not missing, (missing[:4], sorted(k for k in table if "factors" in k)[:4])


@pytest.mark.parametrize("name", DENSE + SPARSE)
def test_no_spill_no_scratch_and_two_workgroups_per_cu(table, name):
    k = table[name]
    assert k["vgpr"] > 0, k
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
    assert k["max_threads"] == 256, k
    assert 2 * k["lds"] <= LDS_PER_CU, (name, k["lds"])
    # ... and the registers allow as many: two workgroups of 256 threads are two wavefronts per SIMD (512 // registers >= 2)
    assert k["vgpr"] + k["agpr"] <= 256, (name, k)


def test_vgpr_and_lds_ranges(table):
    dense = [table[n]["vgpr"] + table[n]["agpr"] for n in DENSE]
    sparse = [table[n]["vgpr"] + table[n]["agpr"] for n in SPARSE]
    print("k_connect_factors VGPRs:", min(dense), "..", max(dense), "LDS:", sorted({table[n]["lds"] for n in DENSE}),
          "k_connect_csr_factors VGPRs:", min(sparse), "..", max(sparse), "LDS:", sorted({table[n]["lds"] for n in SPARSE}))
    assert {table[n]["lds"] for n in DENSE} == {32 * 256 * 8 + 32 * 16 * 8}      # FACTOR_CHUNK x 256 columns + FACTOR_CHUNK x FACTOR_TILE_ROWS
    assert {table[n]["lds"] for n in SPARSE} == {4 * 128 * 8}                    # FACTOR_CSR_CHUNK doubles per wavefront
    assert max(sparse) <= 64, max(sparse)         # at least 8 wavefronts per SIMD, as the plain sparse kernels are held to
