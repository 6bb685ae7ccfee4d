"""Register budget of the graph-query kernels (csrc/snn_kernels_graph_query.hpp): k_graph_lookup, k_graph_edit and both forms of
k_graph_line have no private segment -- no spilled register, no scratch -- and report their register counts.  Same recipe as
tests/test_isa_connect_csr.py: the kernel header compiled alone for gfx950 with -save-temps, the amdhsa.kernels notes read by
tests/isa_metadata.py.  Only metadata fields are read."""
import os
import subprocess

import pytest

import isa_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spiking-neural-networks_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ["snn::k_graph_lookup", "snn::k_graph_edit", "snn::k_graph_line<true>", "snn::k_graph_line<false>"]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_graph_query")
    src = d / "graph_query_only.hip"
    src.write_text(f'#include "{ROOT}/include/snn_amd.h"\n#include "snn_kernels_graph_query.hpp"\n'
                   "template __global__ void snn::k_graph_line<true>(const float *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t *, float *, uint32_t, uint32_t *);\n"
                   "template __global__ void snn::k_graph_line<false>(const float *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t *, float *, uint32_t, uint32_t *);\n"
                   "namespace snn { void *keep_lookup() { return (void *)k_graph_lookup; } void *keep_edit() { return (void *)k_graph_edit; } }\n")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only", "-Wno-unused-result",
                    "-Wno-pass-failed", "-save-temps", f"-I{CSRC}", "-o", "graph_query.o", src.name], cwd=d, check=True, capture_output=True)
    return isa_metadata.parse(str(d / "graph_query_only-hip-amdgcn-amd-amdhsa-gfx950.s"))


@pytest.mark.parametrize("name", KERNELS)
def test_no_private_segment(table, name):
    assert name in table, sorted(table)
    k = table[name]
    print(name, "vgpr", k["vgpr"], "agpr", k["agpr"], "sgpr", k["sgpr"])
    assert k["vgpr"] > 0, k
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
    assert k["max_threads"] == 256, k
