"""Register budget of the input pass over the 24-bit image (k_inputs_dense_w24, both instantiations): no spilled register, no
scratch, and at least the wavefronts per SIMD (512 // registers) of the plain pass over W of the same shape -- three for the
4-column shape, four for the 2-column shape.  Same recipe as tests/test_isa_resources.py: the kernel header compiled alone for
gfx950 with -save-temps, the amdhsa.kernels notes read by tests/isa_metadata.py."""
import os
import subprocess

import pytest

import isa_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spiking-neural-networks_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SHAPES = (1, 2)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_w24")
    src = d / "w24_only.hip"
    inst = "\n".join(f"template __global__ void snn::k_inputs_dense_w24<true, {s}>(const snn::InputsArgs, const snn::v4u *, uint32_t);\n"
                     f"template __global__ void snn::k_inputs_dense<true, false, {s}, 3, 0>(const snn::InputsArgs);" for s in SHAPES)
    src.write_text(f'#include "{ROOT}/include/snn_amd.h"\n#include "snn_kernels_inputs.hpp"\n{inst}\n')
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only", "-Wno-unused-result",
                    "-Wno-pass-failed", "-save-temps", f"-I{CSRC}", "-o", "w24.o", src.name], cwd=d, check=True, capture_output=True)
    return isa_metadata.parse(str(d / "w24_only-hip-amdgcn-amd-amdhsa-gfx950.s"))


@pytest.mark.parametrize("shape", SHAPES)
def test_the_image_pass_keeps_the_occupancy_of_the_plain_pass_without_spilling(table, shape):
    plain_name, image_name = f"snn::k_inputs_dense<true, false, {shape}, 3, 0>", f"snn::k_inputs_dense_w24<true, {shape}>"
    assert plain_name in table, sorted(table)                  # (a renamed plain pass must not let the comparison pass vacuously)
    assert image_name in table, sorted(table)
    plain, image = table[plain_name], table[image_name]
    assert plain["vgpr"] > 0 and plain["vgpr_spill"] == 0 and plain["scratch"] == 0, plain
    assert image["vgpr_spill"] == 0 and image["sgpr_spill"] == 0 and image["scratch"] == 0, image
    want = min(512 // plain["vgpr"], 3 if shape == 1 else 4)
    assert 512 // (image["vgpr"] + image["agpr"]) >= want, (image["vgpr"], image["agpr"], "plain", plain["vgpr"])
    assert image["max_threads"] == 256 and image["lds"] == plain["lds"], (image, plain)
