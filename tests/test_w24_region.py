"""The fit predicate of the region hand-over (csrc/snn_w24.hpp, w24_fits_matrix) on the host: tests/cpp/w24_region_test.cpp includes
the header alone, holds the predicate to a restatement of the layout for every n_tot of 1 .. 4200 and every ld of 64 .. 4224 in
steps of 64, and writes whole images into buffers of W's size whose slack holds a canary.  Built twice: plain, and as a stand-alone
program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spiking-neural-networks_amd", "csrc")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_w24_region_fit_predicate(tmp_path, flags):
    exe = tmp_path / "w24_region_test"
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "w24_region_test.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.strip().endswith("w24 region ok"), r.stdout[-2000:]
