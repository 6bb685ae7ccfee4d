"""The 24-bit code and image layout of csrc/snn_w24.hpp on the host: tests/cpp/w24_codec.cpp includes the header alone and checks
the round trip of all 2^24 codes for three bases (0, 0x3F000000, a negative one), the encodability rule at spans 0, 0xFFFFFE and
0xFFFFFF, and that the byte index of (row, column) is a bijection onto the unpadded entries for ragged sizes (n_tot 5183 with ld
5184, n_tot 4101 with ld 4160).  Built twice: plain, and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spiking-neural-networks_amd", "csrc")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_w24_codec_round_trip_encodability_and_layout(tmp_path, flags):
    exe = tmp_path / "w24_codec"
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "w24_codec.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.strip().endswith("w24 codec ok"), r.stdout[-2000:]
