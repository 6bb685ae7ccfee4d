"""The host-built half of the sparse step image (csrc/snn_step_image_plan.hpp: slice headers, window pieces cut greedily, plan
words with 16-bit window offsets): tests/cpp/step_image_plan_test.cpp includes the header alone, fills a 1024-word window from
the pieces exactly as the kernel's LDS-DMA loop does, walks every entry's plan word and compares with a direct gather and a naive
restatement of the cut over a std::set -- every subset of 14 sources around the neuron | cell | receive-buffer boundaries and the
span ends, directed slices (the window exactly full and one source more, 512 cells up to the last cell of the array and 513,
pieces with gaps, trimmed pieces, empty slices in the middle and at the end), random networks.  Built twice: plain, and under
the address and undefined-behaviour sanitizers (a stand-alone program, run directly)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spiking-neural-networks_amd", "csrc")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_the_window_the_plan_describes_holds_every_entrys_source(tmp_path, flags):
    exe = tmp_path / "step_image_plan"
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "step_image_plan_test.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.splitlines() == [f"step image plan ok: {2 ** 14 + 2 ** 8} exhaustive subsets, 32 directed slices, 400 random networks, "
                                     "18041 slices in all"], r.stdout[-2000:]
