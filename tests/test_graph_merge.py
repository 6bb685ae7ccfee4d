"""The index arithmetic of a structural edit of a sparse graph (csrc/snn_graph_merge.hpp: the span of a row's edits, the merged
row length, the position of every old entry and of every inserting edit, last-wins ordering of the call):
tests/cpp/graph_merge_test.cpp includes the header alone, merges by its formulas and by a naive std::map, and compares -- every
old row over 6 presynaptic indices x every edit list of at most 3 edits, and random graphs with rows of 0 .. 300 entries and
0 .. 200 edits per row.  Built twice: plain, and under the address and undefined-behaviour sanitizers (a stand-alone program, run
directly)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spiking-neural-networks_amd", "csrc")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_merge_by_the_formulas_equals_the_naive_merge(tmp_path, flags):
    exe = tmp_path / "graph_merge"
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "graph_merge_test.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines == [f"graph merge ok: {64 * (1 + 12 + 144 + 1728)} exhaustive cases, 150 random graphs"], lines[-3:]


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_pair_list_check_and_last_wins_order_equal_their_naive_forms(tmp_path, flags):
    """csrc/snn_graph_pairs.hpp, included alone by tests/cpp/graph_pairs_test.cpp: the last-wins ordering of a call under both key
    orders against a std::map, and the walk over a pair list (first offender and its reason, strictly ascending or not) against a
    loop -- exhaustively over index ranges that straddle q0 and q0 + n_loc (q0 > 0 and post < q0 included), and random lists"""
    exe = tmp_path / "graph_pairs"
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "graph_pairs_test.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    orders, checks = 1 + 9 + 81 + 729 + 6561, 7 * (1 + 28 * 2 + 784 * 4 + 21952 * 8)
    assert r.stdout.splitlines() == [f"graph pairs ok: {orders} orderings and 200 random lists under both key orders, "
                                     f"{checks} exhaustive checks, 300 random lists"], r.stdout[-2000:]
