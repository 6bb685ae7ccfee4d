"""The region hand-over of the 24-bit image (ensure_w24, csrc/snn_network_step.hpp): the image of a static matrix takes over the
allocation W's placement search chose, and W moves to a fresh one.  71 x 73 lattice (5183 neurons, W 107 MB), the hand-over's 1 GiB
threshold lowered by SNN_AMD_W24_REGION_MIN around handle creation, the library's SNN_DEBUG_PLACEMENT lines read from file
descriptor 2.  Every outcome is compared bit for bit: with a handle created under SNN_AMD_W24=0 (the pass over W, no image, no
hand-over) that is given the same calls, and -- the plain run -- with the oracle.

The issue's allocation-failure case names two allocations and one expectation ("no hand-over").  It is read here as: a failure
of the hand-over's own allocation leaves no hand-over line; a failure of the fresh candidate's leaves the hand-over in place and
no candidate line; in both the handle runs on with identical results."""
import contextlib
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import parity
from test_gpu_dense_w24 import LATTICE, assert_equals_oracle, assert_same, static_net

pytestmark = pytest.mark.gpu

STEPS = 30
MOVED_OUT, MOVED_BACK, PACKED_AGAIN, CANDIDATE = "W moves out of", "W moves back from", "packed again into", "image placement: held"
# After a hand-over one fresh allocation is still timed against W's region (1 % rule).  At this size either may win, so the tests
# hold under both verdicts: a fresh winner sends W back into its region at once ("W moves back"), and the image stays fresh.


@contextlib.contextmanager
def environ(**values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update({k: v for k, v in values.items() if v is not None})
    for k, v in values.items():
        if v is None:
            os.environ.pop(k, None)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class PlacementLog:
    """file descriptor 2 redirected into a file while the block runs (the library writes with fprintf(stderr))"""

    def __enter__(self):
        self.file = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.file.fileno(), 2)
        self.seen = 0
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.text = self._read(0)
        self.file.close()
        os.write(2, self.text.encode())                     # what was captured still reaches the test's own stderr
        return False

    def _read(self, start):
        self.file.seek(start)
        return self.file.read().decode(errors="replace")

    def new_lines(self):
        """the lines written since the last call"""
        text = self._read(self.seen)
        self.seen += len(text.encode())
        return [ln for ln in text.splitlines() if ln.startswith("[snn]")]


def count(lines, what):
    return sum(what in ln for ln in lines)


def create(snn, net, image=True, region=True, shape=0):
    with environ(SNN_AMD_W24="1" if image else "0", SNN_AMD_W24_REGION="1" if region else "0",
                 SNN_AMD_W24_REGION_MIN=str(1 << 20), SNN_DEBUG_PLACEMENT="1"):
        dn = parity.device_from_oracle(snn, net)
    if shape:
        dn.set_option("input_shape", shape)
    dn.set_history(voltage=True, spikes=True)
    return dn


def outcome(dn, net):
    out = {"state": parity.pull_state(dn, net), "bytes": dn.input_kernel_bytes()}
    for i, _, _ in net.layout.lattices:
        out[("v", i)] = dn.voltage_history(i)
        out[("s", i)] = dn.spike_history(i)
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """the lattice and its oracle outcome after STEPS steps, computed once (the device never writes into either)"""
    net, ref = static_net(LATTICE, [], 21), static_net(LATTICE, [], 21)
    ref.run(STEPS, voltage_history=True, spike_history=True)
    assert ref.spike_history.sum() > 0
    return net, ref


@functools.lru_cache(maxsize=None)
def w_outcome(shape):
    """the same steps on a handle that reads W (SNN_AMD_W24=0), once per shape"""
    import snn_amd
    net, _ = reference()
    dn = create(snn_amd, net, image=False, shape=shape)
    dn.run(STEPS)
    out = outcome(dn, net)
    dn.close()
    return out


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("shape", [1, 2], ids=["shape_1", "shape_2"])
def test_hand_over_equals_w_handle_and_oracle(snn, shape):
    net, ref = reference()
    n = net.n_tot * net.n_neurons
    with environ(SNN_DEBUG_PLACEMENT="1"), PlacementLog() as log:
        dn = create(snn, net, shape=shape)
        dn.run(STEPS)
        lines = log.new_lines()
        a = outcome(dn, net)
        parity.assert_graph_equal(net, dn)                  # every row of W as it was set: W moved intact
        assert log.new_lines() == []                        # (reading W back moves nothing)
        dn.close()
    stays = [ln for ln in lines if "the image stays in" in ln]
    assert count(lines, MOVED_OUT) == 1 and len(stays) == 1, lines
    assert count(lines, MOVED_BACK) == (0 if "W's region" in stays[0] else 1), lines
    b = w_outcome(shape)
    assert (a["bytes"], b["bytes"]) == (3 * n, 4 * n)
    assert_same(a, b)
    assert_equals_oracle(ref, a)


def test_switch_off_keeps_a_fresh_image(snn):
    net, ref = reference()
    n = net.n_tot * net.n_neurons
    with environ(SNN_DEBUG_PLACEMENT="1"), PlacementLog() as log:
        dn = create(snn, net, region=False)
        dn.run(STEPS)
        lines = log.new_lines()
        a = outcome(dn, net)
        dn.close()
    assert count(lines, "image region") == 0, lines
    assert a["bytes"] == 3 * n
    assert_same(a, w_outcome(0))
    assert_equals_oracle(ref, a)


def both(snn, net):
    return create(snn, net), create(snn, net, image=False)


def assert_handles_agree(a, b, net):
    assert_same(outcome(a, net), outcome(b, net))


def test_row_edit_packs_again_into_the_kept_region(snn):
    net, _ = reference()
    n = net.n_tot * net.n_neurons
    conns = net["connections"].astype(np.uint32)
    rows = (net["weights"][1000:1003].astype(np.float32) * np.float32(0.75) + np.float32(0.25) * conns[1000:1003].astype(np.float32))
    assert rows.dtype == np.float32                             # still within [0.5, 1.5): the matrix stays encodable
    with environ(SNN_DEBUG_PLACEMENT="1"), PlacementLog() as log:
        a, b = both(snn, net)
        a.run(10)
        b.run(10)
        first = log.new_lines()
        for dn in (a, b):
            dn.set_graph_rows(1000, rows, conns[1000:1003])
            dn.run(10)
        second = log.new_lines()
        assert a.input_kernel_bytes() == 3 * n and b.input_kernel_bytes() == 4 * n
        assert_handles_agree(a, b, net)
        wa, ca = a.get_graph_rows(0, net.n_tot)
        wb, cb = b.get_graph_rows(0, net.n_tot)
        assert np.array_equal(parity.bits(wa), parity.bits(wb)) and np.array_equal(ca, cb)
        assert np.array_equal(parity.bits(wa[1000:1003]), parity.bits(np.where(conns[1000:1003] != 0, rows, np.float32(0))))
        a.close()
        b.close()
    assert count(first, MOVED_OUT) == 1, first
    assert count(second, PACKED_AGAIN) == 1 and count(second, MOVED_OUT) == 0 and count(second, MOVED_BACK) == 0, second
    if count(first, MOVED_BACK) == 0:
        assert "W's region" in [ln for ln in second if PACKED_AGAIN in ln][0], second


def test_plasticity_brings_w_back_into_its_region(snn):
    net, _ = reference()
    n = net.n_tot * net.n_neurons
    v = np.array(net["current_voltage"], np.float32)
    v[::89] = np.float32(35.0)                                  # spikes in the plastic stretch: weights that move
    v2 = v.copy()
    v2[::89] = np.float32(-65.0)
    v2[1::89] = np.float32(35.0)
    with environ(SNN_DEBUG_PLACEMENT="1"), PlacementLog() as log:
        a, b = both(snn, net)
        a.run(10)
        b.run(10)
        first = log.new_lines()
        for dn in (a, b):
            dn.set_attr(0, "current_voltage", v)
            dn.set_plasticity(0, float(net["stdp_a_plus"][0]), float(net["stdp_a_minus"][0]), float(net["stdp_tau_plus"][0]),
                              float(net["stdp_tau_minus"][0]), float(net["stdp_dt"][0]), True)
            dn.run(5)
            dn.set_attr(0, "current_voltage", v2)               # a second group fires five steps after the first: pairs for the rule
            dn.run(5)
        second = log.new_lines()
        assert a.input_kernel_bytes() == 4 * n and b.input_kernel_bytes() == 4 * n
        assert_handles_agree(a, b, net)
        wa, ca = a.get_graph_rows(0, net.n_tot)
        wb, cb = b.get_graph_rows(0, net.n_tot)
        assert np.array_equal(parity.bits(wa), parity.bits(wb)) and np.array_equal(ca, cb)
        assert not np.array_equal(parity.bits(wa), parity.bits(np.where(ca != 0, net["weights"], np.float32(0)))), "no weight moved"
        a.close()
        b.close()
    out = [ln for ln in first if MOVED_OUT in ln]
    back = [ln for ln in first + second if MOVED_BACK in ln]
    assert len(out) == 1 and len(back) == 1 and count(second, MOVED_OUT) == 0, (first, second)
    # "W moves out of <region> to ..." and "... back from ... into its region <region>": the same address
    assert out[0].split(MOVED_OUT)[1].split()[0] == back[0].split("into its region")[1].split()[0].rstrip(","), (out, back)


def test_checkpoint_restore_after_the_hand_over(snn):
    net, _ = reference()
    with environ(SNN_DEBUG_PLACEMENT="1"), PlacementLog() as log:
        a, b = both(snn, net)
        for dn in (a, b):
            dn.run(10)
            dn.checkpoint()
            dn.run(10)
        once = outcome(a, net)
        assert_same(once, outcome(b, net))
        for dn in (a, b):
            dn.restore_checkpoint()
            dn.run(10)
        again = outcome(a, net)
        lines = log.new_lines()
        assert_same(again, outcome(b, net))
        for name in once["state"]:
            assert np.array_equal(parity.bits(once["state"][name]), parity.bits(again["state"][name])), name
        parity.assert_graph_equal(net, a)
        a.close()
        b.close()
    assert count(lines, MOVED_OUT) == 1 and count(lines, MOVED_BACK) <= 1, lines


def arm(snn, n):
    seen = C.c_uint64()
    snn._lib.check(snn._lib.load().snn_debug_fail_alloc_at(int(n), C.byref(seen)))
    return int(seen.value)


def test_failed_allocations_leave_the_handle_running(snn):
    """the n-th allocation of the first run fails, for n = 1, 2, ... until both the hand-over's allocation and the fresh
    candidate's have been hit (told apart by the lines): the run either reports the failure or, where it goes through, computes
    what the W handle computes"""
    net, _ = reference()
    want = w_outcome(0)
    hit_hand_over = hit_candidate = False
    with environ(SNN_DEBUG_PLACEMENT="1"), PlacementLog() as log:
        for nth in range(1, 13):
            dn = create(snn, net)
            arm(snn, nth)
            try:
                dn.run(STEPS)
            except snn._lib.SnnError:
                log.new_lines()
                dn.close()
                continue                                        # an allocation the run cannot do without (tests/test_gpu_alloc_failures.py)
            finally:
                arm(snn, 0)
            lines = log.new_lines()
            try:
                got = outcome(dn, net)
                assert_same(got, want)
            finally:
                dn.close()
            if count(lines, MOVED_OUT) == 0:
                # W stayed where it was.  With the image in use all the same (3 bytes per synapse) it was the hand-over's
                # allocation that failed -- today's path, a fresh image; otherwise an earlier one, and the handle reads W
                assert count(lines, "image region") == 0, lines
                hit_hand_over = hit_hand_over or got["bytes"] == 3 * net.n_tot * net.n_neurons
            elif count(lines, CANDIDATE) == 0:
                hit_candidate = True                            # handed over, nothing to compare the region with
            if hit_hand_over and hit_candidate:
                break
    assert hit_hand_over and hit_candidate


def test_destroy_gives_all_memory_back(snn):
    net, _ = reference()
    dn = create(snn, net)                                       # (the first handle of a process leaves the runtime's own pools behind)
    dn.run(2)
    dn.close()
    before = free_bytes()
    with environ(SNN_DEBUG_PLACEMENT="1"), PlacementLog() as log:
        dn = create(snn, net)
        dn.run(STEPS)
        lines = log.new_lines()
        dn.close()
    assert count(lines, MOVED_OUT) == 1, lines
    assert free_bytes() == before
