"""The plain electrical input pass over the 24-bit image of W (k_inputs_dense_w24, csrc/snn_w24.hpp) against the oracle and
against a handle created under SNN_AMD_W24=0 (k_inputs_dense over W): state, voltage history and raster bit for bit, at sizes just
past the 64 MiB above which a matrix is streamed.  After each run snn_input_kernel_bytes says which of the two the handle reads:
3 bytes per synapse from the image, 4 from W.

Deviation from the issue's invalidation case, which asks for a band of rows with doubled weights to be encoded again: U[0.5, 1.5)
next to a doubled band spans 0x3F000000 .. 0x40400000, more than 2^24 patterns, so that matrix is NOT encodable.  The test asks
for both: the band alone must fall back to W (4 bytes) with results equal to the oracle, and once the remaining rows are doubled
too -- the base moves from 0x3F000000 to 0x3F800000 -- the image is back (3 bytes), again equal to the oracle."""
import functools
import os

import numpy as np
import pytest

import oracle_binding as ob
import parity
from test_gpu_fused_step import build

pytestmark = pytest.mark.gpu

STEPS = 24
LATTICE = [(0, 71, 73)]                    # 5183 neurons: the last chunk has 63 rows = three units + one of 15 rows; ragged last tile
ROW = [(0, 1, 4099)]                       # 4099 x 4160 x 4 B = 65.04 MiB: the smallest streamed matrix with this padding
CELLS = [(3, 2, 3)]                        # rows past n_neurons: per-row kinds, a chunk that mixes neurons and cells


def static_net(lattices, st, seed):
    net = build(ob.IZHIKEVICH, True, False, lattices, st, seed)
    net["do_plasticity"] = 0               # static weights: what the image is for
    # 24 steps of a gap-coupled lattice started below threshold pull the voltages together before anything fires: every 97th
    # neuron starts above it, so the raster that is compared holds spikes and the resets they cause
    net["current_voltage"][::97] = np.float32(35.0)
    assert net.n_tot * (-(-net.n_neurons // 64) * 64) * 4 > 64 << 20
    return net


def run_device(snn, net, w24, shape=0):
    old = os.environ.get("SNN_AMD_W24")
    os.environ["SNN_AMD_W24"] = "1" if w24 else "0"
    try:
        dn = parity.device_from_oracle(snn, net)
    finally:
        if old is None:
            del os.environ["SNN_AMD_W24"]
        else:
            os.environ["SNN_AMD_W24"] = old
    if shape:
        dn.set_option("input_shape", shape)
    dn.set_history(voltage=True, spikes=True)
    dn.run(STEPS // 2)
    i0 = net.layout.lattices[0][0]
    first, count, _ = net.layout.ranges()[i0]
    dn.set_attr(i0, "gap_conductance", net["gap_conductance"][first:first + count])       # identical values: nothing may change
    dn.run(STEPS - STEPS // 2)
    out = {"state": parity.pull_state(dn, net), "bytes": dn.input_kernel_bytes()}
    for i, _, _ in net.layout.lattices:
        out[("v", i)] = dn.voltage_history(i)
        out[("s", i)] = dn.spike_history(i)
    dn.close()
    return out


def assert_equals_oracle(net, out):
    """net: the oracle after its run with both histories"""
    parity.assert_state_equal(net, out["state"])
    rng = net.layout.ranges()
    for i, _, _ in net.layout.lattices:
        first, count, _ = rng[i]
        assert np.array_equal(out[("s", i)], net.spike_history[:, first:first + count])
        assert np.array_equal(parity.bits(out[("v", i)]), parity.bits(net.voltage_history[:, first:first + count]))


def assert_same(a, b):
    for key in a:
        if key in ("state", "bytes"):
            continue
        assert np.array_equal(parity.bits(a[key]), parity.bits(b[key])), key
    for name in a["state"]:
        assert np.array_equal(parity.bits(a["state"][name]), parity.bits(b["state"][name])), name


@functools.lru_cache(maxsize=None)
def lattice_reference():
    """the 71 x 73 lattice and its oracle outcome, computed once for both shapes (the device never writes into it)"""
    net, ref = static_net(LATTICE, [], 11), static_net(LATTICE, [], 11)
    ref.run(STEPS, voltage_history=True, spike_history=True)
    assert ref.spike_history.sum() > 0
    return net, ref


@pytest.mark.parametrize("shape", [0, 1], ids=["shape_by_size", "shape_1"])
def test_lattice_71x73_image_equals_w_and_oracle(snn, shape):
    net, ref = lattice_reference()
    n = net.n_tot * net.n_neurons
    a = run_device(snn, net, True, shape)
    b = run_device(snn, net, False, shape)
    assert (a["bytes"], b["bytes"]) == (3 * n, 4 * n)
    assert_same(a, b)
    assert_equals_oracle(ref, a)


def test_row_with_spike_train_cells(snn):
    net = static_net(ROW, CELLS, 12)
    assert net.n_cells and net.n_tot > net.n_neurons and net.n_neurons % 256 != 0
    n = net.n_tot * net.n_neurons
    a = run_device(snn, net, True)
    b = run_device(snn, net, False)
    assert (a["bytes"], b["bytes"]) == (3 * n, 4 * n)
    assert_same(a, b)
    net.run(STEPS, voltage_history=True, spike_history=True)
    assert_equals_oracle(net, a)
    assert net.spike_history.sum() > 0


def _bits_to_f32(x):
    return np.array([x], np.uint32).view(np.float32)[0]


def _all_ones(w, c):
    w[...] = np.where(c != 0, np.float32(1.0), np.float32(0.0))


def _span(top_bits):
    def edit(w, c):
        present = np.argwhere(c != 0)
        lo, hi = tuple(present[0]), tuple(present[-1])
        w[...] = np.where(c != 0, np.clip(w, np.float32(0.5), np.float32(1.5)), np.float32(0.0))
        w[lo] = np.float32(0.5)                            # bits 0x3F000000
        w[hi] = _bits_to_f32(top_bits)
    return edit


def _half_negated(w, c):
    w[::2] *= np.float32(-1.0)


@pytest.mark.parametrize("edit,encoded", [(_all_ones, True), (_span(0x3FFFFFFE), True), (_span(0x3FFFFFFF), False), (_half_negated, False)],
                         ids=["span_0", "span_fffffe", "span_ffffff_falls_back", "mixed_signs_fall_back"])
def test_encoding_edges(snn, edit, encoded):
    net = static_net(ROW, [], 13)
    edit(net["weights"], net["connections"])
    n = net.n_tot * net.n_neurons
    a = run_device(snn, net, True)
    assert a["bytes"] == (3 if encoded else 4) * n
    net.run(STEPS, voltage_history=True, spike_history=True)
    assert_equals_oracle(net, a)


def test_graph_and_plasticity_changes_invalidate_the_image(snn):
    net = static_net(ROW, [], 14)
    n = net.n_tot * net.n_neurons
    old = os.environ.get("SNN_AMD_W24")
    os.environ["SNN_AMD_W24"] = "1"
    try:
        dn = parity.device_from_oracle(snn, net)
    finally:
        if old is None:
            del os.environ["SNN_AMD_W24"]
        else:
            os.environ["SNN_AMD_W24"] = old
    conns = net["connections"].astype(np.uint32)

    def both_run(steps):
        dn.run(steps)
        net.run(steps)
        parity.assert_state_equal(net, parity.pull_state(dn, net))

    both_run(8)
    assert dn.input_kernel_bytes() == 3 * n
    # a band of doubled rows: [0.5, 1.5) next to [1, 3) is more than 2^24 bit patterns -- back on W
    net["weights"][100:400] *= np.float32(2.0)
    dn.set_graph_rows(100, net["weights"][100:400], conns[100:400])
    both_run(8)
    assert dn.input_kernel_bytes() == 4 * n
    # the other rows doubled too: encodable again, with another base
    net["weights"][:100] *= np.float32(2.0)
    net["weights"][400:] *= np.float32(2.0)
    dn.set_graph_rows(0, net["weights"][:100], conns[:100])
    dn.set_graph_rows(400, net["weights"][400:], conns[400:])
    both_run(8)
    assert dn.input_kernel_bytes() == 3 * n
    # plasticity on: the weights move, the handle reads W
    net["do_plasticity"] = 1
    net["current_voltage"][::89] = np.float32(35.0)             # spikes in this run: weights that move
    dn.set_attr(0, "current_voltage", net["current_voltage"])
    dn.set_plasticity(0, float(net["stdp_a_plus"][0]), float(net["stdp_a_minus"][0]), float(net["stdp_tau_plus"][0]),
                      float(net["stdp_tau_minus"][0]), float(net["stdp_dt"][0]), True)
    both_run(8)
    assert dn.input_kernel_bytes() == 4 * n
    parity.assert_graph_equal(net, dn)
    dn.close()
