"""snn_connect_by_rules_csr under the allocation-failure hook (snn_debug_fail_alloc_at), as tests/test_gpu_alloc_failures.py walks the
other calls: whichever allocation of a create / finalize / set_graph_csr / connect_sparse / run / destroy sequence fails -- device
temporaries of the merge, host tables of the download, the arrays of the commit -- the outcome is a status code with a message;
a failure inside connect_sparse leaves the previous graph, its weights and its next steps; the handle can be destroyed and the
next handle computes the oracle's bits.  The hook fails allocations on the host side only."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import parity
import test_gpu_connect_rule as dense_tests
from snn_amd import ConnectionRule, WeightRule

pytestmark = pytest.mark.gpu

LAYOUT = dense_tests.RAGGED
BEFORE = dense_tests.PLAN[:2]                      # graph A, uploaded as CSR
EDIT = [(1, 1, ConnectionRule.all_to_all(self_edges=False), WeightRule.constant(0.25)),
        (2, 1, ConnectionRule.same_position(), WeightRule.constant(2.0)),
        (0, 0, ConnectionRule.chebyshev(2, probability=0.5, seed=2), WeightRule.uniform(0.5, 1.5, seed=3))]
STEPS_BEFORE, STEPS_AFTER = 4, 5


def arm(snn, n):
    seen = C.c_uint64()
    snn._lib.check(snn._lib.load().snn_debug_fail_alloc_at(int(n), C.byref(seen)))
    return int(seen.value)


def oracle(plan):
    net = parity.make_oracle(LAYOUT, st_kind=ob.ST_RATE, electrical=True, chemical=False)
    net["current_voltage"] = ob.uniform_array(6, net.n_neurons, -65.0, 30.0)
    net["gap_conductance"] = 10.0
    net["st_rate"] = ob.uniform_array(7, net.n_cells, 0.3, 1.5)
    net["weights"][...] = 0
    net["connections"][...] = 0
    dense_tests.twin_graph(net, plan)
    return net


def sequence(snn, net_a):
    """create ... destroy; returns what the getters read after the edit"""
    dn = parity.device_from_oracle(snn, net_a, csr=True)
    try:
        dn.run(STEPS_BEFORE)
        dn.connect_sparse(EDIT)
        dn.run(STEPS_AFTER)
        rp, pi = dn.graph_csr_structure()
        return {"v": dn.get_attr(0, "current_voltage"), "v1": dn.get_attr(1, "current_voltage"), "rp": rp, "pi": pi,
                "w": dn.get_graph_csr(), "clock": dn.clock}
    finally:
        dn.close()


def same(got, want, what):
    for k in want:
        assert np.array_equal(np.atleast_1d(got[k]).view(np.uint8), np.atleast_1d(want[k]).view(np.uint8)), (what, k)


def test_every_allocation_of_a_sequence_with_connect_sparse_may_fail(snn):
    net_a = oracle(BEFORE)
    try:
        before = arm(snn, 0)
        want = sequence(snn, net_a)
        total = arm(snn, 0) - before
        assert total > 40, f"only {total} allocations counted: is the hook wired to the allocators?"
        errors, messages = 0, set()
        for n in range(1, total + 1):
            arm(snn, n)
            try:
                got = sequence(snn, net_a)
            except snn.SnnError as e:
                assert e.code in (3, 4, 5, 6, 8, 12) and str(e).split(":", 1)[1].strip(), f"allocation {n} of {total}: {e.code}: {e}"
                errors += 1
                messages.add(str(e)[:120])
                continue
            finally:
                arm(snn, 0)
            same(got, want, n)                     # (the library had a fall-back for this allocation)
        assert errors >= total * 0.8, (errors, total)
        assert any("bad_alloc" in m for m in messages) and any("bad_alloc" not in m for m in messages), messages
        # after all those failures the process still computes the oracle's bits: the edit, then the steps
        got = sequence(snn, net_a)
        same(got, want, "afterwards")
        onet = oracle(BEFORE)
        onet.run(STEPS_BEFORE)
        dense_tests.twin_graph(onet, EDIT)
        onet.run(STEPS_AFTER)
        assert np.array_equal(parity.bits(onet["current_voltage"][:15]), parity.bits(want["v"]))
        assert np.array_equal(parity.bits(onet["current_voltage"][15:50]), parity.bits(want["v1"]))
        _, pre, w = parity.csr_for_posts(onet, np.arange(50))
        assert np.array_equal(pre, want["pi"]) and np.array_equal(parity.bits(w), parity.bits(want["w"]))
    finally:
        arm(snn, 0)


def test_a_failed_connect_sparse_keeps_the_previous_graph(snn):
    net_a = oracle(BEFORE)

    def handle_on_a():
        dn = parity.device_from_oracle(snn, net_a, csr=True)
        dn.run(STEPS_BEFORE)
        return dn

    try:
        dn = handle_on_a()
        before = arm(snn, 0)
        dn.connect_sparse(EDIT)
        total = arm(snn, 0) - before
        dn.close()
        assert total > 25, f"only {total} allocations counted in connect_sparse"
        onet = oracle(BEFORE)
        onet.run(STEPS_BEFORE + STEPS_AFTER)
        failed = 0
        for n in range(1, total + 1):
            dn = handle_on_a()
            try:
                rp, pi = dn.graph_csr_structure()
                w_a = dn.get_graph_csr()
                arm(snn, n)
                try:
                    dn.connect_sparse(EDIT)
                except snn.SnnError as e:
                    arm(snn, 0)
                    assert e.code in (3, 4, 5, 6, 8, 12) and str(e).split(":", 1)[1].strip(), (n, total, str(e))
                else:
                    arm(snn, 0)
                    continue
                failed += 1
                rp2, pi2 = dn.graph_csr_structure()
                assert np.array_equal(rp, rp2) and np.array_equal(pi, pi2), (n, total)
                assert np.array_equal(dn.get_graph_csr().view(np.uint32), w_a.view(np.uint32)), (n, total)
                dn.run(STEPS_AFTER)
                v = dn.get_attr(0, "current_voltage")
                assert np.array_equal(parity.bits(v), parity.bits(onet["current_voltage"][:v.size])), (n, total)
            finally:
                arm(snn, 0)
                dn.close()
        assert failed == total, (failed, total)
    finally:
        arm(snn, 0)
