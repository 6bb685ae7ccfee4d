"""snn_connect_by_spec and snn_connect_by_specs_csr under the allocation-failure hook (snn_debug_fail_alloc_at), as
tests/test_gpu_alloc_failures_connect_csr.py walks the older sparse call: whichever allocation of the call fails -- the device
buffer of the displacement table among them -- the outcome is a status code with a message, the previous graph is readable and
unchanged, and the same call succeeds afterwards with the restatement's bits."""
import ctypes as C

import numpy as np
import pytest

import parity
import test_gpu_alloc_failures_connect_csr as model
import test_gpu_connect_rule as dense_tests
import test_gpu_connect_rule_csr as csr_tests
import test_gpu_connect_spec as spec_tests

pytestmark = pytest.mark.gpu

RAGGED = dense_tests.RAGGED
arm = model.arm


def walk(snn, fresh, call, read, total_at_least):
    """every allocation of `call` on a fresh handle fails once; returns how many calls failed"""
    try:
        dn = fresh()
        before = arm(snn, 0)
        call(dn)
        total = arm(snn, 0) - before
        want = read(dn)
        dn.close()
        assert total >= total_at_least, f"only {total} allocations counted: is the hook wired to the allocators?"
        failed, messages = 0, set()
        for n in range(1, total + 1):
            dn = fresh()
            try:
                was = read(dn)
                arm(snn, n)
                try:
                    call(dn)
                except snn.SnnError as e:
                    arm(snn, 0)
                    assert e.code in (3, 4, 5, 6, 8, 12) and str(e).split(":", 1)[1].strip(), (n, total, str(e))
                    failed += 1
                    messages.add(str(e)[:100])
                    for x, y in zip(read(dn), was):
                        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"allocation {n} of {total}: the graph changed"
                arm(snn, 0)
                call(dn)                                       # ... and the call succeeds afterwards
                for x, y in zip(read(dn), want):
                    assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"allocation {n} of {total}: the call after the failure"
            finally:
                arm(snn, 0)
                dn.close()
        return failed, total, messages
    finally:
        arm(snn, 0)


def test_every_allocation_of_a_dense_spec_call_may_fail(snn):
    record = spec_tests.PLAN[0]
    w, c = dense_tests.pattern(RAGGED)

    def fresh():
        dn = dense_tests.handle(snn, RAGGED)
        dn.set_graph_rows(0, w, c)
        return dn
    failed, total, messages = walk(snn, fresh, lambda dn: dn.connect_by_rule(*record), lambda dn: dn.get_graph_rows(0, dn.n_tot), 1)
    assert failed == total >= 1, (failed, total, messages)         # the table's buffer is the call's allocation
    ww, cc = spec_tests.apply_host(w.copy(), c.copy(), RAGGED, [record])
    dn = fresh()
    dn.connect_by_rule(*record)
    dense_tests.assert_rows(dn, ww, cc, what="after the walk")
    dn.close()


def test_every_allocation_of_a_sparse_specs_call_may_fail(snn):
    plan = spec_tests.PLAN
    tables = sum(weight.table is not None for _, _, _, weight in plan)

    def fresh():
        return csr_tests.patterned(snn, RAGGED)[0]
    failed, total, messages = walk(snn, fresh, lambda dn: dn.connect_sparse(plan), csr_tests.read, 25 + tables)
    assert failed == total, (failed, total, messages)
    w, c = dense_tests.pattern(RAGGED)
    spec_tests.apply_host(w, c, RAGGED, plan)
    dn = fresh()
    dn.connect_sparse(plan)
    csr_tests.assert_csr(dn, csr_tests.csr_of(w, c, dn.owned), "after the walk")
    dn.close()
