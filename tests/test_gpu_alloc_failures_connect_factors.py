"""snn_connect_by_factors and snn_connect_by_factors_csr under the allocation-failure hook (snn_debug_fail_alloc_at), as
tests/test_gpu_alloc_failures_connect_spec.py walks the spec calls: whichever allocation of the call fails -- the device copies of
the two factor arrays among them -- the outcome is a status code with a message, the previous graph is readable and unchanged,
and the same call succeeds afterwards with the twin's bits."""
import numpy as np
import pytest

import test_gpu_alloc_failures_connect_spec as model
import test_gpu_connect_factors as dense_factors
import test_gpu_connect_factors_csr as csr_factors
import test_gpu_connect_rule as dense_tests
import test_gpu_connect_rule_csr as csr_tests
from snn_amd import ConnectionRule, WeightRule

pytestmark = pytest.mark.gpu

PAIR = dense_factors.PAIR


def test_every_allocation_of_a_dense_factors_call_may_fail(snn):
    u, v = dense_factors.random_factors(11, 3, 15, 24)
    record = (0, 1, ConnectionRule.chebyshev(2, probability=0.7, seed=2), WeightRule.factors(u, v, drop_zero=True))
    w, c = dense_tests.pattern(PAIR)

    def fresh():
        dn = dense_tests.handle(snn, PAIR)
        dn.set_graph_rows(0, w, c)
        return dn
    failed, total, messages = model.walk(snn, fresh, lambda dn: dn.connect_by_rule(*record), lambda dn: dn.get_graph_rows(0, dn.n_tot), 2)
    assert failed == total >= 2, (failed, total, messages)         # the two factor buffers are the call's allocations
    ww, cc = dense_factors.apply_host(w.copy(), c.copy(), PAIR, [record])
    dn = fresh()
    dn.connect_by_rule(*record)
    dense_tests.assert_rows(dn, ww, cc, what="after the walk")
    dn.close()


def test_every_allocation_of_a_sparse_factors_call_may_fail(snn):
    plan = csr_factors.mixed_plan()

    def fresh():
        return csr_tests.patterned(snn, PAIR)[0]
    failed, total, messages = model.walk(snn, fresh, lambda dn: dn.connect_sparse(plan), csr_tests.read, 25 + 4 + 1)
    assert failed == total, (failed, total, messages)
    w, c = dense_tests.pattern(PAIR)
    dense_factors.apply_host(w, c, PAIR, plan)
    dn = fresh()
    dn.connect_sparse(plan)
    csr_tests.assert_csr(dn, csr_tests.csr_of(w, c, dn.owned), "after the walk")
    dn.close()
