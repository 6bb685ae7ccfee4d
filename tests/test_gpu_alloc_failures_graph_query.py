"""The four Graph-trait calls under the allocation-failure hook (snn_debug_fail_alloc_at), in the manner of
tests/test_gpu_alloc_failures_connect_csr.py: whichever allocation of one call fails -- the device lists, the host tables of an
edit -- the call returns a status with a message, the graph, read through
get_graph_rows, is as before, and the same call then succeeds."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_graph_query as q

pytestmark = pytest.mark.gpu


def arm(snn, n):
    seen = C.c_uint64()
    snn._lib.check(snn._lib.load().snn_debug_fail_alloc_at(int(n), C.byref(seen)))
    return int(seen.value)


def edit_args():
    rng = np.random.default_rng(4)
    pre, post = rng.integers(0, 56, 40).astype(np.uint32), rng.integers(0, 50, 40).astype(np.uint32)        # unordered, with repeats
    pre[7], post[7] = pre[3], post[3]
    return pre, post, rng.uniform(1.0, 2.0, 40).astype(np.float32), rng.random(40) < 0.7


CALLS = {"lookup": lambda dn: dn.graph_lookup(*q.all_pairs(dn)), "edit": lambda dn: dn.graph_edit(*edit_args()),
         "incoming": lambda dn: dn.graph_incoming(17), "outgoing": lambda dn: dn.graph_outgoing(52)}


@pytest.mark.parametrize("name", list(CALLS))
def test_every_allocation_of_a_call_may_fail(snn, name):
    call = CALLS[name]
    w, c = q.pattern(q.RAGGED)

    def fresh():
        dn = q.handle(snn, q.RAGGED)
        dn.set_graph_rows(0, w, c)
        return dn

    try:
        dn = fresh()
        before = arm(snn, 0)
        want = call(dn)
        total = arm(snn, 0) - before
        after = dn.get_graph_rows(0, dn.n_tot)
        dn.close()
        assert total >= 3, f"only {total} allocations counted in {name}: is the hook wired to the allocators?"
        failed = 0
        for n in range(1, total + 1):
            dn = fresh()
            try:
                arm(snn, n)
                try:
                    call(dn)
                except snn.SnnError as e:
                    arm(snn, 0)
                    assert e.code in (3, 4, 5, 6, 8) and str(e).split(":", 1)[1].strip(), (name, n, total, str(e))
                else:
                    arm(snn, 0)
                    continue
                failed += 1
                gw, gc = dn.get_graph_rows(0, dn.n_tot)
                assert np.array_equal(gc, c) and np.array_equal(gw.view(np.uint32), w.view(np.uint32)), (name, n, "the graph changed")
                got = call(dn)                   # the same call now succeeds
                if want is not None:
                    assert all(np.array_equal(a, b) for a, b in zip(got, want)), (name, n)
                gw, gc = dn.get_graph_rows(0, dn.n_tot)
                assert np.array_equal(gc, after[1]) and np.array_equal(gw.view(np.uint32), after[0].view(np.uint32)), (name, n)
            finally:
                arm(snn, 0)
                dn.close()
        assert failed == total, (name, failed, total)
    finally:
        arm(snn, 0)
