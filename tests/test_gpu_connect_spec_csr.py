"""snn_connect_by_specs_csr: wrap-around windows and displacement tables merged into the sparse graph on the device, against the
per-pair restatement of the header's formulas (connect_spec_cases) patched into a dense host matrix and taken in CSR order.  The
plan of test_gpu_connect_spec.py on an unsharded handle and on contiguous shards; windows that wrap at both ends, that cover the
ring, that need more than one round of 64 candidates, and of extent 0; refusals.  Helpers are test_gpu_connect_rule_csr.py's."""
import ctypes as C

import numpy as np
import pytest

import connect_spec_cases as cases
import parity
import test_gpu_connect_rule as dense_tests
import test_gpu_connect_rule_csr as csr_tests
import test_gpu_connect_spec as spec_tests
from snn_amd import ConnectionRule, WeightRule, _lib

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_STATE = 11, 12
RAGGED, SPLIT = dense_tests.RAGGED, dense_tests.SPLIT
csr_of, assert_csr, patterned, read = csr_tests.csr_of, csr_tests.assert_csr, csr_tests.patterned, csr_tests.read
apply_host = spec_tests.apply_host
# a 9x11 lattice (wrapped Chebyshev 4: 9 rows x 9 columns = 81 candidates, two rounds of 64), a smaller one, cells
WINDOWS = parity.Layout([(0, 9, 11), (1, 3, 5)], [(2, 2, 3)])


def test_block_by_block_and_as_one_batch(snn):
    one, w, c = patterned(snn, RAGGED)
    batch, _, _ = patterned(snn, RAGGED)
    for k, record in enumerate(spec_tests.PLAN):
        one.connect_sparse([record])
        apply_host(w, c, RAGGED, [record])
        # the block as the per-pair loop has it; every stored edge outside the blocks written so far still the pattern's
        assert_csr(one, csr_of(w, c, one.owned), f"after record {k}: {record[0]} -> {record[1]}")
    batch.connect_sparse(spec_tests.PLAN)
    for x, y in zip(read(one), read(batch)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "the batch and the sequence of calls differ"
    untouched, cu = dense_tests.pattern(RAGGED)
    assert np.array_equal(w[15:, 0:15], untouched[15:, 0:15]) and np.array_equal(c[15:, 0:15], cu[15:, 0:15]) and cu[15:, 0:15].any()
    # plain records and spec records in one batch; a later record for the same pair wins
    mixed = dense_tests.PLAN[:2] + spec_tests.PLAN[1:3] + dense_tests.PLAN[3:]
    batch.connect_sparse(mixed)
    dense_tests.apply_host(w, c, RAGGED, dense_tests.PLAN[:2])
    apply_host(w, c, RAGGED, spec_tests.PLAN[1:3])
    dense_tests.apply_host(w, c, RAGGED, dense_tests.PLAN[3:])
    assert_csr(batch, csr_of(w, c, batch.owned), "after a batch of plain and spec records")
    one.close()
    batch.close()


@pytest.mark.parametrize("layout,plan,n_shards", [(RAGGED, spec_tests.PLAN, 2), (SPLIT, spec_tests.SPLIT_SPEC_PLAN, 2), (SPLIT, spec_tests.SPLIT_SPEC_PLAN, 3)],
                         ids=["ragged-2-one-empty", "split-2", "split-3"])
def test_contiguous_shards_write_the_rows_they_own(snn, layout, plan, n_shards):
    whole, w, c = patterned(snn, layout)
    whole.connect_sparse(plan)
    apply_host(w, c, layout, plan)
    assert_csr(whole, csr_of(w, c, whole.owned), "on the unsharded handle")
    owned = 0
    for k in range(n_shards):
        dn, _, _ = patterned(snn, layout, shard=(k, n_shards))
        dn.connect_sparse(plan)
        assert_csr(dn, csr_of(w, c, dn.owned), f"on shard {k} of {n_shards} (rows {dn.post_begin}..{dn.post_end})")
        owned += dn.owned.size
        dn.close()
    assert owned == layout.n_neurons
    whole.close()


def test_windows_on_rings(snn):
    dn, w, c = patterned(snn, WINDOWS)
    geo = dense_tests.geometry(WINDOWS)

    def after(pre, post, rule, weight=None):
        dn.connect_sparse([(pre, post, rule, weight)])
        apply_host(w, c, WINDOWS, [(pre, post, rule, weight or WeightRule.constant(1.0))])
        assert_csr(dn, csr_of(w, c, dn.owned), f"after {rule!r} on {pre} -> {post}")
        (f0, s0), (f1, s1) = geo[pre], geo[post]
        return c[f0:f0 + s0[0] * s0[1], f1:f1 + s1[0] * s1[1]] != 0

    def table(pre, post, wrap):
        return WeightRule.displacement(cases.holed(WeightRule.table_shape(geo[pre][1], geo[post][1], wrap)), wrap=wrap)

    # 81 candidates per row, two rounds; the rows cover their ring (2 e + 1 = P_r), the columns wrap at both ends
    on = after(0, 0, ConnectionRule.chebyshev(4, self_edges=False, wrap=True), table(0, 0, True))
    assert 40 < on[:, 0].sum() <= 80 and on[98, 0] and on[10, 0]               # the corner's column reaches the other three corners' sides
    on = after(0, 0, ConnectionRule.chebyshev(4, wrap=True))
    assert (on.sum(axis=0) == 81).all()
    # the centre in the first and the last row and column: two runs of rows and two of columns
    on = after(0, 0, ConnectionRule.chebyshev(1, wrap=True), WeightRule.uniform(1.0, 2.0, seed=8))
    assert (on.sum(axis=0) == 9).all() and on[:, 0].nonzero()[0].tolist() == [0, 1, 10, 11, 12, 21, 88, 89, 98]
    assert on[:, 98].nonzero()[0].tolist() == [0, 9, 10, 77, 86, 87, 88, 97, 98]
    on = after(0, 0, ConnectionRule.euclidean(2, wrap=(False, True), probability=0.7, seed=12), table(0, 0, (False, True)))
    on = after(0, 0, ConnectionRule.euclidean(5, wrap=(True, False), self_edges=False), table(0, 0, (True, False)))
    # the window is everything: 2 e + 1 >= P in both dimensions, and far beyond
    for e in (5, 6, 2 ** 32 - 1):
        on = after(0, 0, ConnectionRule.chebyshev(e, wrap=True), WeightRule.uniform(-1.0, 1.0, seed=e % 7))
        assert on.all()
    # extent 0 is position to position, wrapped or not
    on = after(0, 0, ConnectionRule.chebyshev(0, wrap=True), WeightRule.displacement(cases.ramp((9, 11), 1.0, 2.0), wrap=True))
    assert on.sum() == 99 and (w[0:99, 0:99][on] == 2.0).all()
    on = after(0, 0, ConnectionRule.chebyshev(0, wrap=True), table(0, 0, True))          # ... and the table's None at displacement 0 removes them all
    assert not on.any()
    # two grids of different shapes: the periods are the larger grid's, the centre may lie outside the smaller presynaptic grid
    on = after(1, 0, ConnectionRule.chebyshev(2, wrap=True), table(1, 0, True))
    assert on.any() and not on.all()
    on = after(0, 1, ConnectionRule.chebyshev(2, wrap=True), table(0, 1, True))
    assert on.any() and not on.all()
    on = after(2, 1, ConnectionRule.euclidean(4, wrap=(False, True)), table(2, 1, (False, True)))
    on = after(2, 0, ConnectionRule.chebyshev(3, wrap=True, probability=0.5, seed=2))
    # the table under the rules without a window: every presynaptic cell, the one cell at the post position
    on = after(1, 1, ConnectionRule.all_to_all(self_edges=False, wrap=True), table(1, 1, True))
    on = after(1, 0, ConnectionRule.same_position(), table(1, 0, False))
    on = after(0, 1, ConnectionRule.all_to_all(probability=0.4, seed=6), table(0, 1, False))
    dn.run(3)                                                                  # the committed graph steps
    dn.close()


def test_refusals_are_all_or_nothing(snn):
    dn, w, c = patterned(snn, RAGGED)
    L = dn._L
    before = read(dn)

    def raw_call(handle, specs):
        arr = (_lib.ConnectSpec * max(len(specs), 1))(*[s for s, _ in specs])
        code = L.snn_connect_by_specs_csr(handle, arr, len(specs))
        return code, (L.snn_last_error() or b"").decode()

    good = spec_tests.spec
    inf = cases.ramp((3, 5))
    inf[1, 1] = np.inf
    assert raw_call(None, [good()])[0] == BAD_ARG
    assert L.snn_connect_by_specs_csr(dn._h, None, 0) == 0
    assert L.snn_connect_by_specs_csr(dn._h, None, 2) == BAD_ARG
    for args, change, name in [((), dict(wrap=4), "wrap"), ((False,), {}, "table"), ((), dict(rows=4), "table_rows"), ((), dict(cols=4), "table_cols"),
                               ((inf,), {}, "table"), ((), dict(weight_rule=3), "weight_rule"), ((), dict(rule=4), "rule"), ((), dict(post_id=2), "post_id")]:
        code, msg = raw_call(dn._h, [good(), good(*args, **change), good()])
        assert code == BAD_ARG and "record 1: " in msg and name in msg, (change, code, msg)
        assert_csr(dn, before, f"after a batch whose second record has a bad {name}")
    with pytest.raises(ValueError, match="wrap"):
        dn.connect_sparse([(0, 0, ConnectionRule.all_to_all(), WeightRule.displacement(cases.ramp((3, 5)), wrap=True))])
    assert_csr(dn, before, "after a plan whose table and rule disagree")
    # the accepted call, for contrast, does change it
    dn.connect_sparse(spec_tests.PLAN[:1])
    apply_host(w, c, RAGGED, spec_tests.PLAN[:1])
    assert_csr(dn, csr_of(w, c, dn.owned), "after the accepted call")
    dn.close()

    dense = dense_tests.handle(snn, RAGGED)
    code, msg = raw_call(dense._h, [good()])
    assert code == BAD_STATE and "dense graph" in msg, msg
    dense.close()

    slab = dense_tests.handle(snn, RAGGED, finalize=False)
    slab.finalize(0, 2, csr=True, by_lattice=True)
    w, c = dense_tests.pattern(RAGGED)
    slab.set_graph_csr(*csr_of(w, c, slab.owned))
    code, msg = raw_call(slab._h, [good()])
    assert code == BAD_STATE and "not covered" in msg and "by lattice" in msg
    assert_csr(slab, csr_of(w, c, slab.owned), "on the by-lattice shard after the refusal")
    slab.close()
