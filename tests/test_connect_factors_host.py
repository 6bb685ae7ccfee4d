"""WeightRule.factors / hopfield / per_post / per_pre on the host: the float64 twin of the formula in include/snn_amd.h against
the reference's own results (tests/golden/hopfield_weights.npz), bit for bit; slices; validation.  No device."""
import numpy as np
import pytest

import connect_factors_cases as cases
from snn_amd import ConnectionRule, WeightRule
from snn_amd.network import rule_pairs

NO_SELF = ConnectionRule.all_to_all(self_edges=False)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", cases.CASES)
def test_hopfield_values_are_the_reference_matrix(name):
    patterns, a, b, scalar, want = cases.case(name)
    shape = cases.GRIDS[name]
    n = shape[0] * shape[1]
    assert patterns.shape[1] == n and want.shape == (n, n) and not np.diagonal(want).any()
    weight = cases.hopfield(WeightRule, name)
    w64 = weight.values(shape, shape)
    off = ~np.eye(n, dtype=bool)
    # the weights: every off-diagonal pair, bit for bit in float64 (NaN where w == 0 was dropped)
    kept = off & (want != 0)
    assert w64.dtype == np.float64 and np.array_equal(bits64(w64[kept]), bits64(want[kept]))
    assert np.isnan(w64[off & (want == 0)]).all() and not np.isnan(w64[kept]).any()
    # the graph: the reference's edge set (w != 0; the diagonal is zero) and its weights as the device stores them
    on, w32 = rule_pairs(NO_SELF, weight, shape, shape)
    assert np.array_equal(on, want != 0)
    assert np.array_equal(w32.view(np.uint32), np.where(want != 0, want, 0.0).astype(np.float32).view(np.uint32))
    # without drop_zero a zero weight is an edge of weight 0
    on0, w0 = rule_pairs(NO_SELF, cases.hopfield(WeightRule, name, drop_zero=False), shape, shape)
    assert np.array_equal(on0, off) and np.array_equal(w0[off].view(np.uint32), want[off].astype(np.float32).view(np.uint32))


def test_the_single_pattern_exercises_drop_zero():
    _, _, _, _, want = cases.case("single")
    assert ((want == 0) & ~np.eye(35, dtype=bool)).sum() == 1008


def test_the_normal_case_separates_float64_from_float32_accumulation():
    patterns, a, b, scalar, want = cases.case("normal")
    u, v = (patterns - b).astype(np.float32), (patterns - a).astype(np.float32)
    s = np.zeros(want.shape, np.float32)
    for p in range(patterns.shape[0]):
        s = s + u[p][:, None] * v[p][None, :]
    low = (s * np.float32(scalar)).astype(np.float32)
    off = ~np.eye(want.shape[0], dtype=bool)
    assert (low[off].view(np.uint32) != want[off].astype(np.float32).view(np.uint32)).any()


def test_per_post_and_per_pre_are_the_table():
    table = cases.ie_table()
    assert table.size == 35
    w = WeightRule.per_post(table).values((3, 3), (5, 7))
    assert w.shape == (9, 35) and np.array_equal(bits64(w), bits64(np.broadcast_to(table[None, :], (9, 35))))
    on, w32 = rule_pairs(ConnectionRule.all_to_all(), WeightRule.per_post(table), (3, 3), (5, 7))
    assert on.all() and np.array_equal(w32.view(np.uint32), np.broadcast_to(table.astype(np.float32)[None, :], (9, 35)).view(np.uint32))
    w = WeightRule.per_pre(table).values((5, 7), (2, 3))
    assert np.array_equal(bits64(w), bits64(np.broadcast_to(table[:, None], (35, 6))))


@pytest.mark.parametrize("name", ["general", "normal"])
def test_slices_are_slices_of_the_full_result(name):
    shape = cases.GRIDS[name]
    weight = cases.hopfield(WeightRule, name)
    full = weight.values(shape, shape)
    pre, post = np.array([3, 0, 17, 3]), np.array([19, 2])
    assert np.array_equal(bits64(weight.values(shape, shape, pre_index=pre)), bits64(full[pre]))
    assert np.array_equal(bits64(weight.values(shape, shape, post_index=post)), bits64(full[:, post]))
    assert np.array_equal(bits64(weight.values(shape, shape, pre, post)), bits64(full[np.ix_(pre, post)]))
    on, w = rule_pairs(NO_SELF, weight, shape, shape)
    on1, w1 = rule_pairs(NO_SELF, weight, shape, shape, pre, post)
    assert np.array_equal(on1, on[np.ix_(pre, post)]) and np.array_equal(w1.view(np.uint32), w[np.ix_(pre, post)].view(np.uint32))


def test_validation():
    ones = np.ones((2, 6))
    with pytest.raises(ValueError, match="fit grids"):
        WeightRule.factors(ones, ones).values((2, 3), (2, 4))                  # length mismatch with the post grid
    with pytest.raises(ValueError, match="fit grids"):
        WeightRule.per_post(np.ones(5)).values((2, 3), (2, 3))
    with pytest.raises(ValueError, match="one of each"):
        WeightRule.factors(ones, np.ones((3, 6)))
    for bad in (np.nan, np.inf, -np.inf):
        broken = ones.copy()
        broken[1, 4] = bad
        with pytest.raises(ValueError, match="finite"):
            WeightRule.factors(broken, ones)
        with pytest.raises(ValueError, match="finite"):
            WeightRule.factors(ones, broken)
        with pytest.raises(ValueError, match="finite"):
            WeightRule.factors(ones, ones, scale=bad)
    with pytest.raises(ValueError, match="2\\^127"):
        WeightRule.factors(ones * 2.0 ** 63, ones * 2.0 ** 63)                 # 2 * 2^63 * 2^63 = 2^127
    WeightRule.factors(ones * 2.0 ** 63, ones * 2.0 ** 63, scale=0.999)       # just below
    with pytest.raises(ValueError, match="1 .. 65536"):
        WeightRule.factors(np.ones((0, 6)), np.ones((0, 6)))                   # P = 0
    with pytest.raises(ValueError, match="1 .. 65536"):
        WeightRule.hopfield(np.ones((0, 6)))


def test_lattice_classes_refuse_lengths_that_do_not_fit_at_connect():
    import snn_amd
    lat = snn_amd.Lattice(0)
    lat.populate(snn_amd.IzhikevichNeuron(), 2, 3)
    with pytest.raises(ValueError, match="fit grids"):
        lat.connect(ConnectionRule.all_to_all(), WeightRule.hopfield(np.ones((2, 7))))
    lat.connect(ConnectionRule.all_to_all(self_edges=False), WeightRule.hopfield(np.ones((2, 6))))
    assert lat.rule_held and lat.get_weight((0, 0), (1, 2)) == 2.0 and lat.get_weight((1, 1), (1, 1)) == 0.0
    with pytest.raises(ValueError, match="unknown weight rule"):
        WeightRule(3)
