"""What snn_connect_by_rule (include/snn_amd.h) writes for one block, restated pair by pair from the header's formulas:
positions, integer distances, synthetic.hash32 and one float32 multiply-add for the weight.  Deliberately a plain loop -- it
uses neither ConnectionRule.mask nor WeightRule.values, so that the device, the vectorised host twin and this restatement
are three statements held to each other.  Test infrastructure only."""
import functools

import numpy as np

from snn_amd import synthetic

ALL, CHEBYSHEV, EUCLIDEAN, SAME_POSITION = 0, 1, 2, 3
CONSTANT, UNIFORM = 0, 1
F = np.float32


def _u24(seed, idx):
    return F(int(synthetic.hash32(seed, idx)) >> 8) * F(2.0 ** -24)


@functools.lru_cache(maxsize=None)
def _block(pre_shape, post_shape, kind, extent, self_edges, probability, edge_seed, weight_kind, lo, hi, weight_seed):
    (pr, pc), (qr, qc) = pre_shape, post_shape
    n_pre, n_post = pr * pc, qr * qc
    on = np.zeros((n_pre, n_post), bool)
    w = np.zeros((n_pre, n_post), np.float32)
    p = F(probability)
    for i in range(n_pre):
        a = (i // pc, i % pc)
        for j in range(n_post):
            b = (j // qc, j % qc)
            dr, dc = abs(a[0] - b[0]), abs(a[1] - b[1])
            idx = i * n_post + j
            edge = {ALL: True, CHEBYSHEV: max(dr, dc) <= extent, EUCLIDEAN: dr * dr + dc * dc <= extent, SAME_POSITION: a == b}[kind]
            if not self_edges and a == b:
                edge = False
            if p <= 0:
                edge = False
            elif p < 1 and edge:
                edge = bool(_u24(edge_seed, idx) < p)
            on[i, j] = edge
            if edge:
                w[i, j] = F(lo) if weight_kind == CONSTANT else F(lo) + (F(hi) - F(lo)) * _u24(weight_seed, idx)
    on.setflags(write=False)
    w.setflags(write=False)
    return on, w


def expected_block(pre_shape, post_shape, kind, extent=0, self_edges=True, probability=1.0, edge_seed=0,
                   weight_kind=CONSTANT, lo=1.0, hi=0.0, weight_seed=0):
    """(connected bool[n_pre, n_post], weight float32[n_pre, n_post], 0 where there is no edge) -- computed once per case and
    shared read-only between the tests that need it"""
    return _block(tuple(pre_shape), tuple(post_shape), kind, extent, bool(self_edges), float(probability), edge_seed,
                  weight_kind, float(lo), float(hi), weight_seed)


def expected_for(rule, weight, pre_shape, post_shape):
    """the same for a ConnectionRule / WeightRule pair (only their fields are read)"""
    return expected_block(pre_shape, post_shape, rule.kind, rule.extent, rule.self_edges, rule.probability, rule.seed,
                          weight.kind, weight.lo, weight.hi, weight.seed)
