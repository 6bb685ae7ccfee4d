"""The fixture of the factored-weight connect calls (tests/golden/hopfield_weights.npz: the reference's get_weights / weights_ie
results, see tests/golden/README) and what the tests of both handle forms share: the cases as WeightRule.hopfield / per_post
rules, and the expected block of a rule pair from the host twins.  Test infrastructure only."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hopfield_weights.npz")
CASES = ("general", "single", "many", "normal")
GRIDS = {"general": (5, 7), "single": (5, 7), "many": (4, 5), "normal": (4, 6)}       # n = rows * cols of each case

_data = None


def data():
    global _data
    if _data is None:
        with np.load(GOLDEN) as z:
            _data = {k: z[k] for k in z.files}
        for v in _data.values():
            v.setflags(write=False)
    return _data


def case(name):
    """(patterns [P, n], a, b, scalar, w float64 [n, n]) of a fixture case"""
    d = data()
    a, b, scalar = d[name + "_params"]
    return d[name + "_patterns"], float(a), float(b), float(scalar), d[name + "_w"]


def hopfield(WeightRule, name, **kw):
    patterns, a, b, scalar, _ = case(name)
    return WeightRule.hopfield(patterns, a=a, b=b, scalar=scalar, **kw)


def ie_table():
    """the weights_ie result as the reference uses it on a 5 x 7 grid: w_ie[row][col] of the post position, row-major"""
    return np.ascontiguousarray(data()["ie_table"][:5, :7]).reshape(-1)


def expected(rule_pairs, rule, weight, pre_shape, post_shape):
    """(connected uint32, weights float32) of a record on two grids, from the host twins"""
    on, w = rule_pairs(rule, weight, pre_shape, post_shape)
    return on.astype(np.uint32), w
