"""What snn_connect_by_spec / snn_connect_by_specs_csr (include/snn_amd.h) write for one block, restated pair by pair from the
header's formulas: periods, wrapped integer distances, the displacement table's index, synthetic.hash32 for the draw and the
uniform weight.  A plain double loop that takes wrap and the table as numbers -- it uses neither ConnectionRule.mask nor
WeightRule.values, so that the device, the vectorised host twins and this restatement are three statements held to each other.
With wrap == 0 and the two older weight kinds it is connect_rule_cases.expected_block (test_connect_spec_host.py holds it to that
on every case of the existing plans).  Test infrastructure only."""
import numpy as np

from snn_amd import synthetic

ALL, CHEBYSHEV, EUCLIDEAN, SAME_POSITION = 0, 1, 2, 3
CONSTANT, UNIFORM, DISPLACEMENT = 0, 1, 2
WRAP_ROWS, WRAP_COLS = 1, 2
F = np.float32

_cache = {}


def _u24(seed, idx):
    return F(int(synthetic.hash32(seed, idx)) >> 8) * F(2.0 ** -24)


def table_shape(pre_shape, post_shape, wrap):
    (pr, pc), (qr, qc) = pre_shape, post_shape
    return (max(pr, qr) if wrap & WRAP_ROWS else pr + qr - 1, max(pc, qc) if wrap & WRAP_COLS else pc + qc - 1)


def _block(pre_shape, post_shape, kind, extent, self_edges, probability, edge_seed, weight_kind, lo, hi, weight_seed, wrap, table):
    (pr, pc), (qr, qc) = pre_shape, post_shape
    n_pre, n_post = pr * pc, qr * qc
    period_r, period_c = max(pr, qr), max(pc, qc)
    if weight_kind == DISPLACEMENT:
        assert table.shape == table_shape(pre_shape, post_shape, wrap) and not np.isinf(table).any()
    on = np.zeros((n_pre, n_post), bool)
    w = np.zeros((n_pre, n_post), np.float32)
    p = F(probability)
    for i in range(n_pre):
        ra, ca = i // pc, i % pc
        for j in range(n_post):
            rb, cb = j // qc, j % qc
            dr, dc = abs(ra - rb), abs(ca - cb)
            if wrap & WRAP_ROWS:
                dr = min(dr, period_r - dr)
            if wrap & WRAP_COLS:
                dc = min(dc, period_c - dc)
            idx = i * n_post + j
            edge = {ALL: True, CHEBYSHEV: max(dr, dc) <= extent, EUCLIDEAN: dr * dr + dc * dc <= extent,
                    SAME_POSITION: (ra, ca) == (rb, cb)}[kind]
            if not self_edges and (ra, ca) == (rb, cb):
                edge = False
            if p <= 0:
                edge = False
            elif p < 1 and edge:
                edge = bool(_u24(edge_seed, idx) < p)
            if weight_kind == DISPLACEMENT:
                u = (rb - ra) % period_r if wrap & WRAP_ROWS else rb - ra + (pr - 1)
                v = (cb - ca) % period_c if wrap & WRAP_COLS else cb - ca + (pc - 1)
                value = table[u, v]
                if value != value:                       # a NaN entry: None, whatever the rule says
                    edge = False
            elif weight_kind == CONSTANT:
                value = F(lo)
            else:
                value = F(lo) + (F(hi) - F(lo)) * _u24(weight_seed, idx)
            on[i, j] = edge
            if edge:
                w[i, j] = value
    on.setflags(write=False)
    w.setflags(write=False)
    return on, w


def expected_block(pre_shape, post_shape, kind, extent=0, self_edges=True, probability=1.0, edge_seed=0,
                   weight_kind=CONSTANT, lo=1.0, hi=0.0, weight_seed=0, wrap=0, table=None):
    """(connected bool[n_pre, n_post], weight float32[n_pre, n_post], 0 where there is no edge) -- computed once per case and
    shared read-only between the tests that need it"""
    table = None if table is None else np.ascontiguousarray(table, np.float32)
    key = (tuple(pre_shape), tuple(post_shape), kind, extent, bool(self_edges), float(probability), edge_seed, weight_kind,
           float(lo), float(hi), weight_seed, wrap, None if table is None else (table.shape, table.tobytes()))
    if key not in _cache:
        _cache[key] = _block(*key[:12], table)
    return _cache[key]


def expected_for(rule, weight, pre_shape, post_shape):
    """the same for a ConnectionRule / WeightRule pair (only their fields are read)"""
    return expected_block(pre_shape, post_shape, rule.kind, rule.extent, rule.self_edges, rule.probability, rule.seed,
                          weight.kind, weight.lo, weight.hi, weight.seed, rule.wrap, weight.table)


# ---- the plan of the device tests on the ragged network of test_gpu_connect_rule.py (3x5 and 5x7 neurons, 2x3 cells) ----------
def ramp(shape, scale=1.0, offset=0.0):
    """a table whose every entry names its displacement: (offset + 16 u + v) * scale"""
    u, v = np.arange(shape[0], dtype=np.float32)[:, None], np.arange(shape[1], dtype=np.float32)[None, :]
    return ((F(offset) + F(16) * u + v) * F(scale)).astype(np.float32)


def holed(shape):
    """the same, negative weights among it, with NaN (None) where (3 u + 5 v) % 7 == 0"""
    t = ramp(shape, scale=-0.125, offset=-40.0)
    u, v = np.arange(shape[0])[:, None], np.arange(shape[1])[None, :]
    t[(3 * u + 5 * v) % 7 == 0] = np.nan
    return t


def plan(ConnectionRule, WeightRule, shapes=((3, 5), (5, 7), (2, 3))):
    """four records on a network of two neuron lattices (ids 0, 1) and a spike-train lattice (id 2) of these shapes -- by default
    the ragged network's, where the tables are 3x5, 5x11 and 9x13:
    (0->0) Chebyshev 1, wrap both, no self edges, a wrapped table; (0->1) Euclidean 2, rows wrap, thinned, a table;
    (1->1) all-to-all, no wrap, a table with NaN holes; (2->1) cells -> neurons, Chebyshev 3, columns wrap, uniform weights"""
    s0, s1, _ = shapes
    return [(0, 0, ConnectionRule.chebyshev(1, self_edges=False, wrap=True),
             WeightRule.displacement(ramp(table_shape(s0, s0, 3), 0.25, 1.0), wrap=True)),
            (0, 1, ConnectionRule.euclidean(2, probability=0.37, seed=21, wrap=(True, False)),
             WeightRule.displacement(ramp(table_shape(s0, s1, WRAP_ROWS), -0.5, 3.0), wrap=(True, False))),
            (1, 1, ConnectionRule.all_to_all(), WeightRule.displacement(holed(table_shape(s1, s1, 0)))),
            (2, 1, ConnectionRule.chebyshev(3, wrap=(False, True)), WeightRule.uniform(0.5, 1.5, seed=22))]


# ---- the three weight forms of ring and torus attractors, from their mathematical form; each a closure (pre_pos, post_pos) ----
def ring_distance(n, i, j):
    d = abs(i - j)
    return min(d, n - d)


def signed_ring_displacement(n, i, j):
    """the way round the ring from i to j, in (-n/2, n/2]"""
    d = (j - i) % n
    return d if 2 * d <= n else d - n


def bump(shape, amplitude, k, offset):
    """A exp(-2 d^2 / (n k)) - B of the toroidal distance d (a ring where one dimension is 1); n the larger side"""
    rows, cols = shape
    n = max(rows, cols)

    def weight(a, b):
        d2 = ring_distance(rows, a[0], b[0]) ** 2 + ring_distance(cols, a[1], b[1]) ** 2
        return amplitude * np.exp(-2.0 * d2 / (n * k)) - offset
    return weight


def scaled_bump(shape, scale, k, offset):
    """C (exp(-2 d^2 / (n k)) - B): the scaled variant"""
    inner = bump(shape, 1.0, k, offset)
    return lambda a, b: scale * inner(a, b)


def shift(shape, amplitude):
    """A s''(delta / 5): the sigmoid's second derivative e^x (1 - e^x) / (1 + e^x)^3 of the signed circular displacement along the
    rows (an odd function: the two shift layers take +A and -A)"""
    rows = shape[0]

    def weight(a, b):
        e = np.exp(signed_ring_displacement(rows, a[0], b[0]) / 5.0)
        return amplitude * e * (1.0 - e) / (1.0 + e) ** 3
    return weight


def attractor_forms(shape):
    return {"bump": bump(shape, 3.0, 10.0, 0.9), "scaled_bump": scaled_bump(shape, 1.5, 10.0, 0.2), "shift": shift(shape, 20.0)}
