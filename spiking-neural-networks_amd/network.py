"""`DeviceNetwork`: thin numpy-facing owner of one C-ABI handle (include/snn_amd.h).

Mirrors the reference's GPU containers at buffer level -- `LatticeGPU` /
`LatticeNetworkGPU` (backend/src/neuron/gpu_lattices/mod.rs:327-350, 1517-1558):
named per-cell buffers (`IterateAndSpikeGPU::convert_to_gpu`,
neuron/iterate_and_spike/mod.rs:3156-3189), the flattened graph
(`InterleavingGraphGPU`, graph/mod.rs:579-943) and `run_lattices`.
The Lixirnet-style classes in `lattice.py` sit on top of this.
"""
import ctypes as C
import os

import numpy as np

from . import _lib

IZHIKEVICH, LIF, HODGKIN_HUXLEY, QUADRATIC_INTEGRATE_AND_FIRE, SIMPLE_LIF = 0, 1, 2, 3, 4
ADAPTIVE_LIF, ADAPTIVE_EXP_LIF, LEAKY_IZHIKEVICH, BCM_IZHIKEVICH = 5, 6, 7, 8
CUSTOM = 100          # the generated model of a library built by _lib.build_custom (modelgen.py)
NT_APPROXIMATE, NT_DESTEXHE, NT_DISCRETE_SPIKE, NT_EXPONENTIAL_DECAY = 0, 1, 2, 3
RC_APPROXIMATE, RC_DESTEXHE, RC_EXPONENTIAL_DECAY = 0, 1, 2
ST_NONE, ST_POISSON, ST_RATE, ST_PRESET, ST_BCM_POISSON = 0, 1, 2, 3, 4
ST_CUSTOM = 100       # the generated spike train of a library built by _lib.build_custom (modelgen.parse_description)
NT_CUSTOM = RC_CUSTOM = 100   # generated [neurotransmitter_kinetics] / [receptor_kinetics] of such a library
REFRACTORINESS_CUSTOM = 2   # neural_refractoriness$kind of the generated refractoriness of such a library
NUM_NT_TYPES = 3

_DT = {np.dtype(np.float32): "f32", np.dtype(np.uint32): "u32", np.dtype(np.int32): "i32"}
_POISON = os.environ.get("SNN_HOST_POISON", "")


def _out(shape, dtype=np.float32):
    """A buffer the library is about to fill.  SNN_HOST_POISON=1 (campaigns): pre-filled with a pattern no result holds --
    a signalling-NaN-like word for floats, 0xDB bytes otherwise -- so that a getter which returns before its transfer has
    landed, or fills less than it reports, shows in every comparison instead of depending on what the allocator handed out."""
    a = np.empty(shape, dtype)
    if _POISON:
        if a.dtype == np.float32:
            a.view(np.uint32)[...] = 0x7FA0DEAD
        else:
            a.view(np.uint8)[...] = 0xDB
    return a
_PTR = {"f32": _lib.f32p, "u32": _lib.u32p, "i32": _lib.i32p}

RULE_ALL, RULE_CHEBYSHEV, RULE_EUCLIDEAN, RULE_SAME_POSITION = 0, 1, 2, 3      # snn_connection_rule
WEIGHT_CONSTANT, WEIGHT_UNIFORM, WEIGHT_DISPLACEMENT, WEIGHT_FACTORS = 0, 1, 2, 3    # snn_weight_rule
WRAP_ROWS, WRAP_COLS = 1, 2                                                    # snn_connect_spec.wrap


def _wrap_flags(wrap):
    """wrap=True / False / (rows, cols) as WRAP_ROWS | WRAP_COLS"""
    if isinstance(wrap, (bool, np.bool_)):
        return (WRAP_ROWS | WRAP_COLS) if wrap else 0
    try:
        rows, cols = wrap
    except (TypeError, ValueError):
        raise ValueError(f"wrap is True, False or (rows, cols), not {wrap!r}") from None
    return (WRAP_ROWS if rows else 0) | (WRAP_COLS if cols else 0)


def _wrap_pair(flags):
    return bool(flags & WRAP_ROWS), bool(flags & WRAP_COLS)


def _periods(flags, pre_shape, post_shape):
    """(P_r, P_c): the ring a wrapped dimension closes on -- the larger of the two grids' sizes -- and 0 where it does not wrap"""
    return (max(pre_shape[0], post_shape[0]) if flags & WRAP_ROWS else 0,
            max(pre_shape[1], post_shape[1]) if flags & WRAP_COLS else 0)


def _pair_grid(pre_shape, post_shape, pre_index=None, post_index=None):
    """positions and pair index of every (pre, post) pair of two grids (rows, cols): pre row / col as columns [n_pre, 1], post
    row / col as rows [1, n_post], idx = i_pre * n_post + i_post as uint64 [n_pre, n_post].  pre_index / post_index (arrays of
    lattice-local indices): only those rows / columns of the grid of pairs, in the order given -- the same positions and the
    same idx, so a row, a column or a single pair costs O(N)"""
    (pr, pc), (qr, qc) = pre_shape, post_shape

    def pick(index, n, name):
        if index is None:
            return np.arange(n, dtype=np.int64)
        index = np.asarray(index, dtype=np.int64).reshape(-1)
        if index.size and (index.min() < 0 or index.max() >= n):
            raise IndexError(f"{name} outside the lattice's {n} cells")
        return index
    i, j = pick(pre_index, pr * pc, "pre_index")[:, None], pick(post_index, qr * qc, "post_index")[None, :]
    idx = i.astype(np.uint64) * np.uint64(qr * qc) + j.astype(np.uint64)
    return i // max(pc, 1), i % max(pc, 1), j // max(qc, 1), j % max(qc, 1), idx


def _u24(seed, idx):
    """(float)(hash32(seed, idx) >> 8) * 2^-24 in float32, as csrc/snn_math.hpp computes it"""
    from . import synthetic
    return (synthetic.hash32(seed, idx) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


class ConnectionRule:
    """Which pairs (pre position, post position) of two lattices are connected: the predicates the reference's users hand to
    connect(&|x, y| ...) (neuron/mod.rs:1134-1157, 1845-1935), as data the device evaluates (snn_connect_by_rule of
    include/snn_amd.h, whose wording `mask` restates in numpy).  kind RULE_ALL | RULE_CHEBYSHEV (max(dr, dc) <= extent) |
    RULE_EUCLIDEAN (dr^2 + dc^2 <= extent, the squared radius) | RULE_SAME_POSITION; self_edges=False is `x != y`;
    0 < probability < 1 adds a coin flip per pair drawn from `seed`.  wrap=True, or (rows, cols): the distances of the two radius
    rules are taken on a ring of max(pre, post) rows / columns (snn_connect_by_spec)."""

    def __init__(self, kind, extent=0, self_edges=True, probability=1.0, seed=0, wrap=False):
        if kind not in (RULE_ALL, RULE_CHEBYSHEV, RULE_EUCLIDEAN, RULE_SAME_POSITION):
            raise ValueError(f"unknown connection rule {kind!r}")
        if not 0 <= int(extent) < 2 ** 32 or not 0 <= int(seed) < 2 ** 64:
            raise ValueError("extent is a uint32, seed a uint64")
        if probability != probability:
            raise ValueError("probability is NaN")
        self.kind, self.extent, self.self_edges = int(kind), int(extent), bool(self_edges)
        self.probability, self.seed = float(probability), int(seed)
        self.wrap = _wrap_flags(wrap)

    @classmethod
    def all_to_all(cls, **kw):
        return cls(RULE_ALL, **kw)

    @classmethod
    def chebyshev(cls, r, **kw):
        return cls(RULE_CHEBYSHEV, extent=r, **kw)

    @classmethod
    def euclidean(cls, r_squared, **kw):
        return cls(RULE_EUCLIDEAN, extent=r_squared, **kw)

    @classmethod
    def same_position(cls, **kw):
        return cls(RULE_SAME_POSITION, **kw)

    def __repr__(self):
        wrap = f", wrap={_wrap_pair(self.wrap)}" if self.wrap else ""
        return (f"ConnectionRule(kind={self.kind}, extent={self.extent}, self_edges={self.self_edges}, "
                f"probability={self.probability}, seed={self.seed}{wrap})")

    def mask(self, pre_shape, post_shape, pre_index=None, post_index=None):
        """bool[n_pre, n_post]: the pairs the device call connects, for grids (rows, cols); with pre_index / post_index (lattice-local
        indices) those rows / columns of it only"""
        ra, ca, rb, cb, idx = _pair_grid(pre_shape, post_shape, pre_index, post_index)
        dr, dc = np.abs(ra - rb), np.abs(ca - cb)
        same = (dr | dc) == 0
        p_r, p_c = _periods(self.wrap, pre_shape, post_shape)
        if p_r:
            dr = np.minimum(dr, p_r - dr)
        if p_c:
            dc = np.minimum(dc, p_c - dc)
        on = np.ones(idx.shape, bool)
        if self.kind == RULE_CHEBYSHEV:
            on = np.maximum(dr, dc) <= self.extent
        elif self.kind == RULE_EUCLIDEAN:
            on = dr * dr + dc * dc <= self.extent
        elif self.kind == RULE_SAME_POSITION:
            on = same
        if not self.self_edges:
            on = on & ~same
        p = np.float32(self.probability)
        if p <= 0:
            on = np.zeros(idx.shape, bool)
        elif p < 1:
            on = on & (_u24(self.seed, idx) < p)
        return on


class WeightRule:
    """The weight of every pair a ConnectionRule connects: WeightRule.constant(w), WeightRule.uniform(lo, hi, seed) =
    lo + (hi - lo) * u24(hash(seed, idx)) in float32 -- synthetic.uniform on the pair index -- or
    WeightRule.displacement(table, wrap): the entry of a 2-D float32 table for the displacement post - pre (a convolution kernel;
    on a ring or torus with wrap), NaN where that displacement carries no edge.  The table's shape follows from the two grids:
    per dimension max(pre, post) where it wraps, pre + post - 1 where it does not (SNN_WEIGHT_DISPLACEMENT of include/snn_amd.h).
    WeightRule.factors(U, V, scale, drop_zero): w(i, j) = scale * sum_p U[p][i] * V[p][j] in float64, patterns added in order
    (SNN_WEIGHT_FACTORS) -- WeightRule.hopfield(patterns, a, b, scalar) is the reference's auto-associative matrix (U = patterns - b,
    V = patterns - a, an edge where w != 0), WeightRule.per_post(table) / per_pre(table) a weight that depends on one position only."""

    def __init__(self, kind, lo=0.0, hi=0.0, seed=0, table=None, wrap=False, _factors=None):
        # (WEIGHT_FACTORS comes from WeightRule.factors, which has checked its arrays: _factors = (U, V, scale, drop_zero))
        if kind not in (WEIGHT_CONSTANT, WEIGHT_UNIFORM, WEIGHT_DISPLACEMENT) and not (kind == WEIGHT_FACTORS and _factors is not None):
            raise ValueError(f"unknown weight rule {kind!r}")
        if not (np.isfinite(np.float32(lo)) and np.isfinite(np.float32(hi))):
            raise ValueError("weights must be finite (NaN marks the absent edge)")
        with np.errstate(over="ignore"):
            span = np.float32(hi) - np.float32(lo)
        if kind == WEIGHT_UNIFORM and not np.isfinite(span):
            raise ValueError("hi - lo overflows float32: the uniform weights would be infinite or NaN")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed is a uint64")
        self.kind, self.lo, self.hi, self.seed = int(kind), float(lo), float(hi), int(seed)
        self.table, self.wrap = None, _wrap_flags(wrap)
        self.pre_factors, self.post_factors, self.scale, self.drop_zero = _factors or (None, None, 1.0, False)      # WEIGHT_FACTORS
        if kind == WEIGHT_DISPLACEMENT:
            table = np.ascontiguousarray(table, dtype=np.float32)
            if table.ndim != 2:
                raise ValueError("the displacement table is 2-D: [row displacement, column displacement]")
            if np.isinf(table).any():
                raise ValueError("the displacement table holds an infinite weight (NaN marks a displacement without an edge)")
            self.table = table
        elif table is not None:
            raise ValueError("a table goes with WEIGHT_DISPLACEMENT")

    @classmethod
    def constant(cls, w):
        return cls(WEIGHT_CONSTANT, w)

    @classmethod
    def uniform(cls, lo, hi, seed=0):
        return cls(WEIGHT_UNIFORM, lo, hi, seed)

    @classmethod
    def displacement(cls, table, wrap=False):
        return cls(WEIGHT_DISPLACEMENT, table=table, wrap=wrap)

    @classmethod
    def factors(cls, pre_factors, post_factors, scale=1.0, drop_zero=False):
        """w(i, j) = scale * sum_p pre_factors[p][i] * post_factors[p][j]: float64 arrays [P, cells of the pre lattice] and
        [P, cells of the post lattice] (one row: [cells]), lattice-local row-major index.  drop_zero: a pair whose float64 weight
        is 0 has no edge (the reference's `w != 0` predicate); without it such a pair is an edge of weight 0."""
        u = np.atleast_2d(np.ascontiguousarray(pre_factors, dtype=np.float64))
        v = np.atleast_2d(np.ascontiguousarray(post_factors, dtype=np.float64))
        if u.ndim != 2 or v.ndim != 2:
            raise ValueError("factors are [P, cells] arrays")
        if u.shape[0] != v.shape[0]:
            raise ValueError(f"{u.shape[0]} pre factors and {v.shape[0]} post factors: one of each per term of the sum")
        if not 1 <= u.shape[0] <= 65536:
            raise ValueError(f"a factors rule takes 1 .. 65536 factors, not {u.shape[0]}")
        scale = float(scale)
        if not (np.isfinite(u).all() and np.isfinite(v).all() and np.isfinite(scale)):
            raise ValueError("factors and scale must be finite")
        # the device call's sufficient bound that no weight leaves float32, in float64 as it computes it
        bound = np.float64(u.shape[0]) * (np.abs(u).max() if u.size else 0.0) * (np.abs(v).max() if v.size else 0.0) * abs(scale)
        if not bound < 2.0 ** 127:
            raise ValueError("n_factors * max|pre_factors| * max|post_factors| * |scale| is not below 2^127: a weight could overflow float32")
        return cls(WEIGHT_FACTORS, _factors=(np.ascontiguousarray(u), np.ascontiguousarray(v), scale, bool(drop_zero)))

    @classmethod
    def hopfield(cls, patterns, a=0.0, b=0.0, scalar=1.0, drop_zero=True):
        """the reference's get_weights(n, patterns, a, b, scalar) as a rule: w[i][j] = scalar * sum_p (xi_p[i] - b)(xi_p[j] - a), an
        edge where w != 0; the zero diagonal is the connection rule's self_edges=False"""
        xi = np.atleast_2d(np.asarray(patterns, dtype=np.float64))
        return cls.factors(xi - np.float64(b), xi - np.float64(a), scalar, drop_zero)

    @classmethod
    def per_post(cls, table):
        """a weight that depends on the post position only (connect(..., lambda x, y: w[pos(y)])): one factor, the pre side all ones.
        The pre lattice's size is taken from the grids the rule is used on."""
        rule = cls.factors(np.ones((1, 1)), np.asarray(table, dtype=np.float64).reshape(1, -1))
        rule.pre_factors = None
        return rule

    @classmethod
    def per_pre(cls, table):
        """the mirror: a weight that depends on the pre position only"""
        rule = cls.factors(np.asarray(table, dtype=np.float64).reshape(1, -1), np.ones((1, 1)))
        rule.post_factors = None
        return rule

    def factor_arrays(self, pre_shape, post_shape):
        """(pre_factors [P, n_pre], post_factors [P, n_post]) of a factors rule on two grids -- the all-ones side of per_post /
        per_pre sized here -- or ValueError when the factor lengths do not match the grids"""
        n_pre, n_post = int(pre_shape[0]) * int(pre_shape[1]), int(post_shape[0]) * int(post_shape[1])
        u = np.ones((1, n_pre)) if self.pre_factors is None else self.pre_factors
        v = np.ones((1, n_post)) if self.post_factors is None else self.post_factors
        if u.shape[1] != n_pre or v.shape[1] != n_post:
            raise ValueError(f"factors of {u.shape[1]} pre and {v.shape[1]} post cells do not fit grids {tuple(pre_shape)} -> {tuple(post_shape)} "
                             f"of {n_pre} and {n_post} cells")
        return u, v

    @staticmethod
    def table_shape(pre_shape, post_shape, wrap=False):
        """the table two grids take: per dimension the ring's period where it wraps, pre + post - 1 where it does not"""
        return tuple(p or (a + b - 1) for p, a, b in zip(_periods(_wrap_flags(wrap), pre_shape, post_shape), pre_shape, post_shape))

    @classmethod
    def from_displacement_function(cls, fn, pre_shape, post_shape, wrap=False):
        """the table of a weight that depends on the displacement between the two positions only -- the reference's attractor
        experiments: connect(lambda x, y: True, w) -- filled by calling fn(pre_pos, post_pos) ONCE per displacement, on a pair of
        positions that has it; np.float32(result), or NaN (no edge) where fn returns None"""
        flags = _wrap_flags(wrap)
        periods = _periods(flags, pre_shape, post_shape)

        def pair(k, period, n_pre, n_post):
            """(pre, post) coordinates whose displacement has table index k"""
            if period:                                  # k = (post - pre) mod period; the grid that spans the ring moves
                return (0, k) if n_post == period else ((-k) % period, 0)
            d = k - (n_pre - 1)                         # k = post - pre + (n_pre - 1)
            return (0, d) if d >= 0 else (-d, 0)
        table = np.empty(cls.table_shape(pre_shape, post_shape, wrap), np.float32)
        for u in range(table.shape[0]):
            ra, rb = pair(u, periods[0], pre_shape[0], post_shape[0])
            for v in range(table.shape[1]):
                ca, cb = pair(v, periods[1], pre_shape[1], post_shape[1])
                w = fn((ra, ca), (rb, cb))
                table[u, v] = np.nan if w is None else np.float32(w)
        return cls.displacement(table, wrap)

    def __repr__(self):
        if self.kind == WEIGHT_FACTORS:
            shape = lambda f: "ones" if f is None else f.shape
            return (f"WeightRule(kind={self.kind}, pre_factors={shape(self.pre_factors)}, post_factors={shape(self.post_factors)}, "
                    f"scale={self.scale}, drop_zero={self.drop_zero})")
        if self.kind == WEIGHT_DISPLACEMENT:
            return f"WeightRule(kind={self.kind}, table={self.table.shape}, wrap={_wrap_pair(self.wrap)})"
        return f"WeightRule(kind={self.kind}, lo={self.lo}, hi={self.hi}, seed={self.seed})"

    def values(self, pre_shape, post_shape, pre_index=None, post_index=None):
        """[n_pre, n_post]: the weight the device call gives each pair (whether or not the rule connects it) -- float32, NaN where a
        displacement table says None; float64 for a factors rule; with pre_index / post_index (lattice-local indices) those rows /
        columns of it only.  A factors rule: the FLOAT64 weight w64 of include/snn_amd.h (the device stores its float32 rounding), NaN where drop_zero
        drops the pair -- one `s = s + U[p][:, None] * V[p][None, :]` per factor, in order: O(P) per pair asked for"""
        ra, ca, rb, cb, idx = _pair_grid(pre_shape, post_shape, pre_index, post_index)
        if self.kind == WEIGHT_FACTORS:
            u, v = self.factor_arrays(pre_shape, post_shape)
            i, j = (ra * max(pre_shape[1], 1) + ca).reshape(-1), (rb * max(post_shape[1], 1) + cb).reshape(-1)
            total = np.zeros((i.size, j.size), np.float64)
            for p in range(u.shape[0]):
                total = total + u[p][i][:, None] * v[p][j][None, :]
            total = total * np.float64(self.scale)
            if self.drop_zero:
                total[total == 0.0] = np.nan
            return total
        if self.kind == WEIGHT_DISPLACEMENT:
            if self.table.shape != self.table_shape(pre_shape, post_shape, _wrap_pair(self.wrap)):
                raise ValueError(f"a displacement table of shape {self.table.shape} does not fit grids {tuple(pre_shape)} -> {tuple(post_shape)}: "
                                 f"they take {self.table_shape(pre_shape, post_shape, _wrap_pair(self.wrap))}")
            p_r, p_c = _periods(self.wrap, pre_shape, post_shape)
            u = (rb - ra) % p_r if p_r else rb - ra + (pre_shape[0] - 1)
            v = (cb - ca) % p_c if p_c else cb - ca + (pre_shape[1] - 1)
            return self.table[u, v]
        lo, hi = np.float32(self.lo), np.float32(self.hi)
        if self.kind == WEIGHT_CONSTANT:
            return np.full(idx.shape, lo, np.float32)
        return (lo + (hi - lo) * _u24(self.seed, idx)).astype(np.float32)


def check_rule_pair(rule, weight):
    """a displacement table is indexed on the rings its rule measures distances on: the two wrap settings must agree"""
    if weight.kind == WEIGHT_DISPLACEMENT and weight.wrap != rule.wrap:
        raise ValueError(f"the displacement table was built with wrap={_wrap_pair(weight.wrap)}, its rule with wrap={_wrap_pair(rule.wrap)}")


def rule_pairs(rule, weight, pre_shape, post_shape, pre_index=None, post_index=None):
    """(connected bool, weights float32, 0 where there is no edge) [n_pre, n_post]: the graph one connect record writes on the
    device, from the records' host twins -- a NaN of the weight twin (a None of the displacement table, a pair that drop_zero of a
    factors rule drops) is an absent edge; a factors rule's float64 weights are rounded to float32 here, as the device stores them"""
    check_rule_pair(rule, weight)
    on, w = rule.mask(pre_shape, post_shape, pre_index, post_index), weight.values(pre_shape, post_shape, pre_index, post_index)
    on = on & ~np.isnan(w)
    return on, np.where(on, w, np.float32(0)).astype(np.float32)


class DeviceNetwork:
    def __init__(self, model=IZHIKEVICH, nt_kinetics=NT_APPROXIMATE, receptor_kinetics=RC_APPROXIMATE,
                 spike_train=ST_NONE, device=0, lib_path=None):
        self._L = _lib.load(lib_path)
        self._h = _lib.H()
        self._check(self._L.snn_network_create(device, model, nt_kinetics, receptor_kinetics, spike_train,
                                              C.byref(self._h)))
        self.model = model
        self.lattices = {}          # id -> (rows, cols, is_spike_train)
        self._peak_totals_rows = {}  # id -> n_windows of set_peak_totals
        self.finalized = False

    def _check(self, code):
        _lib.check(code, self._L)

    # ---- lifetime -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.snn_network_destroy(self._h)
            self._h = _lib.H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- construction ---------------------------------------------------------------------
    def add_lattice(self, id, rows, cols):
        self._check(self._L.snn_network_add_lattice(self._h, id, rows, cols))
        self.lattices[id] = (rows, cols, False)

    def add_spike_train_lattice(self, id, rows, cols):
        self._check(self._L.snn_network_add_spike_train_lattice(self._h, id, rows, cols))
        self.lattices[id] = (rows, cols, True)

    def finalize(self, shard_index=None, n_shards=None, csr=False, by_lattice=False):
        """csr=True: the handle holds a sparse CSR graph (set_graph_csr) instead of a dense matrix; by_lattice=True
        (sparse shard handles): the shard owns slab `shard_index` of EVERY neuron lattice instead of one contiguous slot"""
        if csr:
            self._check(self._L.snn_network_use_csr(self._h, 1))
        self.csr = bool(csr)
        if shard_index is None:
            self._check(self._L.snn_network_finalize(self._h))
        elif by_lattice:
            self._check(self._L.snn_network_finalize_shard_by_lattice(self._h, shard_index, n_shards))
        else:
            self._check(self._L.snn_network_finalize_shard(self._h, shard_index, n_shards))
        self.finalized = True
        nn, nc, q0, q1 = (C.c_uint32() for _ in range(4))
        self._check(self._L.snn_network_sizes(self._h, C.byref(nn), C.byref(nc), C.byref(q0), C.byref(q1)))
        self.n_neurons, self.n_cells = nn.value, nc.value
        self.n_tot = self.n_neurons + self.n_cells
        self.post_begin, self.post_end = q0.value, q1.value
        n = C.c_uint32()
        self._check(self._L.snn_shard_ranges(self._h, None, None, 0, C.byref(n)))
        b, e = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
        if n.value:
            self._check(self._L.snn_shard_ranges(self._h, b.ctypes.data_as(_lib.u32p), e.ctypes.data_as(_lib.u32p), n.value, C.byref(n)))
        self.ranges = [(int(x), int(y)) for x, y in zip(b, e)]          # owned [begin, end), ascending
        return self

    @property
    def owned(self):
        """global indices of the neurons this handle owns, ascending (the row order of set_graph_csr)"""
        return (np.concatenate([np.arange(b, e, dtype=np.int64) for b, e in self.ranges]) if self.ranges
                else np.zeros(0, np.int64))

    def lattice_range(self, id):
        first, count = C.c_uint32(), C.c_uint32()
        self._check(self._L.snn_network_lattice_range(self._h, id, C.byref(first), C.byref(count)))
        return first.value, count.value

    # ---- attributes -----------------------------------------------------------------------
    def set_attr(self, id, name, values):
        a = np.ascontiguousarray(values)
        if a.dtype not in _DT:
            raise TypeError(f"attribute arrays must be float32 / uint32 / int32, not {a.dtype}")
        kind = _DT[a.dtype]
        fn = getattr(self._L, f"snn_set_attr_{kind}")
        self._check(fn(self._h, id, name.encode(), a.ctypes.data_as(_PTR[kind]), a.size))

    def get_attr(self, id, name, dtype=np.float32, per_type=False):
        rows, cols, _ = self.lattices[id]
        n = rows * cols
        out = _out((n, NUM_NT_TYPES) if per_type else (n,), dtype=dtype)
        kind = _DT[np.dtype(dtype)]
        fn = getattr(self._L, f"snn_get_attr_{kind}")
        self._check(fn(self._h, id, name.encode(), out.ctypes.data_as(_PTR[kind]), out.size))
        return out

    # ---- graph ----------------------------------------------------------------------------
    def set_graph_dense(self, weights, connections):
        w = np.ascontiguousarray(weights, dtype=np.float32)
        c = np.ascontiguousarray(connections, dtype=np.uint32)
        if w.shape != c.shape or w.ndim != 2 or w.shape[0] != w.shape[1]:
            raise ValueError("weights / connections must be equal square matrices [n_tot, n_tot]")
        self._check(self._L.snn_set_graph_dense(self._h, w.ctypes.data_as(_lib.f32p), c.ctypes.data_as(_lib.u32p),
                                               w.shape[0]))

    def get_graph_dense(self):
        n = self.n_tot
        w = np.zeros((n, n), np.float32)
        c = np.zeros((n, n), np.uint32)
        self._check(self._L.snn_get_graph_dense(self._h, w.ctypes.data_as(_lib.f32p), c.ctypes.data_as(_lib.u32p), n))
        return w, c

    def set_graph_rows(self, pre_begin, weights, connections):
        """rows [pre_begin, pre_begin+len) of the [n_tot, n_neurons] matrix"""
        w = np.ascontiguousarray(weights, dtype=np.float32)
        c = np.ascontiguousarray(connections, dtype=np.uint32)
        if w.shape != c.shape or w.ndim != 2 or w.shape[1] != self.n_neurons:
            raise ValueError("row blocks must be [rows, n_neurons]")
        self._check(self._L.snn_set_graph_rows(self._h, pre_begin, w.shape[0], w.ctypes.data_as(_lib.f32p),
                                              c.ctypes.data_as(_lib.u32p)))

    def get_graph_rows(self, pre_begin, pre_count):
        w = np.zeros((pre_count, self.n_neurons), np.float32)
        c = np.zeros((pre_count, self.n_neurons), np.uint32)
        self._check(self._L.snn_get_graph_rows(self._h, pre_begin, pre_count, w.ctypes.data_as(_lib.f32p),
                                              c.ctypes.data_as(_lib.u32p)))
        return w, c

    # the Graph trait on the device graph (graph/mod.rs:42-72); interleaved global indices.  A dense handle is asked through
    # snn_graph_*, a sparse one (finalize(csr=True)) through snn_graph_csr_*: the same answers, and a structure that is fixed
    # unless graph_edit is asked to change it (structure=True: snn_graph_csr_edit_structure)
    def _graph_fn(self, name):
        return getattr(self._L, ("snn_graph_csr_" if getattr(self, "csr", False) else "snn_graph_") + name)

    @staticmethod
    def _pairs(pre, post):
        p = np.ascontiguousarray(np.asarray(pre).reshape(-1), dtype=np.uint32)
        q = np.ascontiguousarray(np.asarray(post).reshape(-1), dtype=np.uint32)
        if p.size != q.size:
            raise ValueError("pre and post must have equal lengths")
        if np.any(p != np.asarray(pre).reshape(-1)) or np.any(q != np.asarray(post).reshape(-1)):
            raise ValueError("indices must be non-negative integers below 2^32")
        return p, q

    def graph_lookup(self, pre, post):
        """lookup_weight for the pairs (pre[k], post[k]): (weights float32[n], connected bool[n]); an absent edge reads 0.0 / False"""
        p, q = self._pairs(pre, post)
        w, c = _out(p.size, np.float32), _out(p.size, np.uint8)
        self._check(self._graph_fn("lookup")(self._h, p.ctypes.data_as(_lib.u32p), q.ctypes.data_as(_lib.u32p), p.size,
                                               w.ctypes.data_as(_lib.f32p), c.ctypes.data_as(_lib.u8p)))
        return w, c != 0

    def graph_edit(self, pre, post, weights, connected=None, structure=False):
        """edit_weight for the pairs (pre[k], post[k]): Some(weights[k]) where connected[k] (None: everywhere), None elsewhere.  Applied
        as if one after another: of a pair listed twice the last wins.  A NaN weight of a connected pair is refused.
        On a sparse handle the structure is fixed by default: connected[k] on a stored edge sets its weight and not connected[k] on
        an absent pair is a no-op; connecting an absent pair or disconnecting a stored edge is refused (SnnError, BAD_ARG, the pair
        named) before anything is written.  structure=True lifts that (snn_graph_csr_edit_structure): absent pairs are connected and
        stored edges removed, merged on the device and committed as by set_graph_csr; kept edges keep their current weights, traces,
        dw and counters, and the edge order of get_graph_csr is graph_csr_structure()'s afterwards.  A dense handle takes the
        keyword and does what it always does: its edits are structural already."""
        p, q = self._pairs(pre, post)
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
        if np.ndim(weights) == 0:                # one weight for every pair
            w = np.full(p.size, w[0], np.float32)
        c = np.ones(p.size, np.uint8) if connected is None else np.ascontiguousarray(np.asarray(connected).reshape(-1) != 0, dtype=np.uint8)
        if w.size != p.size or c.size != p.size:
            raise ValueError("weights / connected must have one entry per pair")
        sparse = getattr(self, "csr", False)
        fn = self._L.snn_graph_csr_edit_structure if structure and sparse else self._graph_fn("edit")
        self._check(fn(self._h, p.ctypes.data_as(_lib.u32p), q.ctypes.data_as(_lib.u32p), w.ctypes.data_as(_lib.f32p),
                       c.ctypes.data_as(_lib.u8p), p.size))
        if structure and sparse:
            nnz = C.c_uint64()
            self._check(self._L.snn_graph_csr_nnz(self._h, C.byref(nnz)))
            self._nnz = int(nnz.value)

    def _graph_line(self, fn, which):
        n = C.c_uint64()
        self._check(fn(self._h, which, None, None, 0, C.byref(n)))
        index, w = _out(int(n.value), np.uint32), _out(int(n.value), np.float32)
        if n.value:
            self._check(fn(self._h, which, index.ctypes.data_as(_lib.u32p), w.ctypes.data_as(_lib.f32p), index.size, C.byref(n)))
            if n.value != index.size:
                raise RuntimeError("the graph changed between the two calls of a line query")
        return index, w

    def graph_incoming(self, post):
        """get_incoming_connections: (pre index uint32[count] ascending, weights float32[count]) of the edges into `post`; dense
        and sparse handles alike"""
        return self._graph_line(self._graph_fn("incoming"), int(post))

    def graph_outgoing(self, pre):
        """get_outgoing_connections: (post index uint32[count] ascending, weights float32[count]) of the edges out of `pre` (a shard
        handle: into the columns it owns); dense and sparse handles alike"""
        return self._graph_line(self._graph_fn("outgoing"), int(pre))

    def set_graph_csr(self, row_ptr, pre_index, weights):
        """CSR by OWNED postsynaptic neuron in ascending global order (self.owned): row_ptr[n_owned + 1], pre_index
        ascending inside each row"""
        rp = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        pi = np.ascontiguousarray(pre_index, dtype=np.uint32)
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if rp.size != sum(e - b for b, e in self.ranges) + 1 or pi.size != w.size:
            raise ValueError("row_ptr must have one entry per owned neuron + 1 and pre_index / weights equal lengths")
        self._check(self._L.snn_set_graph_csr(self._h, rp.ctypes.data_as(_lib.u64p), pi.ctypes.data_as(_lib.u32p),
                                             w.ctypes.data_as(_lib.f32p), w.size))
        self._nnz = int(w.size)                  # (a failed call leaves the previous graph in place)

    def get_graph_csr(self):
        w = _out(getattr(self, "_nnz", 0), np.float32)
        self._check(self._L.snn_get_graph_csr(self._h, w.ctypes.data_as(_lib.f32p), w.size))
        return w

    def fill_graph_synthetic(self, seed, lo, hi, with_diagonal=False):
        self._check(self._L.snn_fill_graph_synthetic(self._h, seed, lo, hi, int(with_diagonal)))

    def _lattice_shape(self, lattice_id):
        """(rows, cols) of a lattice of this handle, None for an id it does not know (the device call names it)"""
        shape = self.lattices.get(int(lattice_id))
        return None if shape is None else tuple(shape[:2])

    def _connect_factors(self, pre_id, post_id, rule, weight, what):
        """snn_connect_factors of one (ConnectionRule, WeightRule or None) pair, and the arrays it points into (they must outlive the
        call).  Without a factors rule the extension stays empty: the call then writes what snn_connect_by_spec writes."""
        spec = self._connect_spec(pre_id, post_id, rule, weight, what)
        if weight is None or weight.kind != WEIGHT_FACTORS:
            return _lib.ConnectFactors(spec, 0, 0, 0.0, None, None), ()
        shapes = self._lattice_shape(pre_id), self._lattice_shape(post_id)
        if None in shapes:                               # an unknown id: sized for nothing, refused by the call before it reads them
            u = v = np.zeros((weight.pre_factors if weight.pre_factors is not None else weight.post_factors).shape[0])
        else:
            u, v = (np.ascontiguousarray(f) for f in weight.factor_arrays(*shapes))       # ValueError: lengths that do not fit
        item = _lib.ConnectFactors(spec, (u.shape[0]), int(weight.drop_zero), weight.scale, u.ctypes.data_as(_lib.f64p), v.ctypes.data_as(_lib.f64p))
        return item, (u, v)

    def _connect_spec(self, pre_id, post_id, rule, weight, what):
        """snn_connect_spec of one (ConnectionRule, WeightRule or None) pair; the spec points into weight.table"""
        weight = WeightRule.constant(1.0) if weight is None else weight
        if not isinstance(rule, ConnectionRule) or not isinstance(weight, WeightRule):
            raise TypeError(f"{what} takes a ConnectionRule and a WeightRule")
        check_rule_pair(rule, weight)
        record = _lib.ConnectRecord(int(pre_id), int(post_id), rule.kind, rule.extent, int(rule.self_edges), rule.probability,
                                    rule.seed, weight.kind, weight.lo, weight.hi, weight.seed)
        if weight.kind != WEIGHT_DISPLACEMENT:
            return _lib.ConnectSpec(record, rule.wrap, 0, 0, None)
        return _lib.ConnectSpec(record, rule.wrap, weight.table.shape[0], weight.table.shape[1], weight.table.ctypes.data_as(_lib.f32p))

    def connect_by_rule(self, pre_id, post_id, rule, weight=None):
        """the reference's connect(...) between lattice `pre_id` and neuron lattice `post_id` (the same id: internally), evaluated
        on the device (snn_connect_by_spec): `rule` a ConnectionRule, `weight` a WeightRule (None: every edge weighs 1).
        rule.mask / weight.values are the same graph on the host (rule_pairs: a NaN of a displacement table is no edge)."""
        if weight is not None and isinstance(weight, WeightRule) and weight.kind == WEIGHT_FACTORS:
            item, keep = self._connect_factors(pre_id, post_id, rule, weight, "connect_by_rule")
            self._check(self._L.snn_connect_by_factors(self._h, C.byref(item)))
            return
        spec = self._connect_spec(pre_id, post_id, rule, weight, "connect_by_rule")
        self._check(self._L.snn_connect_by_spec(self._h, C.byref(spec)))

    def connect_sparse(self, plan):
        """connect(...) on a sparse handle, the graph merged on the device (snn_connect_by_specs_csr): `plan` is a list of
        (pre_id, post_id, ConnectionRule, WeightRule or None), applied in order and committed once.  Every edge outside the plan's
        blocks keeps its current weight; traces, dw and counters of the whole graph restart at 0.  The committed edge order is
        graph_csr_structure()'s.  A displacement table visits the candidates of its rule: on a large handle give it a radius."""
        for k, entry in enumerate(plan):
            if not isinstance(entry, (tuple, list)) or len(entry) != 4:
                raise TypeError(f"plan[{k}] must be (pre_id, post_id, ConnectionRule, WeightRule or None)")
        if any(isinstance(entry[3], WeightRule) and entry[3].kind == WEIGHT_FACTORS for entry in plan):
            # record kinds mix in one call: the factors form takes every spec, and reads its extension for factors records only
            items, keep = (_lib.ConnectFactors * len(plan))(), []
            for k, entry in enumerate(plan):
                items[k], arrays = self._connect_factors(*entry, f"plan[{k}]: connect_sparse")
                keep.append(arrays)
            self._check(self._L.snn_connect_by_factors_csr(self._h, items, len(plan)))
        else:
            specs = (_lib.ConnectSpec * max(len(plan), 1))()
            for k, entry in enumerate(plan):
                specs[k] = self._connect_spec(*entry, f"plan[{k}]: connect_sparse")
            self._check(self._L.snn_connect_by_specs_csr(self._h, specs, len(plan)))
        nnz = C.c_uint64()
        self._check(self._L.snn_graph_csr_nnz(self._h, C.byref(nnz)))
        self._nnz = int(nnz.value)

    def graph_csr_structure(self):
        """(row_ptr uint64[n_owned + 1], pre_index uint32[nnz]) of a sparse handle: the edge order of get_graph_csr"""
        nnz = C.c_uint64()
        self._check(self._L.snn_graph_csr_nnz(self._h, C.byref(nnz)))
        rp = _out(sum(e - b for b, e in self.ranges) + 1, np.uint64)
        pi = _out(int(nnz.value), np.uint32)
        self._check(self._L.snn_get_graph_csr_structure(self._h, rp.ctypes.data_as(_lib.u64p), pi.ctypes.data_as(_lib.u32p), pi.size))
        return rp, pi

    # ---- switches -------------------------------------------------------------------------
    def set_synapses(self, electrical=True, chemical=False):
        self._check(self._L.snn_set_synapses(self._h, int(electrical), int(chemical)))

    def set_plasticity(self, id, a_plus=2.0, a_minus=2.0, tau_plus=4.5, tau_minus=4.5, dt=0.1, do_plasticity=True):
        self._check(self._L.snn_set_plasticity(self._h, id, a_plus, a_minus, tau_plus, tau_minus, dt,
                                              int(do_plasticity)))

    def set_history(self, voltage=False, spikes=False):
        self._check(self._L.snn_set_history(self._h, int(voltage), int(spikes)))

    def reset_history(self):
        self._check(self._L.snn_reset_history(self._h))

    def reset_timing(self):
        self._check(self._L.snn_reset_timing(self._h))

    @property
    def clock(self):
        v = C.c_uint64()
        self._check(self._L.snn_get_clock(self._h, C.byref(v)))
        return v.value

    def set_clock(self, clock):
        """internal_clock of the network (LatticeNetworkGPU::from_network): firing times are absolute step numbers"""
        self._check(self._L.snn_set_clock(self._h, int(clock)))

    def set_spike_train_clock(self, id, clock):
        self._check(self._L.snn_set_spike_train_clock(self._h, id, int(clock)))

    def spike_train_clock(self, id):
        v = C.c_uint64()
        self._check(self._L.snn_get_spike_train_clock(self._h, id, C.byref(v)))
        return v.value

    # ---- test support ---------------------------------------------------------------------
    def checkpoint(self):
        """keeps everything a later run call reads (snn_debug_checkpoint); restore_checkpoint puts it back"""
        self._check(self._L.snn_debug_checkpoint(self._h, 0))

    def restore_checkpoint(self):
        self._check(self._L.snn_debug_checkpoint(self._h, 1))

    def verify_report(self):
        """what the last mismatch of the option "verify" was ("" when there was none)"""
        return (self._L.snn_debug_verify_report(self._h) or b"").decode()

    # ---- stepping -------------------------------------------------------------------------
    def run(self, iterations):
        self._check(self._L.snn_run(self._h, iterations))

    def step_begin(self):
        self._check(self._L.snn_step_begin(self._h))

    def step_end(self):
        self._check(self._L.snn_step_end(self._h))

    def step_begin_local(self):
        self._check(self._L.snn_step_begin_local(self._h))

    def refresh_begin(self):
        """packs the current state of the plan's planes when the mirror lacks one of them (snn_refresh_begin); True if so"""
        needed = C.c_int(0)
        self._check(self._L.snn_refresh_begin(self._h, C.byref(needed)))
        return bool(needed.value)

    def refresh_end(self):
        self._check(self._L.snn_refresh_end(self._h))

    def exchange_plan(self):
        """The shard handle's exchange plan (snn_exchange_plan + per-peer segments): a dict with mode ("allgather" |
        "halo"), n_shards, shard_index, shard_stride, planes, plane_id, send / recv (device pointers), send_words /
        recv_words, and per-peer arrays send_offset / send_count / recv_offset / recv_count in 32-bit words."""
        plan = _lib.ExchangePlan()
        self._check(self._L.snn_exchange_plan_get(self._h, C.byref(plan)))
        g = plan.n_shards
        arrs = [np.zeros(g, np.uint64) for _ in range(4)]
        self._check(self._L.snn_exchange_peers(self._h, *[a.ctypes.data_as(_lib.u64p) for a in arrs]))
        return {"mode": "halo" if plan.mode == _lib.EXCHANGE_HALO else "allgather", "n_shards": g,
                "shard_index": plan.shard_index, "shard_stride": plan.shard_stride, "planes": plan.planes,
                "plane_id": list(plan.plane_id)[:plan.planes], "send": plan.send, "recv": plan.recv,
                "send_words": plan.send_words, "recv_words": plan.recv_words,
                "send_offset": arrs[0], "send_count": arrs[1], "recv_offset": arrs[2], "recv_count": arrs[3]}

    def p2p_local(self):
        """the peer form's endpoints of this handle (snn_p2p_local): recv0, recv1, flags addresses + per-shard offsets / counts"""
        r0, r1, fl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        g = self.exchange_plan()["n_shards"]
        off, cnt = np.zeros(g, np.uint64), np.zeros(g, np.uint64)
        self._check(self._L.snn_p2p_local(self._h, C.byref(r0), C.byref(r1), C.byref(fl), off.ctypes.data_as(_lib.u64p),
                                          cnt.ctypes.data_as(_lib.u64p)))
        return {"recv": (r0.value, r1.value), "flags": fl.value, "offsets": off, "counts": cnt}

    def p2p_ipc_export(self):
        """192 bytes: the IPC handles of the two receive sets and the done counters (snn_p2p_ipc_export), for a peer in ANOTHER process"""
        buf = C.create_string_buffer(192)
        self._check(self._L.snn_p2p_ipc_export(self._h, buf))
        return bytes(buf.raw)

    def p2p_ipc_import(self, handles, device=0):
        """maps a peer's exported handles into this process: (recv0, recv1, flags) addresses for p2p_connect"""
        r0, r1, fl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.snn_p2p_ipc_import(device, C.create_string_buffer(handles, 192), C.byref(r0), C.byref(r1), C.byref(fl)))
        return r0.value, r1.value, fl.value

    def p2p_ipc_close(self, recv0, recv1, flags, device=0):
        """unmaps what p2p_ipc_import mapped (after the peers have stopped stepping in the peer form)"""
        self._check(self._L.snn_p2p_ipc_close(device, int(recv0), int(recv1), int(flags)))

    def p2p_connect(self, peer, recv0, recv1, flags, recv_offset):
        self._check(self._L.snn_p2p_connect(self._h, peer, int(recv0), int(recv1), int(flags), int(recv_offset)))

    def p2p_commit(self):
        self._check(self._L.snn_p2p_commit(self._h))

    def halo_needs(self, peer):
        """ascending global indices of shard `peer`'s neurons that this handle's CSR rows read"""
        n = C.c_uint32()
        self._check(self._L.snn_halo_needs(self._h, peer, None, 0, C.byref(n)))
        out = _out(n.value, np.uint32)
        if n.value:
            self._check(self._L.snn_halo_needs(self._h, peer, out.ctypes.data_as(_lib.u32p), out.size, C.byref(n)))
        return out

    def cells_read(self):
        """indices (into the cell population) of the spike-train cells this handle advances: all of them, or -- sparse
        shard handles of a multi-rank run -- the ones its own rows read"""
        n = C.c_uint32()
        self._check(self._L.snn_cells_read(self._h, None, 0, C.byref(n)))
        out = _out(n.value, np.uint32)
        if n.value:
            self._check(self._L.snn_cells_read(self._h, out.ctypes.data_as(_lib.u32p), out.size, C.byref(n)))
        return out

    def halo_set_sends(self, peer, indices):
        a = np.ascontiguousarray(indices, dtype=np.uint32)
        self._check(self._L.snn_halo_set_sends(self._h, peer, a.ctypes.data_as(_lib.u32p), a.size))

    def halo_commit(self):
        self._check(self._L.snn_halo_commit(self._h))

    def exchange(self, comm):
        """one RCCL exchange of the packed segments on the handle's stream (comm: parallel.LibraryComm or ncclComm_t)"""
        self._check(self._L.snn_exchange(self._h, C.c_void_p(int(comm))))

    def exchange_halo_lists(self, comm):
        self._check(self._L.snn_comm_exchange_halo_lists(self._h, C.c_void_p(int(comm))))

    def run_sharded_without_exchange(self, iterations):
        """the library's sharded step loop with snn_exchange_noop as the transport (timing of one rank's step)"""
        fn = C.cast(self._L.snn_exchange_noop, C.c_void_p)
        self._check(self._L.snn_run_sharded_custom(self._h, fn, None, int(iterations)))

    def run_sharded_custom(self, exchange, iterations):
        """the library's sharded step loop with the caller's transport: `exchange(hip_stream)` is called once per step
        after the outgoing segments were enqueued and must have moved the plan's segments when it returns (with the option
        "halo_direct" 2 it reads the pointers of `exchange_plan()` anew at every call: two sets of segments alternate)"""
        err = []

        def thunk(_user, stream):
            try:
                exchange(stream)
                return 0
            except BaseException as e:      # never let an exception cross the C frame
                err.append(e)
                return 1

        cb = _lib.EXCHANGE_FN(thunk)
        try:
            self._check(self._L.snn_run_sharded_custom(self._h, C.cast(cb, C.c_void_p), None, int(iterations)))
        except Exception:
            if err:
                raise err[0]
            raise

    def run_sharded(self, comm, iterations):
        """`iterations` steps with the library's own RCCL loop (every rank calls it with its shard handle)"""
        self._check(self._L.snn_run_sharded(self._h, C.c_void_p(int(comm)), int(iterations)))

    def set_stream(self, hip_stream):
        """Adopt a caller's hipStream_t (int handle): step_begin / step_end then only enqueue on it.
        None returns to the handle's own stream.  The legacy default stream (handle 0) cannot be adopted --
        create a real stream (e.g. torch.cuda.Stream()) so that collectives can be ordered against it."""
        if hip_stream is None:
            self._check(self._L.snn_set_stream(self._h, None))
            return
        if int(hip_stream) == 0:
            raise ValueError("the default (null) stream cannot be adopted: pass a non-default stream handle")
        self._check(self._L.snn_set_stream(self._h, C.c_void_p(int(hip_stream))))

    def synchronize(self):
        self._check(self._L.snn_synchronize(self._h))

    def stream(self):
        p = C.c_void_p()
        self._check(self._L.snn_stream(self._h, C.byref(p)))
        return p.value

    # ---- histories ------------------------------------------------------------------------
    def history_steps(self):
        v = C.c_uint64()
        self._check(self._L.snn_history_steps(self._h, C.byref(v)))
        return v.value

    def voltage_history(self, id):
        rows, cols, _ = self.lattices[id]
        steps = self.history_steps()
        out = _out((steps, rows * cols), np.float32)
        self._check(self._L.snn_get_voltage_history(self._h, id, out.ctypes.data_as(_lib.f32p), out.size))
        return out

    def spike_history(self, id):
        rows, cols, _ = self.lattices[id]
        steps = self.history_steps()
        out = _out((steps, rows * cols), np.uint8)
        self._check(self._L.snn_get_spike_history(self._h, id, out.ctypes.data_as(_lib.u8p), out.size))
        return out

    def set_bcm(self, id, decay=0.1, average_scalar=0.1, dt=0.1, do_plasticity=True):
        """BCM rule (plasticity/mod.rs:72-116) for lattice `id` instead of STDP"""
        self._check(self._L.snn_set_bcm(self._h, id, decay, average_scalar, dt, int(do_plasticity)))

    # ---- reward modulation (RewardModulatedLattice, neuron/mod.rs:2719-3417) -----------------
    def set_reward_modulator(self, id, dopamine=0.0, tau_d=20.0, tau_c=0.0001, a_plus=2.0, a_minus=2.0, tau_plus=4.5,
                             tau_minus=4.5, dt=0.1, do_modulation=True):
        self._check(self._L.snn_set_reward_modulator(self._h, id, dopamine, tau_d, tau_c, a_plus, a_minus, tau_plus,
                                                    tau_minus, dt, int(do_modulation)))

    def dopamine(self, id):
        out = C.c_float()
        self._check(self._L.snn_get_dopamine(self._h, id, C.byref(out)))
        return np.float32(out.value)

    def apply_reward(self, reward):
        self._check(self._L.snn_apply_reward(self._h, reward))

    def run_with_reward(self, reward):
        self._check(self._L.snn_run_with_reward(self._h, reward))

    def set_trace_rows(self, pre_begin, traces):
        t = np.ascontiguousarray(traces, dtype=np.float32)
        if t.ndim != 2 or t.shape[1] != self.n_neurons:
            raise ValueError("traces must be [rows][n_neurons]")
        self._check(self._L.snn_set_trace_rows(self._h, pre_begin, t.shape[0], t.ctypes.data_as(_lib.f32p)))

    def get_trace_rows(self, pre_begin, pre_count):
        t = np.zeros((pre_count, self.n_neurons), np.float32)
        self._check(self._L.snn_get_trace_rows(self._h, pre_begin, pre_count, t.ctypes.data_as(_lib.f32p)))
        return t

    # ---- connections between lattices of a reward-modulated network (include/snn_amd.h, snn_set_connection_kind) ----
    def set_connection_kind(self, pre_id, post_id, kind):
        """0 a plain network's connection, 1 RewardModulatedConnection::RewardModulatedWeight, 2 RewardModulatedConnection::Weight"""
        self._check(self._L.snn_set_connection_kind(self._h, pre_id, post_id, int(kind)))

    def set_pending_rows(self, pre_begin, pending):
        t = np.ascontiguousarray(pending, dtype=np.float32)
        if t.ndim != 2 or t.shape[1] != self.n_neurons:
            raise ValueError("pending must be [rows][n_neurons]")
        self._check(self._L.snn_set_pending_rows(self._h, pre_begin, t.shape[0], t.ctypes.data_as(_lib.f32p)))

    def get_pending_rows(self, pre_begin, pre_count):
        t = np.zeros((pre_count, self.n_neurons), np.float32)
        self._check(self._L.snn_get_pending_rows(self._h, pre_begin, pre_count, t.ctypes.data_as(_lib.f32p)))
        return t

    def set_counter_rows(self, pre_begin, counters):
        """TraceRSTDP::counter (0 / 1) per connection, rows as set_pending_rows"""
        t = np.ascontiguousarray(counters, dtype=np.uint8)
        if t.ndim != 2 or t.shape[1] != self.n_neurons:
            raise ValueError("counters must be [rows][n_neurons]")
        self._check(self._L.snn_set_counter_rows(self._h, pre_begin, t.shape[0], t.ctypes.data_as(_lib.u8p)))

    def get_counter_rows(self, pre_begin, pre_count):
        t = np.zeros((pre_count, self.n_neurons), np.uint8)
        self._check(self._L.snn_get_counter_rows(self._h, pre_begin, pre_count, t.ctypes.data_as(_lib.u8p)))
        return t

    def set_traces_csr(self, traces):
        t = np.ascontiguousarray(traces, dtype=np.float32)
        self._check(self._L.snn_set_traces_csr(self._h, t.ctypes.data_as(_lib.f32p), t.size))

    def get_traces_csr(self):
        t = _out(getattr(self, "_nnz", 0), np.float32)
        self._check(self._L.snn_get_traces_csr(self._h, t.ctypes.data_as(_lib.f32p), t.size))
        return t

    def set_pending_csr(self, pending):
        """TraceRSTDP::dw per stored edge of a sparse handle, in the edge order of set_graph_csr"""
        t = np.ascontiguousarray(pending, dtype=np.float32)
        self._check(self._L.snn_set_pending_csr(self._h, t.ctypes.data_as(_lib.f32p), t.size))

    def get_pending_csr(self):
        t = _out(getattr(self, "_nnz", 0), np.float32)
        self._check(self._L.snn_get_pending_csr(self._h, t.ctypes.data_as(_lib.f32p), t.size))
        return t

    def set_counters_csr(self, counters):
        t = np.ascontiguousarray(counters, dtype=np.uint8)
        self._check(self._L.snn_set_counters_csr(self._h, t.ctypes.data_as(_lib.u8p), t.size))

    def get_counters_csr(self):
        t = _out(getattr(self, "_nnz", 0), np.uint8)
        self._check(self._L.snn_get_counters_csr(self._h, t.ctypes.data_as(_lib.u8p), t.size))
        return t

    def set_firing_times(self, id, cell_ptr, times):
        """PresetSpikeTrain firing times of spike-train lattice `id`: cell i fires through
        times[cell_ptr[i]:cell_ptr[i+1]] cyclically (spike_train/mod.rs:753-833)."""
        cp = np.ascontiguousarray(cell_ptr, dtype=np.uint32)
        t = np.ascontiguousarray(times, dtype=np.float32)
        rows, cols, _ = self.lattices[id]
        if cp.size != rows * cols + 1:
            raise ValueError("cell_ptr must have rows*cols + 1 entries")
        self._check(self._L.snn_set_firing_times(self._h, id, cp.ctypes.data_as(_lib.u32p),
                                                t.ctypes.data_as(_lib.f32p), t.size))

    def set_graph_history(self, id, enable=True):
        """enable: 0 off, 1 (True) snapshot after the step's weight updates (a lone Lattice), 2 before them (the order of
        LatticeNetwork::iterate)"""
        self._check(self._L.snn_set_graph_history(self._h, id, int(enable)))

    def graph_history(self, id):
        """[steps][n][n] snapshots of lattice `id`'s internal weights (update_graph_history)"""
        rows, cols, _ = self.lattices[id]
        n = rows * cols
        out = _out((self.history_steps(), n, n), np.float32)
        self._check(self._L.snn_get_graph_history(self._h, id, out.ctypes.data_as(_lib.f32p), out.shape[0]))
        return out

    def set_edge_history(self, pre, post, when=1):
        """Records the weights of the pairs (pre[k], post[k]) at every recorded step (snn_set_edge_history), dense and sparse
        handles alike; interleaved global indices, spike-train cells are valid `pre`.  when: 1 after the step's weight updates
        (the connecting graph, a lone Lattice), 2 before them (a lattice's own graph inside a network); a scalar or one value
        per pair.  Replaces any earlier list and restarts the record; empty lists switch the recorder off."""
        p, q = self._pairs(pre, post)
        given = np.full(p.size, when) if np.ndim(when) == 0 else np.asarray(when).reshape(-1)
        if given.size != p.size:
            raise ValueError("when must be a scalar or have one entry per pair")
        w = np.ascontiguousarray(given, dtype=np.uint8)
        if np.any(w != given):                   # (what fits a byte goes to the library, which names the offending pair)
            raise ValueError("when must be 1 or 2")
        self._check(self._L.snn_set_edge_history(self._h, p.ctypes.data_as(_lib.u32p), q.ctypes.data_as(_lib.u32p),
                                                w.ctypes.data_as(_lib.u8p), p.size))

    def edge_history_count(self):
        n = C.c_uint64()
        self._check(self._L.snn_edge_history_count(self._h, C.byref(n)))
        return int(n.value)

    def edge_history(self):
        """(weights float32[steps, n], connected bool[steps, n]) of the installed list, in its order; an absent pair reads 0.0 / False"""
        steps, n = self.history_steps(), self.edge_history_count()
        w, c = _out((steps, n), np.float32), _out((steps, n), np.uint8)
        self._check(self._L.snn_get_edge_history(self._h, w.ctypes.data_as(_lib.f32p), c.ctypes.data_as(_lib.u8p), steps))
        return w, c != 0

    def set_peak_history(self, id, threshold, enable=True):
        """Voltage-peak record of neuron lattice `id` (snn_set_peak_history): one bit per neuron and recorded step where
        scipy.signal.find_peaks of the recorded voltage series has a peak above `threshold` -- the experiments'
        find_peaks_above_threshold, kept on the device.  Switching it or changing the threshold restarts the record."""
        self._check(self._L.snn_set_peak_history(self._h, id, int(bool(enable)), float(threshold)))

    def peak_raster(self, id):
        """bool[steps, rows*cols]; peaks whose plateau is still open are not in it yet"""
        rows, cols, _ = self.lattices[id]
        out = _out((self.history_steps(), rows * cols), np.uint8)
        self._check(self._L.snn_get_peak_raster(self._h, id, out.ctypes.data_as(_lib.u8p), out.shape[0]))
        return out != 0

    def peak_counts(self, id, first_step=0):
        """uint32[rows*cols]: per neuron the peaks at step indices >= first_step"""
        rows, cols, _ = self.lattices[id]
        out = _out(rows * cols, np.uint32)
        self._check(self._L.snn_get_peak_counts(self._h, id, int(first_step), out.ctypes.data_as(_lib.u32p), out.size))
        return out

    def peaks(self, id, first_step=0):
        """per neuron (row-major) the ascending step indices >= first_step of its peaks, a list of int arrays"""
        rows, cols, _ = self.lattices[id]
        total = C.c_uint64()
        ptr, steps = np.zeros(rows * cols + 1, np.uint64), np.zeros(0, np.uint32)
        for _ in range(2):                       # the two-call idiom: the total first, then the lists
            self._check(self._L.snn_get_peaks(self._h, id, int(first_step), ptr.ctypes.data_as(_lib.u64p),
                                              steps.ctypes.data_as(_lib.u32p), steps.size, C.byref(total)))
            if total.value <= steps.size:
                break
            steps = np.zeros(int(total.value), np.uint32)
        flat = steps.astype(np.int64)
        return [flat[int(ptr[i]):int(ptr[i + 1])] for i in range(rows * cols)]

    def set_peak_totals(self, id, threshold, origin=0, window=0, n_windows=1, enable=True):
        """Voltage-peak totals of neuron lattice `id` (snn_set_peak_totals): per neuron the NUMBER of peaks above `threshold`
        of its voltage series over every step since the call, in buckets b = (index - origin) // window (window 0: one
        open-ended bucket from `origin` on).  No step form changes; a call that changes something restarts the totals of
        every lattice, and so does reset_history."""
        self._check(self._L.snn_set_peak_totals(self._h, id, int(bool(enable)), float(threshold), int(origin), int(window),
                                                int(n_windows)))
        if enable:
            self._peak_totals_rows[id] = int(n_windows)
        else:
            self._peak_totals_rows.pop(id, None)

    def peak_totals(self, id):
        """uint32[n_windows, rows*cols]; a peak is counted once its plateau has ended"""
        rows, cols, _ = self.lattices[id]
        out = _out((self._peak_totals_rows.get(id, 1), rows * cols), np.uint32)
        self._check(self._L.snn_get_peak_totals(self._h, id, out.ctypes.data_as(_lib.u32p), out.shape[0], out.shape[1]))
        return out

    def peak_totals_steps(self):
        """samples the totals have seen since their last restart"""
        n = C.c_uint64()
        self._check(self._L.snn_peak_totals_steps(self._h, C.byref(n)))
        return int(n.value)

    def set_history_stride(self, every):
        self._check(self._L.snn_set_history_stride(self._h, int(every)))

    def set_reduced_history(self, average_voltage=False, eeg=False, spike_counts=False,
                            reference_voltage=0.007, distance=0.8, conductivity=251.0):
        self._check(self._L.snn_set_reduced_history(self._h, int(average_voltage), int(eeg), int(spike_counts),
                                                   reference_voltage, distance, conductivity))

    def average_voltage_history(self, id):
        out = _out(self.history_steps(), np.float32)
        self._check(self._L.snn_get_average_voltage_history(self._h, id, out.ctypes.data_as(_lib.f32p), out.size))
        return out

    def eeg_history(self, id):
        out = _out(self.history_steps(), np.float32)
        self._check(self._L.snn_get_eeg_history(self._h, id, out.ctypes.data_as(_lib.f32p), out.size))
        return out

    def spike_counts(self, id):
        rows, cols, _ = self.lattices[id]
        out = _out(rows * cols, np.uint32)
        self._check(self._L.snn_get_spike_counts(self._h, id, out.ctypes.data_as(_lib.u32p), out.size))
        return out

    def set_option(self, name, value):
        """tuning switches of include/snn_amd.h (fused_step, defer_rstdp, defer_stdp, uniform_params, persistent_run, input_shape)"""
        self._check(self._L.snn_set_option(self._h, name.encode(), int(value)))

    def stat(self, name):
        """launch counters of include/snn_amd.h (persistent_run_launches, persistent_run_steps)"""
        out = C.c_uint64(0)
        self._check(self._L.snn_get_stat(self._h, name.encode(), C.byref(out)))
        return int(out.value)

    # ---- measurement ----------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(self._L.snn_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._check(self._L.snn_profile_reset(self._h))

    def profile_read(self):
        n, ms = C.c_uint64(), C.c_double()
        self._check(self._L.snn_profile_read(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def profile_read_plasticity(self):
        """(steps measured, summed ms) of the plasticity launches (spike compaction + weight updates)"""
        n, ms = C.c_uint64(), C.c_double()
        self._check(self._L.snn_profile_read_plasticity(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def set_synthetic_drive(self, seed, fraction, voltage):
        """benchmark / load-test input: before every step a pseudo-random `fraction` of the neurons is set to `voltage`"""
        self._check(self._L.snn_set_synthetic_drive(self._h, int(seed), float(fraction), float(voltage)))

    def input_kernel_bytes(self):
        v = C.c_uint64()
        self._check(self._L.snn_input_kernel_bytes(self._h, C.byref(v)))
        return v.value


def probe_math(which, x, device=0):
    """Evaluate the stepper's device functions (0 exp, 1 pow3, 2 pow4) on the GPU."""
    L = _lib.load()
    a = np.ascontiguousarray(x, dtype=np.float32)
    out = _out(a.shape, a.dtype)
    _lib.check(L.snn_probe_math(device, which, a.ctypes.data_as(_lib.f32p), out.ctypes.data_as(_lib.f32p), a.size))
    return out


def probe_math_bits(which, first, count, stride=1, y=0.0, device=0):
    """The same over float BIT PATTERNS first + i * stride formed on the device; which = 3: powf(x, y), 4-6: the
    branch-free forms of 0-2, 7-12: tanh, sinh, cosh, sin, cos, tan of generated models."""
    L = _lib.load()
    out = _out(count, np.float32)
    _lib.check(L.snn_probe_math_bits(device, which, first & 0xFFFFFFFF, stride, float(y), out.ctypes.data_as(_lib.f32p),
                                     count))
    return out


def probe_bandwidth(nbytes=8 << 30, repeats=5, device=0):
    """(read-only GB/s, copy GB/s) of the device with the stepper's access shape"""
    L = _lib.load()
    r, c = C.c_double(), C.c_double()
    _lib.check(L.snn_probe_bandwidth(device, nbytes, repeats, C.byref(r), C.byref(c)))
    return r.value, c.value
