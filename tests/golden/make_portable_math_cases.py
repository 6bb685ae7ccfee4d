#!/usr/bin/env python3
"""Regenerate tests/golden/portable_math_cases.npz:  python tests/golden/make_portable_math_cases.py [--check]

Correctly rounded binary32 values of tanh / sinh / cosh / sin / cos / tan -- the six functions generated models call
(csrc/snn_math.hpp, oracle/snn_oracle_math.h) -- computed by mpmath at 256 bits, which shares nothing with either
restatement.  mpmath is needed to GENERATE only; tests/test_oracle_math.py just loads the file.

Per function NAME the file holds three arrays of equal length:
  NAME_x        uint32  bit patterns of the inputs
  NAME_y        uint32  bit patterns of the correctly rounded results (a NaN result is 0x7fc00000)
  NAME_outside  uint8   1 where the input lies outside the function's accurate domain (sin / cos / tan: |x| >= 2^20 * pi/2,
                        beyond the Cody-Waite reduction's exact range), where the test asserts no accuracy

Inputs:
  * every crossover of the implementation with 64 neighbouring floats on each side, both signs: |x| = 0.05, 20 (tanh),
    0.05, 90 (sinh), 90 (cosh), the largest x with a finite sinh / cosh, +-0, +-smallest subnormal, +-FLT_MIN, +-FLT_MAX,
    +-inf, a NaN;
  * sin / cos / tan: of all k, 0 < |k| < 2^20, the 4096 whose nearest float lies closest to k * pi/2 in relative terms
    (there the reduced argument is tiny and its accuracy rests on the low word of pi/2), 64 floats on each side of
    k * pi/2 for |k| = 1 .. 4, 64 on each side of the domain edge 2^20 * pi/2, and 2^12 inputs outside the domain;
  * RANDOM floats per function, fixed seed, both signs, uniform over the bit patterns of the accurate domain (so
    log-uniform in magnitude: as many per binade as the format has): tanh all finite, sinh / cosh |x| <= 90,
    sin / cos / tan |x| < 2^20 * pi/2.  RANDOM is what keeps the compressed file under the repository's 1 MiB limit for a
    committed file; the structured part above is complete."""
import os
import sys

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "portable_math_cases.npz")
mp.prec = 256
RANDOM = 1 << 14
OUTSIDE = 1 << 12
NEIGHBOURS = 64
K_LIMIT = 1 << 20
K_KEPT = 4096
FUNCS = {"tanh": mp.tanh, "sinh": mp.sinh, "cosh": mp.cosh, "sin": mp.sin, "cos": mp.cos, "tan": mp.tan}
NAN = 0x7FC00000
INF = 0x7F800000
FLT_MAX = 0x7F7FFFFF
SIGN = 0x80000000


def to_mpf(bits):
    """the exact value of a finite binary32 bit pattern"""
    e, m = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    v = mpf(m) * mpf(2) ** -149 if e == 0 else mpf(m | 0x800000) * mpf(2) ** (e - 150)
    return -v if bits & SIGN else v


def round_bits(v):
    """bit pattern of the binary32 nearest to the mpf v, ties to even, subnormals and overflow included (v != 0)"""
    sign = SIGN if v < 0 else 0
    a = abs(v)
    e = mp.frexp(a)[1] - 1                                    # 2^e <= a < 2^(e+1)
    if e < -126:
        return sign | int(mp.nint(a * mpf(2) ** 149))         # subnormal quantum; 2^23 lands on FLT_MIN by itself
    n = int(mp.nint(a * mpf(2) ** (23 - e)))                  # 2^23 .. 2^24; 2^24 carries into the exponent
    bits = ((e + 127) << 23) + (n - (1 << 23))
    return sign | min(bits, INF)


def exact(name, bits):
    bits = int(bits)
    mag = bits & 0x7FFFFFFF
    if mag > INF:
        return NAN
    if mag == INF:
        return {"tanh": (bits & SIGN) | 0x3F800000, "sinh": bits, "cosh": INF}.get(name, NAN)
    if mag == 0:
        return 0x3F800000 if name in ("cosh", "cos") else bits
    return round_bits(FUNCS[name](to_mpf(bits)))


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def around(bits, n=NEIGHBOURS):
    """bits - n .. bits + n of a positive pattern, with their negatives"""
    pos = [b for b in range(bits - n, bits + n + 1) if 0 <= b <= INF]
    return pos + [b | SIGN for b in pos]


def nearest_float_bits(v):
    return round_bits(v)


def half_pi_multiples():
    """bits of the float nearest k * pi/2 for the K_KEPT values of k, 0 < |k| < K_LIMIT, with the smallest relative distance.
    A binary64 pass keeps 4 * K_KEPT candidates of k > 0 (its error, 1e-16, is far below the distances that matter,
    about 1e-10); mpmath ranks those exactly; -k mirrors k."""
    k = np.arange(1, K_LIMIT, dtype=np.float64)
    pi_hi = np.float64(np.pi / 2)
    pi_lo = np.float64(float(mp.pi / 2 - mpf(float(pi_hi))))
    f = (k * pi_hi).astype(np.float32).astype(np.float64)
    rel = np.abs((f - k * pi_hi) - k * pi_lo) / f
    cand = np.argsort(rel)[:4 * K_KEPT // 2] + 1
    ranked = []
    for kk in cand:
        v = mp.pi / 2 * int(kk)
        b = nearest_float_bits(v)
        ranked.append((abs(to_mpf(b) - v) / v, int(kk), b))
    ranked.sort()
    kept = ranked[:K_KEPT // 2]                               # K_KEPT values of k: these and their negatives
    worst_kept, best_dropped = kept[-1][0], ranked[K_KEPT // 2][0]
    assert worst_kept < best_dropped and float(best_dropped) < float(np.sort(rel)[4 * K_KEPT // 2 - 1]) * 0.5, "widen the candidate set"
    return [b for _, _, b in kept] + [b | SIGN for _, _, b in kept]


def finite_edge(name):
    """bits of the largest float whose sinh / cosh is finite in binary32"""
    lo, hi = f32_bits(89.0), f32_bits(90.0)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if exact(name, mid) < INF else (lo, mid)
    return lo


def cases():
    rng = np.random.default_rng(20260101)
    special = [0, SIGN, 1, SIGN | 1, 0x00800000, SIGN | 0x00800000, FLT_MAX, SIGN | FLT_MAX, INF, SIGN | INF, NAN]
    edge = mp.pi / 2 * K_LIMIT
    edge_bits = nearest_float_bits(edge)
    first_outside = edge_bits if to_mpf(edge_bits) >= edge else edge_bits + 1
    trig = special + around(edge_bits) + half_pi_multiples()
    for kk in (1, 2, 3, 4):
        trig += around(nearest_float_bits(mp.pi / 2 * kk))
    structured = {
        "tanh": special + around(f32_bits(0.05)) + around(f32_bits(20.0)),
        "sinh": special + around(f32_bits(0.05)) + around(f32_bits(90.0)) + around(finite_edge("sinh")),
        "cosh": special + around(f32_bits(0.05)) + around(f32_bits(90.0)) + around(finite_edge("cosh")),
        "sin": trig, "cos": trig, "tan": trig,
    }
    top = {"tanh": FLT_MAX, "sinh": f32_bits(90.0), "cosh": f32_bits(90.0),
           "sin": first_outside - 1, "cos": first_outside - 1, "tan": first_outside - 1}
    out = {}
    for name in FUNCS:
        mags = rng.integers(1, top[name] + 1, RANDOM, dtype=np.int64)
        signs = rng.integers(0, 2, RANDOM, dtype=np.int64) << 31
        xs = list(structured[name]) + [int(v) for v in mags | signs]
        if name in ("sin", "cos", "tan"):
            mags = rng.integers(first_outside, FLT_MAX + 1, OUTSIDE, dtype=np.int64)
            signs = rng.integers(0, 2, OUTSIDE, dtype=np.int64) << 31
            xs += [int(v) for v in mags | signs]
        xs = np.unique(np.array(xs, np.uint32))               # sorted: neighbours next to each other also compress better
        out[name + "_x"] = xs
        out[name + "_y"] = np.array([exact(name, b) for b in xs], np.uint32)
        mag = xs & np.uint32(0x7FFFFFFF)
        outside = (mag >= first_outside) & (mag < INF) if name in ("sin", "cos", "tan") else np.zeros(xs.shape, bool)
        out[name + "_outside"] = outside.astype(np.uint8)
    return out


if __name__ == "__main__":
    out = cases()
    if "--check" in sys.argv:
        want = np.load(PATH)
        diff = [k for k in want.files if np.asarray(out[k]).tobytes() != want[k].tobytes()]
        print("IDENTICAL" if not diff and set(want.files) == set(out) else "DIFFERS in " + ", ".join(diff))
        sys.exit(bool(diff))
    np.savez_compressed(PATH, **out)
    size = os.path.getsize(PATH)
    print({k: len(v) for k, v in out.items() if k.endswith("_x")}, size, "bytes")
    assert size < (1 << 20), "over the 1 MiB limit for a committed file: lower RANDOM"
