"""The oracle's expf / powf against the container's glibc libm -- the libm the reference's Rust f32::exp / f32::powf
resolve to on Linux.  Bar: BIT-IDENTICAL on every input.  oracle/check_libm.c walks all 2^32 bit patterns of x for expf,
powf(x, 3.) and powf(x, 4.) and 2^28 sampled (x, y) pairs; this module runs it and adds known values.

tanh / sinh / cosh / sin / cos / tan of generated models are not restated from glibc but computed in binary64; they are
held to the EXACT value (tests/golden/portable_math_cases.npz, written by mpmath: crossovers, floats next to multiples of
pi/2, random inputs) within 1 ULP, and to glibc within its documented error on all 2^32 inputs (check_libm.c again)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob

libm = ctypes.CDLL("libm.so.6")
libm.expf.argtypes = [ctypes.c_float]
libm.expf.restype = ctypes.c_float
libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
libm.powf.restype = ctypes.c_float

ORACLE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")


def ulp_diff(a, b):
    ia = np.float32(a).view(np.int32).astype(np.int64)
    ib = np.float32(b).view(np.int32).astype(np.int64)
    return abs(int(ia) - int(ib))


def has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return True


def run_check(*args):
    subprocess.run(["make", "-s", "-C", ORACLE_DIR], check=True)
    r = subprocess.run([os.path.join(ORACLE_DIR, "_build", "check_libm")] + [str(a) for a in args],
                       capture_output=True, text=True)
    lines = {ln.split()[0]: dict(kv.split("=") for kv in ln.split()[1:]) for ln in r.stdout.splitlines() if ln}
    return r, lines


@pytest.mark.skipif(not has_fma(), reason="glibc selects its non-FMA expf/powf on this CPU; the oracle restates the FMA build")
def test_expf_pow3_pow4_exhaustive_against_libm():
    """All 2^32 inputs of expf, powf(x, 3.), powf(x, 4.) and 2^28 sampled (x, y) pairs of powf: zero mismatches
    (about half a minute on 8 cores)."""
    r, lines = run_check("all", 1)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("expf", "pow3", "pow4"):
        assert int(lines[name]["checked"]) == 1 << 32 and int(lines[name]["mismatches"]) == 0, r.stdout
    assert int(lines["powf"]["checked"]) >= 1 << 28 and int(lines["powf"]["mismatches"]) == 0, r.stdout


def test_array_entry_point_matches_scalar_and_libm():
    first, n, stride = 0x3D000000, 4096, 40009
    for which, ref in ((0, lambda x: libm.expf(x)), (1, lambda x: libm.powf(x, 3.0)), (2, lambda x: libm.powf(x, 4.0)),
                       (3, lambda x: libm.powf(x, -2.0))):
        got = ob.math_bits(which, first, n, stride, y=-2.0)
        xs = ((first + np.arange(n, dtype=np.uint64) * stride) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
        want = np.array([ref(float(x)) for x in xs], np.float32)
        ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert ok.all(), which


def test_expf_special_values():
    assert ob.expf(0.0) == 1.0
    assert ob.expf(np.float32(-0.0)) == 1.0
    assert ob.expf(1.0) == np.float32(np.e)
    assert ob.expf(100.0) == np.inf and ob.expf(88.8) == np.inf
    assert ob.expf(-200.0) == 0.0 and ob.expf(-np.inf) == 0.0 and ob.expf(np.inf) == np.inf
    assert np.isnan(ob.expf(np.nan))
    assert ob.expf(88.7) == libm.expf(88.7)            # largest finite decade
    assert ob.expf(-103.0) == libm.expf(-103.0)        # subnormal result
    assert ob.expf(-103.5) == np.float32(2.0 ** -149)  # glibc's may-underflow branch


def test_powf_special_values_follow_libm():
    vals = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 3.0, -3.0, 4.0, 1e-40, -1e-40, 0.75, 1e30, -1e30, np.inf, -np.inf, np.nan]
    for x in vals:
        for y in vals:
            a, b = np.float32(ob.powf(x, y)), np.float32(libm.powf(float(np.float32(x)), float(np.float32(y))))
            assert (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32), (x, y, a, b)


def test_integer_power_literals_fold_as_llvm_folds_them():
    """powf(x, 2.) -> x * x, powf(x, 1.) -> x, powf(x, 0.) -> 1, powf(x, -1.) -> 1 / x; everything else is libm powf."""
    rng = np.random.default_rng(3)
    for x in rng.uniform(-3, 3, 500).astype(np.float32):
        assert np.float32(ob.powif(x, 2)) == np.float32(x * x)
        assert np.float32(ob.powif(x, 1)) == x and ob.powif(x, 0) == 1.0
        assert np.float32(ob.powif(x, -1)) == np.float32(np.float32(1.0) / x)
        for n in (3, 4, 7, -2, -3):
            assert np.float32(ob.powif(x, n)).view(np.uint32) == np.float32(libm.powf(float(x), float(n))).view(np.uint32)


def test_synthetic_generator_twins_agree():
    """oracle C, the numpy twin in the binding and the product's numpy twin generate the same stream."""
    import snn_amd
    a = ob.uniform_array(7, 1000, -65.0, 30.0, offset=123)
    b = np.array([ob.uniform(7, 123 + i, -65.0, 30.0) for i in range(1000)], np.float32)
    c = snn_amd.synthetic.uniform(7, 1000, -65.0, 30.0, offset=123)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    assert a.min() >= -65.0 and a.max() < 30.0


def test_generated_model_functions_within_one_ulp_of_libm():
    """tanh / sinh / cosh / sin / cos / tan of generated models (the reference forwards them to libm,
    build_test/nb_macro/src/lib.rs:9152-9175) against glibc's float functions.  Ours are the correctly rounded values on
    every input of the mpmath fixture inside the functions' accurate domains (test_generated_model_functions_against_exact_values
    measures it: 0 of 116 195 inputs not correctly rounded); glibc documents up to 2 ULP for the hyperbolic functions and
    tanf, 1 ULP for sinf / cosf -- so that is the distance allowed here, and
    test_generated_model_functions_exhaustive_against_libm holds every input to it."""
    rng = np.random.default_rng(2)
    xs = np.concatenate([rng.uniform(-12, 12, 6000), rng.uniform(-0.1, 0.1, 1500), rng.uniform(-100, 100, 3000),
                         rng.uniform(-1e5, 1e5, 1500), [0.0, -0.0, 0.05, -0.05, 20.5, -45.0]]).astype(np.float32)
    for name, bar in (("tanhf", 2), ("sinhf", 2), ("coshf", 2), ("sinf", 1), ("cosf", 1), ("tanf", 2)):
        ref = getattr(libm, name)
        ref.argtypes, ref.restype = [ctypes.c_float], ctypes.c_float
        ours = getattr(ob, name)
        worst, mism = 0, 0
        for x in xs:
            if name in ("sinhf", "coshf") and abs(x) > 88.0:
                continue
            a, b = np.float32(ours(x)), np.float32(ref(float(x)))
            if a.view(np.uint32) != b.view(np.uint32):
                mism += 1
                worst = max(worst, ulp_diff(a, b))
        assert worst <= bar, (name, worst)
        assert mism / len(xs) < 0.25, f"{name}: {mism} of {len(xs)} differ from libm"
    assert np.isnan(ob.sinf(np.inf)) and np.isnan(ob.tanf(np.nan)) and ob.coshf(200.0) == np.inf
    assert np.signbit(np.float32(ob.sinf(np.float32(-0.0)))) and ob.tanhf(50.0) == 1.0


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "portable_math_cases.npz")
PORTABLE = ("tanh", "sinh", "cosh", "sin", "cos", "tan")


def on_number_line(bits):
    """binary32 bit patterns as integers in the order of the values they encode (-0 and +0 coincide, inf one past FLT_MAX),
    so that a difference is a distance in ULP and subnormal results count like any other"""
    b = bits.astype(np.int64)
    mag = b & 0x7FFFFFFF
    return np.where(b >> 31 != 0, -mag, mag)


def test_generated_model_functions_against_exact_values(capsys):
    """The oracle's tanh / sinh / cosh / sin / cos / tan against correctly rounded values computed by mpmath at 256 bits
    (tests/golden/make_portable_math_cases.py: every crossover with 64 floats on each side, the 4096 multiples of pi/2 a
    float comes closest to, the edges of the format, 2^14 random inputs per function).  Inside the accurate domain: at
    most 1 ULP, nothing filtered out; zeros, infinities and NaN results exactly.  Outside it (sin / cos / tan,
    |x| >= 2^20 * pi/2) nothing is asserted, the worst distance is reported."""
    data = np.load(GOLDEN)
    total = wrong = 0
    report = []
    for name in PORTABLE:
        x, want, outside = data[name + "_x"], data[name + "_y"], data[name + "_outside"].astype(bool)
        assert x.dtype == np.uint32 and want.dtype == np.uint32 and len(x) == len(want) == len(outside) > 16000
        got = ob.math_array(ob.MATH_SELECTORS[name + "f"], x)
        nan_want, nan_got = (want & 0x7FFFFFFF) > 0x7F800000, (got & 0x7FFFFFFF) > 0x7F800000
        dist = np.abs(on_number_line(got) - on_number_line(want))
        dist[nan_want & nan_got] = 0
        inside = ~outside
        # special results compare exactly: the sign of a zero, an infinity, NaN for NaN; no finite value for an infinite one
        exact = inside & (((want & 0x7FFFFFFF) == 0) | ((want & 0x7FFFFFFF) >= 0x7F800000))
        assert (nan_got == nan_want)[inside].all(), name
        assert (got == want)[exact & ~nan_want].all(), name
        assert (((got & 0x7FFFFFFF) == 0x7F800000) == ((want & 0x7FFFFFFF) == 0x7F800000))[inside].all(), name
        worst = int(dist[inside].max())
        bad = np.flatnonzero(inside & (dist > 1))[:5]
        assert worst <= 1, (f"{name}: {worst} ULP from the exact value at {[hex(int(v)) for v in x[bad]]}: "
                            f"oracle {[hex(int(v)) for v in got[bad]]}, exact {[hex(int(v)) for v in want[bad]]}")
        total += int(inside.sum())
        wrong += int((dist[inside] > 0).sum())
        report.append(f"{name}: inside {int(inside.sum())} inputs, worst {worst} ULP, not correctly rounded "
                      f"{int((dist[inside] > 0).sum())}; outside {int(outside.sum())} inputs, worst "
                      f"{int(dist[outside].max()) if outside.any() else 0} ULP")
    with capsys.disabled():
        print("\n" + "\n".join(report) + f"\nnot correctly rounded: {wrong} of {total} ({wrong / total:.6f})")
    # measured against the mpmath values (x86-64, gcc -O2 -ffp-contract=off): 0 of 116 195 -- it does not grow
    assert wrong / total <= 0.0


def test_generated_model_functions_special_values():
    f = {name: (lambda x, w=ob.MATH_SELECTORS[name + "f"]: ob.math_array(w, np.array([x], np.float32).view(np.uint32)).view(np.float32)[0])
         for name in PORTABLE}
    for name in ("sin", "cos", "tan"):
        assert np.isnan(f[name](np.inf)) and np.isnan(f[name](-np.inf)) and np.isnan(f[name](np.nan))
    for name in ("tanh", "sinh", "sin", "tan"):
        assert f[name](0.0) == 0 and not np.signbit(f[name](0.0)) and np.signbit(f[name](-0.0))
    assert f["tanh"](np.inf) == 1.0 and f["tanh"](-np.inf) == -1.0 and np.isnan(f["tanh"](np.nan))
    assert f["sinh"](np.inf) == np.inf and f["sinh"](-np.inf) == -np.inf and f["cosh"](-np.inf) == np.inf
    assert f["cosh"](0.0) == 1.0 and f["cos"](-0.0) == 1.0 and np.isnan(f["sinh"](np.nan)) and np.isnan(f["cosh"](np.nan))


def test_unknown_function_selectors_are_rejected():
    """13 and beyond are nothing; 4, 5, 6 are the values of 0, 1, 2 by name, not by falling through to powf"""
    for which in (-1, 13, 99):
        with pytest.raises(ValueError):
            ob.math_bits(which, 0, 4)
        with pytest.raises(ValueError):
            ob.math_array(which, np.zeros(4, np.uint32))
    for which in (0, 1, 2):
        a, b = ob.math_bits(which, 0x3F000000, 4096, 1021), ob.math_bits(which + 4, 0x3F000000, 4096, 1021)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_generated_model_functions_exhaustive_against_libm(capsys):
    """All 2^32 inputs of the six functions against glibc (the libm the reference calls for them): inside the accurate
    domains no result further from glibc's than glibc's documented error -- 2 ULP tanhf / sinhf / coshf / tanf, 1 ULP
    sinf / cosf, the bars of the sampled test above, now on every input.  The share that differs is reported (DESIGN.md
    section 2), outside the domains nothing is asserted."""
    r, lines = run_check("portable", 1)
    with capsys.disabled():
        print("\n" + r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    for name, bar in (("tanhf", 2), ("sinhf", 2), ("coshf", 2), ("sinf", 1), ("cosf", 1), ("tanf", 2)):
        got = {k: int(v) for k, v in lines[name].items()}
        assert got["checked"] == 1 << 32 and got["over_bar_inside"] == 0 and got["worst_inside"] <= bar, r.stdout + r.stderr
        assert got["inside"] >= {"tanhf": 1 << 32}.get(name, 1 << 31), r.stdout
