"""The pure-python pieces the GPU tests of the small device routines lean on (tests/_scalar_ref.py): the bit-OR reference,
the branch classifier of the logarithmic mean, its log1p reference and the structured input sets. No GPU."""
import math

import numpy as np
import pytest

import _scalar_ref as R


def test_or_bits_on_hand_made_arrays():
    assert R.or_bits(np.zeros(7, np.float32), 7) == 0
    assert R.or_bits(np.array([0.0, -0.0], np.float32), 2) == 0x80000000
    assert R.or_bits(np.array([0.0, -0.0], np.float32), 1) == 0                    # only the first nwords count
    assert R.or_bits(np.array([0.0, -0.0], np.float64), 4) == 0x80000000           # the high word of the second double
    assert R.or_bits(np.array([0.0, -0.0], np.float64), 3) == 0                    # ... which is word 3
    assert R.or_bits(np.array([5e-324], np.float64), 2) == 1                       # a denormal's low word
    assert R.or_bits(np.array([1.0, 2.0], np.float32), 2) == 0x3F800000 | 0x40000000
    assert R.or_bits(np.array([0x0F0F0000, 0x00000F0F, 0xFFFFFFFF], np.uint32), 2) == 0x0F0F0F0F
    assert R.or_bits(np.zeros(0, np.float32), 0) == 0


def test_step_ulps_and_around():
    one = np.float64(1)
    assert R.step_ulps(one, 1) == 1 + 2.0 ** -52 and R.step_ulps(one, -1) == 1 - 2.0 ** -53 and R.step_ulps(one, 0) == 1
    a = R.around(np.float32(2), 2)
    assert a.dtype == np.float32 and a.tolist() == [2 - 2.0 ** -22, 2 - 2.0 ** -23, 2.0, 2 + 2.0 ** -22, 2 + 2.0 ** -21]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_branch_classifier(dtype):
    eps = np.finfo(dtype).eps
    aL = np.array([1.0, 1.0, 1.0, 1.0, 3.0, 1.01, 0.99], dtype)
    aR = np.array([1.0, 1.019, 1.021, 1 / 1.021, 3.0, 0.99, 1.01], dtype)           # the switch: ratio 1.01 / 0.99 = 1.0202...
    got = R.ln_mean_branch(aL, aR, dtype, 16 * eps)
    want = [R.SERIES, R.SERIES, R.LOG, R.LOG, R.SERIES]
    assert got[:5].tolist() == want
    assert set(got[5:].tolist()) <= {R.EITHER, R.SERIES, R.LOG} and got[5] == got[6]   # symmetric in its operands
    # a wide margin turns the pairs at the switch, and only those, into EITHER
    wide = R.ln_mean_branch(aL, aR, dtype, 1e-3)
    assert wide.tolist() == want + [R.EITHER, R.EITHER]
    # the exact value of u at the constant: f = 0.01 <=> (R - L) / (R + L) = 0.01
    L, Rr = np.longdouble(0.99), np.longdouble(1.01)
    f = (Rr - L) / (Rr + L)
    assert abs(float(f * f) - 1e-4) < 1e-19 * 10


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_input_sets(dtype):
    aL, aR = R.ln_mean_inputs(dtype)
    assert aL.dtype == dtype and aR.dtype == dtype and (aL > 0).all() and (aR > 0).all()
    n = aL.size // 2
    assert np.array_equal(aL[:n], aR[n:]) and np.array_equal(aR[:n], aL[n:])       # operands swapped
    for form in ("fast", "ref"):
        allowed, br = R.ln_mean_allowed(aL, aR, dtype, form)
        assert np.isfinite(allowed.astype(np.float64)).all() and (allowed > 0).all()
    allowed, br = R.ln_mean_allowed(aL, aR, dtype, "fast")
    assert (br == R.SERIES).sum() >= 1000 and (br == R.LOG).sum() >= 1000
    assert (br == R.EITHER).sum() <= 200          # (one ulp of aR moves u by ~100 eps at the switch: few pairs are that close)
    assert (aL == aR).sum() >= 2 * 16 * (21 if dtype == np.float32 else 61)
    x = R.log_inputs(dtype, True)
    assert x.dtype == dtype and np.isfinite(x).all() and (x >= np.finfo(dtype).tiny).all() and dtype(1) in x
    a, b = R.binary_operands(dtype)
    assert a.size == b.size == 25 * (4104 + 64)
    with np.errstate(over="raise", under="raise"):                                   # every product the helpers form stays normal
        for z in (a.astype(np.longdouble) / b, a.astype(np.longdouble) * b):
            assert (np.abs(z) >= np.finfo(dtype).tiny).all() and (np.abs(z) <= np.finfo(dtype).max).all()
    dt, vol = R.rk_scale_operands(dtype)
    q = dt / vol
    assert q.dtype == dtype and np.isfinite(q).all() and (np.abs(q) >= np.finfo(dtype).tiny).all()
    f = np.finfo(dtype)
    for e in (f.minexp - f.nmant, f.minexp - 1, f.minexp, f.minexp + 1, 0, f.maxexp - 3, f.maxexp - 2, f.maxexp - 1):
        assert (vol == np.ldexp(dtype(1), e)).any(), e                                # denormal .. largest powers of two all met


def test_ln_mean_reference_has_no_cancellation():
    """against the closed form at ratios next to 1, where (R - L) / log(R / L) in long double is off by 1e-12 and more"""
    L = np.full(4, 1.5)
    Rr = L * (1 + np.array([0.0, 2.0 ** -40, 2.0 ** -30, -2.0 ** -35]))
    x = ((Rr - L) / L).astype(np.longdouble)                                         # exact: powers of two
    series = L * (1 + x / 2 - x * x / 12 + x ** 3 / 24)                                # L x / log1p(x), to O(x^4) ~ 1e-36
    got = R.ln_mean_reference(L, Rr)
    assert (np.abs(got - series) <= 4 * np.finfo(np.longdouble).eps * series).all()
    assert got[0] == 1.5


def test_ln_mean_reference_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.prec = 200
    for dtype in (np.float64, np.float32):
        aL, aR = R.ln_mean_inputs(dtype)
        idx = np.random.default_rng(1).choice(aL.size, 600, replace=False)
        ref = R.ln_mean_reference(aL[idx], aR[idx])
        for a, b, r in zip(aL[idx], aR[idx], ref):
            a, b = mp.mpf(float(a)), mp.mpf(float(b))
            want = a if a == b else (b - a) / mp.log(b / a)
            hi = mp.mpf(float(r))                                                    # long double -> mpf through its two halves
            lo = mp.mpf(float(r - np.longdouble(float(r))))
            assert abs(hi + lo - want) <= 8 * mp.mpf(2) ** -64 * want                 # a few long-double roundings


def test_integral_bound_formula():
    """the bound test_gpu_reduce.py asserts: (ceil(n / (blocks 256)) + 24) 2^-53 sum |vol x|, blocks = min(1024, ceil(n / 256))"""
    assert [R.integral_terms(n) for n in (1, 256, 257, 262144, 262145, 524305, 1 << 21)] == [25, 25, 25, 25, 26, 27, 32]
    assert math.ceil(524305 / (1024 * 256)) == 3
