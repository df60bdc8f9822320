"""Accuracy of the fast-tier scalar helpers (csrc/hip/flux_math.hpp) against the host libm, through the
diagnostic entry t8gpu_hip_math_probe_*: the fused kernels replace IEEE division / sqrt / log by
reciprocal + Newton sequences and a short log, which is only admissible if they stay within a few ulp on
the operand ranges the solver produces. Random operands, and the structured places where such helpers break (table and
switch boundaries, 1 -+ ulp, powers of two, the branch switch of the logarithmic mean): inputs and references in _scalar_ref.py.
Every new figure is printed before it is asserted (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import _scalar_ref as R

pytestmark = pytest.mark.gpu

RCP, DIV, SQRT, LOG, LN_MEAN, LN_MEAN_REF, LOG_TAB, SQRT_RATIO, DIV_SHARED, RSQRT, RK_SCALE, LN_MEAN_RS, LN_MEAN_INV_RS = range(13)
LD = np.longdouble


def probe(op, a, b=None):
    import torch
    from t8gpu_amd import hip
    ta = torch.from_numpy(a).cuda()
    tb = torch.from_numpy(b).cuda() if b is not None else None
    out = torch.empty_like(ta)
    hip.call("t8gpu_hip_math_probe", ta.dtype, C.c_int(op), C.c_int(ta.numel()), hip.ptr(ta), hip.ptr(tb), hip.ptr(out),
             hip.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def ulps(got, want):
    want = want.astype(got.dtype)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize("dtype,limit", [(np.float64, 2.0), (np.float32, 2.5)])
def test_division_sqrt_within_ulps(dtype, limit):
    rng = np.random.default_rng(3)
    a = np.exp(rng.uniform(-12, 12, 200000)).astype(dtype) * rng.choice([-1.0, 1.0], 200000).astype(dtype)
    b = np.exp(rng.uniform(-12, 12, 200000)).astype(dtype)
    exact_div = (a.astype(np.longdouble) / b.astype(np.longdouble))
    assert ulps(probe(DIV, a, b), exact_div.astype(dtype)).max() <= limit
    assert ulps(probe(RCP, b), (1 / b.astype(np.longdouble)).astype(dtype)).max() <= limit
    assert ulps(probe(SQRT, b), np.sqrt(b.astype(np.longdouble)).astype(dtype)).max() <= limit
    assert ulps(probe(DIV_SHARED, a, b), exact_div.astype(dtype)).max() <= limit
    c = np.exp(rng.uniform(-12, 12, 200000)).astype(dtype)
    ratio = np.sqrt(c.astype(np.longdouble) / b.astype(np.longdouble))
    assert ulps(probe(SQRT_RATIO, c, b), ratio.astype(dtype)).max() <= limit + 1.0


@pytest.mark.parametrize("dtype,k,op", [(np.float64, 1.5, LOG), (np.float32, 4.0, LOG),   # fp32: hardware log2 x ln 2
                                        (np.float64, 2.0, LOG_TAB)])   # fp64 in the plain tile kernels: 128-entry table
def test_log_matches_libm(dtype, k, op):
    rng = np.random.default_rng(4)
    span = 40 if dtype == np.float64 else 20      # (fp32: the range of densities / pressures / ratios with a wide margin)
    x = np.concatenate([np.exp(rng.uniform(-span, span, 300000)), rng.uniform(0.5, 2.0, 300000),
                        1.0 + rng.uniform(-1e-6, 1e-6, 1000), [1.0, 0.5, 2.0, np.sqrt(0.5), np.sqrt(2.0)]]).astype(dtype)
    worst = log_error_over_tolerance(dtype, k, op, x)
    assert worst <= 1.0, worst


def log_error_over_tolerance(dtype, k, op, x):
    """max of |got - log x| / tol, tol = k max(ulp(log x), eps / 2)"""
    want = np.log(x.astype(np.longdouble))
    got = probe(op, x).astype(np.longdouble)
    # relative to max(|log x|, ulp-scale of the argument error): 1 ulp of the result, or 1 ulp of x near x = 1
    tol = k * np.maximum(np.spacing(np.abs(want).astype(dtype)).astype(np.longdouble), np.finfo(dtype).eps / 2)
    return float((np.abs(got - want) / tol).max())


def name_of(dtype):
    return "f64" if dtype == np.float64 else "f32"


@pytest.mark.parametrize("dtype,k,op", [(np.float64, 1.5, LOG), (np.float32, 4.0, LOG), (np.float64, 2.0, LOG_TAB)])
def test_log_at_table_boundaries_and_switch_points(dtype, k, op):
    """The same limits at the places uniform samples never hit: the 128 interval boundaries of t8_log_tab's table with their
    neighbours and the interval midpoints (where |r| is largest), at binary exponents from one end of the normal range to the
    other; for t8_log_fast also the neighbours of its mantissa switch sqrt(1/2) (and sqrt(2)) and of 1."""
    x = R.log_inputs(dtype, switch_points=(op == LOG))
    worst = log_error_over_tolerance(dtype, k, op, x)
    print(f"FIG {'LOG' if op == LOG else 'LOG_TAB'} {name_of(dtype)} structured: worst error / limit = {worst:.3f} (limit k = {k}), {x.size} inputs")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("dtype,limit", [(np.float64, 2.0), (np.float32, 2.5)])
def test_division_sqrt_at_structured_operands(dtype, limit):
    """Mantissas 1, 1 -+ ulp, 2 - ulp, sqrt(2) -+ ulp, 1.5 and 4096 equally spaced ones at the exponents -300, -40, 0, 40, 300
    (fp32: -30, -8, 0, 8, 30), against long double; the limits of test_division_sqrt_within_ulps. RSQRT: the SQRT limit."""
    fig = {}
    # RCP, SQRT, RSQRT: unary; 1 / x, x, x^2-sized intermediates of 2^+-300 (fp32 2^+-30) and the residuals 2^-52 below them are
    # all normal. SQRT and RSQRT also at each exponent + 1: their mantissa period is [1, 4).
    x = R.unary_operands(dtype)
    fig["RCP"] = ulps(probe(RCP, x), (1 / x.astype(LD)).astype(dtype)).max()
    x = R.unary_operands(dtype, odd_exponents=True)
    fig["SQRT"] = ulps(probe(SQRT, x), np.sqrt(x.astype(LD)).astype(dtype)).max()
    fig["RSQRT"] = ulps(probe(RSQRT, x), (1 / np.sqrt(x.astype(LD))).astype(dtype)).max()
    # DIV, DIV_SHARED: every pair of exponents: 1 / b, a / b (2^+-600, fp32 2^+-60) and the residual a - b q (2^-52 below a) are normal
    a, b = R.binary_operands(dtype)
    exact = (a.astype(LD) / b.astype(LD)).astype(dtype)
    fig["DIV"] = ulps(probe(DIV, a, b), exact).max()
    fig["DIV_SHARED"] = ulps(probe(DIV_SHARED, a, b), exact).max()
    # SQRT_RATIO(y, x) = sqrt(y / x) forms y x (2^+-601, fp32 2^+-61), its reciprocal root, y / sqrt(y x) and the residual
    # y - a^2 x: all normal for every pair; y > 0
    y, x = R.binary_operands(dtype, odd_exponents=True)
    y = np.abs(y)
    fig["SQRT_RATIO"] = ulps(probe(SQRT_RATIO, y, x), np.sqrt(y.astype(LD) / x.astype(LD)).astype(dtype)).max()
    for op, worst in fig.items():
        print(f"FIG {op} {name_of(dtype)} structured: worst = {worst:.3f} ulp (limit {limit + (op == 'SQRT_RATIO')})")
    for op, worst in fig.items():
        assert worst <= limit + (1.0 if op == "SQRT_RATIO" else 0.0), (op, worst)
    assert probe(RSQRT, np.ones(1, dtype))[0] == 1


@pytest.mark.parametrize("dtype,limit", [(np.float64, 2.0), (np.float32, 2.5)])
def test_rsqrt_within_ulps(dtype, limit):
    """t8_rsqrt_fast (the normalisation of every per-face frame of a curved mesh) over the operand range of the other helpers"""
    rng = np.random.default_rng(6)
    b = np.exp(rng.uniform(-12, 12, 200000)).astype(dtype)
    worst = ulps(probe(RSQRT, b), (1 / np.sqrt(b.astype(LD))).astype(dtype)).max()
    print(f"FIG RSQRT {name_of(dtype)} random: worst = {worst:.3f} ulp (limit {limit})")
    assert worst <= limit, worst


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rk_scale_is_ieee_division(dtype):
    """rk_scale(dt, vol) == dt / vol BIT FOR BIT: for every power of two of the format as the volume (denormal ones and those
    outside the window of the exponent arithmetic must take the division), negative ones, 2^k (1 -+ ulp) and 3 * 2^k, and dt
    random or a power of two; pairs whose quotient is not a normal number are left out (R.rk_scale_operands has the rule)."""
    dt, vol = R.rk_scale_operands(dtype)
    want = dt / vol                                    # numpy divides in the operands' own format: IEEE, round to nearest
    assert want.dtype == dtype and dt.size > 20000
    got = probe(RK_SCALE, dt, vol)
    bad = np.nonzero(got.view(np.uint64 if dtype == np.float64 else np.uint32) != want.view(np.uint64 if dtype == np.float64 else np.uint32))[0]
    print(f"FIG RK_SCALE {name_of(dtype)}: {bad.size} of {dt.size} pairs differ from IEEE dt / vol")
    assert bad.size == 0, [(float(dt[i]).hex(), float(vol[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]]


# ---- logarithmic mean -----------------------------------------------------------------------------------------------------------
# Reference: (aR - aL) / log1p((aR - aL) / aL) in long double (R.ln_mean_reference: no cancellation next to aR = aL). Bounds: by the
# branch the formula takes, derived from the limits asserted above for the helpers underneath (R.ln_mean_bounds has the derivation).
def ln_mean_worst(got, aL, aR, dtype, form, inverse=False):
    """max of (relative error / bound) over the SERIES, the LOG and the EITHER inputs, and the largest relative error in eps"""
    exact = R.ln_mean_reference(aL, aR)
    if inverse:
        exact = 1 / exact
    allowed, br = R.ln_mean_allowed(aL, aR, dtype, form)
    rel = np.abs(got.astype(LD) - exact) / np.abs(exact)
    ratio = (rel / allowed).astype(np.float64)
    worst = [float(ratio[br == b].max()) if (br == b).any() else 0.0 for b in (R.SERIES, R.LOG, R.EITHER)]
    return worst, float(rel.max() / np.finfo(dtype).eps), [int((br == b).sum()) for b in (R.SERIES, R.LOG, R.EITHER)]


def report(label, dtype, worst, raw, counts):
    print(f"FIG {label} {name_of(dtype)}: worst rel / bound: series {worst[0]:.3f}, log {worst[1]:.3f}, at the switch {worst[2]:.3f}; "
          f"largest rel = {raw:.1f} eps; inputs per branch {counts}")


@pytest.mark.parametrize("dtype,rtol", [(np.float64, 2e-13), (np.float32, 3e-5)])
def test_ln_mean_fast_vs_reference_formula(dtype, rtol):
    """ln_mean of the fast tier and the compat tier's restatement of kernels.cu:24-36 against the exact logarithmic mean,
    across the series / log branch switch (u = 1e-4 <=> ratio ~ 1.02), each within the bound of the branch it takes (all of
    them far inside the flat rtol this test used to assert against a reference that cancelled next to ratio 1)."""
    rng = np.random.default_rng(5)
    aL = np.exp(rng.uniform(-3, 3, 400000))
    ratio = np.concatenate([np.exp(rng.uniform(-3, 3, 200000)), 1 + rng.uniform(-0.05, 0.05, 199000), np.ones(1000)])
    aR = aL * ratio
    aL, aR = aL.astype(dtype), aR.astype(dtype)
    for label, op, form in (("LN_MEAN random", LN_MEAN, "fast"), ("LN_MEAN_REF random", LN_MEAN_REF, "ref")):
        worst, raw, counts = ln_mean_worst(probe(op, aL, aR), aL, aR, dtype, form)
        report(label, dtype, worst, raw, counts)
        assert max(worst) <= 1.0, (label, worst)
        assert raw * np.finfo(dtype).eps <= rtol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("op", [LN_MEAN, LN_MEAN_RS, LN_MEAN_INV_RS], ids=["ln_mean_dlog", "ln_mean_dlog_rs", "ln_mean_inv_dlog_rs"])
def test_ln_mean_forms_at_the_switch_and_across_scales(op, dtype):
    """The three fast forms (kepes_core calls ln_mean_dlog and ln_mean_inv_dlog_rs; ln_mean_dlog_rs has no caller but the probe,
    which hands both _rs forms the sum and its shared reciprocal as kepes_core forms them for the inverse one) on operands of
    e^-30 .. e^30 (fp32 e^-10 .. e^10) with ratios at both switch points to within ulps, in 1 +- 0.05, in e^+-3 and exactly 1,
    both ways round. LN_MEAN_INV_RS: the same bounds on the reciprocal."""
    aL, aR = R.ln_mean_inputs(dtype)
    worst, raw, counts = ln_mean_worst(probe(op, aL, aR), aL, aR, dtype, "fast", inverse=(op == LN_MEAN_INV_RS))
    report({LN_MEAN: "LN_MEAN", LN_MEAN_RS: "LN_MEAN_RS", LN_MEAN_INV_RS: "LN_MEAN_INV_RS"}[op] + " structured", dtype, worst, raw, counts)
    assert counts[0] >= 1000 and counts[1] >= 1000, counts
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("op", [LN_MEAN, LN_MEAN_RS], ids=["ln_mean_dlog", "ln_mean_dlog_rs"])
def test_ln_mean_of_equal_values_is_the_value(op, dtype):
    """ln_mean(a, a) == a bit for bit, 1 000 values of e^-30 .. e^30 (fp32 e^-10 .. e^10).

    The series branch alone does not give this: for aL == aR it returns (2 a * 52.5) / 105, the formula of kernels.cu:24-36,
    and rounding 105 a and dividing by 105 does not give a back for every a. Before the helpers returned aL for aR == aL, 132 of
    these 1 000 fp64 values and 440 of the fp32 ones came back one ulp off (IEEE arithmetic on the host, (a * 105) / 105, misses
    the same 132 in fp64 and 114 in fp32: the formula, not t8_div)."""
    rng = np.random.default_rng(7)
    a = np.exp(rng.uniform(-30, 30, 1000) if dtype == np.float64 else rng.uniform(-10, 10, 1000)).astype(dtype)
    got = probe(op, a, a.copy())
    off = ulps(got, a)
    print(f"FIG ln_mean(a, a) {name_of(dtype)} op {op}: {(got != a).sum()} of 1000 differ from a, by at most {off.max():.1f} ulp")
    assert np.array_equal(got, a), int((got != a).sum())
