"""Host-side references and structured inputs for the GPU tests of the small device routines: the bit-OR of planes
(test_gpu_planes_or_bits.py), the fast-tier scalar helpers (test_gpu_fastmath.py). Pure numpy: tested without a GPU in
test_scalar_ref_host.py. Long double is the 80-bit x87 format here (64-bit mantissa): 2^-11 of a double's rounding."""
import numpy as np

LD = np.longdouble


# ---- OR of the raw bits of a plane ------------------------------------------------------------------------------------------
def or_bits(plane, nwords):
    """OR of the first `nwords` 32-bit words of `plane` (any dtype whose item size is a multiple of 4)."""
    w = np.ascontiguousarray(plane).view(np.uint32)[:nwords]
    return int(np.bitwise_or.reduce(w)) if w.size else 0


def integral_terms(n, reduce_blocks=1024):
    """Roundings on the longest path of the device integral of n cells (kernels_reduce.hip): a lane sums serially the
    ceil(n / (blocks 256)) products of its grid-stride loop, blocks = min(reduce_blocks, ceil(n / 256)); then two trees of
    8 + 2 levels each (64 lanes by shuffles, 4 wavefronts: per workgroup and once more over the partials) = 20, the serial
    sum of up to 4 partials per lane of the final kernel = 3, and one rounding of the product vol * x = 1: + 24."""
    blocks = max(1, min(reduce_blocks, -(-n // 256)))
    return -(-n // (blocks * 256)) + 24


# ---- neighbours ---------------------------------------------------------------------------------------------------------------
def step_ulps(x, k):
    """x moved by k representable values (k < 0: towards -inf), element-wise, in x's dtype"""
    x = np.array(x)
    to = np.array(np.inf if k > 0 else -np.inf, dtype=x.dtype)
    for _ in range(abs(k)):
        x = np.nextafter(x, to)
    return x


def around(x, k):
    """x and its k neighbours on each side"""
    x = np.atleast_1d(np.asarray(x))
    return np.concatenate([step_ulps(x, j) for j in range(-k, k + 1)])


# ---- structured arguments of the logarithms ------------------------------------------------------------------------------------
LOG_EXPONENTS = {np.float64: (-1021, -40, -2, -1, 0, 1, 2, 40, 1023), np.float32: tuple(range(-20, 21))}


def log_inputs(dtype, switch_points):
    """m = 1 + i/128 for i = 0 .. 128 (the interval boundaries of t8_log_tab's table; 128 is the wrap into the next binade) with
    three neighbours on each side, the 128 interval midpoints, each at the binary exponents above; with `switch_points` also the
    neighbours of sqrt(1/2) and sqrt(2) (t8_log_fast's mantissa switch) at those exponents, and 1 -+ k ulp, k = 1 .. 4.
    Only 2^1024 and its upper neighbours (no numbers of the format) fall out; everything else is a positive normal number."""
    i = np.arange(129)
    m = np.concatenate([around((1 + i / 128).astype(dtype), 3), (1 + (2 * i[:128] + 1) / 256).astype(dtype)])
    if switch_points:
        m = np.concatenate([m, around(np.sqrt(dtype(0.5)), 3), around(np.sqrt(dtype(2.0)), 3)])
    with np.errstate(over="ignore"):
        x = np.concatenate([np.ldexp(m, e).astype(dtype) for e in LOG_EXPONENTS[dtype]])
    if switch_points:
        x = np.concatenate([x, around(dtype(1.0), 4)])
    x = x[np.isfinite(x)]
    assert (x >= np.finfo(dtype).tiny).all()
    return x


# ---- structured operands of reciprocal / division / square roots -----------------------------------------------------------------
ARITH_EXPONENTS = {np.float64: (-300, -40, 0, 40, 300), np.float32: (-30, -8, 0, 8, 30)}


def special_mantissas(dtype):
    """1, 1 -+ ulp, 2 - ulp, sqrt(2) and sqrt(2) -+ ulp, 1.5"""
    one, two, r2 = dtype(1), dtype(2), np.sqrt(dtype(2))
    return np.array([one, np.nextafter(one, two), np.nextafter(one, dtype(0)), np.nextafter(two, one), r2, np.nextafter(r2, two),
                     np.nextafter(r2, one), dtype(1.5)], dtype=dtype)


def mantissas(dtype):
    """the special ones and 4096 equally spaced in [1, 2)"""
    return np.concatenate([special_mantissas(dtype), (1 + np.arange(4096) / 4096).astype(dtype)])


def unary_operands(dtype, odd_exponents=False):
    """every mantissa at every exponent of ARITH_EXPONENTS (odd_exponents: and at each of them + 1, the other half of a
    square root's period)"""
    exps = [e + o for e in ARITH_EXPONENTS[dtype] for o in ((0, 1) if odd_exponents else (0,))]
    return np.concatenate([np.ldexp(mantissas(dtype), e).astype(dtype) for e in exps])


def binary_operands(dtype, odd_exponents=False):
    """(a, b): every pair of exponents; per pair every mantissa of a beside a rotated copy for b (so that the 4096 spaced ones
    meet others than themselves), and the 8 x 8 pairs of special mantissas. Signs of a alternate."""
    m, sp = mantissas(dtype), special_mantissas(dtype)
    ma = np.concatenate([m, np.repeat(sp, sp.size)])
    ma[1::2] *= -1
    mb = np.concatenate([np.roll(m, 1237), np.tile(sp, sp.size)])
    exps = [e + o for e in ARITH_EXPONENTS[dtype] for o in ((0, 1) if odd_exponents else (0,))]
    a, b = [], []
    for ea in exps:
        for eb in ARITH_EXPONENTS[dtype]:
            a.append(np.ldexp(ma, ea).astype(dtype))
            b.append(np.ldexp(mb, eb).astype(dtype))
    return np.concatenate(a), np.concatenate(b)


# ---- dt / vol ------------------------------------------------------------------------------------------------------------------
def rk_scale_operands(dtype, seed=11):
    """(dt, vol) pairs for rk_scale against IEEE dt / vol.
    vol: every power of two of the format, denormal ones included (fp64 2^-1074 .. 2^1023, fp32 2^-149 .. 2^127); their negatives;
    2^k (1 -+ ulp) and 3 * 2^k for 32 values of k spread over the normal range. dt: 64 random normal values (random sign, mantissa
    and exponent) and 17 powers of two. THE RULE for a pair: it is kept iff the exact quotient is a normal number of the format,
    tiny <= |dt / vol| <= max; a denormal or overflowing quotient is not asserted (dt * 2^-k and dt / 2^k round differently
    there, and the routine documents the normal range only)."""
    f = np.finfo(dtype)
    lo, hi = f.minexp - f.nmant, f.maxexp - 1                       # smallest denormal .. largest power of two
    rng = np.random.default_rng(seed)
    pw = np.ldexp(dtype(1), np.arange(lo, hi + 1)).astype(dtype)
    ks = np.linspace(f.minexp + 1, f.maxexp - 3, 32).astype(int)
    pk = np.ldexp(dtype(1), ks).astype(dtype)
    vol = np.concatenate([pw, -pw, np.nextafter(pk, dtype(np.inf)), np.nextafter(pk, dtype(0)), dtype(3) * pk])
    assert np.isfinite(vol).all() and (vol != 0).all()
    dt_e = rng.integers(f.minexp, f.maxexp - 1, 64)
    dt = np.ldexp((1 + rng.random(64)) * rng.choice([-1.0, 1.0], 64), dt_e).astype(dtype)
    dt = np.concatenate([dt, np.ldexp(dtype(1), np.linspace(f.minexp, f.maxexp - 1, 17).astype(int)).astype(dtype)])
    D, V = (x.ravel() for x in np.meshgrid(dt, vol, indexing="ij"))
    q = np.abs(D.astype(LD) / V.astype(LD))
    keep = (q >= LD(f.tiny)) & (q <= LD(f.max))
    return D[keep], V[keep]


# ---- logarithmic mean ----------------------------------------------------------------------------------------------------------
def ln_mean_reference(aL, aR):
    """(aR - aL) / log1p((aR - aL) / aL) in long double, aL where the two are equal: no cancellation near aR = aL (the plain
    (R - L) / log(R / L) loses what R / L loses by rounding next to 1, relative to log(R / L))."""
    L, R = np.asarray(aL).astype(LD), np.asarray(aR).astype(LD)
    d = R - L
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(d == 0, L, d / np.log1p(d / L))


SERIES, LOG, EITHER = 0, 1, 2


def ln_mean_branch(aL, aR, dtype, margin):
    """The branch the formula takes: SERIES where u = ((aR - aL) / (aR + aL))^2 < 1e-4 (the constant as the format holds it), LOG
    otherwise -- and EITHER where the exact u is within `margin` (relative) of the constant: the helper forms u with a few
    roundings and may land on the other side there; whichever branch it takes, that branch's bound holds for it."""
    L, R = np.asarray(aL).astype(LD), np.asarray(aR).astype(LD)
    f = (R - L) / (R + L)
    u, thr = f * f, LD(dtype(1.0e-4))
    out = np.where(u < thr, SERIES, LOG)
    out[np.abs(u - thr) <= margin * thr] = EITHER
    return out


FAST_MARGIN = 16.0     # x eps: u = f * f, f = d * rcp(s) or t8_div(d, s) -- a few ulp each, squared


def ref_margin(dtype):
    """the compat formula forms u = (xi (xi - 2) + 1) / (xi (xi + 2) + 1): the numerator cancels to (xi - 1)^2 ~ 4e-4 from terms
    of size 1, 2, 1 -- an ABSOLUTE error of a few eps, i.e. 4 eps / 1e-4 relative to the constant"""
    return 4.0 * np.finfo(dtype).eps / 1.0e-4


def ln_mean_bounds(aL, aR, dtype, form):
    """(series bound, log bound) on the relative error, element-wise, derived from the limits test_gpu_fastmath.py asserts for
    the helpers underneath (eps = 2^-52 / 2^-23 bounds one ulp relative to the value):

    series, every form: the sum s (1/2), its product by 52.5 (1/2), the three-fma polynomial (its last fma 1/2, the inner ones
      and the error of u enter scaled by u <= 1e-4), one division at the DIV limit (fp64 2, fp32 2.5), the truncation
      u^4 / 9 <= 1.2e-17: under 4 eps, asserted as 6 eps.
    log, fast fp64: two STORED logarithms at the LOG limit (1.5 ulp each, of log aL and of log aR), relative to their
      difference log(aR / aL): 1.5 (|log aL| + |log aR|) / |log(aR / aL)|; the difference itself, d = aR - aL (1/2 each) and one
      t8_div (2) with second-order terms: + 6. The first term depends on the SCALE of the operands.
    log, fast fp32: the logarithm is taken of the quotient q = t8_div(aR, aL): q at the DIV limit (2.5 ulp, an absolute error
      of 2.5 eps in log q), the logarithm at the LOG limit (4 max(ulp(log q), eps / 2)), both relative to log q = l:
      2.5 / |l| + max(4, 2 / |l|); d (1/2), the final t8_div (2.5) and second-order terms: + 4. No |log a| term.
    log, compat (`ref`): xi = aR / aL rounded (1/2, absolute in log xi), the library logarithm (1), d (1/2), the division (1/2):
      0.5 / |l| + 3 with second-order terms."""
    eps = LD(np.finfo(dtype).eps)
    L, R = np.asarray(aL).astype(LD), np.asarray(aR).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.abs(np.log1p((R - L) / L))
        if form == "ref":
            log_bound = eps * (0.5 / l + 3)
        elif dtype == np.float64:
            log_bound = eps * (1.5 * (np.abs(np.log(L)) + np.abs(np.log(R))) / l + 6)
        else:
            log_bound = eps * (2.5 / l + np.maximum(4, 2 / l) + 4)
    return np.full(L.shape, 6 * eps), log_bound


def ln_mean_allowed(aL, aR, dtype, form):
    """the bound on the relative error of each pair, by the branch it takes"""
    margin = ref_margin(dtype) if form == "ref" else FAST_MARGIN * np.finfo(dtype).eps
    br = ln_mean_branch(aL, aR, dtype, margin)
    sb, lb = ln_mean_bounds(aL, aR, dtype, form)
    with np.errstate(invalid="ignore"):
        return np.where(br == SERIES, sb, np.where(br == LOG, lb, np.maximum(sb, np.where(np.isfinite(lb), lb, sb)))), br


def ln_mean_inputs(dtype, seed=12):
    """(aL, aR), every pair also with its operands swapped. aL = e^k (1 + u), u uniform in [0, 1), k = -30 .. 30 (fp32 -10 .. 10);
    per k: ratios aR / aL within +-1e-9 relative (fp32 +-1e-5) of both switch points 1.01 / 0.99 and 0.99 / 1.01; aR at
    -+1, 2, 3 ulp of aL times a switch point; ratios in 1 +- 0.05; ratios in e^+-3; aR = aL."""
    rng = np.random.default_rng(seed)
    span, near = (30, 1e-9) if dtype == np.float64 else (10, 1e-5)
    sw = (LD(1.01) / LD(0.99), LD(0.99) / LD(1.01))
    aL, aR = [], []
    for k in range(-span, span + 1):
        def left(n):
            return (np.exp(LD(k)) * (1 + rng.random(n).astype(LD))).astype(dtype)
        for s in sw:
            a = left(32)
            aL.append(a)
            aR.append((a.astype(LD) * s * (1 + rng.uniform(-near, near, 32).astype(LD))).astype(dtype))
            a = left(4)
            base = (a.astype(LD) * s).astype(dtype)
            for j in (-3, -2, -1, 1, 2, 3):
                aL.append(a)
                aR.append(step_ulps(base, j))
        a = left(64)
        aL.append(a)
        aR.append((a.astype(LD) * (1 + rng.uniform(-0.05, 0.05, 64).astype(LD))).astype(dtype))
        a = left(64)
        aL.append(a)
        aR.append((a.astype(LD) * np.exp(rng.uniform(-3, 3, 64).astype(LD))).astype(dtype))
        a = left(16)
        aL.append(a)
        aR.append(a.copy())
    aL, aR = np.concatenate(aL), np.concatenate(aR)
    return np.concatenate([aL, aR]), np.concatenate([aR, aL])
