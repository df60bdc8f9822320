"""Host-side references and structured inputs for the GPU tests of the small device routines: the bit-OR of planes
(test_gpu_planes_or_bits.py), the fast-tier scalar helpers (test_gpu_fastmath.py), the per-cell KEPES record
(test_gpu_inflow_table.py; its reference alone uses mpmath). Otherwise pure numpy: tested without a GPU in
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


# ---- the per-cell KEPES record (flux_math.hpp: prim_from_state) -----------------------------------------------------------------
# Words 5-13 of an inflow-table row (t8gpu_hip.h: T8GPU_INFLOW_WORDS): rho, vx, vy, vz, p, beta, lrho, lbeta, v0.
PRIM_WORDS = ("rho", "vx", "vy", "vz", "p", "beta", "lrho", "lbeta", "v0")
DIV_ULP = 2.5                                   # t8_rcp, t8_div: the limit pinned in test_gpu_fastmath.py (fp64 2.0, fp32 2.5)
LOG_K = {np.float64: 2.0, np.float32: 4.0}      # the logs prim_from_state calls there: fp64 t8_log_tab, fp32 t8_log_fast


def prim_reference(states):
    """The nine quantities from the states AS ROUNDED to their type, evaluated with mpmath at 160 bits and returned as long
    double arrays (dict by PRIM_WORDS, plus C = E / (p / 0.4), the cancellation factor of the pressure, B = beta |v|^2 and
    lp = ln p). kappa = 1.4 and 0.4 are the decimal constants."""
    import mpmath
    out = {k: [] for k in PRIM_WORDS + ("C", "B", "lp")}
    with mpmath.workprec(160):
        kappa, km1, half = mpmath.mpf("1.4"), mpmath.mpf("0.4"), mpmath.mpf("0.5")
        for s in np.asarray(states):
            rho, mx, my, mz, E = (mpmath.mpf(float(x)) for x in s)
            v = (mx / rho, my / rho, mz / rho)
            v2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
            p = km1 * (E - half * rho * v2)
            beta = rho / (2 * p)
            lrho, lp = mpmath.log(rho), mpmath.log(p)
            vals = dict(rho=rho, vx=v[0], vy=v[1], vz=v[2], p=p, beta=beta, lrho=lrho, lbeta=lrho - lp,
                        v0=(kappa - (lp - kappa * lrho)) / (kappa - 1) - beta * v2, C=E / (p / km1), B=beta * v2, lp=lp)
            for k, x in vals.items():
                out[k].append(LD(mpmath.nstr(x, 30)))
    return {k: np.array(x, LD) for k, x in out.items()}


def prim_bounds(ref, dtype):
    """Absolute bounds on words 5-13, by PRIM_WORDS, from the operation sequence of prim_from_state. eps = 2^-23 / 2^-52; a
    rounding is eps / 2 relative, t8_rcp and t8_div DIV_ULP eps, a logarithm LOG_K max(eps |log x|, eps / 2) absolute.
      rho    copied: 0.
      v      m * rcp(rho): (DIV_ULP + 0.5) eps = 3 eps relative.
      ke     = 0.5 (vx^2 + vy^2 + vz^2) by a product and two FMAs: each square 6 eps, three roundings of a sum of positive
             terms 1.5 eps: 7.5 eps relative.
      p      = km1 fma(-rho, ke, E): rho ke carries 7.5 eps of itself = 7.5 (C - 1) eps of e = E - rho ke, C = E / e the
             cancellation factor; the FMA 0.5 eps; km1 = T(1.4) - 1 is 0.5 eps (fp32) / 1 eps (fp64) off 0.4; the product 0.5 eps:
             (7.5 C + 2) eps relative (C - 1 taken as C).
      beta   = 0.5 t8_div(rho, p): p's bound + DIV_ULP = (7.5 C + 4.5) eps relative.
      lrho   LOG_K max(eps |ln rho|, eps / 2) absolute.
      lp     the same at p, + p's relative bound (d ln p = dp / p); lbeta = lrho - lp: both + 0.5 eps |lbeta|.
      v0     = fma(-rp, ke, (kappa - fma(-kappa, lrho, lp)) (1 / km1)):
             s = lp - kappa lrho: lp's bound + 1.4 lrho's bound + 0.5 eps 1.4 |ln rho| (kappa as rounded) + 0.5 eps |s|;
             kappa - s: + 0.5 eps (1.4 + |kappa - s|); A = (kappa - s) (1 / km1): that / 0.4 + 2 eps |A| (km1 1 eps, its
             reciprocal and the product 0.5 eps each); rp ke = B = beta |v|^2: (7.5 C + 4.5 + 7.5) eps B; the FMA 0.5 eps |v0|."""
    e = LD(np.finfo(dtype).eps)
    k = LD(LOG_K[dtype])
    C = ref["C"]
    rel_p = (LD(7.5) * C + 2) * e
    b = {"rho": np.zeros_like(C)}
    for w in ("vx", "vy", "vz"):
        b[w] = (DIV_ULP + LD(0.5)) * e * np.abs(ref[w])
    b["p"] = rel_p * np.abs(ref["p"])
    b["beta"] = (rel_p + DIV_ULP * e) * np.abs(ref["beta"])
    b["lrho"] = k * np.maximum(e * np.abs(ref["lrho"]), e / 2)
    lp = k * np.maximum(e * np.abs(ref["lp"]), e / 2) + rel_p
    b["lbeta"] = b["lrho"] + lp + LD(0.5) * e * np.abs(ref["lbeta"])
    s = ref["lp"] - LD(1.4) * ref["lrho"]
    err_s = lp + LD(1.4) * b["lrho"] + LD(0.5) * e * LD(1.4) * np.abs(ref["lrho"]) + LD(0.5) * e * np.abs(s)
    err_d = err_s + LD(0.5) * e * (LD(1.4) + np.abs(LD(1.4) - s))
    A = (LD(1.4) - s) / LD(0.4)
    b["v0"] = err_d / LD(0.4) + 2 * e * np.abs(A) + (rel_p + (DIV_ULP + LD(7.5)) * e) * ref["B"] + LD(0.5) * e * np.abs(ref["v0"])
    return b


def _state(dtype, rho, p, v):
    rho, p, v = np.asarray(rho, np.float64), np.asarray(p, np.float64), np.asarray(v, np.float64)
    E = p / 0.4 + 0.5 * rho * (v * v).sum(1)
    return np.concatenate([rho[:, None], rho[:, None] * v, E[:, None]], 1).astype(dtype)


def log_table_edges(dtype, seed=5):
    """200 arguments at the interval edges of t8_log_tab's table: 2^e (1 + i / 128), i = 0 .. 127, the value just below each
    (the last of the interval before) and just above, e in -20 .. 20; the powers of two are the i = 0 ones (all kept)."""
    rng = np.random.default_rng(seed)
    i, ex = rng.integers(1, 128, 138), rng.integers(-20, 21, 138)
    i[:8] = 127
    x = np.ldexp(1 + i / 128, ex).astype(dtype)
    x = np.where(np.arange(138) % 3 == 0, x, np.where(np.arange(138) % 3 == 1, step_ulps(x, -1), step_ulps(x, 1)))
    pw = np.ldexp(1.0, np.arange(-20, 21)).astype(dtype)
    out = np.concatenate([pw, step_ulps(pw[::2], -1), x])          # 41 + 21 + 138
    assert out.size == 200
    return out


def pressure_to_energy(dtype, p):
    """E of a state AT REST whose device pressure km1 * E is exactly p (km1 = T(1.4) - 1, one rounded product): the quotient
    rounded, or one of its four neighbours; where none gives p (a product cannot reach every value) the nearest one is kept"""
    T = np.dtype(dtype).type
    km1 = T(1.4) - T(1)
    E0 = (p.astype(LD) / LD(km1)).astype(dtype)
    best = E0.copy()
    gap = np.abs((km1 * E0).astype(LD) - p.astype(LD))
    for j in (-2, -1, 1, 2):
        Ej = step_ulps(E0, j)
        g = np.abs((km1 * Ej).astype(LD) - p.astype(LD))
        best, gap = np.where(g < gap, Ej, best), np.minimum(g, gap)
    return best


def inflow_state_families(dtype, seed=21):
    """{family: states [200, 5] of `dtype`}: 25 calls of 8 states each."""
    rng = np.random.default_rng(seed)
    n = 200

    def logu(lo, hi, k=n):
        return np.exp(rng.uniform(np.log(lo), np.log(hi), k))

    def directions(k=n):
        d = rng.standard_normal((k, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        axis = np.eye(3)[rng.integers(0, 3, k)] * rng.choice([-1.0, 1.0], k)[:, None]
        return np.where((np.arange(k) % 2 == 0)[:, None], d, axis)          # oblique and single-axis, alternating

    fam = {}
    # at rest, zero momenta of either sign (every combination of signs occurs; vz = -0 in half of them)
    s = _state(dtype, logu(0.1, 10), logu(0.1, 10), np.zeros((n, 3)))
    sign = ((np.arange(n)[:, None] >> np.arange(3)) & 1).astype(bool)
    s[:, 1:4] = np.where(sign, dtype(-0.0), dtype(0.0))
    fam["at rest"] = s
    # Mach 0.1 .. 20: E / e_int = 1 + 0.28 M^2 up to 113
    rho, p = logu(0.5, 2), logu(0.5, 2)
    mach = logu(0.1, 20)
    mach[:2] = 0.1, 20.0
    fam["Mach 0.1 - 20"] = _state(dtype, rho, p, (mach * np.sqrt(1.4 * p / rho))[:, None] * directions())
    # rho and p each over 1e-6 .. 1e6, Mach up to 2
    rho, p = logu(1e-6, 1e6), logu(1e-6, 1e6)
    rho[:4], p[:4] = (1e-6, 1e-6, 1e6, 1e6), (1e-6, 1e6, 1e-6, 1e6)
    fam["twelve decades"] = _state(dtype, rho, p, (rng.uniform(0, 2, n) * np.sqrt(1.4 * p / rho))[:, None] * directions())
    # rho and the DEVICE pressure at powers of two and at the edges of the log table's intervals (at rest: p = km1 * E)
    edges = log_table_edges(dtype)
    s = np.zeros((n, 5), dtype)
    s[:, 0], s[:, 4] = edges, pressure_to_energy(dtype, rng.permutation(edges))
    fam["table edges"] = s
    # moving, with one or two momenta a zero of either sign
    rho, p = logu(0.5, 2), logu(0.5, 2)
    s = _state(dtype, rho, p, rng.uniform(-1, 1, (n, 3)))
    zero = ((np.arange(n)[:, None] % 7 + 1) >> np.arange(3)) & 1
    zero[zero.sum(1) == 3] = (0, 0, 1)
    s[:, 1:4] = np.where(zero.astype(bool), np.where(sign, dtype(-0.0), dtype(0.0)), s[:, 1:4])
    s[:, 4] = (p / 0.4 + 0.5 * (s[:, 1:4].astype(np.float64) ** 2).sum(1) / s[:, 0].astype(np.float64)).astype(dtype)
    fam["signed zeros"] = s
    for a in fam.values():
        assert a.shape == (n, 5) and a.dtype == dtype and (a[:, 0] > 0).all() and np.isfinite(a).all()
    return fam
