"""Face frames: a long-double reference, the metrics the frame tests share, a numpy emulation of the device construction
and the seeded normals both the host and the -m gpu tests run on. Test infrastructure only.

The frame of a unit normal n (flux_math.hpp: face_basis / face_basis_fast, tile_plan.cpp: geometry_dictionary, oracle.hpp:
face_basis) is t1 = normalised projection of a seed onto the tangent plane, t2 = n x t1. The seed is (ny, nz, -nx); where the
squared length of the projection, |r|^2 = 1 - (n . seed)^2, is below 2^-6 it is (nz, -nx, ny) (the first seed is antiparallel
to n at +-(1, -1, 1) / sqrt 3; the reference has the first seed only).

eps is numpy's: 2^-23 (fp32), 2^-52 (fp64).
  DEFECT_LIMIT = 64 eps on max |G G^T - I|, G = rows (n, t1, t2): the defect of the construction is K eps / |r| with K <= 4
      (emulated here: 2.2 in fp32, 3.8 in fp64), 1 / |r| <= 8 outside the cone, times 2 for the fast reciprocal root.
  ANGLE_LIMIT = DEFECT_LIMIT / 2 eps radians between a tangent and the reference's.
  SWITCH_BAND: the device decides on |r|^2 as rounded in T. Each component of r is a difference of O(1) terms and carries an
      absolute error of up to ~1.5 eps (two products and a difference around 0.6), so |r|^2 = sum r_k^2 with |r| = 1/8 moves by up
      to 2 |r| sqrt(3) 1.5 eps ~ 0.65 eps plus its own roundings: inside |exact |r|^2 - 2^-6| <= 2 eps either seed is the rule
      applied correctly, and the tangents are compared with the nearer of the two reference frames. Outside, the seed is fixed."""
import glob
import os

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2.0 ** -60, "the reference needs an extended long double"
SWITCH = 2.0 ** -6
DEFECT_LIMIT = 64.0
ANGLE_LIMIT = DEFECT_LIMIT / 2
SWITCH_BAND = 2.0
BAD = np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def eps(dtype):
    return float(np.finfo(np.dtype(dtype)).eps)


def _seeds(n):
    return (np.stack([n[:, 1], n[:, 2], -n[:, 0]], 1), np.stack([n[:, 2], -n[:, 0], n[:, 1]], 1))


def _gram_schmidt(n, seed):
    """(t1, t2, |r|^2) in long double: the seed minus its component along n / |n|, normalised, and (n / |n|) x t1"""
    nh = n / np.sqrt((n * n).sum(1))[:, None]
    r = seed - (nh * seed).sum(1)[:, None] * nh
    r2 = (r * r).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t1 = r / np.sqrt(r2)[:, None]
    return t1, np.cross(nh, t1), r2


def reference_frames(normals):
    """normals (k, 3), already rounded to their type. Returns (t1, t2, r2, alt1, alt2): the long-double frame under the
    two-seed rule on the exact |r|^2 of the first seed, that |r|^2, and the frame of the OTHER seed (for SWITCH_BAND)."""
    n = np.asarray(normals).astype(LD)
    a, b = _seeds(n)
    ta1, ta2, r2 = _gram_schmidt(n, a)
    tb1, tb2, _ = _gram_schmidt(n, b)
    second = (r2 < LD(SWITCH))[:, None]
    return (np.where(second, tb1, ta1), np.where(second, tb2, ta2), r2, np.where(second, ta1, tb1), np.where(second, ta2, tb2))


def defect(normals, t1, t2):
    """max |G G^T - I| per frame, G = rows (n, t1, t2), in units of the eps of `normals`' type; inf where not finite"""
    G = np.stack([np.asarray(normals).astype(LD), np.asarray(t1).astype(LD), np.asarray(t2).astype(LD)], 1)   # (k, 3, 3)
    with np.errstate(invalid="ignore"):
        d = np.abs(np.einsum("kij,klj->kil", G, G) - np.eye(3, dtype=LD)).reshape(len(G), 9).max(1)
    d = np.where(np.isfinite(d), d, np.inf)
    return (d / LD(eps(np.asarray(normals).dtype))).astype(np.float64)


def _angle(a, b):
    with np.errstate(invalid="ignore"):
        c = np.cross(a, b)
        ang = np.arctan2(np.sqrt((c * c).sum(1)), (a * b).sum(1))
    return np.where(np.isfinite(ang), ang, np.inf)


def pair_angle(t1, t2, r1, r2):
    """the larger of the angles (radians, long double) between t1 and r1 and between t2 and r2, per frame"""
    return np.maximum(_angle(np.asarray(t1).astype(LD), np.asarray(r1).astype(LD)), _angle(np.asarray(t2).astype(LD), np.asarray(r2).astype(LD)))


def tangent_angle(normals, t1, t2):
    """angle between the tangent pair and the reference's, in eps of the normals' type (SWITCH_BAND: the nearer reference)"""
    r1, r2, rr, a1, a2 = reference_frames(normals)
    e = LD(eps(np.asarray(normals).dtype))
    ang = pair_angle(t1, t2, r1, r2)
    band = np.abs(rr - LD(SWITCH)) <= SWITCH_BAND * e
    ang = np.where(band, np.minimum(ang, pair_angle(t1, t2, a1, a2)), ang)
    return (ang / e).astype(np.float64)


def check_frames(normals, t1, t2, what=""):
    """the assertions every construction must pass; returns (worst defect, worst angle) in eps"""
    d, a = defect(normals, t1, t2), tangent_angle(normals, t1, t2)
    i, j = int(np.argmax(d)), int(np.argmax(a))
    print(f"{what}: {np.asarray(normals).dtype} worst defect {d[i]:.1f} eps of {DEFECT_LIMIT:.0f} at n = {np.asarray(normals)[i]}, "
          f"worst tangent angle {a[j]:.1f} eps of {ANGLE_LIMIT:.0f} at n = {np.asarray(normals)[j]}")
    assert d[i] <= DEFECT_LIMIT, (what, d[i], np.asarray(normals)[i])
    assert a[j] <= ANGLE_LIMIT, (what, a[j], np.asarray(normals)[j])
    return float(d[i]), float(a[j])


def emulate(normals, two_seeds=True, fast=False):
    """The device construction in numpy, one rounding per operation in the normals' type (fast: the normalisation as a
    product with ONE correctly rounded 1 / sqrt, as face_basis_fast does with the hardware's). two_seeds = False is the
    reference's rule, kept to show that the assertions above fail on it."""
    n = np.asarray(normals)
    T = n.dtype.type

    def project(s):
        dp = (n[:, 0] * s[:, 0] + n[:, 1] * s[:, 1]) + n[:, 2] * s[:, 2]
        t = np.stack([s[:, k] - dp * n[:, k] for k in range(3)], 1)
        return t, (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]

    a, b = _seeds(n)
    t, r2 = project(a)
    if two_seeds:
        tb, rb = project(b)
        sw = r2 < T(SWITCH)
        t, r2 = np.where(sw[:, None], tb, t), np.where(sw, rb, r2)
    with np.errstate(invalid="ignore", divide="ignore"):
        if fast:
            t1 = t * (1.0 / np.sqrt(r2.astype(LD))).astype(n.dtype)[:, None]
        else:
            t1 = t / np.sqrt(r2)[:, None]
    t2 = np.stack([n[:, 1] * t1[:, 2] - n[:, 2] * t1[:, 1], n[:, 2] * t1[:, 0] - n[:, 0] * t1[:, 2], n[:, 0] * t1[:, 1] - n[:, 1] * t1[:, 0]], 1)
    return t1, t2


def axis_frames(dtype):
    """(n, t1, t2) of flux_math.hpp: axis_basis for +e_x, -e_x, +e_y, -e_y, +e_z, -e_z, signed zeros as it writes them (+0)"""
    n, t1, t2 = (np.zeros((6, 3), dtype) for _ in range(3))
    for axis in range(3):
        for j, s in enumerate((1.0, -1.0)):
            i = 2 * axis + j
            n[i, axis] = s
            if axis == 0:
                t1[i, 2], t2[i, 1] = -s, 1.0
            elif axis == 1:
                t1[i, 0], t2[i, 2] = s, -1.0
            else:
                t1[i, 1], t2[i, 0] = s, -1.0
    return n, t1, t2


def exact_r2(normals):
    n = np.asarray(normals).astype(LD)
    return _gram_schmidt(n, _seeds(n)[0])[2]


def golden_normal_arrays():
    """every normal array under tests/golden as (name, (k, 3) array): `xyz_n_*` of the flux vectors, `*|normals` of the kernel
    vectors (2D ones padded with nz = 0, as the kernels read them)"""
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        z = np.load(path)
        for key in z.files:
            low = key.lower()
            if low.endswith("normal_dim") or not ("normals" in low or low.startswith("xyz_n_") or low.endswith("_n") or "|n|" in low):
                continue
            a = z[key]
            if not np.issubdtype(a.dtype, np.floating):
                continue
            dim = int(z[key[: -len("normals")] + "normal_dim"][0]) if low.endswith("normals") else 3
            a = a.reshape(-1, dim)
            if dim == 2:
                a = np.concatenate([a, np.zeros((len(a), 1), a.dtype)], 1)
            out.append((os.path.basename(path) + ":" + key, a))
    return out


_cache = {}


def normals(dtype, seed=20261020):
    """The families of the frame tests, {name: (k, 3) array of `dtype`}; seeded, cached, read-only."""
    dtype = np.dtype(dtype)
    if (dtype, seed) in _cache:
        return _cache[(dtype, seed)]
    rng = np.random.default_rng(seed)
    fam = {"axes": axis_frames(dtype)[0]}
    ang = rng.uniform(0, 2 * np.pi, 64)
    fam["planar"] = np.stack([np.cos(ang), np.sin(ang), np.zeros(64)], 1).astype(dtype)
    fam["bad"] = np.stack([BAD, -BAD]).astype(dtype)          # rounded from double to T
    # an orthonormal completion of the bad direction, and normals at angle theta from +-BAD with random azimuth
    e1 = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    e2 = np.cross(BAD, e1)

    def around(theta, phi, sign):
        return sign[:, None] * (np.cos(theta)[:, None] * BAD + np.sin(theta)[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2))

    k = 512
    theta = np.exp(rng.uniform(np.log(1e-7), np.log(0.6), k))
    fam["sweep"] = around(theta, rng.uniform(0, 2 * np.pi, k), np.where(np.arange(k) % 2 == 0, 1.0, -1.0)).astype(dtype)
    # the cone boundary: per azimuth the theta with |r|^2 = 2^-6 by bisection, moved by a random +-8 eps (relative) and rounded
    # to T, which scatters the exact |r|^2 of the rounded normals by about +-eps around 2^-6 (an ulp of 2^-6 is eps / 64); of
    # 8192 such normals the 24 nearest on either side: within a few ulp
    k = 8192
    phi, sign = rng.uniform(0, 2 * np.pi, k), np.where(rng.random(k) < 0.5, 1.0, -1.0)
    lo, hi = np.full(k, 0.01), np.full(k, 0.3)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        below = exact_r2(around(mid, phi, sign)) < SWITCH
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    cand = around(lo * (1 + 8 * eps(dtype) * rng.uniform(-1, 1, k)), phi, sign).astype(dtype)
    d = (exact_r2(cand) - LD(SWITCH)).astype(np.float64)
    inside, outside = np.flatnonzero(d < 0), np.flatnonzero(d >= 0)
    pick = np.concatenate([inside[np.argsort(-d[inside])[:24]], outside[np.argsort(d[outside])[:24]]])
    fam["boundary"] = cand[pick]
    g = rng.standard_normal((4096, 3))
    fam["sphere"] = (g / np.linalg.norm(g, axis=1)[:, None]).astype(dtype)
    gold = [a for _, a in golden_normal_arrays() if a.dtype == dtype]
    fam["golden"] = np.unique(np.concatenate(gold), axis=0)
    for a in fam.values():
        a.setflags(write=False)
    _cache[(dtype, seed)] = fam
    return fam


def all_normals(dtype):
    """the families in one array, axes first"""
    return np.concatenate(list(normals(dtype).values()))


def rotation_to_bad():
    """R (double, 3 x 3) with R e_x = (1, -1, 1) / sqrt 3: columns = an explicit orthonormal completion, det +1"""
    c0 = BAD
    c1 = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    c2 = np.cross(c0, c1)
    R = np.stack([c0, c1, c2], 1)
    assert np.abs(R.T @ R - np.eye(3)).max() < 4e-16 and np.linalg.det(R) > 0.999
    return R


def rotation_map(R):
    """a mesh mapping (unstructured.PrismHexMesh / TetHexMesh): the unit cube turned by R"""
    def mapping(x, y, z):
        return np.stack([R[k, 0] * x + R[k, 1] * y + R[k, 2] * z for k in range(3)], axis=-1)
    return mapping


def dictionary_rows(normals, areas):
    """geo_table (rows {n, area, t1, 0, t2, 0}, double) of a tile plan with one wall face per (normal, area), read through
    t8gpu_plan_plain_compressed; the rows are in the planner's order (sorted by bit pattern), one per distinct tuple"""
    from t8gpu_amd import synth
    from t8gpu_amd.plan import HostPlainPlan, _lib
    k = len(normals)
    plan = HostPlainPlan(k, 0, 0, k, 3, np.arange(k, dtype=np.int32), np.ascontiguousarray(normals, np.float64).reshape(-1),
                         np.ascontiguousarray(areas, np.float64))
    table = np.full((plan.geo_table.shape[0], 12), np.nan)
    _lib().t8gpu_plan_plain_compressed(plan._owner.h, None, None, synth._p(table))
    assert np.array_equal(table.view(np.uint8), np.ascontiguousarray(plan.geo_table).view(np.uint8))
    return table


def identity_map(x, y, z):
    return np.stack([x, y, z], axis=-1)
