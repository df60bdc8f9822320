"""Host side of the face-frame tests (no GPU): the geometry dictionary of tile_plan.cpp and the oracle's face_basis against
the long-double reference of tests/_frame_ref.py, on the normals the -m gpu test (test_gpu_frames.py) runs on too.

Both are compiled without contraction and use the correctly rounded square root and division of the host, so they must ALSO
equal the one-rounding-per-operation numpy emulation bit for bit -- that is the bit-for-bit agreement the comment above
flux_math.hpp: face_basis demands of the dictionary, and it catches a copy that lost the second seed."""
import numpy as np
import pytest

import _frame_ref as FR
import _oracle as O
from t8gpu_amd.plan import HostPlainPlan
from t8gpu_amd.unstructured import PrismHexMesh

DTYPES = [np.float32, np.float64]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def check_rows(table, normals, areas):
    """every (normal, area) has its row; n and area copied unchanged, words 7 and 11 zero; returns the rows' (n, t1, t2)"""
    key = {bits(np.append(n, a)).tobytes() for n, a in zip(np.asarray(normals, np.float64), areas)}
    assert {bits(r[:4]).tobytes() for r in table} == key and len(table) == len(key)
    assert np.array_equal(bits(table[:, [7, 11]]), bits(np.zeros((len(table), 2))))          # +0, bitwise
    return table[:, 0:3].copy(), table[:, 4:7].copy(), table[:, 8:11].copy()


def test_reference_frames_are_rotations_and_the_old_rule_fails_the_assertions():
    """the metrics on the reference itself; then the mutation check of these tests: the reference's single-seed rule, emulated
    in numpy, must FAIL the shared assertions at the bad direction (fp32: t1 = -n, t2 = 0; fp64: NaN or the same)"""
    for T in DTYPES:
        n = FR.all_normals(T)
        t1, t2, r2, _, _ = FR.reference_frames(n)
        assert FR.defect(n, t1, t2).max() < 4 and FR.tangent_angle(n, t1, t2).max() == 0     # (|n|^2 - 1 of the rounded normal)
        bad = FR.normals(T)["bad"]
        assert (FR.exact_r2(bad) < 1e-6).all()
        FR.check_frames(bad, *FR.emulate(bad), "two seeds, emulated")
        with pytest.raises(AssertionError):
            FR.check_frames(bad, *FR.emulate(bad, two_seeds=False), "one seed, emulated")
        sweep = FR.normals(T)["sweep"]
        with pytest.raises(AssertionError):
            FR.check_frames(sweep, *FR.emulate(sweep, two_seeds=False), "one seed, emulated")


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("fast", [False, True])
def test_emulated_construction_keeps_the_limits(T, fast):
    for name, n in FR.normals(T).items():
        FR.check_frames(n, *FR.emulate(n, fast=fast), f"emulation fast={fast} {name}")


def test_generator_covers_what_it_promises():
    for T in DTYPES:
        fam = FR.normals(T)
        e = FR.eps(T)
        d = (FR.exact_r2(fam["boundary"]) - FR.LD(FR.SWITCH)).astype(np.float64) / (e / 64)      # in ulp of 2^-6
        assert (d < 0).sum() == 24 and (d >= 0).sum() == 24 and np.abs(d).max() < 4
        r2 = FR.exact_r2(fam["sweep"]).astype(np.float64)
        assert r2.min() < 1e-12 and (r2 < FR.SWITCH).sum() > 300 and (r2 > FR.SWITCH).sum() > 30
        assert (fam["planar"][:, 2] == 0).all() and len(fam["golden"]) > 500
        for a in fam.values():
            assert a.dtype == T and np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1).max() < 2 * e


def test_no_golden_normal_lies_in_the_cone():
    """so that the second seed changes no committed fixture: every normal array under tests/golden stays at |r|^2 >= 2^-6, with
    the band in which the rounded |r|^2 could decide otherwise to spare (the flux vectors: min |r|^2 = 0.0271; the kernel and AMR
    vectors hold axis-aligned normals, |r|^2 = 1)"""
    arrays = FR.golden_normal_arrays()
    assert {a.dtype for _, a in arrays} == {np.dtype(np.float32), np.dtype(np.float64)} and len(arrays) >= 16
    for name, a in arrays:
        assert FR.exact_r2(a).min() > FR.SWITCH + FR.SWITCH_BAND * FR.eps(a.dtype), name
    flux = [a for name, a in arrays if "xyz_n_" in name]
    assert len(flux) == 2 and all(len(a) == 1024 for a in flux)
    assert 0.0271 < min(float(FR.exact_r2(a).min()) for a in flux) < 0.0272


def test_axis_frames_are_the_construction_on_axis_normals():
    """axis_basis == the frame of +-e_axis. (Numerically: the construction leaves -0 in five places -- -n[0] for n = e_y, e_z, and
    (-0) - (+0) in the cross product -- where axis_basis writes +0; zeros of either sign are equal here.)"""
    for T in DTYPES:
        n, t1, t2 = FR.axis_frames(T)
        e1, e2 = FR.emulate(n)
        assert np.array_equal(e1, t1) and np.array_equal(e2, t2)
        f1, f2 = FR.emulate(n, fast=True)
        assert np.array_equal(f1, t1) and np.array_equal(f2, t2)


def test_dictionary_frames_on_the_generated_normals():
    n = FR.all_normals(np.float64)
    n = n[np.sort(np.unique(n, axis=0, return_index=True)[1])]
    areas = np.random.default_rng(3).uniform(0.5, 2.0, len(n))
    rows_n, t1, t2 = check_rows(FR.dictionary_rows(n, areas), n, areas)
    FR.check_frames(rows_n, t1, t2, "tile_plan.cpp dictionary")
    e1, e2 = FR.emulate(rows_n)
    assert np.array_equal(bits(t1), bits(e1)) and np.array_equal(bits(t2), bits(e2))         # face_basis's arithmetic, bit for bit
    # outside the cone the arithmetic and the bits are the reference's single-seed construction
    out = FR.exact_r2(rows_n) > FR.SWITCH + FR.SWITCH_BAND * FR.eps(np.float64)
    o1, o2 = FR.emulate(rows_n[out], two_seeds=False)
    assert out.sum() > 4000 and np.array_equal(bits(t1[out]), bits(o1)) and np.array_equal(bits(t2[out]), bits(o2))
    ax = FR.axis_frames(np.float64)
    for a, b1, b2 in zip(*ax):
        i = int(np.flatnonzero((rows_n == a).all(1))[0])
        assert np.array_equal(t1[i], b1) and np.array_equal(t2[i], b2)


def test_dictionary_frames_on_a_mesh_rotated_into_the_cone():
    """PrismHexMesh mapped by the rotation that takes e_x to (1, -1, 1) / sqrt 3: every x-face has its normal at the bad
    direction to rounding, where the single-seed frame is no rotation"""
    R = FR.rotation_to_bad()
    part = PrismHexMesh((2, 2, 2), split="checker", mapping=FR.rotation_map(R), periodic=True).partition()
    plan = HostPlainPlan.from_partition(part)
    assert plan.geo_table.shape[0] > 0
    n, t1, t2 = plan.geo_table[:, 0:3].copy(), plan.geo_table[:, 4:7].copy(), plan.geo_table[:, 8:11].copy()
    r2 = FR.exact_r2(n).astype(np.float64)
    assert (r2 < 1e-20).sum() >= 1 and (r2 > 0.5).sum() >= 3, r2
    nr = part.normals.reshape(-1, 3)
    assert {bits(x).tobytes() for x in n} == {bits(x).tobytes() for x in nr}
    assert (plan.geo_table[:, [7, 11]] == 0).all()
    FR.check_frames(n, t1, t2, "dictionary of the rotated mesh")
    with pytest.raises(AssertionError):
        FR.check_frames(n, *FR.emulate(n, two_seeds=False), "one seed on the rotated mesh")


def test_curved_digest_mesh_has_nine_rows_in_the_cone():
    """tests/golden/tile_plan_digests.json, case curved_prism_hex: 9 of the 2 794 distinct normals of that mesh lie in the cone
    (|r|^2 = 8.9e-4); their tangent words are what the second seed changed in that plan (README there), every other row is the
    single-seed construction bit for bit"""
    import _plan_digests as D
    plan = HostPlainPlan.from_partition(PrismHexMesh((8, 8, 10)).partition(), **D.CAPS, patches=True)
    g = plan.geo_table
    r2 = FR.exact_r2(g[:, 0:3]).astype(np.float64)
    cone = r2 < FR.SWITCH
    assert len(g) == 2794 and cone.sum() == 9 and np.abs(r2[cone] - 8.8565e-4).max() < 1e-8
    assert not (np.abs(r2 - FR.SWITCH) <= FR.SWITCH_BAND * FR.eps(np.float64)).any()
    o1, o2 = FR.emulate(g[~cone, 0:3].copy(), two_seeds=False)
    assert np.array_equal(bits(g[~cone, 4:7]), bits(o1)) and np.array_equal(bits(g[~cone, 8:11]), bits(o2))
    FR.check_frames(g[:, 0:3].copy(), g[:, 4:7].copy(), g[:, 8:11].copy(), "dictionary of the curved digest mesh")


@pytest.mark.parametrize("T", DTYPES)
def test_oracle_frames(T):
    n = np.ascontiguousarray(FR.all_normals(T))
    t1, t2 = np.full_like(n, np.nan), np.full_like(n, np.nan)
    getattr(O.lib(), "oracle_face_basis_" + O.suf(T))(len(n), O.p(n), O.p(t1), O.p(t2))
    FR.check_frames(n, t1, t2, "oracle.hpp face_basis")
    e1, e2 = FR.emulate(n)
    assert np.array_equal(bits(t1), bits(e1)) and np.array_equal(bits(t2), bits(e2))
