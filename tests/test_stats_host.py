"""The time statistics without a GPU: closed forms on the numpy reference (tests/_stats_ref.py), the transfer's conservation,
and the validation of names and weights in t8gpu_amd/stats.py that touches no device."""
import numpy as np
import pytest

import _stats_ref as ref
from t8gpu_amd import stats
from t8gpu_amd.synth import SynthMesh


def state_of(rho, v, p, cells):
    v = np.asarray(v, np.float64)
    one = np.array([rho, rho * v[0], rho * v[1], rho * v[2], p / 0.4 + 0.5 * rho * (v ** 2).sum()])
    return np.repeat(one[:, None], cells, axis=1)


def test_tables_agree_with_the_package():
    assert ref.PLANES == stats.PLANES == len(stats.SLOTS) and ref.RESULT_PLANES == stats.RESULT_PLANES
    for name, (first, count) in stats.RESULTS.items():
        assert ref.SLOTS[name] == list(range(first, first + count)), name
    assert sorted(k for rows in ref.SLOTS.values() for k in rows) == list(range(ref.RESULT_PLANES))


def test_quantities_of_a_known_state():
    q = ref.quantities(state_of(2.0, (3.0, -1.0, 0.5), 1.6, 1))[:, 0]
    c = np.sqrt(1.4 * 1.6 / 2.0)
    want = [2.0, 6.0, -2.0, 1.0, 1.6 / 0.4 + 10.25, 1.6, 4.0, 2.56, 18.0, 2.0, 0.5, -6.0, 3.0, -1.0, np.sqrt(10.25) / c]
    assert np.allclose(q, want, rtol=1e-14, atol=0)


def test_constant_state_has_no_fluctuation():
    """under any weights: rms = 0 and stress = 0 up to the rounding of 50 additions -- two terms of about 100 * 2^-53
    relative error each, under a square root for the rms: 1e-6 of the mean; the stress is linear in them: 1e-12 rho |u|^2"""
    rng = np.random.default_rng(1)
    rho, v, p = 1.3, (0.4, -0.7, 0.2), 0.9
    st = state_of(rho, v, p, 7)
    sums, W = np.zeros((ref.PLANES, 7)), 0.0
    for w in rng.uniform(0.01, 3.0, 50):
        sums, W = ref.accumulate(sums, st, w), W + w
    r = ref.results(sums, W)
    assert np.allclose(r[0], rho, rtol=1e-13) and np.allclose(r[7:10], np.array(v)[:, None], rtol=1e-13)
    assert np.allclose(r[5], p, rtol=1e-13)
    assert r[10].max() <= 1e-6 * rho and r[11].max() <= 1e-6 * p
    assert np.abs(r[12:18]).max() <= 1e-12 * rho * sum(x * x for x in v)
    assert np.abs(r[18]).max() <= 1e-12 * sum(x * x for x in v)


def test_two_alternating_states_give_the_weighted_variance():
    """states a, b with total weights w1, w2: variance w1 w2 (a - b)^2 / (w1 + w2)^2 for rho and p; the Favre stress
    w1 w2 rho_a rho_b (u_a - u_b)_i (u_a - u_b)_j / ((w1 rho_a + w2 rho_b) (w1 + w2))"""
    w1, w2 = 0.75, 2.5
    ra, rb, pa, pb = 1.0, 1.5, 1.0, 0.7
    ua, ub = np.array([0.5, -0.25, 0.125]), np.array([-0.5, 0.75, 0.25])
    a, b = state_of(ra, ua, pa, 3), state_of(rb, ub, pb, 3)
    sums, W = np.zeros((ref.PLANES, 3)), 0.0
    for _ in range(4):                                   # alternating: the order does not matter to the closed form
        sums, W = ref.accumulate(sums, a, w1 / 4), W + w1 / 4
        sums, W = ref.accumulate(sums, b, w2 / 4), W + w2 / 4
    r = ref.results(sums, W)
    f = w1 * w2 / (w1 + w2) ** 2
    assert np.allclose(r[10], np.sqrt(f) * abs(ra - rb), rtol=1e-13)
    assert np.allclose(r[11], np.sqrt(f) * abs(pa - pb), rtol=1e-13)
    d = ua - ub
    g = w1 * w2 * ra * rb / ((w1 * ra + w2 * rb) * (w1 + w2))
    for k, (i, j) in enumerate(ref.STRESS_PAIRS):
        assert np.allclose(r[12 + k], g * d[i - 1] * d[j - 1], rtol=1e-12, atol=1e-15), k
    mean_rho = (w1 * ra + w2 * rb) / (w1 + w2)
    assert np.allclose(r[18], 0.5 * g * (d ** 2).sum() / mean_rho, rtol=1e-12)
    assert np.allclose(r[7:10], ((w1 * ra * ua + w2 * rb * ub) / (w1 * ra + w2 * rb))[:, None], rtol=1e-13)


def marks_for(mesh):
    """coarsen what was refined, refine some of the rest"""
    part = mesh.partition()
    lev = part.levels[:part.N]
    marks = np.where(lev == lev.max(), -1, 0).astype(np.int8)
    coarse = np.flatnonzero(lev == lev.min())
    marks[coarse[len(coarse) // 2::7]] = 1
    return marks


def refined(dim, level, lo=0.3, hi=0.8):
    mesh = SynthMesh(dim, level, level)
    part = mesh.partition()
    c = part.centres[:part.N, :dim]
    marks = np.all((c > lo) & (c < hi), axis=1).astype(np.int8)
    marks[0] = 1
    return mesh.adapt(marks)[0]


@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("dim,level,lo", [(2, 3, 0.3), (3, 2, 0.2)])
def test_transfer_keeps_the_volume_integrals(dim, level, lo, subgrid):
    mesh = refined(dim, level, lo)
    part = mesh.partition(subgrid=subgrid)
    assert part.N == (115 if dim == 2 else 127)
    S = part.cells_per_element
    new_mesh, ad = mesh.adapt(marks_for(mesh))
    children, kept, coarsened = ref.cases_of(ad)
    assert children > 0 and kept > 0 and coarsened > 0
    new_part = new_mesh.partition(subgrid=subgrid)
    assert children + kept + coarsened == new_part.N
    sums = np.random.default_rng(2).uniform(0.5, 2.0, (ref.PLANES, part.N * S))
    new = ref.transfer(sums, ad, S, dim)
    assert new.shape == (ref.PLANES, new_part.N * S)
    before = (sums * np.repeat(part.volumes[:part.N] / S, S)).sum(axis=1)
    after = (new * np.repeat(new_part.volumes[:new_part.N] / S, S)).sum(axis=1)
    assert np.abs(after - before).max() <= 1e-13 * np.abs(before).max()
    const = ref.transfer(np.full((2, part.N * S), 0.375), ad, S, dim)
    assert np.all(const == 0.375)                                       # a constant stays one, exactly


def test_names_are_checked_without_a_device():
    assert stats.check_names("tke") == ["tke"]
    assert stats.check_names(["tke", "mean_density", "tke"]) == ["tke", "mean_density"]
    with pytest.raises(ValueError) as e:
        stats.check_names(["tke", "skewness"])
    for name in stats.RESULTS:
        assert name in str(e.value)
    assert stats.plane_names("reynolds_stress") == [f"reynolds_stress_{c}" for c in ("xx", "yy", "zz", "xy", "xz", "yz")]
    assert stats.plane_names("tke") == ["tke"]


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), None, "x"])
def test_weights_are_checked_without_a_device(bad):
    with pytest.raises(ValueError):
        stats.check_weight(bad)
    assert stats.check_weight(0.25) == 0.25 and stats.check_weight(np.float32(2.0)) == 2.0


def test_accumulate_refuses_a_bad_weight_before_touching_the_device():
    class NoDevice:                                      # any attribute access would be a use of the solver
        def __getattr__(self, name):
            raise AssertionError(f"accumulate touched solver.{name} before validating the weight")

    s = stats.Statistics.__new__(stats.Statistics)
    s.solver, s.sums, s.weight = NoDevice(), None, 0.0
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            s.accumulate(bad)
    with pytest.raises(ValueError):
        s.results(["tke"])                               # weight == 0
    with pytest.raises(ValueError):
        s.results(["nonsense"])
    assert s.weight == 0.0
