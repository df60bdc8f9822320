"""The numpy definitions of the tracer pass (t8gpu_amd/tracers.py: host_velocity, host_map, host_predict, host_correct;
DESIGN.md §15) and the coverage of the inputs the GPU tests run on (_tracers_ref.py). No GPU."""
import numpy as np
import pytest

import _sample_ref as sref
import _tracers_ref as ref
from t8gpu_amd import sample, tracers
from t8gpu_amd.synth import SynthMesh
from t8gpu_amd.tracers import ACTIVE, BELOW_ONE, LEFT, LOST, OK, OPEN, PERIODIC, WALL

PP = np.array([PERIODIC] * 4, np.int32)
WW_PP = np.array([WALL, WALL, PERIODIC, PERIODIC], np.int32)
OO_WW = np.array([OPEN, OPEN, WALL, WALL], np.int32)
WO_PP = np.array([WALL, OPEN, PERIODIC, PERIODIC], np.int32)


# ---- 1: constant velocity on a periodic mesh ---------------------------------------------------------------------------------
def test_constant_velocity_on_a_periodic_mesh():
    """Heun's step in a constant field adds dt u; every step rounds x + dt u once (half an ulp of a value below 1, 2^-54) and
    the wrap is exact or rounds once more, so n steps stay within n ulp of 1 (n 2^-52) of x0 + n dt u wrapped. The distance is
    taken on the circle: a particle next to the wrap may sit on its other side."""
    mesh = SynthMesh(2, 3, 3)
    part = mesh.partition()
    u = np.array([0.37, -0.61])
    state = np.zeros((5, part.N))
    state[0], state[1], state[2], state[4] = 2.0, 2.0 * u[0], 2.0 * u[1], 5.0
    kinds = tracers.side_kinds(mesh.sides)
    assert np.array_equal(kinds, PP)
    x0 = np.random.default_rng(3).uniform(0.0, 1.0, (500, 2))
    t, dt, n = ref.initial(x0), 0.11, 40
    for _ in range(n):
        _, t, det = ref.host_round(part, kinds, state, state, dt, t)
        assert np.all(det["held"] == 1) and np.all(det["k"] == u)
    assert np.all(t["status"] == ACTIVE)
    want = x0 + n * dt * u
    want -= np.floor(want)
    d = np.abs(t["x"] - want)
    d = np.minimum(d, 1.0 - d)
    assert np.all((t["x"] >= 0.0) & (t["x"] < 1.0))
    assert d.max() <= n * 2.0 ** -52, d.max()
    # and backwards again
    for _ in range(n):
        _, t, _ = ref.host_round(part, kinds, state, state, -dt, t)
    d = np.abs(t["x"] - x0)
    assert np.minimum(d, 1.0 - d).max() <= 2 * n * 2.0 ** -52


# ---- 2: map on hand-picked points ----------------------------------------------------------------------------------------------
def test_map_periodic():
    p = np.array([[0.25, 0.5], [1.25, -0.25], [1.0, 0.0], [-1e-300, 0.3], [-0.0, 3.75], [np.nextafter(1.0, 0.0), -2.0]])
    y, out = tracers.host_map(p, PP)
    assert out.tolist() == [OK] * 6
    assert np.array_equal(y, [[0.25, 0.5], [0.25, 0.75], [0.0, 0.0], [0.0, 0.3], [0.0, 0.75], [np.nextafter(1.0, 0.0), 0.0]])
    assert np.all((y >= 0.0) & (y < 1.0))


def test_map_walls_mirror():
    p = np.array([[-0.25, 0.5], [1.25, 0.5], [1.0, 0.5], [-1.0, 0.5], [-1e-300, 0.5], [2.0, 0.5], [-1.5, 0.5], [2.5, 0.5],
                  [0.0, 0.5]])
    y, out = tracers.host_map(p, WW_PP)
    assert out.tolist() == [OK, OK, OK, OK, OK, OK, LOST, LOST, OK]
    assert np.array_equal(y[:6, 0], [0.25, 0.75, BELOW_ONE, BELOW_ONE, 1e-300, 0.0])
    assert BELOW_ONE < 1.0 and np.nextafter(BELOW_ONE, 2.0) == 1.0
    assert y[8, 0] == 0.0


def test_map_open_sides_and_non_finite():
    p = np.array([[-0.25, 1.25], [1.0, 0.5], [-1e-300, -0.5], [0.5, 1.25], [np.nan, 0.5], [0.5, np.inf], [-0.25, np.nan],
                  [0.5, -3.0]])
    y, out = tracers.host_map(p, OO_WW)
    assert out.tolist() == [LEFT, LEFT, LEFT, OK, LOST, LOST, LOST, LOST]
    for i in range(3):                                              # left: the raw point on EVERY axis, the mirrored one too
        assert np.array_equal(y[i], p[i])
    assert np.array_equal(y[3], [0.5, 0.75])
    # one side a wall, the other open
    y, out = tracers.host_map(np.array([[-0.25, 0.1], [1.25, 0.1]]), WO_PP)
    assert out.tolist() == [OK, LEFT] and y[0, 0] == 0.25 and y[1, 0] == 1.25
    # provider codes: periodic, wall, and every open kind
    assert tracers.side_kinds([-1, -1, 0, 0, 1, 2, 9, 10, 15]).tolist() == [PERIODIC] * 2 + [WALL] * 2 + [OPEN] * 5


# ---- 3: left and lost particles stay frozen ----------------------------------------------------------------------------------------
def test_left_and_lost_stay_frozen():
    x = np.array([[0.95, 0.5], [0.5, 0.5], [0.5, 0.5], [0.2, 0.2], [0.9, 0.9]])
    k = np.array([[1.0, 0.0], [np.inf, 0.0], [0.1, 0.1], [0.1, 0.1], [0.1, 4.0]])
    held = np.array([1, 1, 0, 1, 1], np.int32)
    t = ref.initial(x)
    dt = 0.1
    xs, k1, flag, status = tracers.host_predict(t["x"], t["status"], t["xs"], t["k1"], t["flag"], k, held, dt, OO_WW)
    assert status.tolist() == [ACTIVE, LOST, LOST, ACTIVE, ACTIVE] and flag.tolist() == [1, 0, 0, 0, 0]
    assert np.array_equal(xs[0], [0.95 + 0.1 * 1.0, 0.5]) and np.array_equal(xs[1], x[1]) and np.array_equal(xs[2], x[2])
    assert np.array_equal(k1, k)
    # correct: the flagged particle ignores k2 and held, and leaves at predict's raw point
    k2 = np.array([[-9.0, 7.0], [0.0, 0.0], [0.0, 0.0], [0.3, 0.1], [0.1, 4.0]])
    held2 = np.array([0, 1, 1, 1, 0], np.int32)
    x1, status1 = tracers.host_correct(x, status, k1, flag, k2, held2, dt, OO_WW)
    assert status1.tolist() == [LEFT, LOST, LOST, ACTIVE, LOST]
    assert np.array_equal(x1[0], xs[0]) and x1[0, 0] >= 1.0
    assert np.array_equal(x1[1], x[1]) and np.array_equal(x1[2], x[2]) and np.array_equal(x1[4], x[4])
    assert np.array_equal(x1[3], x[3] + (0.5 * dt) * (k1[3] + k2[3]))
    # further rounds with any velocity: the three inactive ones keep every entry
    wild = np.full((5, 2), 30.0)
    t1 = {"x": x1, "status": status1, "xs": xs, "k1": k1, "flag": flag}
    xs2, k12, flag2, status2 = tracers.host_predict(x1, status1, xs, k1, flag, wild, np.ones(5, np.int32), dt, OO_WW)
    x2, status3 = tracers.host_correct(x1, status2, k12, flag2, wild, np.ones(5, np.int32), dt, OO_WW)
    for i in (0, 1, 2, 4):
        assert ref.bits_equal(x2[i], t1["x"][i]) and ref.bits_equal(xs2[i], xs[i]) and ref.bits_equal(k12[i], k1[i])
        assert status3[i] == status1[i] and flag2[i] == flag[i]
    assert status3[3] == LEFT                                          # (3 dt to the right and up: out through x)


# ---- 4: k and held summed over partitions ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3, 5])
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", ["refined-2d-walls", "open-2d", "walls-open-3d"])
def test_partitions_sum_to_the_single_partition_result(mesh, subgrid, nranks):
    part, kinds = ref.partition(mesh, subgrid), ref.kinds_of(mesh)
    u = ref.states_of(mesh, subgrid)
    parts = [ref.partition(mesh, subgrid, r, nranks) for r in range(nranks)]
    states = [[ref.rank_state(mesh, subgrid, s, p) for s in u] for p in parts]
    t = ref.initial(ref.points_of(mesh, subgrid)[0])
    inside = sample.host_locate(part, t["x"]) >= 0
    for r in range(ref.ROUNDS):
        order = [[s[r % 2], s[(r + 1) % 2]] for s in states]
        mid, end, det = ref.host_round(part, kinds, None, None, ref.DT[mesh], t, parts=parts, states=order)
        want_mid, want_end, want_det = ref.reference(mesh, subgrid, np.float64)[r]
        if r == 0:
            assert np.array_equal(det["held"], inside.astype(np.int64))          # exactly one claim per point inside
        assert det["held"].max() == 1 and np.array_equal(det["held"], want_det["held"])
        for name in ("xs", "k1", "flag", "status"):
            assert ref.bits_equal(mid[name], want_mid[name]), (r, name)
        for name in ("x", "status"):
            assert ref.bits_equal(end[name], want_end[name]), (r, name)
        t = end


# ---- 5: what the inputs of the GPU tests cover -------------------------------------------------------------------------------------
def crossings(raw, kinds, kind):
    """per particle: does the raw point cross a side of `kind` on some axis"""
    hit = np.zeros(raw.shape[0], bool)
    with np.errstate(invalid="ignore"):
        for a in range(raw.shape[1]):
            if kinds[2 * a] == kind:
                hit |= raw[:, a] < 0.0
            if kinds[2 * a + 1] == kind:
                hit |= raw[:, a] >= 1.0
    return hit


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", ref.NAMES)
def test_reference_inputs_cover_the_cases(mesh, subgrid, dtype):
    part, kinds, dt = ref.partition(mesh, subgrid), ref.kinds_of(mesh), ref.DT[mesh]
    points, cls = ref.points_of(mesh, subgrid)
    m = points.shape[0]
    assert m % 64 != 0 and m > 1003
    a, b = ref.planted(mesh, subgrid)
    u = [s.astype(dtype) for s in ref.states_of(mesh, subgrid)]
    assert all(s[0, a] == 0 and np.isnan(s[1, b]) for s in u)
    seeds_outside = np.zeros(m, bool)
    seeds_outside[sample.host_locate(part, points) < 0] = True
    assert seeds_outside[cls["outside"]].all() and seeds_outside[cls["bad"]].all() and not seeds_outside[cls["random"]].any()
    wraps = mirrors = leaves = 0
    x, status = points, np.zeros(m, np.uint8)
    for r, (mid, end, det) in enumerate(ref.reference(mesh, subgrid, dtype)):
        act = status == ACTIVE
        # the cells the velocities came from, and where the particles went
        c0 = sample.host_locate(part, x)
        cs = sample.host_locate(part, mid["xs"])
        c1 = sample.host_locate(part, end["x"])
        still = act & (end["status"] == ACTIVE)
        changed = np.count_nonzero(c1[still] != c0[still])
        assert changed >= 0.05 * np.count_nonzero(act), (r, changed, np.count_nonzero(act))
        with np.errstate(all="ignore"):
            raw1 = x + dt * mid["k1"]
            raw2 = x + (0.5 * dt) * (mid["k1"] + np.where((mid["flag"] != 0)[:, None], mid["k1"], det["k2"]))
        ok1, ok2 = act & (mid["status"] == ACTIVE) & (mid["flag"] == 0), act & (end["status"] != LOST)
        stay = act & (end["status"] == ACTIVE)                      # (wraps and mirrors count where map's outcome was OK)
        wraps += np.count_nonzero(ok1 & crossings(raw1, kinds, PERIODIC)) + np.count_nonzero(stay & crossings(raw2, kinds, PERIODIC))
        mirrors += np.count_nonzero(ok1 & crossings(raw1, kinds, WALL)) + np.count_nonzero(stay & crossings(raw2, kinds, WALL))
        leaves += np.count_nonzero(act & (end["status"] == LEFT))
        assert np.array_equal(act & (end["status"] == LEFT), act & (mid["flag"] != 0) | (ok2 & crossings(raw2, kinds, OPEN)))
        # lost: only through a planted cell or an outside / NaN seed
        lost_now = act & (end["status"] == LOST)
        in_predict = act & (mid["status"] == LOST)
        cause = np.where(in_predict, c0, cs)
        allowed = seeds_outside | (cause == a) | (cause == b)
        assert np.all(allowed[lost_now]), (r, np.flatnonzero(lost_now & ~allowed))
        x, status = end["x"], end["status"]
    has = {k: bool(np.any(kinds == k)) for k in (PERIODIC, WALL, OPEN)}
    print(f"{mesh} subgrid={subgrid} {np.dtype(dtype).name}: M={m} wraps={wraps} mirrors={mirrors} leaves={leaves} "
          f"lost={np.count_nonzero(status == LOST)} inactive={np.count_nonzero(status != ACTIVE)}")
    assert not has[PERIODIC] or wraps >= 20
    assert not has[WALL] or mirrors >= 20
    assert not has[OPEN] or leaves >= 20
    lost = status == LOST
    assert lost[cls["outside"]].all() and lost[cls["bad"]].all()
    assert np.count_nonzero(lost & ~seeds_outside) >= 2                  # ... and the planted cells took some
    assert np.count_nonzero(status != ACTIVE) <= m // 2


def test_seeds():
    lat = tracers.lattice(2, 4)
    assert lat.shape == (16, 2) and np.array_equal(lat[:5, 0], [0.125, 0.375, 0.625, 0.875, 0.125]) and lat[4, 1] == 0.375
    lat = tracers.lattice(3, (2, 1, 3), lo=(0.0, 0.5, 0.0), hi=(1.0, 1.0, 0.5))
    assert lat.shape == (6, 3) and np.array_equal(lat[1], [0.75, 0.75, 0.5 / 6])
    with pytest.raises(ValueError):
        tracers.lattice(2, (2, 2, 2))
    for subgrid in (False, True):
        part = sref.partition("refined-3d-periodic", subgrid)

        class Solver:
            pass
        s = Solver()
        s.part = part
        if subgrid:
            s.S = 64
        c = tracers.cell_centres(s)
        assert c.shape == (part.N * part.cells_per_element, 3)
        assert np.array_equal(sample.host_locate(part, c), np.arange(c.shape[0], dtype=np.int32))
        lo, edge, _ = sref.cell_boxes(part)
        assert np.array_equal(c, lo + 0.5 * edge[:, None])
