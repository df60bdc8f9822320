"""Inputs and the host reference of the tracer tests (test_tracers_host.py, test_gpu_tracers.py).

Meshes: the four of _sample_ref.MESHES, a 2D mesh open on both x sides (outflow, far field) and a 3D mesh with walls in x,
periodic in y and open in z (outflow, inflow), all at the small sizes of _sample_ref: base level 2-3, a box refined once.
Points: _sample_ref.point_set -- 1003 random points plus corner, face, outside and NaN points, M no multiple of 64.
States: perturbed_state with two seeds for u^n and u^(n+1) (round r advects from states[r % 2] to states[(r + 1) % 2]), with
two planted cells, both holding a random point: one with rho = 0 (its velocity is infinite) and one with NaN momentum.
dt: displacements of about one coarse cell per step (speeds of 0.5 to 0.7 on cells of 2^-3, in 3D 2^-2).

`reference(mesh, subgrid, dtype)` runs ROUNDS rounds of tracers.host_* and keeps everything after every phase; it is
computed once per case and never written. test_tracers_host.py asserts the coverage conditions on it that keep the GPU
comparisons from passing vacuously."""
import functools

import numpy as np

import _sample_ref as sref
from _gpu import perturbed_state
from t8gpu_amd import sample, tracers
from t8gpu_amd.synth import SynthMesh

ROUNDS = 3
POINT_SEED = 5
STATE_SEEDS = (11, 12)
INFLOW_STATES = np.array([[1.0, 0.1, 0.0, 0.0, 2.5]])


def refined_sides(dim, level, sides, lo, hi):
    """_sample_ref.refined with sides of its own"""
    mesh = SynthMesh(dim, level, level, sides=sides)
    part = mesh.partition()
    c = part.centres[: part.N, :dim]
    marks = np.all((c > lo) & (c < hi), axis=1).astype(np.int8)
    marks[0] = 1
    return mesh.adapt(marks)[0]


MESHES = dict(sref.MESHES)
MESHES["open-2d"] = lambda: refined_sides(2, 3, ("outflow", ("farfield", 0), "periodic", "periodic"), 0.3, 0.8)
MESHES["walls-open-3d"] = lambda: refined_sides(3, 2, ("wall", "wall", "periodic", "periodic", "outflow", 0), 0.2, 0.8)
SIZES = dict(sref.SIZES, **{"open-2d": 115, "walls-open-3d": 127})
DT = {"refined-2d-periodic": 0.2, "refined-2d-walls": 0.2, "refined-3d-periodic": 0.4, "band-2d": 0.2, "open-2d": 0.2,
      "walls-open-3d": 0.4}
NAMES = list(MESHES)


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    mesh = MESHES[name]()
    assert mesh.num_elements == SIZES[name]
    return mesh


@functools.lru_cache(maxsize=None)
def partition(name, subgrid, rank=0, nranks=1):
    return mesh_of(name).partition(rank, nranks, subgrid=subgrid)


def kinds_of(name):
    return tracers.side_kinds(mesh_of(name).sides)


@functools.lru_cache(maxsize=None)
def points_of(name, subgrid):
    points, cls = sref.point_set(partition(name, subgrid), POINT_SEED)
    assert points.shape[0] % 64 != 0 and cls["random"].stop == 1003
    points.setflags(write=False)
    return points, cls


@functools.lru_cache(maxsize=None)
def planted(name, subgrid):
    """(cell with rho = 0, cell with NaN momentum): the cells of the first two random points that lie in different cells"""
    part = partition(name, subgrid)
    cells = sample.host_locate(part, points_of(name, subgrid)[0][:64])
    a = int(cells[0])
    b = int(next(c for c in cells[1:] if c != a))
    assert a >= 0 and b >= 0
    return a, b


@functools.lru_cache(maxsize=None)
def states_of(name, subgrid):
    """(u^n, u^(n+1)) as float64 [5, all cells of the single-rank partition], with the planted cells"""
    part = partition(name, subgrid)
    a, b = planted(name, subgrid)
    out = []
    for seed in STATE_SEEDS:
        u = perturbed_state(part, seed)
        u[0, a] = 0.0
        u[1, b] = np.nan
        u.setflags(write=False)
        out.append(u)
    return tuple(out)


def rank_state(name, subgrid, u, part):
    """the columns of the single-rank state u that a rank's partition holds: owned cells, then ghosts"""
    S = part.cells_per_element
    gidx = np.concatenate([np.arange(part.first_global, part.first_global + part.N), part.ghost_global])
    cols = (gidx[:, None] * S + np.arange(S)[None, :]).reshape(-1)
    return u[:, cols]


def host_round(part, kinds, ua, ub, dt, t, parts=None, states=None):
    """one predict / correct round on the dict t (x, status, xs, k1, flag) with the states ua, ub (already in the solver's float
    type); returns (t after predict, t after correct, details). parts/states: several partitions whose k and held are summed."""
    def velocity(points, u, which):
        if parts is None:
            return tracers.host_velocity(part, u, points)
        k, held = 0.0, 0
        for p, us in zip(parts, states):
            kr, hr = tracers.host_velocity(p, us[which], points)
            with np.errstate(all="ignore"):
                k, held = k + kr, held + hr
        return k, held

    k, held = velocity(t["x"], ua, 0)
    xs, k1, flag, status = tracers.host_predict(t["x"], t["status"], t["xs"], t["k1"], t["flag"], k, held, dt, kinds)
    mid = dict(t, xs=xs, k1=k1, flag=flag, status=status)
    k2, held2 = velocity(xs, ub, 1)
    x, status2 = tracers.host_correct(t["x"], status, k1, flag, k2, held2, dt, kinds)
    end = dict(mid, x=x, status=status2)
    return mid, end, {"k": k, "held": held, "k2": k2, "held2": held2}


def initial(points):
    m, dim = points.shape
    return {"x": points.copy(), "status": np.zeros(m, np.uint8), "xs": points.copy(), "k1": np.zeros((m, dim)),
            "flag": np.zeros(m, np.uint8)}


@functools.lru_cache(maxsize=None)
def reference(name, subgrid, np_dtype):
    """[(after predict, after correct, details)] * ROUNDS of the host functions on the case's inputs"""
    part, kinds = partition(name, subgrid), kinds_of(name)
    u = [s.astype(np_dtype) for s in states_of(name, subgrid)]
    t = initial(points_of(name, subgrid)[0])
    rounds = []
    for r in range(ROUNDS):
        mid, end, det = host_round(part, kinds, u[r % 2], u[(r + 1) % 2], DT[name], t)
        rounds.append((mid, end, det))
        t = end
    return rounds


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return np.array_equal(a.view(np.int64), b.view(np.int64))
    return np.array_equal(a, b)
