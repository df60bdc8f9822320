"""Hand-built boundary-face lists for the compat tier's boundary kernels (tests/test_gpu_compat_boundary.py): every boundary
face has a cell (Subgrid: a block) of its own and there are no interior faces, so on zeroed flux planes no two atomic adds
meet and every output is reproducible to the bit. run_cases() calls the C entry points directly and returns every case's
flux planes (and, plain, speed estimates) by name."""
import numpy as np
import torch

from t8gpu_amd import hip

GAMMA = 1.4
# K = 2 inflow / far-field states (rho, v, p): inflow kinds 2, 3 and far-field kinds 10, 11 name rows 0, 1
ROWS_PRIM = np.array([[1.0, 0.3, -0.2, 0.1, 1.0], [1.2, -0.4, 0.1, 0.05, 1.1]])
ALL_KINDS = (0, 1, 2, 3, 10, 11)
AXES = {2: [(1, 0), (-1, 0), (0, 1), (0, -1)], 3: [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]}


def conservative(rho, v, p):
    return np.concatenate([rho[:, None], rho[:, None] * v, (p / (GAMMA - 1) + 0.5 * rho * (v * v).sum(1))[:, None]], 1)


def inflow_states():
    return conservative(ROWS_PRIM[:, 0], ROWS_PRIM[:, 1:4], ROWS_PRIM[:, 4])


def physical_states(rng, n3, mach):
    """[m, 5] conservative states (fp64) whose velocity along the unit vectors n3[m, 3] is mach[m] sound speeds, with a
    tangential part of about 0.3 sound speeds"""
    m = len(mach)
    rho, p = rng.uniform(0.5, 2.0, m), rng.uniform(0.5, 2.0, m)
    c = np.sqrt(GAMMA * p / rho)
    w = rng.normal(size=(m, 3)) * 0.3 * c[:, None]
    w -= (w * n3).sum(1)[:, None] * n3
    return conservative(rho, (mach * c)[:, None] * n3 + w, p)


def pad3(n):
    return np.concatenate([n, np.zeros((n.shape[0], 3 - n.shape[1]))], 1)


class PlainList:
    """B = 13 boundary faces of 13 cells, F = 0: the axis normals of `ndim` dimensions, the rest oblique unit normals (3D: the
    face frame's degenerate direction (1, -1, 1) / sqrt 3 among them); normal Mach numbers -2.5 .. 2.5 in steps of 5/12"""
    B = 13

    def __init__(self, ndim, np_dtype):
        rng = np.random.default_rng(100 + ndim)
        B = self.B
        obl = rng.normal(size=(B - 2 * ndim, ndim))
        if ndim == 3:
            obl[0] = (1, -1, 1)
        obl /= np.sqrt((obl * obl).sum(1))[:, None]
        self.ndim, self.cells = ndim, B
        self.normals = np.concatenate([np.array(AXES[ndim], np.float64), obl]).astype(np_dtype)
        self.areas = rng.uniform(0.5, 2.0, B).astype(np_dtype)
        self.fn = np.arange(B, dtype=np.int32)
        self.n3 = pad3(self.normals.astype(np.float64))                       # (of the cell that owns each face)
        self.state = physical_states(rng, self.n3, rng.permutation(np.linspace(-2.5, 2.5, B))).astype(np_dtype)
        self.mixed = np.array(list(ALL_KINDS) + [10 + i % 2 for i in range(B - 6)], np.uint8)    # nine far-field faces


class SubgridList:
    """B block faces of B Subgrid blocks of rank `rank`, F = 0, the +- axis normals in turn (variant "b": starting from the
    last); every subcell a random state of its own with a normal Mach number in -2.5 .. 2.5 along its block's face normal"""

    def __init__(self, rank, B, variant, np_dtype):
        rng = np.random.default_rng(200 + 10 * rank + (variant == "b"))
        S, axes = 4 ** rank, AXES[rank]
        first = len(axes) - 1 if variant == "b" else 0
        self.rank, self.B, self.cells = rank, B, B * S
        self.normals = np.array([axes[(first + i) % len(axes)] for i in range(B)], np.float64).astype(np_dtype)
        self.areas = rng.uniform(0.5, 2.0, B).astype(np_dtype)
        self.fn = np.arange(B, dtype=np.int32)
        self.n3 = np.repeat(pad3(self.normals.astype(np.float64)), S, axis=0)
        self.state = physical_states(rng, self.n3, rng.uniform(-2.5, 2.5, B * S)).astype(np_dtype)
        if B >= 6:
            self.mixed = np.array([ALL_KINDS[i % 6] for i in range(B)], np.uint8)
            self.open = np.array([i % 4 for i in range(B)], np.uint8)
        else:       # five faces cannot hold six kinds: the two variants hold them between them
            self.mixed = np.array([0, 1, 2, 10, 11] if variant != "b" else [3, 10, 11, 1, 2], np.uint8)
            self.open = np.array([0, 1, 2, 3, 1] if variant != "b" else [3, 2, 1, 0, 2], np.uint8)


def far_as(kinds, what):
    """the kind list with every far-field face 10 + k turned into the inflow face 2 + k ("inflow") or an outflow face"""
    k = kinds.copy()
    far = k >= 10
    k[far] = k[far] - 8 if what == "inflow" else 1
    return k


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def inflow_table(dtype):
    states = dev(inflow_states()).to(dtype)
    table = torch.zeros((states.shape[0], 16), dtype=dtype, device="cuda")
    hip.call("t8gpu_hip_plain_inflow_table", dtype, hip.ptr(states), int(states.shape[0]), hip.ptr(table), hip.stream_ptr())
    torch.cuda.synchronize()
    return table


class Runner:
    """one face list on the device; run(entry, kinds) -> flux planes [5, cells] (plain: with the speeds, [B]) from zeroed planes"""

    def __init__(self, geo, dtype, flux_kind, table):
        self.geo, self.dtype, self.flux_kind, self.table = geo, dtype, flux_kind, table
        self.planes = torch.zeros((10, geo.cells), dtype=dtype, device="cuda")
        self.planes[0:5] = dev(geo.state.T)
        self.fn, self.normals, self.areas = dev(geo.fn), dev(geo.normals), dev(geo.areas)

    def run(self, entry, kinds=None):
        g, dtype = self.geo, self.dtype
        self.planes[5:10] = 0
        st, fl, s = hip.vars_of(self.planes, 0), hip.vars_of(self.planes, 1), hip.stream_ptr()
        kd = None if kinds is None else dev(kinds)
        geom = (hip.ptr(self.normals), hip.ptr(self.areas), st, fl)
        bc = () if entry.endswith("_boundary") else (hip.ptr(kd), hip.ptr(self.table))
        if isinstance(g, PlainList):
            speed = torch.zeros(g.B, dtype=dtype, device="cuda")
            hip.call(entry, dtype, self.flux_kind, 0, g.B, g.ndim, hip.ptr(self.fn), *bc, *geom, hip.ptr(speed), s)
        else:
            speed = None
            hip.call(entry, dtype, self.flux_kind, g.rank, 0, g.B, hip.ptr(self.fn), *bc, *geom, s)
        torch.cuda.synchronize()            # (kd lives until the kernel is done)
        flux = self.planes[5:10].clone()
        return flux if speed is None else (flux, speed)


def geometries(np_dtype):
    return {"plain2": PlainList(2, np_dtype), "plain3": PlainList(3, np_dtype), "subgrid3a": SubgridList(3, 5, "a", np_dtype),
            "subgrid3b": SubgridList(3, 5, "b", np_dtype), "subgrid2": SubgridList(2, 17, "", np_dtype)}


def run_cases(dtype, flux_kind, geos):
    """every case of every face list: {"<list>/<case>": tensors}. Plain values are (flux planes, speeds) pairs."""
    table = inflow_table(dtype)
    out = {}
    for name, g in geos.items():
        r = Runner(g, dtype, flux_kind, table)
        zeros = np.zeros(g.B, np.uint8)
        if isinstance(g, PlainList):
            walls, bc = "t8gpu_hip_flux_boundary", "t8gpu_hip_flux_boundary_bc"
            out[name + "/walls"] = r.run(walls)
            out[name + "/bc_zero"] = r.run(bc, zeros)
            out[name + "/bc_null"] = r.run(bc, None)
        else:
            walls, bc, far = "t8gpu_hip_subgrid_boundary", "t8gpu_hip_subgrid_boundary_bc", "t8gpu_hip_subgrid_boundary_far"
            out[name + "/walls"] = r.run(walls)
            out[name + "/bc_zero"] = r.run(bc, zeros)
            out[name + "/bc_null"] = r.run(bc, None)
            out[name + "/far_null"] = r.run(far, None)
            out[name + "/bc_open"] = r.run(bc, g.open)
            out[name + "/far_open"] = r.run(far, g.open)
            bc = far
        out[name + "/mixed"] = r.run(bc, g.mixed)
        out[name + "/far_as_inflow"] = r.run(bc, far_as(g.mixed, "inflow"))
        out[name + "/far_as_outflow"] = r.run(bc, far_as(g.mixed, "outflow"))
    return out
