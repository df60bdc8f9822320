"""numpy reference of the scale-free refinement indicator (include/t8gpu_hip.h: t8gpu_hip_*_indicator_*), for
the tests.

Formed by FACE SCATTER, as _fields_ref forms the gradient fields: every interior face (sub-face) adds its terms to the two
cells it separates with np.add.at -- the other way round from the kernels, which gather per cell through the CSR -- with the
forward sub-face map of the compat kernels (sg_face_cells). It starts from the arrays as uploaded, taken to double.

For the faces a | b (n outward from a), d = (h_a + h_b) / 2, w = A |n| per axis:
    a:  N += w (q_b - q_a) / d    D += w (|q_b - q_a| + eps (|q_a| + |q_b|)) / d    b += A n     W += w
    b:  N += w (q_a - q_b) / d    D += the same                                      b -= A n     W += w
    k = W > 0 ? max(0, 1 - |b| / W) : 0;   E_q = |k N| / |D| (0 where |D| = 0);   E = max over the quantities."""
import numpy as np

from _fields_ref import _normals3, pointwise, rounded, sg_face_cells

QUANTITIES = ("density", "pressure", "mach", "entropy")
_POINTWISE_ROW = {"pressure": 0, "mach": 4, "entropy": 5}


def quantity(u, name):
    """q [cells] of the state u [5, cells] (float64)"""
    return u[0] if name == "density" else pointwise(u)[_POINTWISE_ROW[name]]


def root(v, dim):
    return np.sqrt(v) if dim == 2 else np.cbrt(v)


class _Acc:
    def __init__(self, cells, nq):
        self.N, self.D = np.zeros((nq, 3, cells)), np.zeros((nq, 3, cells))
        self.b, self.W = np.zeros((3, cells)), np.zeros((3, cells))

    def scatter(self, a, b, area, n, h, qs, eps):
        """the faces a | b (cell indices, n [faces, 3] outward from a, h [cells])"""
        d = 0.5 * (h[a] + h[b])
        for ax in range(3):
            w = area * np.abs(n[:, ax])
            np.add.at(self.b[ax], a, area * n[:, ax])
            np.add.at(self.b[ax], b, -area * n[:, ax])
            np.add.at(self.W[ax], a, w)
            np.add.at(self.W[ax], b, w)
            for k, q in enumerate(qs):
                dq = q[b] - q[a]
                den = w * (np.abs(dq) + eps * (np.abs(q[a]) + np.abs(q[b]))) / d
                np.add.at(self.N[k, ax], a, w * dq / d)
                np.add.at(self.N[k, ax], b, w * -dq / d)
                np.add.at(self.D[k, ax], a, den)
                np.add.at(self.D[k, ax], b, den)

    def value(self, owned):
        with np.errstate(all="ignore"):
            k = np.where(self.W > 0, np.maximum(0.0, 1.0 - np.abs(self.b) / self.W), 0.0)
            num = np.sqrt(((k[None] * self.N) ** 2).sum(1))
            den = np.sqrt((self.D ** 2).sum(1))
            E = np.where(den > 0, num / den, 0.0)
        return E.max(0)[:owned]


def plain_indicator(u, part, npdt, names, eps):
    """[N] of a plain partition: u [5, N + G] as uploaded (ghosts current)"""
    u = rounded(u, npdt)
    N, F, ndim = part.N, part.F, part.normal_dim
    fn = np.asarray(part.face_neighbors)
    l, r = fn[0:2 * F:2], fn[1:2 * F:2]
    n = _normals3(rounded(part.normals, npdt), ndim, F)
    area = rounded(part.areas, npdt)[:F]
    h = root(rounded(part.volumes, npdt), part.mesh.dim)
    acc = _Acc(u.shape[1], len(names))
    acc.scatter(l, r, area, n, h, [quantity(u, name) for name in names], eps)
    return acc.value(N)


def subgrid_indicator(u, part, npdt, names, eps):
    """[N S] of a Subgrid partition: u [5, (N + G) S] as uploaded, storage order c = i + 4 j + 16 k"""
    u = rounded(u, npdt)
    rank = part.mesh.dim
    S, SF, N, F = 4 ** rank, 4 ** (rank - 1), part.N, part.F
    vol = rounded(part.volumes, npdt)
    hb = root(vol, rank) / 4                                   # per block, owned and ghost
    h = np.repeat(hb, S)
    qs = [quantity(u, name) for name in names]
    acc = _Acc(u.shape[1], len(names))
    c = np.arange(S)
    for d in range(rank):                                      # faces inside the owned blocks: area h^(rank - 1)
        low = c[(c >> (2 * d)) & 3 < 3]
        a = (np.arange(N)[:, None] * S + low[None, :]).reshape(-1)
        n = np.zeros((a.size, 3))
        n[:, d] = 1.0
        acc.scatter(a, a + 4 ** d, np.repeat(hb[:N] ** (rank - 1), low.size), n, h, qs, eps)
    fn = np.asarray(part.face_neighbors)                       # outer faces: SF sub-faces each, area / SF
    l, r = fn[0:2 * F:2].astype(np.int64), fn[1:2 * F:2].astype(np.int64)
    n = _normals3(rounded(part.normals, npdt), rank, F)
    off = np.zeros((F, 3), np.int64)
    off[:, :rank] = np.asarray(part.nb_offset).reshape(F, rank)
    lflat, rflat = sg_face_cells(n, off, np.asarray(part.level_diff) != 0, rank)
    a, b = (l[:, None] * S + lflat).reshape(-1), (r[:, None] * S + rflat).reshape(-1)
    # a sub-face is a subcell face of the finer of the two blocks: its area from that block's volume, as inside the blocks (on
    # dyadic geometry the bits of areas / SF; lengths from ONE source keep E scale-free where areas and volumes round apart)
    acc.scatter(a, b, np.repeat(np.minimum(hb[l], hb[r]) ** (rank - 1), SF), np.repeat(n, SF, axis=0), h, qs, eps)
    return acc.value(N * S)


def reference(u, part, npdt, names=("density",), eps=0.01):
    """per-cell E of the owned cells"""
    names = [names] if isinstance(names, str) else list(names)
    return (subgrid_indicator if part.subgrid else plain_indicator)(u, part, npdt, names, eps)


def block_max(values, part):
    """one value per element / block: the maximum over a block's subcells"""
    return values.reshape(part.N, -1).max(1)


def spread(values, part):
    """one buffer layer on the values [N + G] (ghost entries read): [N]"""
    F = part.F
    fn = np.asarray(part.face_neighbors)
    l, r = fn[0:2 * F:2], fn[1:2 * F:2]
    out = values.copy()
    np.maximum.at(out, l, values[r])
    np.maximum.at(out, r, values[l])
    return out[: part.N]


def step_closed_form(q_own, q_other, eps, tangential_faces):
    """E of the cell with value q_own beside a step to q_other on a uniform Cartesian mesh, every other neighbour at q_own,
    straight from the definition: along the step normal N = D w / d and D_n = (D + eps (|q_other| + |q_own|) + 2 eps |q_own|)
    w / d with D = |q_other - q_own|; each tangential axis a with m_a interior faces has N_a = 0, D_a = m_a 2 eps |q_own| w / d.
    tangential_faces = (m_a, ...) per tangential axis: 2 away from the walls tangent to the step normal, 1 at such a wall.
    In 2D away from those walls this is D / sqrt((D + eps (|qR| + 3 |qL|))^2 + (4 eps |qL|)^2). In 3D the two tangential axes
    add (4 eps |qL|)^2 EACH, since E_q sums D_a^2 per axis: 2 (4 eps |qL|)^2, not the (8 eps |qL|)^2 that lumping the four
    tangential faces into one term would give."""
    D = abs(q_other - q_own)
    dn = D + eps * (abs(q_other) + 3 * abs(q_own))
    return D / np.sqrt(dn ** 2 + sum((m * 2 * eps * abs(q_own)) ** 2 for m in tangential_faces))


# ---- meshes and states shared by the host and the GPU tests ------------------------------------------------------------------
def refined(dim, level, periodic, lo, hi):
    """a uniform mesh with the elements whose centres lie in the box (lo, hi)^dim, and element 0, refined once (the "refined"
    meshes of test_gpu_fields.py: 2:1 faces of both orientations on every axis, 115 / 127 elements)"""
    from t8gpu_amd.synth import SynthMesh
    mesh = SynthMesh(dim, level, level, periodic=periodic)
    part = mesh.partition()
    c = part.centres[: part.N, :dim]
    marks = np.all((c > lo) & (c < hi), axis=1).astype(np.int8)
    marks[0] = 1
    return mesh.adapt(marks)[0]


REFINED = {
    "refined-2d-periodic": lambda: refined(2, 3, True, 0.3, 0.8),
    "refined-2d-walls": lambda: refined(2, 3, False, 0.3, 0.8),
    "refined-3d-periodic": lambda: refined(3, 2, True, 0.2, 0.8),
    "refined-3d-walls": lambda: refined(3, 2, False, 0.2, 0.8),
}


def uniform_walled(dim):
    """the uniform walled meshes of the closed-form tests: 2D level 3, 3D level 2 (x = 0.5 is a block edge of both)"""
    from t8gpu_amd.synth import SynthMesh
    return SynthMesh(2, 3, 3, periodic=False) if dim == 2 else SynthMesh(3, 2, 2, periodic=False)


def cell_centres(part):
    """centres and edge lengths of the cells (subcells of Subgrid blocks, storage order), owned and ghost"""
    dim, tot = part.mesh.dim, part.N + part.G
    edge = 0.5 ** part.levels[:tot].astype(np.float64)
    if not part.subgrid:
        return part.centres[:tot].copy(), edge
    S = 4 ** dim
    c = np.arange(S)
    rel = np.stack([(((c >> (2 * a)) & 3) + 0.5) / 4 - 0.5 if a < dim else np.zeros(S) for a in range(3)], axis=1)   # [S, 3]
    x = part.centres[:tot, None, :] + rel[None, :, :] * edge[:, None, None]
    return x.reshape(-1, 3), np.repeat(edge / 4, S)


Q_LEFT, Q_RIGHT = 1.0, 0.25


def step_state(part, q_left=Q_LEFT, q_right=Q_RIGHT):
    """a density step q_left | q_right at x = 0.5, zero velocity, constant pressure 1"""
    x, _ = cell_centres(part)
    rho = np.where(x[:, 0] < 0.5, q_left, q_right)
    zero = np.zeros_like(rho)
    return np.stack([rho, zero, zero, zero, np.full_like(rho, 2.5)])


def step_expected(part, eps, q_left=Q_LEFT, q_right=Q_RIGHT):
    """E of every owned cell for step_state on a uniform walled mesh, from step_closed_form: the two columns of cells beside
    x = 0.5 (a tangential axis has one interior face at a wall, else two), exactly 0 elsewhere"""
    dim = part.mesh.dim
    x, edge = cell_centres(part)
    cells = part.N * part.cells_per_element
    x, edge = x[:cells], edge[:cells]
    want = np.zeros(cells)
    for i in range(cells):
        if abs(x[i, 0] - 0.5) < edge[i]:
            own, other = (q_left, q_right) if x[i, 0] < 0.5 else (q_right, q_left)
            m = [1 if (x[i, a] < edge[i] or x[i, a] > 1 - edge[i]) else 2 for a in range(1, dim)]
            want[i] = step_closed_form(own, other, eps, m)
    return want
