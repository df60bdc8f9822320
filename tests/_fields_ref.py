"""numpy reference of the derived output fields (include/t8gpu_hip.h: the slot table of t8gpu_hip_*_fields_*), for the tests.

The gradient fields are formed by FACE SCATTER: every interior face (sub-face) adds its term to the two cells it separates
with np.add.at -- the other way round from the kernels, which gather per cell through the CSR. For Subgrid blocks the
forward sub-face -> cell map of the compat kernels (sg_face_cells) is restated here. The term of a face is the same for both
of its cells: with n outward from l, l gets A n (q_r - q_l) and r gets A (-n) (q_l - q_r)."""
import numpy as np

PLANES = 11
SLOTS = {"pressure": [0], "velocity": [1, 2, 3], "mach": [4], "entropy": [5], "vorticity": [6, 7, 8], "dilatation": [9],
         "schlieren": [10]}
GRADIENT_PLANES = (6, 7, 8, 9, 10)


def rounded(a, npdt):
    """what the device holds of a host array uploaded in float type npdt, taken to double"""
    return np.asarray(a).astype(npdt).astype(np.float64)


def pointwise(u):
    """planes 0-5 [6, cells] of the state u [5, cells] (float64)"""
    rho, mx, my, mz, E = u
    with np.errstate(all="ignore"):
        vel = np.stack([mx, my, mz]) / rho
        p = 0.4 * (E - 0.5 * (mx * mx + my * my + mz * mz) / rho)
        mach = np.sqrt((vel ** 2).sum(0)) / np.sqrt(1.4 * p / rho)
        ent = np.log(p) - 1.4 * np.log(rho)
    return np.stack([p, vel[0], vel[1], vel[2], mach, ent])


def _normals3(normals, ndim, F):
    n = np.zeros((F, 3))
    n[:, :ndim] = np.asarray(normals).reshape(-1, ndim)[:F]
    return n


def _scatter(acc, a, b, area, n, rho, vel):
    """adds the term of the faces a | b (cell indices, n outward from a) to acc [7, cells] at both cells"""
    du = vel[:, b] - vel[:, a]                                     # [3, faces]
    drho = rho[b] - rho[a]
    nt = n.T                                                       # [3, faces]
    terms = np.concatenate([area * np.cross(nt, du, axis=0), (area * (nt * du).sum(0))[None], area * nt * drho])
    for k in range(7):
        np.add.at(acc[k], a, terms[k])
        np.add.at(acc[k], b, terms[k])


def _finish(acc, inv2v, owned):
    out = acc[:, :owned] * inv2v
    return np.concatenate([out[0:4], np.sqrt((out[4:7] ** 2).sum(0))[None]])       # curl x y z, div, |grad rho|


def plain_fields(u, part, npdt):
    """[11, N] of a plain partition: u [5, N + G] as uploaded (ghosts current)"""
    u = rounded(u, npdt)
    N, F, ndim = part.N, part.F, part.normal_dim
    fn = np.asarray(part.face_neighbors)
    l, r = fn[0:2 * F:2], fn[1:2 * F:2]
    n = _normals3(rounded(part.normals, npdt), ndim, F)
    area = rounded(part.areas, npdt)[:F]
    acc = np.zeros((7, u.shape[1]))
    _scatter(acc, l, r, area, n, u[0], u[1:4] / u[0])
    return np.concatenate([pointwise(u[:, :N]), _finish(acc, 0.5 / rounded(part.volumes, npdt)[:N], N)])


def sg_face_cells(n, off, hanging, rank):
    """(lflat, rflat) [F, SF] of the sub-faces t = i + 4 j of the faces with normals n [F, 3], anchors off [F, 3] and
    hanging [F] (level difference != 0: ds = 1, else 2) -- kernels_compat.hip: sg_face_cells, for all faces at once"""
    F, SF = n.shape[0], 4 ** (rank - 1)
    axis = np.argmax(np.abs(n), axis=1)
    assert np.all(np.abs(n[np.arange(F), axis]) == 1.0)
    al = np.zeros((F, 3), np.int64)
    al[np.arange(F), axis] = np.where(n[np.arange(F), axis] == 1.0, 3, 0)
    si, sj = np.zeros((F, 3), np.int64), np.zeros((F, 3), np.int64)
    t1 = np.where(axis == 0, 1, 0)
    t2 = np.where(axis == 2, 1, 2)
    si[np.arange(F), t1] = 1
    if rank == 3:
        sj[np.arange(F), t2] = 1
    t = np.arange(SF)
    i, j = (t % 4)[None, :, None], (t // 4)[None, :, None]
    step = i * si[:, None, :] + j * sj[:, None, :]                                  # [F, SF, 3]
    ds = np.where(hanging, 1, 2)[:, None, None]
    lc = al[:, None, :] + step
    rc = off[:, None, :] + ds * step // 2
    w = np.array([1, 4, 16])
    return (lc * w).sum(-1), (rc * w).sum(-1)


def subgrid_fields(u, part, npdt):
    """[11, N S] of a Subgrid partition: u [5, (N + G) S] as uploaded, storage order c = i + 4 j + 16 k"""
    u = rounded(u, npdt)
    rank = part.mesh.dim
    S, SF, N, F = 4 ** rank, 4 ** (rank - 1), part.N, part.F
    rho, vel = u[0], u[1:4] / u[0]
    vol = rounded(part.volumes, npdt)
    acc = np.zeros((7, u.shape[1]))
    # faces inside the owned blocks: area h^(rank - 1), h = vol^(1 / rank) / 4
    h = vol[:N] ** (1.0 / rank) / 4
    c = np.arange(S)
    for d in range(rank):
        low = c[(c >> (2 * d)) & 3 < 3]
        a = (np.arange(N)[:, None] * S + low[None, :]).reshape(-1)
        n = np.zeros((a.size, 3))
        n[:, d] = 1.0
        _scatter(acc, a, a + 4 ** d, np.repeat(h ** (rank - 1), low.size), n, rho, vel)
    # outer faces: SF sub-faces each, area / SF
    fn = np.asarray(part.face_neighbors)
    l, r = fn[0:2 * F:2].astype(np.int64), fn[1:2 * F:2].astype(np.int64)
    n = _normals3(rounded(part.normals, npdt), rank, F)
    off = np.zeros((F, 3), np.int64)
    off[:, :rank] = np.asarray(part.nb_offset).reshape(F, rank)
    lflat, rflat = sg_face_cells(n, off, np.asarray(part.level_diff) != 0, rank)
    a, b = (l[:, None] * S + lflat).reshape(-1), (r[:, None] * S + rflat).reshape(-1)
    _scatter(acc, a, b, np.repeat(rounded(part.areas, npdt)[:F] / SF, SF), np.repeat(n, SF, axis=0), rho, vel)
    return np.concatenate([pointwise(u[:, :N * S]), _finish(acc, np.repeat(0.5 * S / vol[:N], S), N * S)])


def reference(u, part, npdt):
    return subgrid_fields(u, part, npdt) if part.subgrid else plain_fields(u, part, npdt)
