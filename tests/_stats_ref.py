"""numpy reference of the time statistics (t8gpu_amd/stats.py, csrc/hip/stats.hip), in double, from the state
as uploaded (for fp32: the float32 values taken to double): the fifteen accumulated quantities, the results formulas, and
the transfer of the sums through an adapt -- child = parent, kept = copy, coarsened = plain mean of the family; for Subgrid
blocks the subcell rule of the block transfer. Needs no GPU."""
import numpy as np

PLANES = 15
# result name -> rows of the [19, cells] result block (the slot table of include/t8gpu_hip.h)
SLOTS = {"mean_density": [0], "mean_momentum": [1, 2, 3], "mean_energy": [4], "mean_pressure": [5], "mean_mach": [6],
         "mean_velocity": [7, 8, 9], "density_rms": [10], "pressure_rms": [11], "reynolds_stress": [12, 13, 14, 15, 16, 17],
         "tke": [18]}
RESULT_PLANES = 19
STRESS_PAIRS = ((1, 1), (2, 2), (3, 3), (1, 2), (1, 3), (2, 3))       # xx yy zz xy xz yz: the momentum slots of each


def uploaded(state, npdt):
    """the state as the device holds it, in double"""
    return np.asarray(state).astype(npdt).astype(np.float64)


def quantities(state):
    """[15, cells]: q_k of a double state [5, cells]"""
    rho, mx, my, mz, E = state
    m2 = mx * mx + my * my + mz * mz
    p = 0.4 * (E - 0.5 * m2 / rho)
    mach = (np.sqrt(m2) / rho) / np.sqrt(1.4 * p / rho)
    return np.stack([rho, mx, my, mz, E, p, rho * rho, p * p, mx * mx / rho, my * my / rho, mz * mz / rho, mx * my / rho,
                     mx * mz / rho, my * mz / rho, mach])


def accumulate(sums, state, weight):
    """sums + weight q(state): a new array"""
    return sums + weight * quantities(state)


def results(sums, W):
    """[19, cells]: every result plane of sums [15, cells] and the total weight W"""
    A = np.asarray(sums, np.float64)
    out = np.zeros((RESULT_PLANES, A.shape[1]))
    out[0] = A[0] / W
    out[1:4] = A[1:4] / W
    out[4] = A[4] / W
    out[5] = A[5] / W
    out[6] = A[14] / W
    out[7:10] = A[1:4] / A[0]
    out[10] = np.sqrt(np.maximum(0.0, A[6] / W - (A[0] / W) ** 2))
    out[11] = np.sqrt(np.maximum(0.0, A[7] / W - (A[5] / W) ** 2))
    for k, (i, j) in enumerate(STRESS_PAIRS):
        out[12 + k] = A[8 + k] / W - A[i] * A[j] / (A[0] * W)
    out[18] = 0.5 * (out[12] + out[13] + out[14]) / (A[0] / W)
    return out


def scales(sums, W):
    """[19]: what each result plane's error is measured against. The means: max |want| of the plane. The rms and stress planes
    are differences of two nearly equal terms of the size of the raw second moment: max A_k / W of that moment (k = 6, 7,
    8 + component). tke is half the trace of the stress over the mean density: the largest diagonal moment over the smallest
    mean density."""
    A = np.abs(np.asarray(sums, np.float64)) / W
    scale = np.abs(results(sums, W)).max(axis=1)
    scale[10], scale[11] = A[6].max(), A[7].max()
    scale[12:18] = A[8:14].max(axis=1)
    scale[18] = A[8:11].max() / A[0].min()
    return scale


def transfer(sums, adapt_data, cells_per_element=1, dim=2):
    """sums [P, n_old S] on the old mesh -> [P, n_new S] on the new one. adapt_data[n_new + 1]: new element e was made from
    the old elements [adapt_data[e], adapt_data[e + 1]); an empty range or the range of the element before: a child of the
    refined old element adapt_data[e], its position in the family counted from the first child; one old element: kept; 2^dim
    old elements: their coarsened parent.
    S = 1: child = parent, kept = copy, coarsened = the plain mean of the family. S = 4^dim (Subgrid blocks, subcell
    c = i + 4 j + 16 k): a child at family position (I, J, K) takes for its subcell (i, j, k) the parent's subcell
    (2 I + i // 2, 2 J + j // 2, 2 K + k // 2); a coarsened block takes for its subcell (i, j, k) the mean of the 2^dim subcells
    (2 (i % 2) + {0, 1}, ...) of the family member at position (i // 2, j // 2, k // 2)."""
    sums = np.asarray(sums, np.float64)
    ad = np.asarray(adapt_data, np.int64)
    S, n_new, P = cells_per_element, len(ad) - 1, sums.shape[0]
    assert S in (1, 4 ** dim)
    old = sums.reshape(P, -1, S)
    new = np.zeros((P, n_new, S))
    sub = np.arange(S)
    ijk = [(sub >> (2 * a)) & 3 if a < dim else np.zeros(S, np.int64) for a in range(3)]
    for e in range(n_new):
        first, diff = ad[e], ad[e + 1] - ad[e]
        refined = diff == 0 or (e > 0 and ad[e - 1] == first)
        if refined:
            child = 0
            while e - child - 1 >= 0 and ad[e - child - 1] == first:
                child += 1
            if S == 1:
                new[:, e, 0] = old[:, first, 0]
            else:
                pos = [(child >> a) & 1 for a in range(3)]
                src = sum((2 * pos[a] + ijk[a] // 2) << (2 * a) for a in range(dim))
                new[:, e, :] = old[:, first, src]
        elif diff > 1:
            assert diff == 2 ** dim
            if S == 1:
                new[:, e, 0] = old[:, first:first + diff, 0].sum(axis=1) / diff
            else:
                member = sum((ijk[a] // 2) << a for a in range(dim))
                acc = np.zeros((P, S))
                for t in range(2 ** dim):
                    fine = sum((2 * (ijk[a] % 2) + ((t >> a) & 1)) << (2 * a) for a in range(dim))
                    acc += old[:, first + member, fine]
                new[:, e, :] = acc / 2 ** dim
        else:
            new[:, e, :] = old[:, first, :]
    return new.reshape(P, n_new * S)


def cases_of(adapt_data):
    """(children, kept, coarsened): how many new elements of each kind adapt_data describes"""
    ad = np.asarray(adapt_data, np.int64)
    diff = np.diff(ad)
    refined = (diff == 0) | np.concatenate([[False], ad[:-2] == ad[1:-1]])
    return int(refined.sum()), int(((diff == 1) & ~refined).sum()), int((diff > 1).sum())
