"""Brute-force reference of the averaging tests (test_average_host.py, test_gpu_average.py): the sums and
weights of the slabs of a level along a set of averaged mesh axes, from the cell boxes of _sample_ref.cell_boxes alone. A cell
box overlaps a slab fully along an averaged axis, so per bin

    sum    = sum over the cells of (overlap lengths along the kept axes) * edge^|averaged| * q
    weight = the same without q.

It knows nothing of keys, searches, pixels along the averaged axes or summation orders."""
import itertools

import numpy as np

import _sample_ref as ref


def axis_sets(dim):
    """every admissible set of averaged axes: the non-empty proper subsets of the mesh axes, ascending"""
    return [s for k in range(1, dim) for s in itertools.combinations(range(dim), k)]


def average(part, values, axes, level, subgrid=None):
    """(sums[planes, bins...], weights[bins...]) of values[planes, cells] over the slabs of 2^level bins per kept axis, the
    highest kept axis first (3D: axes=(2,) gives [ny, nx], axes=(0, 2) gives [ny])"""
    lo, edge, _ = ref.cell_boxes(part, subgrid)
    dim, n = lo.shape[1], 1 << level
    axes = (axes,) if isinstance(axes, int) else tuple(axes)
    kept = [a for a in range(dim) if a not in axes]
    blo = np.arange(n) / n
    q = np.asarray(values, np.float64)
    w = edge ** len(axes)                                               # [cells]: the full extent along the averaged axes
    ov = []                                                             # per kept axis [bins, cells]: overlap length
    for a in kept:
        left = np.maximum(blo[:, None], lo[None, :, a])
        right = np.minimum(blo[:, None] + 1.0 / n, lo[None, :, a] + edge[None, :])
        ov.append(np.maximum(right - left, 0.0))
    if len(kept) == 1:
        return np.einsum("ac,c,pc->pa", ov[0], w, q), np.einsum("ac,c->a", ov[0], w)
    return np.einsum("bc,ac,c,pc->pba", ov[1], ov[0], w, q), np.einsum("bc,ac,c->ba", ov[1], ov[0], w)
