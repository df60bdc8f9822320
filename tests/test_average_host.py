"""sample.host_average, the numpy definition of average_along, without a GPU: against the brute force of
_average_ref.py on every mesh of _sample_ref.py, the exact weights of a full domain, the order of summation on hand-built
arrays, and the refusals.

Tolerance. host_average adds, per bin, the pixel values of _sample_ref.resample in a tree of depth 64 + 6 + chunks; the brute
force adds overlap * edge^|A| * q over the cells of the slab (at most a few thousand non-zero terms) in storage order. Both
are within a few thousand ulp of max |q| in the worst case, so the bound of test_gpu_sample.py for resample_uniform against
its brute force, 1e-12 of max |q| per plane on the mean, holds with the same margin; its constant is stated again here
because importing that module needs a GPU build of torch."""
import functools

import numpy as np
import pytest

import _average_ref as aref
import _sample_ref as ref
from t8gpu_amd import sample

TOL = 1e-12                                                     # test_gpu_sample.TOL
MESHES = list(ref.MESHES)
B = 2.0 ** 60


def cell_values(part):
    """[2, cells]: two smooth-plus-random planes of order one, one of them of both signs"""
    lo, edge, _ = ref.cell_boxes(part)
    rng = np.random.default_rng(3)
    x = lo + 0.5 * edge[:, None]
    a = 1.0 + 0.5 * np.sin(2 * np.pi * x[:, 1]) + 0.05 * rng.standard_normal(x.shape[0])
    b = np.cos(2 * np.pi * x[:, 0]) * a + 0.2 * rng.standard_normal(x.shape[0])
    return np.stack([a, b])


@functools.lru_cache(maxsize=None)
def image(mesh, subgrid, level):
    part = ref.partition(mesh, subgrid)
    return ref.resample(part, cell_values(part), level)


def top_level(part):
    return int(ref.cell_boxes(part)[2].max()) + 1


@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_host_average_against_the_brute_force_and_exact_weights(mesh, subgrid):
    part = ref.partition(mesh, subgrid)
    dim = part.mesh.dim
    q = cell_values(part)
    scale = np.abs(q).max(axis=1)
    for L in range(top_level(part) + 1):
        sums, weights = image(mesh, subgrid, L)
        for axes in aref.axis_sets(dim):
            kept = dim - len(axes)
            s, w = sample.host_average(sums, weights, axes, L, partial=True)
            assert s.shape == (2,) + (1 << L,) * kept and w.shape == (1 << L,) * kept
            assert np.all(w == 0.5 ** (L * kept)), (L, axes)                  # sums of powers of two: exact
            bs, bw = aref.average(part, q, axes, L)
            assert np.all(bw == w), (L, axes)
            mean = sample.host_average(sums, weights, axes, L)
            assert np.array_equal(mean, s / w)
            err = np.abs(mean - bs / bw).reshape(2, -1).max(axis=1)
            assert np.all(err <= TOL * scale), (L, axes, err / scale)
    one = sample.host_average(*image(mesh, subgrid, 1), 0, 1)                 # an int for one axis
    assert np.array_equal(one, sample.host_average(*image(mesh, subgrid, 1), (0,), 1))


def test_zero_weight_gives_fill():
    sums, weights = np.ones((1, 4, 4)), np.ones((4, 4))
    weights[2, :], sums[0, 2, :] = 0.0, 0.0
    got = sample.host_average(sums, weights, (0,), 2, fill=-7.25)
    assert got.shape == (1, 4) and got[0].tolist() == [1.0, 1.0, -7.25, 1.0]
    assert np.isnan(sample.host_average(sums, weights, (0,), 2)[0, 2])


def place(row, chunk, t, lane, value):
    r = sample.AVERAGE_CHUNK * chunk + 64 * t + lane
    assert row[r] == 0.0
    row[r] = value


def test_summation_order_on_hand_built_rows_2d():
    """[1, n, n] with n = 128 and axes=(0,): a row is a bin, R = 128, one chunk, lane j adds x[j] then x[64 + j].
    Row 0: the 51 distinct powers of two 2^0 .. 2^50 spread over the row, plus +2^60 and -2^60 in the SAME lane at t = 0
    and t = 1. They cancel exactly inside that lane before it meets any other, so the row's sum is 2^51 - 1 exactly; summed in
    ascending r, or lane by lane after the butterfly, 2^60 would swallow the low bits.
    Row 1: +2^60 in lane 3, -2^60 in lane 35 = 3 ^ 32, 1.0 in lane 2. The butterfly starts with s = 32, where the pair cancels;
    the 1.0 arrives at s = 1: the sum is 1.0. A butterfly starting at s = 1 adds 2^60 + 1.0 = 2^60 first and gives 0.0.
    Row 2: all -0.0: every lane starts from +0.0, and +0.0 + -0.0 = +0.0."""
    n = 128
    x = np.zeros((1, n, n))
    place(x[0, 0], 0, 0, 5, B)
    place(x[0, 0], 0, 1, 5, -B)
    free = [r for r in range(n) if r not in (5, 69)]
    for i in range(51):
        x[0, 0, free[(37 * i) % len(free)]] += 2.0 ** i
    assert np.count_nonzero(x[0, 0]) == 53
    place(x[0, 1], 0, 0, 3, B)
    place(x[0, 1], 0, 0, 35, -B)
    place(x[0, 1], 0, 0, 2, 1.0)
    x[0, 2] = -0.0
    s, w = sample.host_average(x, np.ones((n, n)), (0,), 7, partial=True)
    assert s[0, 0] == 2.0 ** 51 - 1 and s[0, 1] == 1.0 and np.all(s[0, 3:] == 0.0)
    assert s[0, 2] == 0.0 and not np.signbit(s[0, 2])
    assert np.all(w == 128.0)
    assert np.cumsum(x[0, 0])[-1] != 2.0 ** 51 - 1 and np.cumsum(x[0, 1])[-1] == 0.0      # ascending r: other bits
    # the other axis: the same rows as columns, r runs along y
    t, _ = sample.host_average(np.ascontiguousarray(x.transpose(0, 2, 1)), np.ones((n, n)), (1,), 7, partial=True)
    assert np.array_equal(t.view(np.int64), s.view(np.int64))


def test_summation_order_of_rounds_and_chunks_3d():
    """[1, n, n, n] with n = 128 and axes=(0, 1): bin = z, r = x + 128 y, R = 16384 = 4 chunks.
    Bin 0, the rounds of one lane: lane 7 of chunk 0 meets +2^60, 1.0, -2^60, 1.0 at t = 0, 1, 2, 3. Ascending t:
    ((2^60 + 1) - 2^60) + 1 = 1.0; descending t or pairs give 0.0 or 2.0.
    Bin 1, the chunks: chunk values +2^60, 1.0, -2^60, 1.0. Ascending c from +0.0: 1.0; descending or a tree: 0.0.
    Bin 2, r = x + 128 y with x fastest: -2^60 at (x, y) = (5, 33) is r = 4229, chunk 1, t = 2, lane 5. That lane holds +2^60 at
    t = 1 and 1.0 at t = 3: the sum is 1.0. Read as r = 33 + 128 * 5 the pair would meet only across chunks, after 2^60 + 1.0."""
    n = 128
    x = np.zeros((1, n, n, n))
    rows = x.reshape(1, n, n * n)                                   # [1, z, r]: y slower than x
    for t, v in enumerate((B, 1.0, -B, 1.0)):
        place(rows[0, 0], 0, t, 7, v)
    for c, v in enumerate((B, 1.0, -B, 1.0)):
        place(rows[0, 1], c, 11 * c, 63 - c, v)
    place(rows[0, 2], 1, 1, 5, B)
    x[0, 2, 33, 5] = -B
    place(rows[0, 2], 1, 3, 5, 1.0)
    assert rows[0, 2, 4229] == -B
    s, w = sample.host_average(x, np.full((n, n, n), 0.5 ** 21), (0, 1), 7, partial=True)
    assert s.shape == (1, n) and s[0, :3].tolist() == [1.0, 1.0, 1.0] and np.all(s[0, 3:] == 0.0)
    assert np.all(w == 0.5 ** 7)                                    # 2^14 times 2^-21, exact


@pytest.mark.parametrize("dim", [2, 3])
def test_refusals(dim):
    n = 4
    sums, weights = np.zeros((1,) + (n,) * dim), np.ones((n,) * dim)
    for bad in ((), tuple(range(dim)), (0, 0), (dim,), (-1,), dim, 0.5, "x"):
        with pytest.raises(ValueError):
            sample.host_average(sums, weights, bad, 2)
    with pytest.raises(ValueError):
        sample.host_average(sums, weights, (0,), 3)                 # not an image of that level
    assert sample.check_axes(1, dim) == (1,) and sample.check_axes((1, 0), 3) == (0, 1)
