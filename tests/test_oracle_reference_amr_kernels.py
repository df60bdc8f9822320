"""The oracle's AMR transfer and indicator functions against executions of the reference's own kernel bodies.

tests/golden/reference_amr_vectors.npz (+ _rank3; tests/golden/make_reference_amr_vectors.py, build container only) holds inputs
and outputs of adapt_variables_and_volume (t8gpu/mesh/mesh_manager.inl:164-193), adapt_volume / adapt_variables for Subgrid<4,4>
and Subgrid<4,4,4> (subgrid_mesh_manager.inl:245-425), compute_refinement_criteria<Subgrid> (examples/subgrid/kernels.inl:
1109-1168), estimate_gradient (examples/compressible_euler/kernels.cu:471-501) and compute_refinement_criteria (solver.cu:
231-241), run on the host through the reference's own accessor classes on real forests: a mixed refine / coarsen pattern, a
coarsened family at element 0 with two refined parents at the end, a new mesh of one element, a refined family at element 0.
Here the oracle's entry points (oracle/oracle_capi.cpp) run on the same inputs.

What this closes: which octant a child takes from its position in the family, the z-order of a coarsened family's members, the
hard-coded 3D volume factors were pinned by reading alone, in the oracle and in the kernels alike. Tolerance:
NONE. Copies, sums in a fixed order, one division; the fixture's estimate_gradient adds in face order, as the oracle does; the
plain criteria are one division by a cbrt of the same libm, and the CPU run gives bit equality there too. Every array of every
case agrees BIT FOR BIT in fp32 and fp64. The stand-ins the generator needs keep parity "unpinned" (DESIGN.md section 2)."""
import ctypes as C

import numpy as np
import pytest

import _amr_vectors as AV
import _oracle as O


def same(a, b, what):
    scale = max(float(np.abs(b).max()), 1e-300)
    assert np.array_equal(a, b), (what, "max rel. difference", float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / scale))


def plain_transfer(ins, dim):
    n_old, n_new, _, _, _ = AV.sizes(ins)
    dt_ = ins["state"].dtype
    got, vol = np.full((5, n_new), -1, dt_), np.full(n_new, -1, dt_)
    getattr(O.lib(), "oracle_adapt_variables_and_volume_" + O.suf(dt_))(
        n_new, dim, O.p(ins["adapt_data"]), O.p(ins["state"]), C.c_size_t(n_old), O.p(got), C.c_size_t(n_new), O.p(ins["volume"]), O.p(vol))
    return got, vol


def roles(adapt_data):
    """per new element: +1 a child of a refined element, -1 a coarsened family, 0 kept"""
    ad = np.asarray(adapt_data)
    step = np.diff(ad)
    child = (step == 0) | np.concatenate([[False], ad[1:-1] == ad[:-2]])
    return np.where(child, 1, np.where(step > 1, -1, 0))


@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", AV.case_names())
def test_plain_transfer_against_the_executed_reference_kernel(case, tag):
    """dim = 3 on the 2D forests too: the reference hard-codes 0.125 / 8.0 (Q5)"""
    ins, outs = AV.load(case, tag)
    n_old, n_new, _, _, _ = AV.sizes(ins)
    got, vol = plain_transfer(ins, 3)
    same(got, outs["variables"].reshape(5, n_new), (case, "variables"))
    same(vol, outs["volumes"], (case, "volumes"))


@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", [c for c in AV.case_names() if c.endswith("2d")])
def test_quirk_q5_dim_2_changes_the_volumes_only(case, tag):
    """The documented deviation: with dim = 2 on a 2D forest the variables are the reference's, the volumes are the stored ones
    times 2 (children: 1/4 for the reference's 1/8), 1 (kept) and 0.5 (coarsened: 4 for 8) -- and THEY sum to the domain's
    volume, which the reference's do not."""
    ins, outs = AV.load(case, tag)
    n_old, n_new, _, _, _ = AV.sizes(ins)
    got, vol = plain_transfer(ins, 2)
    same(got, outs["variables"].reshape(5, n_new), (case, "variables"))
    role = roles(ins["adapt_data"])
    factor = np.where(role == 1, 2.0, np.where(role == -1, 0.5, 1.0)).astype(vol.dtype)
    same(vol, outs["volumes"] * factor, (case, "volumes"))
    domain = float(ins["volume"].astype(np.float64).sum())
    assert domain == 1.0 and float(vol.astype(np.float64).sum()) == domain          # (powers of two: exact)
    if (role != 0).any():
        assert float(outs["volumes"].astype(np.float64).sum()) != domain


@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", AV.subgrid_cases())
def test_subgrid_transfer_and_criteria_against_the_executed_reference_kernels(case, tag):
    ins, outs = AV.load(case, tag)
    n_old, n_new, _, _, rank = AV.sizes(ins)
    S = 4 ** rank
    dt_ = ins["sub_state"].dtype
    sf = O.suf(dt_)
    got, vol = np.full((5, n_new * S), -1, dt_), np.full(n_new, -1, dt_)
    getattr(O.lib(), "oracle_subgrid_adapt_variables_and_volume_" + sf)(
        rank, n_new, O.p(ins["adapt_data"]), O.p(ins["sub_state"]), C.c_size_t(n_old * S), O.p(got), C.c_size_t(n_new * S),
        O.p(ins["volume"]), O.p(vol))
    same(got, outs["sub_variables"].reshape(5, n_new * S), (case, "Subgrid variables"))
    same(vol, outs["sub_volumes"], (case, "Subgrid volumes"))
    # adapt_volume<Subgrid> has the factors of its rank (subgrid_mesh_manager.inl:260 / 289): the new volumes tile the domain
    assert float(vol.astype(np.float64).sum()) == float(ins["volume"].astype(np.float64).sum()) == 1.0
    crit = np.full(n_old, -1, dt_)
    rho = np.ascontiguousarray(ins["sub_state"][0])
    getattr(O.lib(), "oracle_subgrid_refinement_criteria_" + sf)(rank, n_old, O.p(rho), O.p(ins["volume"]), O.p(crit))
    same(crit, outs["sub_criteria"], (case, "Subgrid criteria"))


@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", AV.case_names())
def test_indicator_against_the_executed_reference_kernels(case, tag):
    """estimate_gradient with and without an (identity) element -> slot map, then gradient / cbrt(volume): bit equality, the
    cbrt being the same libm's on both sides."""
    ins, outs = AV.load(case, tag)
    n_old, _, F, _, _ = AV.sizes(ins)
    dt_ = ins["state"].dtype
    sf = O.suf(dt_)
    rho = np.ascontiguousarray(ins["state"][0])
    for idx in (None, np.arange(n_old, dtype=np.int32)):
        grad = np.zeros(n_old, dt_)
        getattr(O.lib(), "oracle_estimate_gradient_" + sf)(F, O.p(ins["fn"]), O.p(idx), O.p(rho), O.p(grad))
        same(grad, outs["gradient"], (case, "gradient", "identity map" if idx is not None else "no map"))
    crit = np.full(n_old, -1, dt_)
    getattr(O.lib(), "oracle_refinement_criteria_" + sf)(n_old, O.p(outs["gradient"]), O.p(ins["volume"]), O.p(crit))
    same(crit, outs["criteria"], (case, "criteria"))


def test_z_order_is_a_permutation_of_every_block():
    """What the fixture's column_major_to_z_order wrote (subgrid_mesh_manager.inl:1007-1049): every block keeps its own values,
    cell 0 stays, cell (1, 0) goes to 1, (0, 1) to 2 and (0, 0, 1) to 4 (the reference's bit order: x lowest), and the
    second-level bits follow the first-level ones."""
    for case in AV.subgrid_cases():
        for tag in AV.TAGS:
            ins, outs = AV.load(case, tag)
            n_old, _, _, _, rank = AV.sizes(ins)
            S = 4 ** rank
            rho = ins["sub_state"][0].reshape(n_old, S)
            z = outs["sub_zorder"].reshape(n_old, S)
            assert np.array_equal(np.sort(z, axis=1), np.sort(rho, axis=1))
            cell = lambda i, j, k=0: i + 4 * j + 16 * k
            assert np.array_equal(z[:, 0], rho[:, 0]) and np.array_equal(z[:, 1], rho[:, cell(1, 0)]) and np.array_equal(z[:, 2], rho[:, cell(0, 1)])
            assert np.array_equal(z[:, 1 << rank], rho[:, cell(2, 0)]) and np.array_equal(z[:, S - 1], rho[:, S - 1])
            if rank == 3:
                assert np.array_equal(z[:, 4], rho[:, cell(0, 0, 1)])


def test_fixture_is_what_it_says():
    z = AV.vectors()
    assert len(z["meta"]) == 2 and all("executed on the host through the reference's own accessor classes" in m for m in z["meta"])
    assert AV.case_names() == sorted(AV.CENSUS)
    subgrid = {}
    for case in AV.case_names():
        n_old, n_new, census = AV.CENSUS[case]
        for tag, dt_ in (("f64", np.float64), ("f32", np.float32)):
            ins, outs = AV.load(case, tag)
            assert AV.sizes(ins)[:2] == (n_old, n_new) and AV.sizes(ins)[3] == int(case[-2])
            ad = ins["adapt_data"]
            assert ad.size == n_new + 1 and ad[0] == 0 and ad[-1] == n_old and (np.diff(ad) >= 0).all()
            step = np.diff(ad)
            assert {int(k): int((step == k).sum()) for k in np.unique(step)} == census
            rank = AV.sizes(ins)[4]
            subgrid[case] = rank
            S = 4 ** rank
            want = {"variables": 5 * n_new, "volumes": n_new, "gradient": n_old, "criteria": n_old}
            if rank:
                want.update({"sub_variables": 5 * n_new * S, "sub_volumes": n_new, "sub_criteria": n_old, "sub_zorder": n_old * S})
                assert ins["sub_state"].shape == (5, n_old * S) and ins["sub_state"].dtype == dt_
            assert ins["state"].shape == (5, n_old)
            assert {k: v.size for k, v in outs.items()} == want
            for v in list(outs.values()) + [ins["state"], ins["volume"]]:
                assert v.dtype == dt_ and np.isfinite(v).all()
            assert outs["gradient"].min() > 0 and outs["criteria"].min() > 0
            for R in AV.PART_RANKS:
                runs, have, noff = ins[f"part{R}_runs"], ins[f"part{R}_have_off"], ins[f"part{R}_new_off"]
                assert have.size == noff.size == R + 1 and have[-1] == noff[-1] == n_new and int(runs[:, 4].sum()) == n_new
                g = have[ins[f"part{R}_ranks"]] + ins[f"part{R}_indices"]
                assert np.array_equal(g, np.arange(n_new))
                if n_new > R:
                    assert (runs[:, 0] != runs[:, 2]).any()                    # some run changes its owner
    assert subgrid == {"mixed2d": 2, "mixed3d": 0, "ends2d": 2, "ends3d": 3, "one2d": 2, "one3d": 3, "refined_ends2d": 0, "refined_ends3d": 0}
    # what the cases are there to reach
    for dim in (2, 3):
        ad = AV.load(f"ends{dim}d", "f64")[0]["adapt_data"]
        assert ad[1] - ad[0] == 2 ** dim                                          # a coarsened family at e = 0
        assert (ad[-2 * 2 ** dim - 1:-1] == np.repeat([ad[-1] - 2, ad[-1] - 1], 2 ** dim)).all()   # two refined parents, the last child last
        assert list(AV.load(f"one{dim}d", "f64")[0]["adapt_data"]) == [0, 2 ** dim]
        assert list(AV.load(f"refined_ends{dim}d", "f64")[0]["adapt_data"][:2 ** dim + 1]) == [0] * 2 ** dim + [1]
