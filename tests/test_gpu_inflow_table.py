"""-m gpu: t8gpu_hip_plain_inflow_table_{f32,f64} (k_inflow_table) against a 160-bit reference of the same quantities.

A row is the state (words 0-4) and the nine-word KEPES cell record of flux_math.hpp: prim_from_state (words 5-13: rho, v, p,
beta = rho / 2p, ln rho, ln rho - ln p, v0 = (kappa - (ln p - kappa ln rho)) / (kappa - 1) - beta |v|^2), words 14-15 zero.
This pins prim_from_state, the body the stage kernels run per cell, in the instantiation the plain tile kernels use: in fp64
the table-driven logarithm (read here from global memory; the same values as the tiles' LDS copy), exercised at its 128
interval edges. prim_from_state_planar, the 2D patch kernels' form, is NOT reachable through this entry point and not covered.

Reference, per-word bounds (operation count times condition number, from the helper limits pinned in test_gpu_fastmath.py)
and the state families: tests/_scalar_ref.py (prim_reference, prim_bounds, inflow_state_families). 8 states per call, 25 calls
per family. Measured worst / bound per word is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import _scalar_ref as R
from _gpu import NP
from t8gpu_amd import hip
from test_gpu_fastmath import LOG, LOG_TAB, probe

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
WORDS = 16
SENTINEL = -777.25
INVALID = 1                                   # hipErrorInvalidValue
LD = np.longdouble


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def inflow_table(dtype, states, n, table, null_states=False, null_table=False):
    fn = getattr(hip.lib(), "t8gpu_hip_plain_inflow_table_" + hip.suffix(dtype))
    fn.restype = C.c_int
    rc = fn(None if null_states else hip.ptr(states), int(n), None if null_table else hip.ptr(table), hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


_rows = {}


def device_rows(dtype):
    """{family: (states, rows [200, 16])}, once per type: 25 calls of 8 states per family, each into a 10-row table pre-filled
    with a sentinel (rows 8 and 9 must stay)"""
    if dtype in _rows:
        return _rows[dtype]
    out = {}
    for name, states in R.inflow_state_families(NP[dtype]).items():
        rows = np.empty((len(states), WORDS), NP[dtype])
        for at in range(0, len(states), 8):
            d_s = torch.from_numpy(np.ascontiguousarray(states[at:at + 8])).cuda()
            d_t = torch.full((10, WORDS), SENTINEL, dtype=dtype, device="cuda")
            assert inflow_table(dtype, d_s, 8, d_t) == 0
            got = d_t.cpu().numpy()
            assert (got[8:] == SENTINEL).all()
            rows[at:at + 8] = got[:8]
        out[name] = (states, rows)
    _rows[dtype] = out
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_records_within_their_bounds(dtype):
    T = NP[dtype]
    for name, (states, rows) in device_rows(dtype).items():
        ref = R.prim_reference(states)
        bound = R.prim_bounds(ref, T)
        worst = {}
        for k, w in enumerate(R.PRIM_WORDS):
            err = np.abs(rows[:, 5 + k].astype(LD) - ref[w])
            err = np.where(np.isfinite(err), err, np.inf)
            if w == "rho":
                assert np.array_equal(bits(rows[:, 5]), bits(states[:, 0]))
                continue
            with np.errstate(invalid="ignore", divide="ignore"):       # (a zero velocity has bound 0: exact, or inf)
                worst[w] = float(np.where(err == 0, 0, err / bound[w]).max())
        print(f"inflow record {T.__name__} {name}: worst error / bound " + ", ".join(f"{w} {x:.3f}" for w, x in worst.items()))
        for w, x in worst.items():
            assert x <= 1.0, (name, w, x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_and_signs(dtype):
    """words 0-4 the state bit for bit, 14-15 +0; the velocities carry the signs of m / rho (rho > 0: those of the momenta,
    zeros included)"""
    for name, (states, rows) in device_rows(dtype).items():
        assert np.array_equal(bits(rows[:, 0:5]), bits(states)), name
        assert np.array_equal(bits(rows[:, 14:16]), bits(np.zeros((len(rows), 2), rows.dtype))), name
        assert np.array_equal(np.signbit(rows[:, 6:9]), np.signbit(states[:, 1:4])), name
        assert ((rows[:, 6:9] == 0) == (states[:, 1:4] == 0)).all(), name
    zeros = device_rows(dtype)["at rest"][0][:, 1:4]
    assert np.signbit(zeros[:, 2]).sum() == len(zeros) // 2 and len({tuple(r) for r in np.signbit(zeros)}) == 8


@pytest.mark.parametrize("dtype", DTYPES)
def test_logs_are_the_tile_kernels_own(dtype):
    """ln rho and ln p are the logarithms the plain tile kernels use for their cells, bit for bit: in fp64 the TABLE-driven one
    (the probe's LOG_TAB), not the polynomial t8_log_fast (LOG), which agrees with it only to an ulp; fp32 has one (LOG)"""
    T = NP[dtype]
    op = LOG_TAB if dtype == torch.float64 else LOG
    differ = 0
    for name, (states, rows) in device_rows(dtype).items():
        rho, p = np.ascontiguousarray(rows[:, 5]), np.ascontiguousarray(rows[:, 9])
        lrho, lp = probe(op, rho), probe(op, p)
        assert np.array_equal(bits(rows[:, 11]), bits(lrho)), name
        assert np.array_equal(bits(rows[:, 12]), bits((lrho - lp).astype(T))), name
        if dtype == torch.float64:
            differ += int((probe(LOG, rho) != lrho).sum())
    if dtype == torch.float64:
        assert differ > 0          # (else the comparison above could not tell the two logarithms apart)


@pytest.mark.parametrize("dtype", DTYPES)
def test_counts_and_argument_checks(dtype):
    T = NP[dtype]
    states = R.inflow_state_families(T)["Mach 0.1 - 20"]
    d_s = torch.from_numpy(np.ascontiguousarray(states[:9])).cuda()
    full = device_rows(dtype)["Mach 0.1 - 20"][1]
    for n in (0, 1, 8):
        d_t = torch.full((10, WORDS), SENTINEL, dtype=dtype, device="cuda")
        assert inflow_table(dtype, d_s, n, d_t) == 0
        got = d_t.cpu().numpy()
        assert np.array_equal(bits(got[:n]), bits(full[:n])) and (got[n:] == SENTINEL).all(), n
    d_t = torch.full((10, WORDS), SENTINEL, dtype=dtype, device="cuda")
    assert inflow_table(dtype, d_s, 9, d_t) == INVALID
    assert inflow_table(dtype, d_s, -1, d_t) == INVALID
    assert inflow_table(dtype, d_s, 4, d_t, null_states=True) == INVALID
    assert inflow_table(dtype, d_s, 4, d_t, null_table=True) == INVALID
    assert inflow_table(dtype, d_s, 0, d_t, null_states=True, null_table=True) == 0
    assert (d_t.cpu().numpy() == SENTINEL).all()
    assert np.array_equal(bits(d_s.cpu().numpy()), bits(states[:9]))
