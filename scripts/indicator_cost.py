#!/usr/bin/env python3
"""usage: scripts/indicator_cost.py [--calls N] [--case c4|c3|both]
Cost of the scale-free refinement indicator on the bench.py meshes: c4 (plain, fp64) and c3 (Subgrid<4,4,4>,
fp32), beside the reference criterion it stands in for. Per mesh, in one process, HIP events around single calls, median of N
after a warm-up:
  reference_ms        amr.refinement_criteria / amr.subgrid_refinement_criteria (the kernels of an adapt cycle of today);
  density_ms          Loehner(("density",)).criteria: one plane per neighbour;
  all_four_ms         Loehner of density, pressure, mach and entropy: five planes per neighbour;
  density_buffer1_ms  density with one buffer layer (one t8gpu_hip_indicator_spread pass more);
  all_four_buffer1_ms the four quantities with one buffer layer;
and the ratios to reference_ms. The CSR of fields._csr is built before the timed calls (csr_build_ms: the host part, once per
solver). Prints one JSON line per mesh."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from t8gpu_amd import amr, fields  # noqa: E402
from t8gpu_amd.solver import PlainSolver, SubgridSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

CASES = {"c4": dict(kind="plain", dim=2, base=7, lmax=12, band=0.1472, dtype=torch.float64),     # (bench.py WORKLOADS)
         "c3": dict(kind="subgrid", dim=3, base=5, lmax=6, band=0.17, dtype=torch.float32)}
ALL = ("density", "pressure", "mach", "entropy")


def event_ms(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--case", default="both", choices=["c4", "c3", "both"])
    a = ap.parse_args()
    for name in (("c4", "c3") if a.case == "both" else (a.case,)):
        w = CASES[name]
        mesh = SynthMesh(w["dim"], w["base"], w["lmax"], band=w["band"])
        subgrid = w["kind"] == "subgrid"
        part = mesh.partition(subgrid=subgrid)
        g = (SubgridSolver if subgrid else PlainSolver)(part, w["dtype"], mode="fused")
        dt = 0.1 * 2.0 ** -(mesh.finest_level + (2 if subgrid else 0))
        g.iterate(dt)                                    # a state with motion in it
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fields._csr(g)
        torch.cuda.synchronize()
        csr_ms = 1e3 * (time.perf_counter() - t0)
        reference = amr.subgrid_refinement_criteria if subgrid else amr.refinement_criteria
        row = {"case": name, "cells": g.owned_cells, "elements": part.N, "faces": part.F,
               "dtype": "f32" if w["dtype"] == torch.float32 else "f64", "csr_build_and_upload_ms": round(csr_ms, 3),
               "reference_ms": round(event_ms(lambda: reference(g), a.calls), 4)}
        for key, ind in (("density", amr.Loehner(("density",))), ("all_four", amr.Loehner(ALL)),
                         ("density_buffer1", amr.Loehner(("density",), buffer=1)), ("all_four_buffer1", amr.Loehner(ALL, buffer=1))):
            ms = event_ms(lambda: ind.criteria(g), a.calls)
            row[key + "_ms"] = round(ms, 4)
            row[key + "_over_reference"] = round(ms / row["reference_ms"], 2)
        crit = amr.Loehner(ALL, buffer=1).criteria(g)
        row["finite"] = bool(torch.isfinite(crit).all())
        row["max"] = round(float(crit.max()), 6)
        row["share_above_0.8"] = round(float((crit > 0.8).double().mean()), 4)
        print(json.dumps(row), flush=True)
        del g


if __name__ == "__main__":
    main()
