#!/usr/bin/env python3
"""usage: scripts/boundary_cost.py [--calls N] [--case c4|c3|both]
Cost of the boundary budgets against one RK stage of the same solver, on the bench.py meshes with open sides:
c4 (plain 2D, fp64; -x inflow, +x outflow, -y wall, +y far field) and c3 (Subgrid<4,4,4>, fp32; the same on x and z, y periodic).
Per mesh, HIP events around single calls, median of N after a warm-up:
  boundary_device_ms   one boundary_fluxes_device() call, grouped by kind (two launches, no copy, no sync);
  step_fluxes_ms       the three accumulating calls a step's budget takes (boundary.Budget.add_step);
  stage_ms             one RK stage of the fused tier (a twelfth of four steps through the native driver);
  boundary_ms          boundary_fluxes(): the same pass plus the pinned copy and the sync (host clock).
Prints one JSON line per mesh."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from monitor_cost import event_ms, host_ms  # noqa: E402
from t8gpu_amd import boundary  # noqa: E402
from t8gpu_amd.solver import PlainSolver, SubgridSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

CASES = {"c4": dict(kind="plain", dim=2, base=7, lmax=12, band=0.1472, dtype=torch.float64,          # (bench.py WORKLOADS)
                    sides=(0, "outflow", "wall", ("farfield", 0))),
         "c3": dict(kind="subgrid", dim=3, base=5, lmax=6, band=0.17, dtype=torch.float32,
                    sides=(0, "outflow", "periodic", "periodic", "wall", ("farfield", 0)))}
AMBIENT = np.array([[1.0, 0.1, 0.0, 0.0, 1.0 / 0.4 + 0.005]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--case", default="both", choices=["c4", "c3", "both"])
    a = ap.parse_args()
    for name in (("c4", "c3") if a.case == "both" else (a.case,)):
        w = CASES[name]
        mesh = SynthMesh(w["dim"], w["base"], w["lmax"], band=w["band"], sides=w["sides"])
        if w["kind"] == "plain":
            g = PlainSolver(mesh.partition(), w["dtype"], mode="fused", inflow_states=AMBIENT)
            dt = 0.1 * 2.0 ** -mesh.finest_level
        else:
            g = SubgridSolver(mesh.partition(subgrid=True), w["dtype"], mode="fused", open_boundaries=True, farfield=True,
                              inflow_states=AMBIENT)
            dt = 0.1 * 2.0 ** -(mesh.finest_level + 2)
        g.use_native_stepper()
        g.iterate(dt)
        torch.cuda.synchronize()
        budget = boundary.Budget(g)
        med, best = event_ms(g.boundary_fluxes_device, a.calls)
        step_ms = event_ms(lambda: budget.add_step(g, dt), a.calls)[0]
        stage_ms = event_ms(lambda: g.iterate_steps(4, dt), max(5, a.calls // 4))[0] / 12
        b = g.boundary_fluxes()
        row = {"case": name, "cells": g.owned_cells, "boundary_faces": int(g.B), "sub_faces": int(b.faces.sum()),
               "dtype": "f32" if w["dtype"] == torch.float32 else "f64", "boundary_device_ms": round(med, 4),
               "boundary_device_min_ms": round(best, 4), "step_fluxes_ms": round(step_ms, 4), "stage_ms": round(stage_ms, 4),
               "ratio_call_to_stage": round(med / stage_ms, 4), "boundary_ms": round(host_ms(g.boundary_fluxes, a.calls), 4),
               "nonfinite": int(b.nonfinite.sum())}
        print(json.dumps(row), flush=True)
        del g, budget


if __name__ == "__main__":
    main()
