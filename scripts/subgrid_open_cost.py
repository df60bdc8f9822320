#!/usr/bin/env python3
"""usage: scripts/subgrid_open_cost.py [--rounds R] [--steps K] [--cases c3,c3q] [--dtype f32|f64]
Cost of open boundaries on Subgrid meshes: the bench.py c3 / c3q meshes with x inflow / outflow and the other sides periodic,
against the same meshes fully periodic (the Subgrid kernels' MODE 1, kBndOpen, against MODE 0, kBndWalls), fused tier, KEPES. Runs alternate (periodic, open, periodic, ...) R times; prints per
case the median ms/step of each and the share of blocks that left the families (one JSON line per case)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from t8gpu_amd import hip  # noqa: E402
from t8gpu_amd.solver import SubgridSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

CASES = {"c3": dict(dim=3, base=5, lmax=6, band=0.17), "c3q": dict(dim=2, base=9, lmax=10, band=0.1)}   # (bench.py WORKLOADS)


def inflow_state(dim):
    rho, v, p = 1.0, (0.3, 0.0, 0.0), 1.0
    return np.array([[rho, rho * v[0], 0.0, 0.0, p / 0.4 + 0.5 * rho * v[0] ** 2]])


def ms_per_step(g, steps, dt):
    g.iterate_steps(2, dt)          # warm-up
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.iterate_steps(steps, dt)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cases", default="c3,c3q")
    ap.add_argument("--dtype", default="f32", choices=("f32", "f64"))
    a = ap.parse_args()
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    for name in a.cases.split(","):
        w = CASES[name]
        dim = w["dim"]
        rest = ("periodic",) * (2 * dim - 2)
        meshes = {"periodic": SynthMesh(dim, w["base"], w["lmax"], band=w["band"]),
                  "open": SynthMesh(dim, w["base"], w["lmax"], band=w["band"], sides=(0, "outflow") + rest)}
        solvers = {}
        for tag, m in meshes.items():
            part = m.partition(subgrid=True)
            solvers[tag] = SubgridSolver(part, dtype, flux_kind=hip.KEPES, mode="fused", open_boundaries=tag == "open",
                                         inflow_states=inflow_state(dim) if tag == "open" else None)
            solvers[tag].use_native_stepper()
        dt = 0.1 * 2.0 ** -(meshes["open"].finest_level + 2)
        times = {t: [] for t in solvers}
        for _ in range(a.rounds):
            for tag in ("periodic", "open"):
                times[tag].append(ms_per_step(solvers[tag], a.steps, dt))
        hp, ho = solvers["periodic"].plan.host, solvers["open"].plan.host
        nb = 1 << dim
        fam_p, fam_o = nb * hp.n_families, nb * ho.n_families
        med = {t: statistics.median(v) for t, v in times.items()}
        print(json.dumps({"case": name, "dtype": a.dtype, "blocks": hp.N, "ms_periodic": round(med["periodic"], 4),
                          "ms_open": round(med["open"], 4), "open_over_periodic": round(med["open"] / med["periodic"] - 1, 4),
                          "family_blocks_periodic": fam_p, "family_blocks_open": fam_o,
                          "left_families": round((fam_p - fam_o) / hp.N, 4),
                          "runs_ms": {t: [round(x, 4) for x in v] for t, v in times.items()}}), flush=True)
        del solvers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
