#!/usr/bin/env python3
"""usage: scripts/subgrid_farfield_cost.py [--rounds R] [--steps K] [--cases c3,c3q] [--dtype f32|f64]
Cost of far-field sides on Subgrid meshes: the bench.py c3 / c3q meshes with x far field and the other sides periodic, against
the same meshes with x inflow / outflow (the Subgrid kernels' MODE 1, kBndOpen), fused tier + native driver, KEPES. The two plans
hold the same blocks in the same families; they differ in the MODE the launcher picks (2, kBndFar, against 1). Runs alternate (open, far,
open, ...) R times; prints per case the median ms/step of each with every run (one JSON line per case)."""
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


def states():
    rho, v, p = 1.0, (0.3, 0.0, 0.0), 1.0
    row = [rho, rho * v[0], 0.0, 0.0, p / 0.4 + 0.5 * rho * v[0] ** 2]
    return np.array([row, row])


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
    name_of = hip.lib().t8gpu_hip_last_stage_kernel
    name_of.restype = __import__("ctypes").c_char_p
    for name in a.cases.split(","):
        w = CASES[name]
        dim = w["dim"]
        rest = ("periodic",) * (2 * dim - 2)
        sides = {"open": (0, "outflow") + rest, "far": (("farfield", 0), ("farfield", 1)) + rest}
        solvers, kernels = {}, {}
        for tag, sd in sides.items():
            part = SynthMesh(dim, w["base"], w["lmax"], band=w["band"], sides=sd).partition(subgrid=True)
            solvers[tag] = SubgridSolver(part, dtype, flux_kind=hip.KEPES, mode="fused", open_boundaries=True, farfield=tag == "far",
                                         inflow_states=states())
            solvers[tag].iterate(1e-6)                       # (python stages once: the launcher's note names the kernel)
            kernels[tag] = name_of().decode()
            solvers[tag].use_native_stepper()
        dt = 0.1 * 2.0 ** -(w["lmax"] + 2)
        times = {t: [] for t in solvers}
        for _ in range(a.rounds):
            for tag in ("open", "far"):
                times[tag].append(ms_per_step(solvers[tag], a.steps, dt))
        ho, hf = solvers["open"].plan.host, solvers["far"].plan.host
        nb = 1 << dim
        med = {t: statistics.median(v) for t, v in times.items()}
        spread = {t: round((max(v) - min(v)) / statistics.median(v), 4) for t, v in times.items()}
        print(json.dumps({"case": name, "dtype": a.dtype, "blocks": ho.N, "ms_open": round(med["open"], 4), "ms_far": round(med["far"], 4),
                          "far_over_open": round(med["far"] / med["open"] - 1, 4), "spread": spread,
                          "family_blocks": [nb * ho.n_families, nb * hf.n_families], "rest_blocks": [ho.n_rest, hf.n_rest],
                          "kernels": kernels, "runs_ms": {t: [round(x, 4) for x in v] for t, v in times.items()}}), flush=True)
        del solvers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
