#!/usr/bin/env python3
"""usage: scripts/farfield_cost.py [--rounds R] [--steps K] [--case c4]
Cost of far-field boundaries on plain meshes: the bench.py c4 mesh (fp64 KEPES, fused tier, native step driver) with x far field
and y periodic, against the same mesh with x outflow and y periodic. Runs alternate (outflow, far field, outflow, ...) R times;
prints the median ms/step of each and the generic tiles of each plan (one JSON line)."""
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
from t8gpu_amd.solver import PlainSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

CASES = {"c4": dict(base=7, lmax=12, band=0.1472), "c2": dict(base=8, lmax=10, band=0.1)}   # (c4: bench.py WORKLOADS)


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
    ap.add_argument("--case", default="c4", choices=sorted(CASES))
    a = ap.parse_args()
    w = CASES[a.case]
    far = np.array([[1.0, 0.0, 0.0, 0.0, 2.5 / 0.4]])   # the KH set-up's pressure, at rest
    sides = {"outflow": ("outflow", "outflow", "periodic", "periodic"),
             "farfield": (("farfield", 0), ("farfield", 0), "periodic", "periodic")}
    solvers, dt = {}, None
    for tag, sd in sides.items():
        m = SynthMesh(2, w["base"], w["lmax"], band=w["band"], sides=sd)
        solvers[tag] = PlainSolver(m.partition(), torch.float64, flux_kind=hip.KEPES, mode="fused",
                                   inflow_states=far if tag == "farfield" else None)
        solvers[tag].use_native_stepper()
        dt = 0.1 * 2.0 ** -m.finest_level
    times = {t: [] for t in solvers}
    for _ in range(a.rounds):
        for tag in ("outflow", "farfield"):
            times[tag].append(ms_per_step(solvers[tag], a.steps, dt))
    med = {t: statistics.median(v) for t, v in times.items()}
    h = {t: s.plan.host for t, s in solvers.items()}
    print(json.dumps({"case": a.case, "elements": solvers["outflow"].N, "ms_outflow": round(med["outflow"], 4),
                      "ms_farfield": round(med["farfield"], 4), "farfield_over_outflow": round(med["farfield"] / med["outflow"] - 1, 4),
                      "generic_tiles": {t: int(x.ntiles - x.n_patches) for t, x in h.items()},
                      "runs_ms": {t: [round(x, 4) for x in v] for t, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
