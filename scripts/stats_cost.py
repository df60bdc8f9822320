#!/usr/bin/env python3
"""usage: scripts/stats_cost.py [--calls N] [--case c4|c3|both] [--stage]
Cost of one Statistics.accumulate() call on the bench.py meshes: c4 (plain, fp64) and c3 (Subgrid<4,4,4>,
fp32). Per mesh, HIP events around single calls, median of N after a warm-up, the two timed calls alternating:
  accumulate_ms   one accumulate() (one launch, no sync), and the bytes it moves / that time: per cell the five state values
                  read and the fifteen doubles read and written, (5 sizeof(T) + 240) B;
  copy_ms         the yardstick: a plain device-to-device copy that moves the same number of bytes (reads half of them,
                  writes the other half) in the same process; ratio = accumulate_ms / copy_ms;
  results_ms      one results() call for the names the Kelvin-Helmholtz example writes.
--stage also times one step of the fused tier on the same mesh through the native driver (what a call is "of the order of").
Prints one JSON line per mesh."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from t8gpu_amd.solver import PlainSolver, SubgridSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

CASES = {"c4": dict(kind="plain", dim=2, base=7, lmax=12, band=0.1472, dtype=torch.float64),     # (bench.py WORKLOADS)
         "c3": dict(kind="subgrid", dim=3, base=5, lmax=6, band=0.17, dtype=torch.float32)}
NAMES = ("mean_density", "mean_velocity", "tke", "pressure_rms")


def event_ms(fns, calls):
    """median and minimum (ms) of each of `fns`, one event pair per call, the functions taking turns"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(calls):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b))
    return [(statistics.median(t), min(t)) for t in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--case", default="both", choices=["c4", "c3", "both"])
    ap.add_argument("--stage", action="store_true")
    a = ap.parse_args()
    for name in (("c4", "c3") if a.case == "both" else (a.case,)):
        w = CASES[name]
        mesh = SynthMesh(w["dim"], w["base"], w["lmax"], band=w["band"])
        mode = "fused" if a.stage else "compat"
        if w["kind"] == "plain":
            g = PlainSolver(mesh.partition(), w["dtype"], mode=mode)
            dt = 0.1 * 2.0 ** -mesh.finest_level
        else:
            g = SubgridSolver(mesh.partition(subgrid=True), w["dtype"], mode=mode)
            dt = 0.1 * 2.0 ** -(mesh.finest_level + 2)
        g.iterate(dt)                                    # a state with motion in it
        torch.cuda.synchronize()
        size = 4 if w["dtype"] == torch.float32 else 8
        nbytes = (5 * size + 2 * 15 * 8) * g.owned_cells
        st = g.statistics()
        src = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        (acc, acc_min), (cp, cp_min) = event_ms([lambda: st.accumulate(dt), lambda: dst.copy_(src)], a.calls)
        (res, _), = event_ms([lambda: st.results(NAMES)], max(5, a.calls // 5))
        row = {"case": name, "cells": g.owned_cells, "dtype": "f32" if size == 4 else "f64", "stride": int(g.planes.shape[1]),
               "rows_16B_aligned": bool(st.sums.stride(0) % 2 == 0 and g.planes.shape[1] * size % 16 == 0),
               "bytes_moved": nbytes, "bytes_per_cell": nbytes // max(1, g.owned_cells), "accumulate_ms": round(acc, 4),
               "accumulate_min_ms": round(acc_min, 4), "TB_per_s": round(nbytes / (acc * 1e-3) / 1e12, 3),
               "copy_ms": round(cp, 4), "copy_min_ms": round(cp_min, 4), "copy_TB_per_s": round(nbytes / (cp * 1e-3) / 1e12, 3),
               "ratio": round(acc / cp, 3), "results_ms": round(res, 4),
               "finite": bool(torch.isfinite(st.sums).all())}
        if a.stage:
            g.use_native_stepper()
            row["step_ms"] = round(event_ms([lambda: g.iterate_steps(4, dt)], max(5, a.calls // 4))[0][0] / 4, 4)
        print(json.dumps(row), flush=True)
        del g, st, src, dst


if __name__ == "__main__":
    main()
