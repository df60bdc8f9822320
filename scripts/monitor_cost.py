#!/usr/bin/env python3
"""usage: scripts/monitor_cost.py [--calls N] [--case c4|c3|both] [--stage]
Cost of the state monitor on the bench.py meshes: c4 (plain, fp64) and c3 (Subgrid<4,4,4>, fp32).
Per mesh, HIP events around single calls, median of N after a warm-up:
  monitor_device_ms   one monitor_device() call (two launches, no copy, no sync), and the bytes it reads / that time;
  replaced_ms         what it stands in for, host-synchronised: on the plain mesh five compute_integral calls plus
                      max_speed; on the Subgrid mesh the host read-back of the state the examples reduced in numpy;
  monitor_ms          monitor(): the same pass plus the 128-byte copy and the sync (host clock).
--stage also times one RK stage of the fused tier on the same mesh (a third of a step through the native driver).
Prints one JSON line per mesh."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from t8gpu_amd.solver import PlainSolver, SubgridSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

CASES = {"c4": dict(kind="plain", dim=2, base=7, lmax=12, band=0.1472, dtype=torch.float64),     # (bench.py WORKLOADS)
         "c3": dict(kind="subgrid", dim=3, base=5, lmax=6, band=0.17, dtype=torch.float32)}


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
    return statistics.median(out), min(out)


def host_ms(fn, calls):
    for _ in range(3):
        fn()
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
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
            volumes = g.N

            def replaced():
                for k in range(5):
                    g.compute_integral(k)
                g.max_speed()
        else:
            g = SubgridSolver(mesh.partition(subgrid=True), w["dtype"], mode=mode)
            dt = 0.1 * 2.0 ** -(mesh.finest_level + 2)
            volumes = g.N

            def replaced():
                g.state().double().cpu().numpy()
        g.iterate(dt)                                    # a state with motion in it, and face speeds for max_speed
        torch.cuda.synchronize()
        size = 4 if w["dtype"] == torch.float32 else 8
        nbytes = (5 * g.owned_cells + volumes) * size
        med, best = event_ms(g.monitor_device, a.calls)
        m = g.monitor()
        row = {"case": name, "cells": g.owned_cells, "dtype": "f32" if size == 4 else "f64", "stride": int(g.planes.shape[1]),
               "bytes_read": nbytes, "monitor_device_ms": round(med, 4), "monitor_device_min_ms": round(best, 4),
               "TB_per_s": round(nbytes / (med * 1e-3) / 1e12, 3), "replaced_ms": round(host_ms(replaced, a.calls), 4),
               "monitor_ms": round(host_ms(g.monitor, a.calls), 4), "nonfinite": m.nonfinite, "unphysical": m.unphysical,
               "max_rate": m.max_rate}
        if a.stage:
            g.use_native_stepper()
            row["stage_ms"] = round(event_ms(lambda: g.iterate_steps(4, dt), max(5, a.calls // 4))[0] / 12, 4)
        print(json.dumps(row), flush=True)
        del g


if __name__ == "__main__":
    main()
