#!/usr/bin/env python3
"""usage: scripts/fields_cost.py [--calls N] [--case c4|c3|both]
Cost of the derived output fields on the bench.py meshes: c4 (plain, fp64) and c3 (Subgrid<4,4,4>, fp32).
Per mesh, in one process, HIP events around single calls, median of N after a warm-up:
  pointwise_ms        derived_fields(pressure, velocity, mach, entropy): no neighbour is read;
  all_fields_ms       derived_fields of all seven fields (eleven planes), the CSR cached;
  monitor_device_ms   one monitor_device() call, for comparison;
  stage_ms            one RK stage of the fused tier of the same build (a third of a step through the native driver).
Beside them csr_build_ms (host: t8gpu_host_cell_faces, without the upload) and the compulsory bytes from the shapes --
every array the pass touches counted once (the gathered neighbour values are re-reads of the state planes) -- with the
rate they give. Prints one JSON line per mesh."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from t8gpu_amd import fields  # noqa: E402
from t8gpu_amd.solver import PlainSolver, SubgridSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

CASES = {"c4": dict(kind="plain", dim=2, base=7, lmax=12, band=0.1472, dtype=torch.float64),     # (bench.py WORKLOADS)
         "c3": dict(kind="subgrid", dim=3, base=5, lmax=6, band=0.17, dtype=torch.float32)}
POINTWISE = ["pressure", "velocity", "mach", "entropy"]


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
        offsets, entries = fields.cell_faces(part.N, part.F, part.face_neighbors)
        csr_ms = 1e3 * (time.perf_counter() - t0)
        size = 4 if w["dtype"] == torch.float32 else 8
        cells, N, F = g.owned_cells, part.N, part.F
        ndim = part.mesh.dim if subgrid else part.normal_dim
        point_bytes = cells * (5 * size + 6 * 8)
        conn = 4 * (N + 1) + 4 * entries.size + 8 * F + (ndim + 1) * size * F + (4 * (1 + ndim) * F if subgrid else 0)
        all_bytes = cells * (5 * size + 11 * 8) + N * size + conn
        point, _ = event_ms(lambda: g.derived_fields(POINTWISE), a.calls)
        full, best = event_ms(lambda: g.derived_fields(list(fields.FIELDS)), a.calls)
        mon, _ = event_ms(g.monitor_device, a.calls)
        g.use_native_stepper()
        stage = event_ms(lambda: g.iterate_steps(4, dt), max(5, a.calls // 4))[0] / 12
        got = g.derived_fields(list(fields.FIELDS))
        finite = all(bool(torch.isfinite(t).all()) for t in got.values())
        row = {"case": name, "cells": cells, "elements": N, "faces": F, "csr_entries": int(entries.size),
               "dtype": "f32" if size == 4 else "f64", "csr_build_ms": round(csr_ms, 3),
               "pointwise_ms": round(point, 4), "pointwise_bytes": point_bytes,
               "pointwise_TB_per_s": round(point_bytes / (point * 1e-3) / 1e12, 3),
               "all_fields_ms": round(full, 4), "all_fields_min_ms": round(best, 4), "all_fields_bytes": all_bytes,
               "all_fields_TB_per_s": round(all_bytes / (full * 1e-3) / 1e12, 3),
               "monitor_device_ms": round(mon, 4), "stage_ms": round(stage, 4), "finite": finite}
        print(json.dumps(row), flush=True)
        del g


if __name__ == "__main__":
    main()
