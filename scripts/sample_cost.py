#!/usr/bin/env python3
"""usage: scripts/sample_cost.py [--calls N]
Cost of sampling on the c4 mesh of bench.py (plain, fp64). In one process, HIP events around single calls,
median of N after a warm-up, with the spread (min, max) beside every median:
  key_build_ms        host: morton_keys(part), numpy, without the upload (best of 3, wall clock);
  sampler_ms          Sampler(solver): the key build plus the upload of keys and levels (wall clock, synchronised);
  grid_1024_1_ms      sample_grid("density", (1024, 1024));
  grid_1024_5_ms      sample_grid(density, momentum, energy): five planes;
  uniform_lm2_ms      resample_uniform("density", max_level - 2);
  uniform_l_ms        resample_uniform("density", max_level);
  points_64_ms        sample_points of 64 points (a device tensor), density;
  pressure_ms         one derived_fields("pressure") pass, for comparison;
  step_ms             one iterate step through the native driver of the same build.
Compare key_build_ms with the adapt cycle scripts/amr_cycle_cost.py reports. Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from t8gpu_amd import sample  # noqa: E402
from t8gpu_amd.solver import PlainSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

C4 = dict(dim=2, base=7, lmax=12, band=0.1472)          # (bench.py WORKLOADS)
FIVE = ["density", "momentum", "energy"]


def event_ms(fn, calls):
    """[median, min, max] of `calls` single calls after three warm-up calls"""
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
    return [round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    mesh = SynthMesh(C4["dim"], C4["base"], C4["lmax"], band=C4["band"])
    part = mesh.partition()
    g = PlainSolver(part, torch.float64, mode="fused")
    dt = 0.1 * 2.0 ** -mesh.finest_level
    g.iterate(dt)                                        # a state with motion in it
    torch.cuda.synchronize()
    builds = []
    for _ in range(3):
        t0 = time.perf_counter()
        keys = sample.morton_keys(part)
        builds.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    s = sample.sampler(g)
    torch.cuda.synchronize()
    sampler_ms = 1e3 * (time.perf_counter() - t0)
    L = mesh.finest_level
    pts = torch.rand((64, 2), dtype=torch.float64, device="cuda")
    row = {"case": "c4", "elements": part.N, "levels": [int(part.levels[:part.N].min()), L], "calls": a.calls,
           "key_build_ms": round(min(builds), 3), "key_bytes": int(keys.nbytes), "sampler_ms": round(sampler_ms, 3),
           "grid_1024_1_ms": event_ms(lambda: g.sample_grid("density", (1024, 1024)), a.calls),
           "grid_1024_5_ms": event_ms(lambda: g.sample_grid(FIVE, (1024, 1024)), a.calls),
           "uniform_lm2_ms": event_ms(lambda: g.resample_uniform("density", L - 2), a.calls),
           "uniform_l_ms": event_ms(lambda: g.resample_uniform("density", L), a.calls),
           "points_64_ms": event_ms(lambda: g.sample_points(pts, "density"), a.calls),
           "pressure_ms": event_ms(lambda: g.derived_fields("pressure"), a.calls)}
    g.use_native_stepper()
    step = event_ms(lambda: g.iterate_steps(4, dt), max(5, a.calls // 4))
    row["step_ms"] = [round(x / 4, 4) for x in step]
    image = g.sample_grid("density", (1024, 1024), cells=True)
    row["finite"] = bool(torch.isfinite(image["density"]).all()) and bool((image["cell"] >= 0).all()) and s is sample.sampler(g)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
