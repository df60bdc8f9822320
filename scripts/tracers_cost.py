#!/usr/bin/env python3
"""usage: scripts/tracers_cost.py [--calls N] [--lattice N]
Cost of the tracer pass on the c4 mesh of bench.py (plain, fp64) for an N x N lattice of particles (default
1000: 1 M). In one process, HIP events around single calls, median of --calls after a warm-up with the spread (min, max)
beside every median; the three particle measurements are taken in one order and then in the reverse order (`forward`,
`backward`), so that a drift of the clocks or of the particles shows as a difference between the two:
  warm_ms       tr.predict(dt) + tr.correct(dt), hints as the last call left them (the fused kernel, two launches);
  cold_ms       the same with both hint arrays dropped (-1) before every pair: every particle searches;
  unfused_ms    the same points pushed twice through sample_points(x, ["momentum", "density"]): the composition the tree had
                before the tracer kernels (locate + gather, four launches, two allocations), without the arithmetic;
  step_ms       one iterate step through the native driver of the same build.
The flow does not advance between the particle calls (the state is the one after the first step): the particles drift with
a frozen field, dt being that of the flow step. Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from t8gpu_amd import tracers  # noqa: E402
from t8gpu_amd.solver import PlainSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

C4 = dict(dim=2, base=7, lmax=12, band=0.1472)          # (bench.py WORKLOADS)


def event_ms(fn, calls, before=None):
    """[median, min, max] of `calls` single calls after three warm-up calls; `before` runs ahead of every call, untimed"""
    for _ in range(3):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        if before:
            before()
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
    ap.add_argument("--lattice", type=int, default=1000)
    a = ap.parse_args()
    mesh = SynthMesh(C4["dim"], C4["base"], C4["lmax"], band=C4["band"])
    part = mesh.partition()
    g = PlainSolver(part, torch.float64, mode="fused")
    dt = 0.1 * 2.0 ** -mesh.finest_level
    g.iterate(dt)                                        # a state with motion in it
    tr = g.tracers(tracers.lattice(2, a.lattice))
    torch.cuda.synchronize()

    def pair():
        tr.predict(dt)
        tr.correct(dt)

    def drop():
        tr.hint_x.fill_(-1)
        tr.hint_xs.fill_(-1)

    def unfused():
        g.sample_points(tr.x, ["momentum", "density"])
        g.sample_points(tr.xs, ["momentum", "density"])

    runs = {"warm_ms": lambda: event_ms(pair, a.calls), "cold_ms": lambda: event_ms(pair, a.calls, drop),
            "unfused_ms": lambda: event_ms(unfused, a.calls)}
    row = {"case": "c4", "elements": part.N, "particles": tr.M, "calls": a.calls}
    row["forward"] = {name: runs[name]() for name in runs}
    row["backward"] = {name: runs[name]() for name in reversed(list(runs))}
    g.use_native_stepper()
    step = event_ms(lambda: g.iterate_steps(4, dt), max(5, a.calls // 4))
    row["step_ms"] = [round(x / 4, 4) for x in step]
    row["counts"] = tr.counts()
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
