#!/usr/bin/env python3
"""usage: scripts/average_cost.py [--calls N]
Cost of averaging along homogeneous axes against what a user did before it existed, on the same mesh in the
same process: `fused` is solver.average_along(names, axes, L); `image` is resample_uniform(names, L, partial=True) followed by
torch.sum over the same axes and the divide. HIP events around single calls, median of N after a warm-up, with the spread
(min, max) beside every median:
  c4 (plain 2D, fp64, bench.py's mesh): density and five planes at L = 10 and L = 12, axes=(0,);
  c5u size (plain 3D uniform 128^3, fp64): density at L = 7, axes=(0, 2) (a profile: 128 bins) and axes=(2,) (a map).
Prints one JSON line per mesh."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from t8gpu_amd.solver import PlainSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

C4 = dict(dim=2, base=7, lmax=12, band=0.1472)          # (bench.py WORKLOADS)
C5U = dict(dim=3, base=7, lmax=7, band=0.0)
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


def image_average(g, names, axes, L):
    """the way without average_along: the whole image to memory, torch.sum along the array axes of `axes`, one divide"""
    sums, w = g.resample_uniform(names, L, partial=True)
    dims = tuple(-1 - a for a in axes)                   # mesh axis a is array axis dim - 1 - a: counted from the end
    w = w.sum(dim=dims)
    return {n: t.sum(dim=dims) / w for n, t in sums.items()}


def rows_of(g, cases, calls):
    out = {}
    for label, names, axes, L in cases:
        fused = g.average_along(names, axes, L)
        image = image_average(g, names, axes, L)
        first = names if isinstance(names, str) else names[0]
        scale = float(image[first].abs().max())
        out[label] = {"fused_ms": event_ms(lambda: g.average_along(names, axes, L), calls),
                      "image_ms": event_ms(lambda: image_average(g, names, axes, L), calls),
                      "max_difference_over_scale": float((fused[first] - image[first]).abs().max()) / scale}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    for case, cfg, cases in (("c4", C4, [("density_L10_x", "density", (0,), 10), ("five_L10_x", FIVE, (0,), 10),
                                         ("density_L12_x", "density", (0,), 12), ("five_L12_x", FIVE, (0,), 12)]),
                             ("c5u", C5U, [("density_L7_xz", "density", (0, 2), 7), ("density_L7_z", "density", (2,), 7)])):
        mesh = SynthMesh(cfg["dim"], cfg["base"], cfg["lmax"], band=cfg["band"])
        part = mesh.partition()
        g = PlainSolver(part, torch.float64, mode="fused")
        g.iterate(0.1 * 2.0 ** -mesh.finest_level)       # a state with motion in it
        torch.cuda.synchronize()
        row = {"case": case, "elements": part.N, "calls": a.calls}
        row.update(rows_of(g, cases, a.calls))
        print(json.dumps(row), flush=True)
        del g


if __name__ == "__main__":
    main()
