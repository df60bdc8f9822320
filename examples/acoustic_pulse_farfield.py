#!/usr/bin/env python3
"""Adaptive 2D acoustic pulse on [0, 1]^2 with far-field boundaries on all four sides (one MI355X): the structure of
riemann2d_amr.py on a mesh whose sides hold the ambient state through the characteristic far-field condition
(SynthMesh(..., sides=(("farfield", 0),) * 4)).

Initial state: the ambient state (rho = 1, at rest, p = 1) with a Gaussian pressure pulse (amplitude 0.1, width 0.05) at
the centre, isentropic in density. The ring it sends out leaves through the sides; what it leaves behind is the residual
max |p - p_inf| printed at the end -- a reflective wall, or a prescribed-state inflow of the ambient state, leaves more.

    python examples/acoustic_pulse_farfield.py --t-end 1.0 --min-level 5 --max-level 8 --out out/pulse
    python examples/acoustic_pulse_farfield.py --sides inflow      # the same with a prescribed-state inflow of the ambient state
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from t8gpu_amd import amr, boundary, hip, vtk  # noqa: E402
from t8gpu_amd.solver import PlainSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

GAMMA = 1.4
AMBIENT = (1.0, 1.0)   # rho, p
SIDES = {"farfield": ("farfield", 0), "inflow": 0, "outflow": "outflow", "wall": "wall"}
PROBES = ((0.5, 0.5), (0.75, 0.5), (0.9, 0.9))   # --probes: the pulse's centre, half way to a side, near a corner
FLUXES = {"kepes": hip.KEPES, "hll": hip.HLL, "hllc": hip.HLLC}


def ambient_state():
    rho, p = AMBIENT
    return np.array([[rho, 0.0, 0.0, 0.0, p / (GAMMA - 1)]])


def initial_state(part, amplitude=0.1, width=0.05):
    x, y = part.centres[:, 0], part.centres[:, 1]
    r2 = (x - 0.5) ** 2 + (y - 0.5) ** 2
    p = AMBIENT[1] * (1 + amplitude * np.exp(-r2 / (width * width)))
    rho = AMBIENT[0] * (p / AMBIENT[1]) ** (1 / GAMMA)
    return np.stack([rho, 0 * rho, 0 * rho, 0 * rho, p / (GAMMA - 1)])


def pressure(solver):
    u = solver.state().double().cpu().numpy()
    return (GAMMA - 1) * (u[4] - 0.5 * (u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0])


def cfl_step(solver, cfl):
    """cfl * finest cell size / max(|v| + c) of the current state (the same rule for every kind of side); the maximum comes
    from the device-side state monitor: 128 bytes cross to the host, not the state"""
    return cfl * 0.5 ** solver.part.mesh.finest_level / solver.monitor().max_speed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--t-end", type=float, default=1.0)
    ap.add_argument("--adapt-every", type=int, default=20)
    ap.add_argument("--min-level", type=int, default=5)
    ap.add_argument("--max-level", type=int, default=8)
    ap.add_argument("--threshold", type=float, default=None, help="refine above this (default 2.0; loehner: 0.8)")
    ap.add_argument("--indicator", choices=["reference", "loehner"], default="reference",
                    help="what steers the adaptation: the reference's dimensional criterion, or the scale-free Loehner "
                         "indicator (amr.Loehner; then --threshold defaults to 0.8, --coarsen to 0.2, --buffer to 1: the customary "
                         "values for this estimator, which nobody has tuned on this solver)")
    ap.add_argument("--quantities", default="density", help="loehner: comma-separated, of density, pressure, mach, entropy")
    ap.add_argument("--coarsen", type=float, default=None, help="loehner: coarsen a family whose mean lies below this (default 0.2)")
    ap.add_argument("--buffer", type=int, default=None, help="loehner: layers of face neighbours refined ahead of a feature (default 1)")
    ap.add_argument("--cfl", type=float, default=0.35)
    ap.add_argument("--sides", choices=list(SIDES), default="farfield", help="the kind of all four sides")
    ap.add_argument("--flux", choices=list(FLUXES), default="kepes")
    ap.add_argument("--out", default=None, help="directory of the .vtu written at the end (density, energy, momentum, pressure, dilatation)")
    ap.add_argument("--toy", action="store_true", help="levels 3-5, t_end 0.05 (a quick check)")
    ap.add_argument("--probes", action="store_true",
                    help="record pressure at three fixed points every step, sampled on the device (sample_points), and save the "
                         "series as acoustic_pulse_probes.npy in --out (default: the working directory): rows t, p_0, p_1, p_2")
    ap.add_argument("--budget", action="store_true",
                    help="print, every 50 steps and at the end, the change of mass and energy (monitor()) against the "
                         "boundary flux integrated in time on the device (boundary.Budget), and their difference")
    args = ap.parse_args()
    if args.toy:
        args.min_level, args.max_level, args.t_end, args.adapt_every = 3, 5, 0.05, 5
    indicator, coarsen = None, None
    if args.indicator == "loehner":
        indicator = amr.Loehner(tuple(args.quantities.split(",")), buffer=1 if args.buffer is None else args.buffer)
        coarsen = 0.2 if args.coarsen is None else args.coarsen
        args.threshold = 0.8 if args.threshold is None else args.threshold
    elif args.threshold is None:
        args.threshold = 2.0

    mesh = SynthMesh(2, args.min_level, args.min_level, sides=(SIDES[args.sides],) * 4)
    part = mesh.partition()
    states = ambient_state() if args.sides in ("farfield", "inflow") else None
    solver = PlainSolver(part, torch.float64, flux_kind=FLUXES[args.flux], mode="fused", state=initial_state(part), inflow_states=states)

    def adapt(s):
        return amr.adapt(s, args.threshold, args.min_level, args.max_level, indicator=indicator, coarsen_below=coarsen)[0]

    for _ in range(args.max_level - args.min_level):      # refine around the pulse, then re-evaluate the state
        solver = adapt(solver)
        ic = torch.from_numpy(initial_state(solver.part)).to(solver.dtype).cuda()
        solver.planes[5 * solver.next:5 * solver.next + 5] = ic
    solver.use_native_stepper()
    budget = boundary.Budget(solver) if args.budget else None
    t, it, cells, t_iter = 0.0, 0, 0, 0.0
    probes = torch.tensor(PROBES, dtype=torch.float64, device="cuda") if args.probes else None
    series = []            # per step [t, p_0, p_1, p_2] on the device: read back once at the end
    while t < args.t_end - 1e-12:
        if it % args.adapt_every == 0:
            if it > 0:
                solver = adapt(solver)
                solver.use_native_stepper()
            dt_cycle = cfl_step(solver, args.cfl)
        dt = min(dt_cycle, args.t_end - t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.iterate(dt)
        torch.cuda.synchronize()
        t_iter += time.perf_counter() - t0
        if budget is not None:
            budget.add_step(solver, dt)
        t += dt
        it += 1
        cells += solver.N
        if probes is not None:
            series.append((t, solver.sample_points(probes, "pressure")["pressure"]))
        if it % 50 == 0:
            print(f"it {it:5d}  t {t:.4f}  elements {solver.N:8d}  finest level {solver.part.mesh.finest_level}  dt {dt:.3e}",
                  flush=True)
            if budget is not None:
                print(budget.line(solver), flush=True)
    if budget is not None and it % 50 != 0:
        print(budget.line(solver))
    assert bool(torch.isfinite(solver.state()).all())
    residual = float(np.abs(pressure(solver) - AMBIENT[1]).max())
    print(f"t = {t:.4f} after {it} steps, {solver.N} elements; {cells / t_iter / 1e6:.1f} M cell-updates/s (host-synchronised)")
    print(f"sides {args.sides}, flux {args.flux}: residual max |p - p_inf| = {residual:.3e}")
    if probes is not None:
        os.makedirs(args.out or ".", exist_ok=True)
        path = os.path.join(args.out or ".", "acoustic_pulse_probes.npy")
        p = torch.stack([s[1] for s in series], dim=1).cpu().numpy()
        np.save(path, np.concatenate([np.array([[s[0] for s in series]]), p]))
        print(f"wrote {path}: pressure at {PROBES} over {len(series)} steps, max |p - p_inf| = "
              f"{', '.join(f'{x:.3e}' for x in np.abs(p - AMBIENT[1]).max(axis=1))}")
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        fields = [vtk.get_host_scalar_variable(solver, solver.next, 0, "density"),
                  vtk.get_host_scalar_variable(solver, solver.next, 4, "energy"),
                  vtk.get_host_vector_variable(solver, solver.next, (1, 2, 3), "momentum")]
        # derived fields, formed on the device (fields.py; the gradient fields take no term from boundary faces)
        fields += [vtk.get_host_derived_variable(solver, name) for name in ("pressure", "dilatation")]
        if indicator is not None:
            fields.append(vtk.get_host_indicator_variable(solver, indicator))
        print("wrote", vtk.save_variables_to_vtk(solver, fields, os.path.join(args.out, "acoustic_pulse")))


if __name__ == "__main__":
    main()
