#!/usr/bin/env python3
"""Adaptive 2D acoustic pulse on Subgrid<4,4> blocks with far-field boundaries on all four sides (one MI355X): the pulse of
acoustic_pulse_farfield.py on blocks of 4 x 4 subcells, every subcell on a block face of the domain boundary with its own
characteristic far-field sub-face flux (SubgridSolver(..., open_boundaries=True, farfield=True)).

    python examples/acoustic_pulse_subgrid_farfield.py --t-end 1.0 --min-level 3 --max-level 6 --out out/pulse
    python examples/acoustic_pulse_subgrid_farfield.py --ramp 0.95      # the ambient pressure moves linearly to 0.95 over the run

--ramp P shows run-time boundary states: before every step SubgridSolver.set_inflow_states refills the device table with the
ambient state whose pressure has moved linearly from 1 towards P (no new solver, no new plan); the fluid follows the far field.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from t8gpu_amd import amr, boundary, hip, vtk  # noqa: E402
from t8gpu_amd.solver import SubgridSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

GAMMA = 1.4
AMBIENT = (1.0, 1.0)   # rho, p
FLUXES = {"kepes": hip.KEPES, "hll": hip.HLL, "hllc": hip.HLLC}
S = 16                 # subcells per block


def ambient_state(p=AMBIENT[1]):
    """at rest, on the isentrope of AMBIENT"""
    rho = AMBIENT[0] * (p / AMBIENT[1]) ** (1 / GAMMA)
    return np.array([[rho, 0.0, 0.0, 0.0, p / (GAMMA - 1)]])


def subcell_centres(part):
    """x, y of every subcell: block centre + (i + 0.5 - 2) * edge / 4; subcell (i, j) of block e at e * 16 + i + 4 j"""
    c = np.asarray(part.centres)[:, :2]
    edge = np.sqrt(np.asarray(part.volumes))
    cell = np.arange(S)
    off = np.stack([(cell & 3) - 1.5, (cell >> 2) - 1.5], 1)
    xy = c[:, None, :] + off[None, :, :] * (edge[:, None, None] / 4)
    return xy[..., 0].reshape(-1), xy[..., 1].reshape(-1)


def initial_state(part, amplitude=0.1, width=0.05):
    x, y = subcell_centres(part)
    r2 = (x - 0.5) ** 2 + (y - 0.5) ** 2
    p = AMBIENT[1] * (1 + amplitude * np.exp(-r2 / (width * width)))
    rho = AMBIENT[0] * (p / AMBIENT[1]) ** (1 / GAMMA)
    return np.stack([rho, 0 * rho, 0 * rho, 0 * rho, p / (GAMMA - 1)])


def pressure(solver):
    u = solver.state().double().cpu().numpy()
    return (GAMMA - 1) * (u[4] - 0.5 * (u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0])


def cfl_step(solver, cfl):
    """cfl * finest subcell size / max(|v| + c) of the current state; the maximum comes from the device-side state monitor:
    128 bytes cross to the host, not the state"""
    return cfl * 0.5 ** (solver.part.mesh.finest_level + 2) / solver.monitor().max_speed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--t-end", type=float, default=1.0)
    ap.add_argument("--adapt-every", type=int, default=20)
    ap.add_argument("--min-level", type=int, default=3, help="coarsest block level (a block holds 4 x 4 subcells)")
    ap.add_argument("--max-level", type=int, default=6)
    ap.add_argument("--threshold", type=float, default=None, help="refine above this (default 0.02; loehner: 0.8)")
    ap.add_argument("--indicator", choices=["reference", "loehner"], default="reference",
                    help="what steers the adaptation: the reference's dimensional criterion, or the scale-free Loehner "
                         "indicator (amr.Loehner; then --threshold defaults to 0.8, --coarsen to 0.2, --buffer to 1: the customary "
                         "values for this estimator, which nobody has tuned on this solver)")
    ap.add_argument("--quantities", default="density", help="loehner: comma-separated, of density, pressure, mach, entropy")
    ap.add_argument("--coarsen", type=float, default=None, help="loehner: coarsen a family whose mean lies below this (default 0.2)")
    ap.add_argument("--buffer", type=int, default=None, help="loehner: layers of face neighbours refined ahead of a feature (default 1)")
    ap.add_argument("--cfl", type=float, default=0.35)
    ap.add_argument("--flux", choices=list(FLUXES), default="kepes")
    ap.add_argument("--ramp", type=float, nargs="?", const=0.95, default=None,
                    help="ambient pressure at t_end: the far-field state is updated before every step (set_inflow_states)")
    ap.add_argument("--out", default=None, help="directory of the .vtu written at the end (density, energy, momentum, pressure, dilatation)")
    ap.add_argument("--toy", action="store_true", help="block levels 2-3, t_end 0.05 (a quick check)")
    ap.add_argument("--budget", action="store_true",
                    help="print, every 50 steps and at the end, the change of mass and energy (monitor()) against the "
                         "boundary flux integrated in time on the device (boundary.Budget), and their difference")
    args = ap.parse_args()
    if args.toy:
        args.min_level, args.max_level, args.t_end, args.adapt_every = 2, 3, 0.05, 5
    indicator, coarsen = None, None
    if args.indicator == "loehner":
        indicator = amr.Loehner(tuple(args.quantities.split(",")), buffer=1 if args.buffer is None else args.buffer)
        coarsen = 0.2 if args.coarsen is None else args.coarsen
        args.threshold = 0.8 if args.threshold is None else args.threshold
    elif args.threshold is None:
        args.threshold = 0.02

    mesh = SynthMesh(2, args.min_level, args.min_level, sides=(("farfield", 0),) * 4)
    part = mesh.partition(subgrid=True)
    solver = SubgridSolver(part, torch.float64, flux_kind=FLUXES[args.flux], mode="fused", state=initial_state(part),
                           open_boundaries=True, farfield=True, inflow_states=ambient_state())

    def adapt(s):
        return amr.adapt_subgrid(s, args.threshold, args.min_level, args.max_level, indicator=indicator, coarsen_below=coarsen)[0]

    for _ in range(args.max_level - args.min_level):      # refine around the pulse, then re-evaluate the state
        solver = adapt(solver)
        ic = torch.from_numpy(initial_state(solver.part)).to(solver.dtype).cuda()
        solver.planes[5 * solver.next:5 * solver.next + 5] = ic
    solver.use_native_stepper()
    budget = boundary.Budget(solver) if args.budget else None
    t, it, cells, t_iter = 0.0, 0, 0, 0.0
    while t < args.t_end - 1e-12:
        if it % args.adapt_every == 0:
            if it > 0:
                solver = adapt(solver)                     # (the new solver takes the current far-field state along)
                solver.use_native_stepper()
            dt_cycle = cfl_step(solver, args.cfl)
        dt = min(dt_cycle, args.t_end - t)
        if args.ramp is not None:
            solver.set_inflow_states(ambient_state(AMBIENT[1] + (args.ramp - AMBIENT[1]) * min(1.0, (t + dt) / args.t_end)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.iterate(dt)
        torch.cuda.synchronize()
        t_iter += time.perf_counter() - t0
        if budget is not None:
            budget.add_step(solver, dt)
        t += dt
        it += 1
        cells += solver.owned_cells
        if it % 50 == 0:
            print(f"it {it:5d}  t {t:.4f}  blocks {solver.N:8d}  finest level {solver.part.mesh.finest_level}  dt {dt:.3e}", flush=True)
            if budget is not None:
                print(budget.line(solver), flush=True)
    if budget is not None and it % 50 != 0:
        print(budget.line(solver))
    assert bool(torch.isfinite(solver.state()).all())
    p_inf = 0.4 * float(solver.inflow_states[0, 4])
    p = pressure(solver)
    print(f"t = {t:.4f} after {it} steps, {solver.N} blocks; {cells / t_iter / 1e6:.1f} M subcell-updates/s (host-synchronised)")
    print(f"flux {args.flux}: far-field pressure {p_inf:.4f}, mean p {p.mean():.4f}, residual max |p - p_inf| = {np.abs(p - p_inf).max():.3e}")
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        fields = [vtk.get_host_scalar_variable(solver, solver.next, 0, "density"),
                  vtk.get_host_scalar_variable(solver, solver.next, 4, "energy"),
                  vtk.get_host_vector_variable(solver, solver.next, (1, 2, 3), "momentum")]
        # derived fields, formed on the device (fields.py; the gradient fields take no term from boundary faces)
        fields += [vtk.get_host_derived_variable(solver, name) for name in ("pressure", "dilatation")]
        if indicator is not None:
            fields.append(vtk.get_host_indicator_variable(solver, indicator))
        print("wrote", vtk.save_variables_to_vtk(solver, fields, os.path.join(args.out, "acoustic_pulse_subgrid")))


if __name__ == "__main__":
    main()
