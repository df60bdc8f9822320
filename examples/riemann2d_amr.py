#!/usr/bin/env python3
"""Adaptive 2D four-quadrant Riemann problem on [0, 1]^2 with outflow on all four sides (one MI355X): the structure of
kelvin_helmholtz_amr.py -- adapt every N steps by the reference's gradient indicator, iterate with the fused kernels and
the native step driver -- on a mesh with open boundaries (SynthMesh(..., sides=...)).

Initial state (Lax & Liu 1998, configuration 3): four constant states meeting at (0.5, 0.5); four shocks run out of the
corners and leave through the sides, which a reflective wall would send back.

    python examples/riemann2d_amr.py --t-end 0.3 --min-level 5 --max-level 9 --out out/riemann2d
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from t8gpu_amd import amr, boundary, tracers, vtk  # noqa: E402
from t8gpu_amd.solver import PlainSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402

GAMMA = 1.4
# (rho, u, v, p) of the quadrants NE, NW, SW, SE
QUADRANTS = ((1.5, 0.0, 0.0, 1.5), (0.5323, 1.206, 0.0, 0.3), (0.138, 1.206, 1.206, 0.029), (0.5323, 0.0, 1.206, 0.3))


def initial_state(part):
    x, y = part.centres[:, 0], part.centres[:, 1]
    q = np.where(x >= 0.5, np.where(y >= 0.5, 0, 3), np.where(y >= 0.5, 1, 2))
    rho, u, v, p = (np.array([s[k] for s in QUADRANTS])[q] for k in range(4))
    return np.stack([rho, rho * u, rho * v, 0 * rho, p / (GAMMA - 1) + 0.5 * rho * (u * u + v * v)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--t-end", type=float, default=0.3)
    ap.add_argument("--adapt-every", type=int, default=20)
    ap.add_argument("--min-level", type=int, default=5)
    ap.add_argument("--max-level", type=int, default=9)
    ap.add_argument("--threshold", type=float, default=None, help="refine above this (default 10.0; loehner: 0.8)")     # mesh_manager.inl:141
    ap.add_argument("--indicator", choices=["reference", "loehner"], default="reference",
                    help="what steers the adaptation: the reference's dimensional density jump, or the scale-free Loehner "
                         "indicator (amr.Loehner; then --threshold defaults to 0.8, --coarsen to 0.2, --buffer to 1: the customary "
                         "values for this estimator, which nobody has tuned on this solver)")
    ap.add_argument("--quantities", default="density", help="loehner: comma-separated, of density, pressure, mach, entropy")
    ap.add_argument("--coarsen", type=float, default=None, help="loehner: coarsen a family whose mean lies below this (default 0.2)")
    ap.add_argument("--buffer", type=int, default=None, help="loehner: layers of face neighbours refined ahead of a feature (default 1)")
    ap.add_argument("--cfl", type=float, default=0.35)
    ap.add_argument("--out", default=None, help="directory of the .vtu written at the end (density, energy, momentum, pressure, schlieren)")
    ap.add_argument("--toy", action="store_true", help="levels 3-5, t_end 0.05 (a quick check)")
    ap.add_argument("--lineout", action="store_true",
                    help="save density along the diagonal (0, 0) - (1, 1), sampled on the device (sample_points), as "
                         "riemann2d_lineout.npy in --out (default: the working directory): rows s, x, y, density")
    ap.add_argument("--budget", action="store_true",
                    help="print, every 50 steps and at the end, the change of mass and energy (monitor()) against the "
                         "boundary flux integrated in time on the device (boundary.Budget), and their difference")
    ap.add_argument("--tracers", type=int, default=None, metavar="N",
                    help="advect an N x N lattice of tracer particles with the flow (solver.tracers: predict before every step, "
                         "correct after it, rebind after every adapt), print how many left through the open sides, and save "
                         "positions and status as riemann2d_tracers_{x,status}.npy in --out (default: the working directory)")
    args = ap.parse_args()
    if args.toy:
        args.min_level, args.max_level, args.t_end, args.adapt_every = 3, 5, 0.05, 5
    indicator, coarsen = None, None
    if args.indicator == "loehner":
        indicator = amr.Loehner(tuple(args.quantities.split(",")), buffer=1 if args.buffer is None else args.buffer)
        coarsen = 0.2 if args.coarsen is None else args.coarsen
        args.threshold = 0.8 if args.threshold is None else args.threshold
    elif args.threshold is None:
        args.threshold = 10.0

    sides = ("outflow",) * 4
    mesh = SynthMesh(2, args.min_level, args.min_level, sides=sides)
    solver = PlainSolver(mesh.partition(), torch.float64, mode="fused", state=initial_state(mesh.partition()))

    def adapt(s):
        return amr.adapt(s, args.threshold, args.min_level, args.max_level, indicator=indicator, coarsen_below=coarsen)[0]

    for _ in range(args.max_level - args.min_level):      # refine around the discontinuities, then re-evaluate the state
        solver = adapt(solver)
        ic = torch.from_numpy(initial_state(solver.part)).to(solver.dtype).cuda()
        solver.planes[5 * solver.next:5 * solver.next + 5] = ic
    solver.use_native_stepper()
    budget = boundary.Budget(solver) if args.budget else None
    tr = solver.tracers(tracers.lattice(2, args.tracers)) if args.tracers else None
    t, it, cells, t_iter = 0.0, 0, 0, 0.0
    while t < args.t_end - 1e-12:
        fresh = it % args.adapt_every == 0 and it > 0
        if fresh:
            solver = adapt(solver)
            solver.use_native_stepper()
            if tr is not None:
                tr.rebind(solver)                                  # particles are coordinates: an adapt does not touch them
        if it == 0:
            dt = 0.1 * 2.0 ** -solver.part.mesh.finest_level
        elif fresh:
            dt = solver.cfl_timestep(cfl=args.cfl)                 # a solver fresh from an adapt has no face speeds yet
        else:
            dt = solver.compute_timestep(cfl=args.cfl)             # CFL step from the speeds of the last step (open faces too)
        dt = min(dt, args.t_end - t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if tr is not None:
            tr.predict(dt)                                         # k1 = u^n(x), xs = x + dt k1
        solver.iterate(dt)
        if tr is not None:
            tr.correct(dt)                                         # x += dt / 2 (k1 + u^(n+1)(xs))
        torch.cuda.synchronize()
        t_iter += time.perf_counter() - t0
        if budget is not None:
            budget.add_step(solver, dt)
        t += dt
        it += 1
        cells += solver.N
        if it % 50 == 0:
            print(f"it {it:5d}  t {t:.4f}  elements {solver.N:8d}  finest level {solver.part.mesh.finest_level}  dt {dt:.3e}",
                  flush=True)
            if budget is not None:
                print(budget.line(solver), flush=True)
    if budget is not None and it % 50 != 0:
        print(budget.line(solver))
    assert bool(torch.isfinite(solver.state()).all())
    print(f"t = {t:.4f} after {it} steps, {solver.N} elements; {cells / t_iter / 1e6:.1f} M cell-updates/s (host-synchronised)")
    if tr is not None:
        active, left, lost = tr.counts()
        print(f"tracers: {tr.M} particles, {left} left through the open sides, {lost} lost, {active} still inside")
        os.makedirs(args.out or ".", exist_ok=True)
        h = tr.host()
        for name in ("x", "status"):
            np.save(os.path.join(args.out or ".", f"riemann2d_tracers_{name}.npy"), h[name])
    if args.lineout:
        n = 2 ** (solver.part.mesh.finest_level + 1)               # two points per finest cell: cell values, not interpolated
        s = (np.arange(n) + 0.5) / n
        rho = solver.sample_points(np.stack([s, s], axis=1), "density")["density"].cpu().numpy()
        os.makedirs(args.out or ".", exist_ok=True)
        path = os.path.join(args.out or ".", "riemann2d_lineout.npy")
        np.save(path, np.stack([s * np.sqrt(2.0), s, s, rho]))
        print(f"wrote {path}: density along the diagonal at {n} points, {rho.min():.4f} .. {rho.max():.4f}")
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        fields = [vtk.get_host_scalar_variable(solver, solver.next, 0, "density"),
                  vtk.get_host_scalar_variable(solver, solver.next, 4, "energy"),
                  vtk.get_host_vector_variable(solver, solver.next, (1, 2, 3), "momentum")]
        # derived fields, formed on the device (fields.py; the gradient fields take no term from boundary faces)
        fields += [vtk.get_host_derived_variable(solver, name) for name in ("pressure", "schlieren")]
        if indicator is not None:
            fields.append(vtk.get_host_indicator_variable(solver, indicator))
        print("wrote", vtk.save_variables_to_vtk(solver, fields, os.path.join(args.out, "riemann2d")))


if __name__ == "__main__":
    main()
