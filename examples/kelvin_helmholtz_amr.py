#!/usr/bin/env python3
"""Adaptive Kelvin-Helmholtz run on one MI355X: the reference's main loop
(examples/compressible_euler/main.cu:30-38 -- adapt every N steps, iterate, periodic output) on the synthetic
2D periodic mesh, with the fused kernels, the native step driver and the device-side adapt path.

    python examples/kelvin_helmholtz_amr.py --steps 400 --adapt-every 50 --min-level 5 --max-level 9 --vtk out/kh

Several GPUs (one process each; adapt + repartition through amr.adapt_partitioned, halo exchange per RK stage):

    python -m torch.distributed.run --nproc-per-node 4 --master-addr 127.0.0.1 examples/kelvin_helmholtz_amr.py ...

T8GPU_REHEARSAL=1 runs the same on ONE GPU (all ranks share it, gloo + host-staged halos) to try the flow out.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from t8gpu_amd import amr, hostmem, tracers, vtk  # noqa: E402
from t8gpu_amd.halo import HaloExchange  # noqa: E402
from t8gpu_amd.solver import PlainSolver  # noqa: E402
from t8gpu_amd.synth import SynthMesh  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--adapt-every", type=int, default=50)
    ap.add_argument("--min-level", type=int, default=5)
    ap.add_argument("--max-level", type=int, default=9)
    ap.add_argument("--threshold", type=float, default=None, help="refine above this (default 10.0; loehner: 0.8)")     # mesh_manager.inl:141
    ap.add_argument("--indicator", choices=["reference", "loehner"], default="reference",
                    help="what steers the adaptation: the reference's dimensional criterion, or the scale-free Loehner "
                         "indicator (amr.Loehner; then --threshold defaults to 0.8, --coarsen to 0.2, --buffer to 1: the customary "
                         "values for this estimator, which nobody has tuned on this solver)")
    ap.add_argument("--quantities", default="density", help="loehner: comma-separated, of density, pressure, mach, entropy")
    ap.add_argument("--coarsen", type=float, default=None, help="loehner: coarsen a family whose mean lies below this (default 0.2)")
    ap.add_argument("--buffer", type=int, default=None, help="loehner: layers of face neighbours refined ahead of a feature (default 1)")
    ap.add_argument("--dtype", default="f64", choices=["f32", "f64"])
    ap.add_argument("--vtk", default=None, help="prefix of the .vtu / .pvtu files written at the end (density, energy, momentum, pressure, mach, vorticity)")
    ap.add_argument("--image", type=int, default=None, metavar="N",
                    help="save N x N images of schlieren and density, sampled on the device (sample_grid), as .npy files beside the "
                         "VTK output (prefix --vtk, or kh): at the end, and every --image-every steps")
    ap.add_argument("--image-every", type=int, default=None, metavar="K")
    ap.add_argument("--stats", action="store_true",
                    help="time-averaged statistics on the device (solver.statistics()): accumulated every --stats-every steps, "
                         "carried through every adapt; mean_density, mean_velocity, tke and pressure_rms go to the VTK output, a "
                         "tke image beside the others with --image")
    ap.add_argument("--stats-every", type=int, default=1, metavar="K", help="accumulate every K steps with weight K dt (default 1)")
    ap.add_argument("--tracers", type=int, default=None, metavar="N",
                    help="advect an N x N lattice of tracer particles with the flow (solver.tracers: predict before every step, "
                         "correct after it, rebind after every adapt; on several ranks every rank holds all particles and the "
                         "velocities are summed, one all_reduce per phase): positions and status are saved as .npy files beside "
                         "the images (prefix --vtk, or kh) at the end, and every --image-every steps")
    ap.add_argument("--profile", type=int, default=None, metavar="LEVEL",
                    help="save profiles against y on 2^LEVEL bins, averaged over x on the device (solver.average_along): mean "
                         "density and Favre x-velocity, with --stats also reynolds_stress and tke formed from the space- and "
                         "time-averaged sums (stats.average_along), as .npy files beside the images (prefix --vtk, or kh): at the "
                         "end, and every --profile-every steps; prints the momentum thickness of the shear layers")
    ap.add_argument("--profile-every", type=int, default=None, metavar="K")
    args = ap.parse_args()
    indicator, coarsen = None, None
    if args.indicator == "loehner":
        indicator = amr.Loehner(tuple(args.quantities.split(",")), buffer=1 if args.buffer is None else args.buffer)
        coarsen = 0.2 if args.coarsen is None else args.coarsen
        args.threshold = 0.8 if args.threshold is None else args.threshold
    elif args.threshold is None:
        args.threshold = 10.0
    dtype = torch.float64 if args.dtype == "f64" else torch.float32
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    rehearsal = os.environ.get("T8GPU_REHEARSAL", "0") == "1"
    dist = None
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(0 if rehearsal else int(os.environ.get("LOCAL_RANK", 0)))
        dist.init_process_group("gloo" if rehearsal else "nccl")
    # (after set_device: pinned memory creates a context on the current device -- every rank's own GPU, not GPU 0)
    hostmem.keep_heap()      # host arrays of an adapt cycle are reused by the next one (t8gpu_amd/hostmem.py)
    if not rehearsal:
        hostmem.use_pinned_uploads()   # ... and uploaded through one pinned staging buffer
    say = print if rank == 0 else (lambda *a, **k: None)

    def adapt(s, carry=()):
        if world == 1:
            return amr.adapt(s, args.threshold, args.min_level, args.max_level, indicator=indicator, coarsen_below=coarsen,
                             carry=carry)[0]
        # refreshes the ghost slots of the current state itself (the indicator reads them), through the run's halo object
        return amr.adapt_partitioned(s, dist, host_staged=rehearsal, halo=halo_of.get(id(s)), threshold=args.threshold,
                                     min_level=args.min_level, max_level=args.max_level, indicator=indicator, coarsen_below=coarsen,
                                     carry=carry)

    def total(x, op="sum"):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device="cpu" if rehearsal else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.SUM if op == "sum" else dist.ReduceOp.MAX)
        return float(t.item())

    def save_images(s, it):
        """schlieren and density of the current state on an N x N grid: one derived_fields pass and one fused sampling launch;
        a pixel belongs to exactly one rank, the others contribute 0"""
        images = s.sample_grid(["schlieren", "density"], (args.image, args.image), halo=halo_of.get(id(s)), fill=0.0)
        prefix = args.vtk or "kh"
        os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
        for name, image in images.items():
            if world > 1:
                image = image.cpu() if rehearsal else image
                dist.all_reduce(image)
            if rank == 0:
                np.save(f"{prefix}_{name}_{it:06d}.npy", image.cpu().numpy())
        if stats is not None and stats.weight > 0:
            image = stats.sample_grid(["tke"], (args.image, args.image), fill=0.0)["tke"]
            if world > 1:
                image = image.cpu() if rehearsal else image
                dist.all_reduce(image)
            if rank == 0:
                np.save(f"{prefix}_tke_{it:06d}.npy", image.cpu().numpy())
        say(f"images at it {it}: {prefix}_{{schlieren,density}}_{it:06d}.npy", flush=True)

    def all_ranks(t):
        """the sum of a device tensor over the ranks, on the device again"""
        if world == 1:
            return t
        t = t.cpu() if rehearsal else t
        dist.all_reduce(t)
        return t.cuda()

    def save_profiles(s, it):
        """profiles against y, homogeneous in x (in 3D: and in z, axes=(0, 2)): every rank's partial sums and weights in
        one block, one all-reduce, one division. The Favre velocity is mean(rho u) / mean(rho); the stresses are formed from
        the averaged SUMS (results_of), never averaged per cell."""
        axes, L = (0,), args.profile
        sums, w = s.average_along(["density", "momentum"], axes, L, partial=True)
        block = all_ranks(torch.cat([sums["density"][None], sums["momentum"], w[None]]))
        rho, mx = (block[0] / block[-1]).cpu().numpy(), (block[1] / block[-1]).cpu().numpy()
        u = mx / rho
        prefix = args.vtk or "kh"
        out = {"mean_density": rho, "favre_velocity_x": u}
        if stats is not None and stats.weight > 0:
            s15, w15 = stats.average_along(["reynolds_stress", "tke"], axes, L, partial=True)
            block = all_ranks(torch.cat([s15, w15[None]]))
            res = stats.results_of(block[:-1] / block[-1], ["reynolds_stress", "tke"])
            out.update({name: t.cpu().numpy() for name, t in res.items()})
        mass = float(s.monitor(dist=dist).integrals[0])
        if rank == 0:
            os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
            for name, a in out.items():
                np.save(f"{prefix}_profile_{name}_{it:06d}.npy", a)
        # theta = int rho (U1 - u)(u - U2) dy / (rho0 (U1 - U2)^2) with U1, U2 the fastest and slowest stream of the profile:
        # the sum over the shear layers of the periodic box
        dy, du = 0.5 ** L, float(u.max() - u.min())
        theta = float((rho * (u.max() - u) * (u - u.min())).sum() * dy / (rho.mean() * du * du)) if du > 0 else 0.0
        say(f"profiles at it {it}: {prefix}_profile_{{{','.join(out)}}}_{it:06d}.npy  mass {mass:.17e}  "
            f"momentum thickness {theta:.6e}", flush=True)

    def save_tracers(it):
        if rank == 0:                                    # (every rank holds the same particles)
            prefix = args.vtk or "kh"
            os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
            h = tr.host()
            np.save(f"{prefix}_tracers_x_{it:06d}.npy", h["x"])
            np.save(f"{prefix}_tracers_status_{it:06d}.npy", h["status"])

    mesh = SynthMesh(2, args.min_level, args.min_level)
    solver = PlainSolver(mesh.partition(rank, world), dtype, mode="fused")
    # refine the initial mesh around the shear layers before starting (the reference adapts at step 0)
    halo_of = {}           # id(solver) -> its HaloExchange, when one exists already
    for _ in range(args.max_level - args.min_level):
        solver = adapt(solver)
        # re-evaluate the initial condition on the refined mesh (sharp layers)
        ic = torch.from_numpy(solver.part.kh_initial_state()).to(dtype).cuda()
        solver.planes[5 * solver.next:5 * solver.next + 5] = ic
    halo = HaloExchange(solver.part, dtype, dist, stage_through_host=rehearsal) if world > 1 else None
    halo_of = {id(solver): halo}
    if world == 1:
        solver.use_native_stepper()
    tr = solver.tracers(tracers.lattice(2, args.tracers)) if args.tracers else None
    stats = solver.statistics() if args.stats else None      # running sums on the device; they follow the run through adapt
    mass0 = solver.monitor(dist=dist).integrals      # the state monitor: one device pass, one all-reduced block of 16 doubles
    t_iter = t_adapt = 0.0
    cells = 0
    for it in range(args.steps):
        if it % args.adapt_every == 0 and it > 0:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            solver = adapt(solver, carry=(stats,) if stats is not None else ())
            say(f"adapt at it {it}: criteria sum {solver.last_adapt_criteria_sum:.12e}  elements {int(total(solver.N))}", flush=True)
            if world > 1:
                halo = HaloExchange(solver.part, dtype, dist, stage_through_host=rehearsal)
                halo_of = {id(solver): halo}
            else:
                solver.use_native_stepper()
            if tr is not None:
                tr.rebind(solver)                        # particles are coordinates: an adapt does not touch them
            torch.cuda.synchronize()
            t_adapt += time.perf_counter() - t0
        if it == 0 or it % args.adapt_every == 0:
            dt = 0.1 * 2.0 ** -solver.part.mesh.finest_level                 # the reference's fixed step (main_2d.cu:27-30)
        elif it % 10 == 0:
            dt = solver.compute_timestep(cfl=0.35, dist=dist)                 # CFL step from the device-side max speed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if tr is not None:
            tr.predict(dt, dist=dist)                    # k1 = u^n(x), xs = x + dt k1
        solver.iterate(dt, halo=halo)
        if tr is not None:
            tr.correct(dt, dist=dist)                    # x += dt / 2 (k1 + u^(n+1)(xs))
        torch.cuda.synchronize()
        t_iter += time.perf_counter() - t0
        cells += solver.N
        if stats is not None and (it + 1) % args.stats_every == 0:
            stats.accumulate(args.stats_every * dt)              # the time the sample stands for: K steps of dt
        if args.image and args.image_every and (it + 1) % args.image_every == 0 and it + 1 < args.steps:
            save_images(solver, it + 1)
        if tr is not None and args.image_every and (it + 1) % args.image_every == 0 and it + 1 < args.steps:
            save_tracers(it + 1)
        if args.profile is not None and args.profile_every and (it + 1) % args.profile_every == 0 and it + 1 < args.steps:
            save_profiles(solver, it + 1)
        if it % 100 == 0:
            mon = solver.monitor(dist=dist)
            drift = float(abs(mon.integrals - mass0).max())
            say(f"it {it:5d}  elements {int(total(solver.N)):8d}  finest level {solver.part.mesh.finest_level}  dt {dt:.3e}  "
                f"conservation drift {drift:.2e}  entropy {mon.entropy:.9e}  min p {mon.min_pressure:.4e}", flush=True)
    assert bool(torch.isfinite(solver.state()).all())
    if args.image:
        save_images(solver, args.steps)
    if args.profile is not None:
        save_profiles(solver, args.steps)
    if tr is not None:
        save_tracers(args.steps)
        active, left, lost = tr.counts()
        say(f"tracers: {tr.M} particles, {active} active, {lost} lost")
    if args.vtk:
        # CompressibleEulerSolver::save_conserved_variables_to_vtk (examples/compressible_euler/solver.cu:177-186)
        os.makedirs(os.path.dirname(os.path.abspath(args.vtk)), exist_ok=True)
        fields = [vtk.get_host_scalar_variable(solver, solver.next, 0, "density"),
                  vtk.get_host_scalar_variable(solver, solver.next, 4, "energy"),
                  vtk.get_host_vector_variable(solver, solver.next, (1, 2, 3), "momentum")]
        # derived fields, formed on the device (fields.py; the gradient fields take no term from boundary faces)
        fields += [vtk.get_host_derived_variable(solver, name, halo=halo) for name in ("pressure", "mach", "vorticity")]
        if indicator is not None:
            fields.append(vtk.get_host_indicator_variable(solver, indicator, halo=halo))
        if stats is not None and stats.weight > 0:
            fields += [vtk.get_host_statistics_variable(stats, name)
                       for name in ("mean_density", "mean_velocity", "tke", "pressure_rms")]
        say("wrote", vtk.save_variables_to_vtk(solver, fields, args.vtk, dist=dist))
    say(f"iterate: {total(cells) / total(t_iter, 'max') / 1e6:.1f} M cell-updates/s (host-synchronised per step), "
        f"adapt: {t_adapt:.2f} s total, iterate: {t_iter:.2f} s total")
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
