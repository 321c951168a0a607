#!/usr/bin/env python3
"""Heat equation on a level-set domain by implicit time stepping: `phifem_amd.HeatSolver`.

    python main.py {bg,sub} [--dim 2|3] [--cubes N] [--steps K] [--dt DT] [--scheme bdf1|bdf2] [--no-warm-start]
                            [--rtol R] [--host]

Unit circle / sphere in [-1.5, 1.5]^d, du/dt - Lap u = f with the manufactured solution
    u = exp(-t) cos(x) cos(y) [cos(z)],    f = (d - 1) u,    u_D = u,
dt = h = 3 / N unless --dt is given.  `bg` steps on the tagged background mesh (box mode), `sub` on the sub-mesh of the
cells tagged 1 or 2.  The matrix is assembled once (BDF2: once more after its backward Euler start); every step
refreshes the right-hand side on the device (`ReactionSolver.update_rhs`) and solves, started from the previous
solution unless --no-warm-start.  Per step: BiCGStab iterations, the seconds of the refresh (host clock around the call,
which ends in a stream synchronisation) and of the solve (`stats["seconds"]`, device events), then the largest nodal
error at the active vertices.  The nodal fields live on the device (torch tensors) unless --host."""
import argparse
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)

import phifem_amd as P  # noqa: E402
from phifem_amd.mesh_scripts import NodalFunction  # noqa: E402


def main():
    ap = argparse.ArgumentParser(prog="main.py", description="heat equation on a level-set domain")
    ap.add_argument("mesh_type", choices=["bg", "sub"])
    ap.add_argument("--dim", type=int, default=2, choices=[2, 3])
    ap.add_argument("--cubes", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dt", type=float, default=None)
    ap.add_argument("--scheme", default="bdf1", choices=["bdf1", "bdf2"])
    ap.add_argument("--no-warm-start", action="store_true")
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--host", action="store_true", help="numpy arrays instead of device tensors")
    args = ap.parse_args()
    d, dt = args.dim, args.dt if args.dt else 3.0 / args.cubes

    bg = P.create_box([-1.5] * d, [1.5] * d, [args.cubes] * d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        _, _, sub, _, _ = P.compute_tags_measures(bg, NodalFunction((bg.x ** 2).sum(axis=1) - 1.0), 1,
                                                  box_mode=args.mesh_type == "bg", single_layer_cut=True)
    work = bg if args.mesh_type == "bg" else sub
    x = work.x
    phi = (x ** 2).sum(axis=1) - 1.0
    space = np.prod(np.cos(x), axis=1)
    if not args.host:
        import torch
        dev = torch.device("cuda", work.device)
        phi, space = torch.as_tensor(phi, device=dev), torch.as_tensor(space, device=dev)
    exact = lambda t: float(np.exp(-t)) * space

    heat = P.HeatSolver(work, dt, scheme=args.scheme)
    t0 = time.perf_counter()
    info = heat.assemble(phi)
    t_host = time.perf_counter() - t0
    print(f"{work.nc} cells, {info['n_active']} active DoFs, nnz {info['nnz']}, dt = {dt:g}, {args.scheme}: assemble "
          f"{1e3 * work.timings()['assemble']:.3f} ms (device events), {1e3 * t_host:.3f} ms (host clock, first call)")
    heat.set_state(exact(0.0))
    total = [0, 0.0, 0.0]
    for k in range(args.steps):
        t = heat.t + dt
        ue = exact(t)
        w = heat.step((d - 1.0) * ue, ue, rtol=args.rtol, warm_start=not args.no_warm_start)
        st = heat.stats
        err = abs(heat.u - ue)[w[:work.nv] != 0.0].max()
        print(f"step {k + 1:3d}  t = {heat.t:.4f}  {st['iterations']:4d} iterations ({st['precond']}, relres "
              f"{st['relres']:.1e})  refresh {1e3 * st['rhs_seconds']:.3f} ms  solve {1e3 * st['seconds']:.3f} ms  "
              f"max nodal error {float(err):.3e}")
        if k > 0:       # the first step pays the set-up of the preconditioner
            total = [total[0] + st["iterations"], total[1] + st["rhs_seconds"], total[2] + st["seconds"]]
    n = max(args.steps - 1, 1)
    print(f"steps 2..{args.steps}: {total[0] / n:.1f} iterations, refresh {1e3 * total[1] / n:.3f} ms, solve "
          f"{1e3 * total[2] / n:.3f} ms per step (warm start {'off' if args.no_warm_start else 'on'})")


if __name__ == "__main__":
    main()
