#!/usr/bin/env python3
"""Diffusion with a conductivity that varies in space: `phifem_amd.DiffusionSolver`, `phifem_amd.HeatSolver(kappa=)`.

    python main.py {bg,sub} [--dim 2|3] [--cubes N] [--contrast R] [--reaction C] [--heat --steps K] [--levels L]
                            [--precond 0|1]

Unit circle / sphere in [-1.5, 1.5]^d, c u - div(kappa grad u) = f, u = u_D on the boundary, with
    kappa = exp(ln(R) / 2 sin 2x cos 1.5y)          (max / min -> R; R = 1 is the Laplacian)
    u     = 0.5 + sin(1.3 x + 0.4) sin(0.9 y + 1.2) [sin(0.7 z + 0.9)],    f = c u - kappa Lap u - grad kappa . grad u.
The problem is solved on N / 2^(L-1), ..., N / 2, N cubes per axis; per size: active DoFs, assembly time (device
events), BiCGStab iterations and solve time, the preconditioner, and the root-mean-square and largest nodal error over
the vertices of inside cells -- they fall like h^2.  `bg` works on the tagged background mesh, `sub` on the sub-mesh of
the cells tagged 1 or 2.  --heat steps du/dt - div(kappa grad u) = f with u(t) = exp(-t) u above by backward Euler,
dt = h, K steps, and prints the error at the last step and the mean iterations and refresh / solve time per step.  The library solves with
the plain lattice preconditioner up to contrast 50 and with Jacobi above; --precond 0 selects Jacobi throughout.  Nodal
fields live on the device (torch tensors); rtol 1e-8."""
import argparse
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)

import phifem_amd as P  # noqa: E402
from phifem_amd import _lib as L  # noqa: E402
from phifem_amd.mesh_scripts import NodalFunction  # noqa: E402


def manufactured(x, contrast):
    """kappa, u, -(kappa Lap u + grad kappa . grad u) at the points x."""
    d = x.shape[1]
    a = 0.5 * np.log(contrast)
    wv, sv = np.array([1.3, 0.9, 0.7])[:d], np.array([0.4, 1.2, 0.9])[:d]
    S, Cc = np.sin(x * wv + sv), np.cos(x * wv + sv)
    prod = S.prod(axis=1)
    grad = np.stack([wv[k] * Cc[:, k] * np.delete(S, k, axis=1).prod(axis=1) for k in range(d)], axis=1)
    kap = np.exp(a * np.sin(2.0 * x[:, 0]) * np.cos(1.5 * x[:, 1]))
    gk = np.zeros_like(x)
    gk[:, 0] = a * kap * 2.0 * np.cos(2.0 * x[:, 0]) * np.cos(1.5 * x[:, 1])
    gk[:, 1] = -a * kap * 1.5 * np.sin(2.0 * x[:, 0]) * np.sin(1.5 * x[:, 1])
    return kap, 0.5 + prod, kap * (wv ** 2).sum() * prod - (gk * grad).sum(axis=1)


def run(args, n):
    d = args.dim
    bg = P.create_box([-1.5] * d, [1.5] * d, [n] * d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        _, _, sub, _, _ = P.compute_tags_measures(bg, NodalFunction((bg.x ** 2).sum(axis=1) - 1.0), 1,
                                                  box_mode=args.mesh_type == "bg", single_layer_cut=True)
    work = bg if args.mesh_type == "bg" else sub
    L.check(L.lib.phx_set_option(work._h, L.OPT_PRECOND, args.precond))
    x = work.x
    phi = (x ** 2).sum(axis=1) - 1.0
    kap, u, minus_div = manufactured(x, args.contrast)
    inside = np.unique(work.cells[work.cell_tag_values() == 1])
    import torch
    dev = torch.device("cuda", work.device)
    to = lambda a: torch.as_tensor(a, device=dev)
    head = f"n = {n:4d}  contrast {kap.max() / kap.min():7.2f}"
    if not args.heat:
        s = P.DiffusionSolver(work, args.reaction)
        info = s.assemble(to(kap), to(phi), to(args.reaction * u + minus_div), to(u))
        w = s.solve(rtol=1e-8)              # without out= the solution comes back as a numpy array
        st = s.stats
        e = w[:work.nv][inside] - u[inside]
        print(f"{head}  {info['n_active']:9d} active DoFs  assemble {1e3 * work.timings()['assemble']:8.3f} ms  "
              f"{st['iterations']:5d} iterations ({st['precond']}, relres {st['relres']:.1e})  solve "
              f"{1e3 * st['seconds']:8.3f} ms  rms error {np.sqrt(np.mean(e * e)):.3e}  max error {np.abs(e).max():.3e}")
        return
    dt = 3.0 / n
    heat = P.HeatSolver(work, dt, kappa=to(kap))
    info = heat.assemble(to(phi))
    asm_ms = 1e3 * work.timings()["assemble"]
    heat.set_state(to(u))
    total = [0, 0.0, 0.0]
    for k in range(args.steps):
        g = float(np.exp(-(heat.t + dt)))
        heat.step(to(g * (minus_div - u)), to(g * u), rtol=1e-8)
        st = heat.stats
        if k > 0 or args.steps == 1:       # the first step pays the set-up of the preconditioner
            total = [total[0] + st["iterations"], total[1] + st["rhs_seconds"], total[2] + st["seconds"]]
    m = max(args.steps - 1, 1)
    e = heat.u.cpu().numpy()[inside] - float(np.exp(-heat.t)) * u[inside]
    print(f"{head}  {info['n_active']:9d} active DoFs  assemble {asm_ms:8.3f} ms  {args.steps} backward Euler steps to "
          f"t = {heat.t:.4f}: {total[0] / m:6.1f} iterations ({st['precond']}), refresh {1e3 * total[1] / m:.3f} ms, solve "
          f"{1e3 * total[2] / m:.3f} ms per step  rms error {np.sqrt(np.mean(e * e)):.3e}  max error {np.abs(e).max():.3e}")


def main():
    ap = argparse.ArgumentParser(prog="main.py", description="variable-coefficient diffusion on a level-set domain")
    ap.add_argument("mesh_type", choices=["bg", "sub"])
    ap.add_argument("--dim", type=int, default=2, choices=[2, 3])
    ap.add_argument("--cubes", type=int, default=64)
    ap.add_argument("--levels", type=int, default=3, help="sizes N / 2^(L-1) .. N")
    ap.add_argument("--contrast", type=float, default=10.0)
    ap.add_argument("--reaction", type=float, default=0.0)
    ap.add_argument("--heat", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--precond", type=int, default=1, choices=[0, 1])
    args = ap.parse_args()
    if not args.contrast >= 1.0:
        ap.error("--contrast: a value >= 1")
    for lev in range(args.levels - 1, -1, -1):
        run(args, max(args.cubes >> lev, 4))


if __name__ == "__main__":
    main()
