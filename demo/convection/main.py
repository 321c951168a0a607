#!/usr/bin/env python3
"""Convection-diffusion in a given flow field: `phifem_amd.ConvectionDiffusionSolver`, `phifem_amd.HeatSolver(velocity=)`.

    python main.py {bg,sub} [--dim 2|3] [--cubes N] [--peclet P] [--supg S] [--reaction C] [--heat --steps K]
                            [--levels L] [--precond 0|1]

Unit circle / sphere in [-1.5, 1.5]^d, c u + beta . grad u - div(kappa grad u) = f, u = u_D on the boundary, with
    kappa = k0 exp(ln(10) / 2 sin 2x cos 1.5y),   beta = (1 - 0.8 y, 0.5 + 0.8 x [, 0]),
    u     = 0.5 + sin(1.3 x + 0.4) sin(0.9 y + 1.2) [sin(0.7 z + 0.9)],    f = c u + beta . grad u - div(kappa grad u).
k0 is chosen so that the largest cell Peclet number h |beta| / kappa on the finest mesh is P (the coarser meshes of the
run keep that kappa, so theirs is larger).  The problem is solved on N / 2^(L-1), ..., N / 2, N cubes per axis; per
size: the cell Peclet number, active DoFs, assembly time (device events), BiCGStab iterations and solve time, the
preconditioner, and the root-mean-square and largest nodal error over the vertices of inside cells.  `bg` works on the
tagged background mesh, `sub` on the sub-mesh of the cells tagged 1 or 2.  --supg S adds streamline diffusion (0.25 is a
good value once P exceeds 1).  --heat steps du/dt + beta . grad u - div(kappa grad u) = f with u(t) = exp(-t) u above
by backward Euler, dt = h, K steps, and prints the error at the last step and the mean iterations and refresh / solve
time per step.  The library solves with the plain lattice preconditioner while the cell Peclet number and the contrast
of kappa are small and with Jacobi otherwise; --precond 0 selects Jacobi throughout.  Nodal fields live on
the device (torch tensors); rtol 1e-8."""
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


def manufactured(x):
    """kappa (k0 = 1), beta, u, -div(kappa grad u) (k0 = 1), beta . grad u at the points x."""
    d = x.shape[1]
    a = 0.5 * np.log(10.0)
    wv, sv = np.array([1.3, 0.9, 0.7])[:d], np.array([0.4, 1.2, 0.9])[:d]
    S, Cc = np.sin(x * wv + sv), np.cos(x * wv + sv)
    prod = S.prod(axis=1)
    grad = np.stack([wv[k] * Cc[:, k] * np.delete(S, k, axis=1).prod(axis=1) for k in range(d)], axis=1)
    kap = np.exp(a * np.sin(2.0 * x[:, 0]) * np.cos(1.5 * x[:, 1]))
    gk = np.zeros_like(x)
    gk[:, 0] = a * kap * 2.0 * np.cos(2.0 * x[:, 0]) * np.cos(1.5 * x[:, 1])
    gk[:, 1] = -a * kap * 1.5 * np.sin(2.0 * x[:, 0]) * np.sin(1.5 * x[:, 1])
    beta = np.zeros_like(x)
    beta[:, 0] = 1.0 - 0.8 * x[:, 1]
    beta[:, 1] = 0.5 + 0.8 * x[:, 0]
    return kap, beta, 0.5 + prod, kap * (wv ** 2).sum() * prod - (gk * grad).sum(axis=1), (beta * grad).sum(axis=1)


def setup(args, n):
    d = args.dim
    bg = P.create_box([-1.5] * d, [1.5] * d, [n] * d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        _, _, sub, _, _ = P.compute_tags_measures(bg, NodalFunction((bg.x ** 2).sum(axis=1) - 1.0), 1,
                                                  box_mode=args.mesh_type == "bg", single_layer_cut=True)
    work = bg if args.mesh_type == "bg" else sub
    L.check(L.lib.phx_set_option(work._h, L.OPT_PRECOND, args.precond))
    return work


def unit_peclet(work, to):
    """The largest cell Peclet number at k0 = 1, from the library's own reduction."""
    kap, beta, *_ = manufactured(work.x)
    zero = to(np.zeros(work.nv))
    s = P.ConvectionDiffusionSolver(work)
    return s.assemble(to(beta), to((work.x ** 2).sum(axis=1) - 1.0), zero, zero, kappa_h=to(kap))["peclet_max"]


def run(args, work, n, k0):
    import torch
    dev = torch.device("cuda", work.device)
    to = lambda a: torch.as_tensor(a, device=dev)
    x = work.x
    phi = (x ** 2).sum(axis=1) - 1.0
    kap, beta, u, minus_div, adv = manufactured(x)
    kap, minus_div = k0 * kap, k0 * minus_div
    inside = np.unique(work.cells[work.cell_tag_values() == 1])
    if not args.heat:
        s = P.ConvectionDiffusionSolver(work, args.reaction, supg_coef=args.supg)
        info = s.assemble(to(beta), to(phi), to(args.reaction * u + adv + minus_div), to(u), kappa_h=to(kap))
        w = s.solve(rtol=1e-8)              # without out= the solution comes back as a numpy array
        st = s.stats
        e = w[:work.nv][inside] - u[inside]
        print(f"n = {n:4d}  Peclet {info['peclet_max']:7.2f}  {info['n_active']:9d} active DoFs  assemble "
              f"{1e3 * work.timings()['assemble']:8.3f} ms  {st['iterations']:5d} iterations ({st['precond']}, relres "
              f"{st['relres']:.1e})  solve {1e3 * st['seconds']:8.3f} ms  rms error {np.sqrt(np.mean(e * e)):.3e}  max error "
              f"{np.abs(e).max():.3e}")
        return
    dt = 3.0 / n
    heat = P.HeatSolver(work, dt, kappa=to(kap), velocity=to(beta), supg_coef=args.supg)
    info = heat.assemble(to(phi))
    asm_ms = 1e3 * work.timings()["assemble"]
    heat.set_state(to(u))
    total = [0, 0.0, 0.0]
    for k in range(args.steps):
        g = float(np.exp(-(heat.t + dt)))
        heat.step(to(g * (adv + minus_div - u)), to(g * u), rtol=1e-8)
        st = heat.stats
        if k > 0 or args.steps == 1:       # the first step pays the set-up of the preconditioner
            total = [total[0] + st["iterations"], total[1] + st["rhs_seconds"], total[2] + st["seconds"]]
    m = max(args.steps - 1, 1)
    e = heat.u.cpu().numpy()[inside] - float(np.exp(-heat.t)) * u[inside]
    print(f"n = {n:4d}  Peclet {info['peclet_max']:7.2f}  {info['n_active']:9d} active DoFs  assemble {asm_ms:8.3f} ms  "
          f"{args.steps} backward Euler steps to t = {heat.t:.4f}: {total[0] / m:6.1f} iterations ({st['precond']}), refresh "
          f"{1e3 * total[1] / m:.3f} ms, solve {1e3 * total[2] / m:.3f} ms per step  rms error {np.sqrt(np.mean(e * e)):.3e}  "
          f"max error {np.abs(e).max():.3e}")


def main():
    ap = argparse.ArgumentParser(prog="main.py", description="convection-diffusion on a level-set domain")
    ap.add_argument("mesh_type", choices=["bg", "sub"])
    ap.add_argument("--dim", type=int, default=2, choices=[2, 3])
    ap.add_argument("--cubes", type=int, default=64)
    ap.add_argument("--levels", type=int, default=3, help="sizes N / 2^(L-1) .. N")
    ap.add_argument("--peclet", type=float, default=3.0, help="largest cell Peclet number on the finest mesh")
    ap.add_argument("--supg", type=float, default=0.25)
    ap.add_argument("--reaction", type=float, default=0.0)
    ap.add_argument("--heat", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--precond", type=int, default=1, choices=[0, 1])
    args = ap.parse_args()
    if not args.peclet > 0.0:
        ap.error("--peclet: a value > 0")
    if not args.supg >= 0.0:
        ap.error("--supg: a value >= 0")
    import torch
    sizes = [max(args.cubes >> lev, 4) for lev in range(args.levels - 1, -1, -1)]
    meshes = {n: setup(args, n) for n in dict.fromkeys(sizes)}
    fine = meshes[sizes[-1]]
    k0 = unit_peclet(fine, lambda a: torch.as_tensor(a, device=torch.device("cuda", fine.device))) / args.peclet
    for n in sizes:
        run(args, meshes[n], n, k0)


if __name__ == "__main__":
    main()
