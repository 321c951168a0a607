#!/usr/bin/env python3
"""Linear elasticity on a level-set domain with the displacement prescribed on {phi = 0}: `phifem_amd.ElasticitySolver`.

    python main.py {bg,sub} [--dim 2|3] [--cubes N] [--levels K] [--adapt] [--repeat R] [--compare-interface]
                            [--skip-errors] [--coarse R]

Unit circle / sphere in [-1.5, 1.5]^d, E = 1, nu = 0.3, manufactured solution
    2-D: u = (sin x cos y, cos(x + y/2)),    3-D: u = (sin x cos y cos z, cos(x + y/2) sin z, sin(x - z) cos y),
f = -div sigma(u), u_D = u.  `bg` assembles on the tagged background mesh (box mode), `sub` on the sub-mesh of the
cells tagged 1 or 2.  Level 0 is the generated box with N cubes per axis; every further level refines the previous
background mesh -- uniformly, or with --adapt the cells `mark_dorfler` selects from the Zienkiewicz-Zhu indicator
`estimate_zz(mesh, u, 1)` of the displacement (the residual indicator of this scheme is not implemented).  Per level:
active DoFs, BiCGStab iterations, relative L2 / H1_0 errors of u_h on Omega_h (`cell_errors`), then the slopes fitted
over the levels, and the tag / assemble / solve times of the last call (`mesh.timings()`: device events on the mesh's
stream; --repeat 2 reports the second, warm call).  --compare-interface also times `InterfaceElasticitySolver.assemble`
on the same mesh (27 / 14 blocks, one workgroup per element): a point of comparison, not the same problem.
--coarse R (0: off, -1: automatic, >= 5: H / h) adds the Galerkin coarse space of `ElasticitySolver(coarse=R)` to the
vertex blocks wherever the level is a generated box lattice solved in box mode: level 0, and the uniformly refined levels,
which are then generated as boxes of N 2^level cubes instead of being refined.  Adapted levels and sub-meshes keep the
vertex blocks alone, and say so.  The line of a level names the preconditioner, the coarse DoFs and the seconds of the
coarse build (paid once per system, inside its first solve)."""
import argparse
import os
import sys
import warnings

import numpy as np
import sympy as sy

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)

import phifem_amd as P  # noqa: E402
from phifem_amd.mesh_scripts import NodalFunction  # noqa: E402
from phifem_amd.postprocess import cell_errors  # noqa: E402

E, NU = 1.0, 0.3


def manufactured(d):
    """(u, f = -div sigma(u)) as numpy functions of points x (d, n) -> (d, n)."""
    X = sy.symbols("x y z")[:d]
    if d == 2:
        u = sy.Matrix([sy.sin(X[0]) * sy.cos(X[1]), sy.cos(X[0] + X[1] / 2)])
    else:
        u = sy.Matrix([sy.sin(X[0]) * sy.cos(X[1]) * sy.cos(X[2]), sy.cos(X[0] + X[1] / 2) * sy.sin(X[2]),
                       sy.sin(X[0] - X[2]) * sy.cos(X[1])])
    lam, mu = E * NU / (1.0 + NU) / (1.0 - 2.0 * NU), E / 2.0 / (1.0 + NU)
    g = u.jacobian(list(X))
    s = lam * g.trace() * sy.eye(d) + mu * (g + g.T)
    f = -sy.Matrix([sum(sy.diff(s[a, b], X[b]) for b in range(d)) for a in range(d)])

    def wrap(vec):
        comps = [sy.lambdify(X, vec[a], "numpy") for a in range(d)]
        return lambda x: np.stack([np.broadcast_to(np.asarray(c(*x), dtype=np.float64), x.shape[1:]) for c in comps])
    return wrap(u), wrap(f)


def main():
    ap = argparse.ArgumentParser(prog="main.py", description="weak-Dirichlet elasticity on a level-set domain")
    ap.add_argument("mesh_type", choices=["bg", "sub"])
    ap.add_argument("--dim", type=int, default=2, choices=[2, 3])
    ap.add_argument("--cubes", type=int, default=16)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--adapt", action="store_true")
    ap.add_argument("--repeat", type=int, default=1, help="assemble + solve this many times, report the last")
    ap.add_argument("--compare-interface", action="store_true")
    ap.add_argument("--skip-errors", action="store_true", help="no cell_errors (timing runs at large sizes)")
    ap.add_argument("--coarse", type=int, default=0, help="coarse space: 0 off, -1 automatic, >= 5 the ratio H / h")
    args = ap.parse_args()
    d = args.dim
    exact, source = manufactured(d)

    def levelset(x):
        return (x ** 2).sum(axis=1) - 1.0

    bg = P.create_box([-1.5] * d, [1.5] * d, [args.cubes] * d)
    rows = []
    for lv in range(args.levels):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _, _, sub, _, maps = P.compute_tags_measures(bg, NodalFunction(levelset(bg.x)), 1, box_mode=args.mesh_type == "bg",
                                                         single_layer_cut=True)
        t_tag = bg.timings()
        work = bg if args.mesh_type == "bg" else sub
        x = work.x
        lattice = args.mesh_type == "bg" and (lv == 0 or not args.adapt)
        solver = P.ElasticitySolver(work, E=E, nu=NU, coarse=args.coarse if lattice else 0)
        builds = []
        for _ in range(max(args.repeat, 1)):
            info = solver.assemble(levelset(x), source(x.T).T, exact(x.T).T)
            w = solver.solve(rtol=1e-8, max_iter=500000)
            builds.append(solver.stats.get("coarse_build_s", 0.0))
        u, _ = solver.split(w)
        u = np.ascontiguousarray(u)
        tags = work.cell_tag_values()
        omega = np.flatnonzero((tags == 1) | (tags == 2)).astype(np.int32)
        # (the degree-3 reference values are evaluated on the host: 20 points per cell, too many for a timing run)
        e = (cell_errors(work, u, exact, degree=1, cells=omega) if not args.skip_errors
             else {"l2_relative": np.nan, "h10_relative": np.nan})
        t = work.timings()
        st = solver.stats
        rows.append((info["n_active"], e["l2_relative"], e["h10_relative"]))
        print(f"level {lv}: {bg.nc} background cells, {info['n_active']} active DoFs, nnz {info['nnz']}, "
              f"{st['iterations']} iterations ({st['precond']}, relres {st['relres']:.1e}), "
              f"L2 {e['l2_relative']:.3e}  H10 {e['h10_relative']:.3e}")
        if args.coarse != 0 and not lattice:
            print("         no coarse space on this level: an adapted level or a sub-mesh is no box lattice")
        elif args.coarse != 0:
            why = f" -- not built: {st['coarse_reason']}" if st["coarse_reason"] else ""
            print(f"         coarse space: H = {st['coarse_ratio']} h, {st['coarse_dofs']} coarse DoFs, build "
                  f"{1e3 * builds[-1]:.3f} ms (host clock, inside the solve of that call){why}")
        print(f"         tag cells {1e3 * t_tag['tag_cells']:.3f} ms, tag facets {1e3 * t_tag['tag_facets']:.3f} ms, "
              f"assemble {1e3 * t['assemble']:.3f} ms, solve {1e3 * t['solve']:.3f} ms "
              f"(slot capacity {info['slot_capacity']})")
        if args.compare_interface and args.mesh_type == "bg" and lv == 0:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                P.compute_tags_measures(bg, NodalFunction(-levelset(bg.x)), 1, box_mode=True)
            bc = np.flatnonzero(np.abs(bg.x).max(axis=1) == 1.5)
            other = P.InterfaceElasticitySolver(bg)
            for _ in range(max(args.repeat, 1)):
                oinfo = other.assemble(-levelset(bg.x), source(bg.x.T).T, exact(bg.x.T).T, bc)
            print(f"         for orientation: InterfaceElasticitySolver.assemble {1e3 * bg.timings()['assemble']:.3f} ms, "
                  f"{oinfo['n_active']} active DoFs, nnz {oinfo['nnz']}")
            other._free()
        if lv + 1 == args.levels:
            break
        if args.adapt:
            eta2 = P.estimate_zz(work, np.ascontiguousarray(u.T), 1)      # (ncomp, nv); the cells tagged 1 or 2
            if args.mesh_type == "sub":       # the marks of the sub-mesh cells on their background cells
                full = np.zeros(bg.nc)
                full[maps[0]] = eta2
                eta2 = full
            marked = P.mark_dorfler(bg, eta2, theta=0.5)
            fine = P.refine(bg, marked=marked)
            print(f"         eta_zz = {np.sqrt(eta2.sum()):.4e}, marked {int(marked.sum())} cells -> "
                  f"{fine.refine_info[0]} edges in {fine.refine_info[1]} sweeps")
            bg = fine
        elif args.coarse != 0:      # the same lattice as a generated box: the coarse space is built on those
            bg = P.create_box([-1.5] * d, [1.5] * d, [args.cubes * 2 ** (lv + 1)] * d)
        else:
            bg = P.refine(bg)
    if len(rows) > 1:
        n, l2, h10 = (np.array(c, dtype=np.float64) for c in zip(*rows))
        print(f"slopes over the DoFs: L2 {np.polyfit(np.log(n), np.log(l2), 1)[0]:.2f}, "
              f"H10 {np.polyfit(np.log(n), np.log(h10), 1)[0]:.2f}  (optimal: {-2.0 / d:.2f}, {-1.0 / d:.2f})")


if __name__ == "__main__":
    main()
