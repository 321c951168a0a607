#!/usr/bin/env python3
"""The adaptive loop for the strong-Dirichlet scheme: tag -> solve -> recover -> Doerfler marking -> marked refinement,
all on the device.

    python adapt.py [mesh.xdmf] [--levels 6] [--theta 0.5] [--compare-uniform]

`StrongDirichletSolver.estimate` refuses (the residuals of `phifem_amd.estimate` are those of the weak-Dirichlet
scheme), so the loop marks with the recovery-based indicator `estimate_zz(mesh, solver.solution(w))`, which needs
nothing of the formulation but u_h.  Same mesh and circle as demo/weak-dirichlet/adapt.py.  The scheme
imposes u = 0 on the circle, so the manufactured solution is that demo's g = sin x cos y (+ 0.3 z) times the level-set:
u = phi g, f = -(g Laplace phi + 2 grad phi . grad g + phi Laplace g).

Per level the line shows the cells of the background mesh, the DoFs of u_h on the cells tagged 1 or 2, eta =
sqrt(sum eta_T^2) of `estimate_zz`, the H1-seminorm error on those cells (`cell_errors`, which needs the exact solution)
and their ratio.  eta is an indicator for marking, not a bound: the ratio is printed, nothing is promised about it.
With --compare-uniform the same columns are printed for uniform refinement of the same start mesh."""
import argparse
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)

import phifem_amd as P  # noqa: E402
from phifem_amd.mesh_scripts import NodalFunction  # noqa: E402
from phifem_amd.postprocess import cell_errors  # noqa: E402


def problem(x0):
    """(levelset, exact, source) for the start vertices x0; each takes x of shape (gdim, n)."""
    d = x0.shape[1]
    centre = x0.mean(axis=0) + np.array([0.013, -0.007, 0.005][:d])
    radius = 0.62 * 0.5 * (x0.max(axis=0) - x0.min(axis=0)).min()

    def levelset(x):
        return ((x - centre[:, None]) ** 2).sum(axis=0) - radius ** 2

    def factor(x):
        return np.sin(x[0]) * np.cos(x[1]) + (0.3 * x[2] if d == 3 else 0.0)

    def exact(x):
        return levelset(x) * factor(x)

    def source(x):
        sc = np.sin(x[0]) * np.cos(x[1])
        grad = [np.cos(x[0]) * np.cos(x[1]), -np.sin(x[0]) * np.sin(x[1])] + ([0.3 + 0.0 * x[0]] if d == 3 else [])
        dot = sum(2.0 * (x[k] - centre[k]) * grad[k] for k in range(d))
        return -(2.0 * d * factor(x) + 2.0 * dot - 2.0 * levelset(x) * sc)

    return levelset, exact, source


def solve_level(mesh, levelset, exact, source):
    """One strong-Dirichlet solve on `mesh` -> dict(nc, ndofs, eta, h10, eta2, tags, u)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        P.compute_tags_measures(mesh, NodalFunction(levelset(mesh.x.T)), 1, box_mode=True)
    solver = P.StrongDirichletSolver(mesh, degree=1, levelset_degree=1)
    solver.assemble(levelset(mesh.x.T), source(mesh.x.T))
    w = solver.solve(rtol=1e-11, max_iter=200000)
    u = solver.solution(w)
    eta2 = P.estimate_zz(mesh, u)
    tags = mesh.cell_tag_values()
    omega = np.flatnonzero((tags == 1) | (tags == 2)).astype(np.int32)
    h10 = np.sqrt(cell_errors(mesh, u, exact, degree=1, cells=omega)["h10_sum"])
    return dict(nc=mesh.nc, ndofs=int(np.unique(mesh.cells[omega]).size), eta=float(np.sqrt(P.estimate_zz.last_sum)),
                h10=float(h10), eta2=eta2, tags=tags, u=u)


def run_loop(cell_type, x0, cells0, levels, theta=0.5, uniform=False, report=print, name="adaptive"):
    """`levels` solves, refining in between: where `mark_dorfler(theta)` says so, or everywhere.  Returns one dict per
    level (solve_level's, plus `marked`, the mask the level was refined by, None on the last one)."""
    levelset, exact, source = problem(x0)
    mesh = P.Mesh.from_arrays(cell_type, x0, cells0)
    rows = []
    for lv in range(levels):
        row = solve_level(mesh, levelset, exact, source)
        row["marked"] = None
        line = (f"{name} level {lv}: {row['nc']} cells, dofs={row['ndofs']}  eta={row['eta']:.4e}  "
                f"H10={row['h10']:.4e}  eta/H10={row['eta'] / row['h10']:.3f}")
        if lv + 1 < levels:
            if uniform:
                mesh = P.refine(mesh)
            else:
                row["marked"] = P.mark_dorfler(mesh, row["eta2"], theta=theta)
                mesh = P.refine(mesh, marked=row["marked"])
                nm, sweeps, _ = mesh.refine_info
                line += f"  marked {int(row['marked'].sum())} cells -> {nm} edges in {sweeps} sweeps"
        report(line)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(prog="adapt.py", description="adaptive refinement driven by the recovery-based indicator.")
    ap.add_argument("mesh", nargs="?", default=os.path.join(ROOT, "tests", "golden", "xdmf", "disk.xdmf"))
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--theta", type=float, default=0.5)
    ap.add_argument("--compare-uniform", action="store_true")
    args = ap.parse_args()
    m = P.io.read_xdmf(args.mesh)
    if m["cell_type"] not in ("triangle", "tetrahedron"):
        raise SystemExit("adapt.py reads triangle and tetrahedron meshes")
    adaptive = run_loop(m["cell_type"], m["x"], m["cells"], args.levels, args.theta)
    if args.compare_uniform:
        uniform = run_loop(m["cell_type"], m["x"], m["cells"], args.levels, uniform=True, name="uniform ")
        for ru in uniform:
            hit = next((ra for ra in adaptive if ra["eta"] <= ru["eta"]), None)
            print(f"eta <= {ru['eta']:.4e}: uniform {ru['nc']} cells / {ru['ndofs']} dofs, adaptive "
                  + (f"{hit['nc']} cells / {hit['ndofs']} dofs" if hit is not None else "not reached"))


if __name__ == "__main__":
    main()
