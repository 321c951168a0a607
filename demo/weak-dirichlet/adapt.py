#!/usr/bin/env python3
"""The adaptive loop: tag -> solve -> estimate -> Doerfler marking -> marked refinement, all on the device.

    python adapt.py [mesh.xdmf] [--levels 6] [--degree {1,2}] [--theta 0.5] [--compare-uniform] [--multilevel]

Same mesh, circle and manufactured solution as estimate.py.  Per level the line shows the DoFs of u_h (the entities of
the cells tagged 1 or 2; the cells of the whole background mesh are printed next to them), eta = sqrt(sum eta_T^2) of
`solver.estimate`, and the H1-seminorm error on those cells (`cell_errors`, which needs the exact solution).
`mark_dorfler(theta)` selects the cells, `refine(mesh, marked=...)` closes the marks by longest-edge bisection and
splits them.  With --compare-uniform the same columns are
printed for uniform refinement of the same start mesh, and then the background cells and DoFs either loop needs to
reach the eta of each uniform level.  (The manufactured solution is smooth: the marked loop saves background cells, which
it refines inside Omega_h only, not DoFs of Omega_h -- DESIGN.md 7e has the figures.)

With --multilevel (degree 1) every refined level is solved a second and a third time, with Jacobi and with the
multilevel preconditioner over the hierarchy built so far: iterations and milliseconds of the warm second
solve, timed with device events on the mesh's stream."""
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


def main():
    ap = argparse.ArgumentParser(prog="adapt.py", description="adaptive refinement driven by the residual indicator.")
    ap.add_argument("mesh", nargs="?", default=os.path.join(ROOT, "tests", "golden", "xdmf", "disk.xdmf"))
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--degree", type=int, default=1, choices=[1, 2])
    ap.add_argument("--theta", type=float, default=0.5)
    ap.add_argument("--compare-uniform", action="store_true")
    ap.add_argument("--multilevel", action="store_true", help="per level: iterations and solve time with and without")
    args = ap.parse_args()

    m = P.io.read_xdmf(args.mesh)
    if m["cell_type"] not in ("triangle", "tetrahedron"):
        raise SystemExit("adapt.py reads triangle and tetrahedron meshes")
    x0 = m["x"]
    d = x0.shape[1]
    centre = x0.mean(axis=0) + np.array([0.013, -0.007, 0.005][:d])
    radius = 0.62 * 0.5 * (x0.max(axis=0) - x0.min(axis=0)).min()

    def levelset(x):                       # x: (gdim, n), as the reference's expressions
        return ((x - centre[:, None]) ** 2).sum(axis=0) - radius ** 2

    def exact(x):
        return np.sin(x[0]) * np.cos(x[1]) + (0.3 * x[2] if d == 3 else 0.0)

    def source(x):
        return 2.0 * np.sin(x[0]) * np.cos(x[1])

    def level(mesh):
        """One solve on `mesh` -> (DoFs of u_h, eta, H10 error, eta_T^2)."""
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            P.compute_tags_measures(mesh, NodalFunction(levelset(mesh.x.T)), 1, box_mode=True, single_layer_cut=True)
        solver = P.PhiFEMSolver(mesh, degree=args.degree, levelset_degree=args.degree)
        pts = mesh.lagrange_dof_points(args.degree)
        solver.assemble(levelset(pts.T), source(pts.T), exact(pts.T))
        w = solver.solve(rtol=1e-11, max_iter=200000)
        eta2 = solver.estimate(w)
        u_h, _ = solver.split(w)
        tags = mesh.cell_tag_values()
        omega = np.flatnonzero((tags == 1) | (tags == 2)).astype(np.int32)
        h10 = np.sqrt(cell_errors(mesh, u_h, exact, degree=args.degree, cells=omega)["h10_sum"])
        ents = [mesh.cells[omega]] + ([mesh.nv + mesh.c2e[omega]] if args.degree == 2 else [])
        ndofs = sum(np.unique(e).size for e in ents)
        return ndofs, float(np.sqrt(eta2.sum())), float(h10), eta2

    def timed(mesh, multilevel):
        """(iterations, ms of the second, warm solve -- `stats["seconds"]` is the time between two events on the mesh's
        stream around the Krylov loop --, preconditioner)"""
        solver = P.PhiFEMSolver(mesh, multilevel=multilevel)
        pts = mesh.x
        solver.assemble(levelset(pts.T), source(pts.T), exact(pts.T))
        for _ in range(2):
            solver.solve(rtol=1e-8, max_iter=200000)
        return solver.stats["iterations"], 1e3 * solver.stats["seconds"], solver.stats["precond"]

    def run(name, step):
        mesh = P.Mesh.from_arrays(m["cell_type"], x0, m["cells"])
        rows = []
        for lv in range(args.levels):
            ndofs, eta, h10, eta2 = level(mesh)
            rows.append((ndofs, eta, h10, mesh.nc))
            line = f"{name} level {lv}: {mesh.nc} cells, dofs={ndofs}  eta={eta:.4e}  H10={h10:.4e}"
            if args.multilevel and args.degree == 1 and getattr(mesh, "coarse", None) is not None:
                (itj, msj, pj), (itm, msm, pm) = timed(mesh, False), timed(mesh, "auto")
                line += f"  | {pj} {itj} it {msj:.2f} ms, {pm} {itm} it {msm:.2f} ms"
            if lv + 1 < args.levels:
                mesh, note = step(mesh, eta2)
                line += note
            print(line)
        return rows

    def adaptive_step(mesh, eta2):
        marked = P.mark_dorfler(mesh, eta2, theta=args.theta)
        fine = P.refine(mesh, marked=marked)
        nm, sweeps, _ = fine.refine_info
        return fine, f"  marked {int(marked.sum())} cells -> {nm} edges in {sweeps} sweeps"

    adaptive = run("adaptive", adaptive_step)
    if args.compare_uniform:
        uniform = run("uniform ", lambda mesh, eta2: (P.refine(mesh), ""))
        # what either loop needs to bring eta below what the uniform loop reaches at each of its levels
        for nd_u, eta_u, _, nc_u in uniform:
            hit = next(((nd, nc) for nd, eta, _, nc in adaptive if eta <= eta_u), None)
            print(f"eta <= {eta_u:.4e}: uniform {nc_u} cells / {nd_u} dofs, adaptive "
                  + (f"{hit[1]} cells / {hit[0]} dofs" if hit is not None else "not reached"))


if __name__ == "__main__":
    main()
