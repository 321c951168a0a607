#!/usr/bin/env python3
"""h-convergence of weak-Dirichlet phi-FEM Poisson on a caller-supplied mesh, refined on the device.

    python refine.py [mesh.xdmf] [--levels 3] [--degree {1,2}]

Reads a triangle or tetrahedron mesh (default: the disk of tests/golden/xdmf), places a circle / sphere of 0.62 times
the half extent of its bounding box inside it and solves  -Laplace u = f,  u = u_D on the circle  for the manufactured
solution u = sin(x) cos(y) (+ 0.3 z).  Per level: level-set and data are interpolated from their EXPRESSIONS on the
current mesh (the level-set is never prolongated), the mesh is tagged, the system assembled and solved, the error
measured by `cell_errors` on the cells tagged 1 or 2; then `phifem_amd.refine` -- the counterpart of
`dolfinx.mesh.refine(mesh)[0]` -- makes the next mesh.  `phifem_amd.prolongate` carries u_h to the finer mesh, where it
is compared with the solution computed there."""
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
    ap = argparse.ArgumentParser(prog="refine.py", description="h-convergence study on a refined mesh hierarchy.")
    ap.add_argument("mesh", nargs="?", default=os.path.join(ROOT, "tests", "golden", "xdmf", "disk.xdmf"))
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--degree", type=int, default=1, choices=[1, 2])
    args = ap.parse_args()

    m = P.io.read_xdmf(args.mesh)
    if m["cell_type"] not in ("triangle", "tetrahedron"):
        raise SystemExit("refine.py reads triangle and tetrahedron meshes")
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

    mesh = P.Mesh.from_arrays(m["cell_type"], x0, m["cells"])
    prev = None                            # (u_h, p_h) of the previous level
    errs = []
    for level in range(args.levels):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            P.compute_tags_measures(mesh, NodalFunction(levelset(mesh.x.T)), 1, box_mode=True, single_layer_cut=True)
        solver = P.PhiFEMSolver(mesh, degree=args.degree, levelset_degree=args.degree)
        pts = mesh.lagrange_dof_points(args.degree)
        info = solver.assemble(levelset(pts.T), source(pts.T), exact(pts.T))
        w = solver.solve(rtol=1e-11, max_iter=200000)
        u_h, _ = solver.split(w)
        tags = mesh.cell_tag_values()
        omega = np.flatnonzero((tags == 1) | (tags == 2)).astype(np.int32)
        e = cell_errors(mesh, u_h, exact, degree=args.degree, cells=omega)
        errs.append((np.sqrt(e["l2_sum"]), np.sqrt(e["h10_sum"])))
        line = (f"level {level}: {mesh.nc} cells, {info['n_active']} active DoFs, "
                f"{solver.stats['iterations']} iterations, L2={errs[-1][0]:.4e} H10={errs[-1][1]:.4e}")
        if level > 0:
            line += (f"  slopes {np.log2(errs[-2][0] / errs[-1][0]):.2f} / {np.log2(errs[-2][1] / errs[-1][1]):.2f}")
            # the transfer: u_h of the coarser level on this mesh, compared on the DoFs of the cells inside the domain
            inside = mesh.cells[tags == 1].reshape(-1)
            if args.degree == 2:
                inside = np.concatenate([inside, mesh.nv + mesh.c2e[tags == 1].reshape(-1)])
            inside = np.unique(inside)
            diff = P.prolongate(mesh, prev, degree=args.degree)[inside] - u_h[inside]
            line += f"  |prolongate(u_H) - u_h| = {np.sqrt(np.mean(diff ** 2)):.3e}"
        print(line)
        prev = np.array(u_h)
        if level + 1 < args.levels:
            mesh = P.refine(mesh)


if __name__ == "__main__":
    main()
