#!/usr/bin/env python3
"""Probing a phi-FEM solution: weak-Dirichlet Poisson on the "flower" domain, solved on two NON-NESTED background
meshes and compared through point evaluation.

    python probe.py [--coarse 200] [--fine 283] [--cell-type {triangle,quadrilateral}]

The flower problem (flower/data.py) has no exact solution, so the only convergence check is a coarse solve against a
fine one.  Neither of 200 and 283 divides the other: the two meshes share no cell, `prolongate` cannot serve, and
`interpolate_nonmatching` -- the counterpart of dolfinx's function of that name -- evaluates the fine solution at the
vertices of the coarse mesh on the GPU.  Printed: the RMS of  I_H u_h - u_H  over the vertices of the coarse cells
tagged 1 (inside the domain), and u_h along a line of 11 points through the domain, evaluated by `evaluate` on both
meshes (nan where a point lies in no cell)."""
import argparse
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, os.path.join(HERE, "flower"))

import phifem_amd as P  # noqa: E402
from phifem_amd.mesh_scripts import NodalFunction  # noqa: E402

from data import detection_levelset, dirichlet_data, levelset, source_term  # noqa: E402


def solve(n, cell_type):
    mesh = P.create_rectangle([[-4.5, -4.5], [4.5, 4.5]], [n, n], cell_type=cell_type)
    xt = mesh.x.T
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        P.compute_tags_measures(mesh, NodalFunction(detection_levelset(xt)), 1, box_mode=True, single_layer_cut=True)
    solver = P.PhiFEMSolver(mesh, pen_coef=1.0, stab_coef=1.0)
    info = solver.assemble(levelset(xt), source_term(xt), dirichlet_data(xt))
    u_h, _ = solver.split(solver.solve(rtol=1e-10, max_iter=100000))
    print(f"{n} x {n} {cell_type}s: {info['n_active']} active DoFs, {solver.stats['iterations']} iterations, "
          f"max u_h = {u_h.max():.6f}")
    return mesh, np.asarray(u_h)


def main():
    ap = argparse.ArgumentParser(prog="probe.py", description="Compare two non-nested phi-FEM solves by point evaluation.")
    ap.add_argument("--coarse", type=int, default=200)
    ap.add_argument("--fine", type=int, default=283)
    ap.add_argument("--cell-type", choices=["triangle", "quadrilateral"], default="triangle")
    args = ap.parse_args()

    coarse, u_c = solve(args.coarse, args.cell_type)
    fine, u_f = solve(args.fine, args.cell_type)

    # the fine solution at the vertices of the coarse mesh; compared on the vertices of the coarse cells inside the domain
    u_fc = P.interpolate_nonmatching(coarse, fine, u_f)
    inside = np.unique(coarse.cells[coarse.cell_tag_values() == 1].reshape(-1))
    diff = u_fc[inside] - u_c[inside]
    print(f"RMS of interpolate_nonmatching(fine -> coarse) - u_coarse over {inside.size} vertices of cells tagged 1: "
          f"{np.sqrt(np.mean(diff ** 2)):.4e}  (max |u_coarse| = {np.abs(u_c[inside]).max():.4f})")
    for m, name in ((coarse, "coarse"), (fine, "fine")):
        print(f"locator of the {name} mesh: {P.locator_info(m)}, timings {m.timings()['locate']:.2e} s locate, "
              f"{m.timings()['evaluate']:.2e} s evaluate")

    # u_h along a line through the domain (from the tip of the left petal to the tip of the right one)
    t = np.linspace(0.0, 1.0, 11)
    line = np.stack([-3.4 + 6.8 * t, 0.3 * np.ones_like(t)], axis=1)
    vc, gc = P.evaluate(coarse, u_c, line, gradient=True)
    vf = P.evaluate(fine, u_f, line)
    print("   x        y      u_coarse     u_fine     d/dx u_coarse")
    for p, a, b, g in zip(line, vc, vf, gc):
        print(f"{p[0]:7.3f} {p[1]:7.3f}  {a:11.6f} {b:11.6f}  {g[0]:11.6f}")


if __name__ == "__main__":
    main()
