"""A posteriori error indicators of the weak-Dirichlet Poisson scheme and the Doerfler selection: host side of
phx_estimate_poisson_wd / phx_mark_dorfler (include/phifem_hip.h).  The reference has no counterpart:
dolfinx users write the residual forms in UFL.  Everything runs on the mesh's GPU; numpy in -> numpy out, tensor in ->
tensor out, as in `evaluate`."""
import ctypes as C

import numpy as np

from . import _lib as L
from .evaluate import _as_f64, _empty


def _check_space(mesh, degree):
    if degree not in (1, 2) or (degree == 2 and mesh.cell_type == "quadrilateral"):
        raise NotImplementedError("estimate: degree 1 on triangles, tetrahedra and rectangles, degree 2 on simplices")


def estimate(mesh, u, p, phi_h, f_h, u_D, degree=1, parts=False):
    """Residual indicator eta_T^2 per cell, shape (nc,), of the weak-Dirichlet Poisson scheme `PhiFEMSolver` solves, on
    the cell tags the mesh holds (call `compute_tags_measures` first).  With h_T the cell diameter and Omega_h the
    cells tagged 1 or 2, for T in Omega_h

        eta_T^2 = R_T + J_T + B_T
        R_T = h_T^2 int_T (f_h + Laplace u_h)^2
        J_T = 1/2 sum over the facets F of T towards a cell T' of Omega_h of h_F int_F [grad u_h . n]^2,
              h_F = (h_T + h_T') / 2
        B_T = h_T^-2 int_T (u_h - phi_h p_h / h_T - u_D)^2   on cells tagged 2, else 0

    and 0 outside Omega_h.  parts=True returns the three rows R, J, B as (3, nc).  This is the residual of the discrete
    scheme's own terms: an indicator for marking and for effectivity studies, NOT a proven two-sided bound.

    u, p, phi_h, f_h, u_D: nodal values of one `degree` in the layout `solve()` / `split()` / `evaluate` use (vertices,
    then edges at degree 2), numpy arrays or tensors on the mesh's GPU -- all of one kind, which is the kind of the
    result -- or NodalFunctions, whose degree must equal `degree`.  Degree 1 on triangles, tetrahedra and rectangles
    (Q1), degree 2 on simplices.  The same inputs give the same bits on every run.

    The three totals (sum R, sum J, sum B) of the LAST call are left in `estimate.last_sums` (a tuple of floats)."""
    from .mesh_scripts import NodalFunction
    _check_space(mesh, degree)
    ndofs = mesh.lagrange_ndofs(degree)
    arrs, kinds = [], set()
    for a, what in ((u, "u"), (p, "p"), (phi_h, "phi_h"), (f_h, "f_h"), (u_D, "u_D")):
        if isinstance(a, NodalFunction):
            if a.degree != degree:
                raise ValueError(f"estimate: {what} is a NodalFunction of degree {a.degree}, degree={degree} expected")
            a = a.values
        v, is_tensor = _as_f64(a, mesh, "estimate")
        if tuple(v.shape) != (ndofs,):
            raise ValueError(f"estimate: {what} of shape ({ndofs},) expected, got {tuple(v.shape)}")
        arrs.append(v)
        kinds.add(is_tensor)
    if len(kinds) != 1:
        raise ValueError("estimate: the five nodal arrays must all be numpy arrays or all tensors on the mesh's GPU")
    is_tensor = kinds.pop()
    out = _empty((3, mesh.nc), "float64", arrs[0], is_tensor)
    ptrs = [L.ptr(a) for a in arrs]
    po, lo = L.ptr(out)
    sums = (C.c_double * 3)()
    L.check(L.lib.phx_estimate_poisson_wd(mesh._h, degree, *(q[0] for q in ptrs), ptrs[0][1], po, lo, sums))
    estimate.last_sums = tuple(float(s) for s in sums)
    return out if parts else out[0] + out[1] + out[2]


estimate.last_sums = None


def mark_dorfler(mesh, eta2, theta=0.5):
    """Doerfler (bulk) marking: a uint8 mask of shape (nc,), of the kind of `eta2` (numpy, or a tensor on the mesh's
    GPU).  Order the cells by (eta2 descending, cell index ascending), let S_k be the inclusive sums in that order:
    marked are the first k* cells, k* the smallest k with S_k >= theta S_n.  Nothing is marked when all of eta2 is 0.
    theta outside (0, 1], or a negative, NaN or infinite entry, raise ValueError.  Sort, scan and mask run on the
    device; only the number of marked cells returns to the host (`mark_dorfler.last_count`)."""
    e, is_tensor = _as_f64(eta2, mesh, "mark_dorfler")
    if tuple(e.shape) != (mesh.nc,):
        raise ValueError(f"mark_dorfler: eta2 of shape ({mesh.nc},) expected, got {tuple(e.shape)}")
    if not (theta > 0.0 and theta <= 1.0):
        raise ValueError("mark_dorfler: theta must lie in (0, 1]")
    n = int(e.shape[0])
    marked = _empty((n,), "uint8", e, is_tensor)
    pe, le = L.ptr(e)
    pm, lm = L.ptr(marked)
    cnt = C.c_int64(0)
    L.check(L.lib.phx_mark_dorfler(mesh._h, n, pe, le, float(theta), pm, lm, C.byref(cnt)))
    mark_dorfler.last_count = int(cnt.value)
    return marked


mark_dorfler.last_count = None
