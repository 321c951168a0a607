"""Gradient recovery and the recovery-based (Zienkiewicz-Zhu) error indicator: host side of phx_recover_gradient
(include/phifem_hip.h).  The reference has no counterpart (dolfinx users project the gradient with a mass
solve).  Needs nothing of the formulation but u_h, so it serves every solver of this package.  Everything runs on the
mesh's GPU; numpy in -> numpy out, tensor in -> tensor out, as in `evaluate` and `estimate`."""
import ctypes as C

import numpy as np

from . import _lib as L
from .evaluate import _as_f64, _empty


def _check_space(mesh, degree):
    if degree not in (1, 2) or (degree == 2 and mesh.cell_type == "quadrilateral"):
        raise NotImplementedError("recover_gradient: degree 1 on triangles, tetrahedra and rectangles, degree 2 on "
                                  "simplices")


def _mask(mesh, cells, is_tensor, what):
    """The uint8 mask of the kind of the values (None: Omega_h from the mesh's tags; the library refuses a mesh
    without tags with the ValueError that names compute_tags_measures)."""
    if cells is None:
        return None
    if hasattr(cells, "data_ptr") != is_tensor:
        raise ValueError(f"{what}: the values and the cell mask must both be numpy arrays or both tensors on the mesh's GPU")
    if is_tensor:
        import torch
        if not cells.is_cuda or cells.device.index != mesh.device:
            raise ValueError(f"{what}: a tensor has to live on the mesh's GPU")
        mask = cells.to(torch.uint8).contiguous()
    else:
        mask = np.ascontiguousarray(cells, dtype=np.uint8)
    if tuple(mask.shape) != (mesh.nc,):
        raise ValueError(f"{what}: a cell mask of shape ({mesh.nc},) expected, got {tuple(mask.shape)}")
    return mask


def _run(mesh, u, degree, cells, want_eta, what):
    from .mesh_scripts import NodalFunction
    if isinstance(u, NodalFunction):
        if u.degree != degree:
            raise ValueError(f"{what}: u is a NodalFunction of degree {u.degree}, degree={degree} expected")
        u = u.values
    _check_space(mesh, degree)
    v, is_tensor = _as_f64(u, mesh, what)
    ndofs = mesh.lagrange_ndofs(degree)
    shape = tuple(v.shape)
    if len(shape) not in (1, 2) or shape[-1] != ndofs or (len(shape) == 2 and shape[0] == 0):
        raise ValueError(f"{what}: expected {ndofs} values per component, got shape {shape}")
    ncomp = 1 if len(shape) == 1 else shape[0]
    mask = _mask(mesh, cells, is_tensor, what)
    grad = _empty(shape[:-1] + (mesh.nv, mesh.gdim), "float64", v, is_tensor)
    eta2 = _empty((mesh.nc,), "float64", v, is_tensor) if want_eta else None
    pv, lv = L.ptr(v)
    pm, lm = L.ptr(mask)
    pg, lo = L.ptr(grad)
    pe, _ = L.ptr(eta2)
    total = C.c_double(0.0)
    L.check(L.lib.phx_recover_gradient(mesh._h, degree, ncomp, pv, lv, pm, lm, pg, pe, lo,
                                       C.byref(total) if want_eta else None))
    return grad, eta2, float(total.value)


def recover_gradient(mesh, u, degree=1, cells=None):
    """The recovered gradient G of the Lagrange function with the nodal values `u` as a nodal (vertex) field: shape
    (nv, gdim) for u of shape (ndofs,), (ncomp, nv, gdim) for (ncomp, ndofs) -- the layout `evaluate` takes, vertices
    first, then edges at degree 2 -- or for a NodalFunction, whose degree must equal `degree`.

        G(v) = sum_{T in S_v} |T| grad u_h|_T (x_v) / sum_{T in S_v} |T|,     exactly 0 where S_v is empty,

    S_v the selected cells that contain the vertex v, |T| the cell volume, grad u_h|_T (x_v) the gradient of T's own
    polynomial at its corner v.  `cells`: a uint8 mask of shape (nc,) of the kind of `u` (numpy, or a tensor on the
    mesh's GPU) selects S; None selects the cells tagged 1 or 2 on the tags the mesh holds (`compute_tags_measures`
    first).  Degree 1 on triangles, tetrahedra and rectangles (Q1), degree 2 on simplices; G is P1 / Q1 in every case.

    A post-processed flux, not a proven approximation order everywhere: on vertices at the rim of S the star is
    one-sided and G is only first-order accurate there.  The same inputs give the same bits on every run."""
    return _run(mesh, u, degree, cells, False, "recover_gradient")[0]


def estimate_zz(mesh, u, degree=1, cells=None, gradient=False):
    """Recovery-based (Zienkiewicz-Zhu) indicator per cell, shape (nc,):

        eta_T^2 = sum over the components c of int_T |G_h,c - grad u_h,c|^2   for T in S,    exactly 0 otherwise,

    G_h the P1 / Q1 interpolant of `recover_gradient(mesh, u, degree, cells)`; the integrals are closed forms, exact
    for both degrees.  Arguments as `recover_gradient`; gradient=True returns (eta2, G).  The total of the LAST call is
    left in `estimate_zz.last_sum`.

    It needs nothing of the formulation but u_h, so it marks for every solver here (`mark_dorfler`, `refine(marked=)`).
    It is an indicator for marking: NEITHER a proven bound of the error NOR the residual of any scheme, and on vertices
    at the rim of S the one-sided star makes G first-order accurate only."""
    grad, eta2, total = _run(mesh, u, degree, cells, True, "estimate_zz")
    estimate_zz.last_sum = total
    return (eta2, grad) if gradient else eta2


estimate_zz.last_sum = None
