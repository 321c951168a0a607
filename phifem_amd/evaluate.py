"""Lagrange functions at arbitrary points (dolfinx `Function.eval` with a bounding-box tree, and
`interpolate_nonmatching`): host side of phx_locate_points / phx_eval_points (include/phifem_hip.h).
Everything runs on the mesh's GPU; numpy in -> numpy out, tensor in -> tensor out, as in `prolongate`."""
import ctypes as C

import numpy as np

from . import _lib as L


def _check_space(mesh, degree):
    if degree not in (1, 2) or (degree == 2 and mesh.cell_type == "quadrilateral"):
        raise NotImplementedError("evaluation: degree 1 on triangles, tetrahedra and rectangles, degree 2 on simplices")


def _as_f64(a, mesh, what):
    """(contiguous float64 array or tensor, is_tensor); a tensor has to live on the mesh's GPU."""
    if hasattr(a, "data_ptr"):
        import torch
        if not a.is_cuda or a.device.index != mesh.device:
            raise ValueError(f"{what}: a tensor has to live on the mesh's GPU")
        return a.to(torch.float64).contiguous(), True
    return np.ascontiguousarray(a, dtype=np.float64), False


def _empty(shape, dtype, like, is_tensor):
    if is_tensor:
        import torch
        return torch.empty(shape, dtype=getattr(torch, dtype), device=like.device)
    return np.empty(shape, dtype=dtype)


def _points(mesh, points, what):
    p, is_tensor = _as_f64(points, mesh, what)
    if p.ndim != 2 or p.shape[1] != mesh.gdim:
        raise ValueError(f"{what}: points of shape (npts, {mesh.gdim}) expected, got {tuple(p.shape)}")
    return p, is_tensor


def locate(mesh, points, tol=1e-12):
    """(cells, xref) of `points` (npts, gdim): cells int32, -1 where no cell holds the point; xref (npts, tdim) the
    reference coordinates in that cell -- simplices lambda_1 .. lambda_d of the stored vertex order (lambda_0 =
    1 - sum), rectangles (xi, eta) -- unspecified where cells is -1.  A cell holds a point when every barycentric
    coordinate is >= -tol; of several such cells the one with the smallest index is returned (generated boxes: the
    closed-form rule of include/phifem_hip.h)."""
    if not tol >= 0.0:
        raise ValueError("locate: tol must be >= 0")
    p, is_tensor = _points(mesh, points, "locate")
    npts = p.shape[0]
    cells = _empty((npts,), "int32", p, is_tensor)
    xref = _empty((npts, mesh.tdim), "float64", p, is_tensor)
    pp, lp = L.ptr(p)
    pc, lo = L.ptr(cells)
    px, _ = L.ptr(xref)
    L.check(L.lib.phx_locate_points(mesh._h, npts, pp, lp, float(tol), pc, px, lo))
    return cells, xref


def evaluate(mesh, values, points, degree=1, gradient=False, fill=float("nan"), tol=1e-12, located=None):
    """The Lagrange function of `degree` with the nodal `values` -- (ndofs,) or (ncomp, ndofs) in the layout `solve()`
    and `split()` return, or a NodalFunction, whose degree is used -- at `points`: (npts,) or (ncomp, npts), with
    gradient=True also the physical gradient in the returned cell, (npts, gdim) or (ncomp, npts, gdim).  Points no
    cell holds get `fill`.  located=(cells, xref) from `locate` skips the search (many functions at one point set).
    The result is of the kind of `points` (numpy or a tensor on the mesh's GPU)."""
    from .mesh_scripts import NodalFunction
    if isinstance(values, NodalFunction):
        values, degree = values.values, values.degree
    _check_space(mesh, degree)
    if not tol >= 0.0:
        raise ValueError("evaluate: tol must be >= 0")
    p, is_tensor = _points(mesh, points, "evaluate")
    npts = p.shape[0]
    v, _ = _as_f64(values, mesh, "evaluate")
    ndofs = mesh.lagrange_ndofs(degree)
    shape = tuple(v.shape)
    if len(shape) not in (1, 2) or shape[-1] != ndofs or (len(shape) == 2 and shape[0] == 0):
        raise ValueError(f"evaluate: expected {ndofs} values per component, got shape {shape}")
    ncomp = 1 if len(shape) == 1 else shape[0]
    if located is None:
        cells, xref = locate(mesh, p, tol)
    else:
        cells, xref = located
        for a, want, what in ((cells, (npts,), "cells"), (xref, (npts, mesh.tdim), "xref")):
            if tuple(a.shape) != want:
                raise ValueError(f"evaluate: located {what} of shape {want} expected, got {tuple(a.shape)}")
        if hasattr(cells, "data_ptr"):
            import torch
            if not cells.is_cuda or cells.device.index != mesh.device or not xref.is_cuda or xref.device != cells.device:
                raise ValueError("evaluate: located tensors have to live on the mesh's GPU")
            cells, xref = cells.to(torch.int32).contiguous(), xref.to(torch.float64).contiguous()
        else:
            cells = np.ascontiguousarray(cells, dtype=np.int32)
            xref = np.ascontiguousarray(xref, dtype=np.float64)
        if hasattr(cells, "data_ptr") != hasattr(xref, "data_ptr"):
            raise ValueError("evaluate: located cells and xref have to be of one kind")
    out = _empty(shape[:-1] + (npts,), "float64", p, is_tensor)
    grad = _empty(shape[:-1] + (npts, mesh.gdim), "float64", p, is_tensor) if gradient else None
    pv, lv = L.ptr(v)
    pc, lc = L.ptr(cells)
    px, _ = L.ptr(xref)
    po, lo = L.ptr(out)
    pg, _ = L.ptr(grad)
    L.check(L.lib.phx_eval_points(mesh._h, degree, ncomp, pv, lv, npts, pc, px, lc, int(bool(gradient)), float(fill),
                                  po, pg, lo))
    return (out, grad) if gradient else out


def interpolate_nonmatching(dst_mesh, src_mesh, values, degree=1, fill=float("nan")):
    """The degree-`degree` function `values` on `src_mesh` at the Lagrange DoF points of `dst_mesh` (any two meshes
    on one GPU, nested or not): `evaluate(src_mesh, values, dst_mesh.lagrange_dof_points(degree, device=True),
    degree)`.  Nothing returns to the host when `values` is a tensor; numpy values give a numpy result."""
    from .mesh_scripts import NodalFunction
    if isinstance(values, NodalFunction):
        return NodalFunction(interpolate_nonmatching(dst_mesh, src_mesh, values.values, values.degree, fill),
                             values.degree)
    _check_space(src_mesh, degree)
    _check_space(dst_mesh, degree)
    if dst_mesh.gdim != src_mesh.gdim or dst_mesh.device != src_mesh.device:
        raise ValueError("interpolate_nonmatching: the meshes have to share the dimension and the GPU")
    pts = dst_mesh.lagrange_dof_points(degree, device=True)
    if hasattr(values, "data_ptr"):
        return evaluate(src_mesh, values, pts, degree, fill=fill)
    import torch
    v = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(pts.device)
    return evaluate(src_mesh, v, pts, degree, fill=fill).cpu().numpy()


def locator_info(mesh):
    """What `phx_locator_info` reports: the path point location takes on this mesh and the size of its bins."""
    info = (C.c_int64 * 8)()
    L.check(L.lib.phx_locator_info(mesh._h, info))
    return {"path": {1: "closed-form", 2: "bins"}[int(info[0])], "bins": tuple(int(v) for v in info[1:1 + mesh.gdim]),
            "pairs": int(info[4]), "bytes": int(info[5]), "halvings": int(info[6]), "built": bool(info[7])}
