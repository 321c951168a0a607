"""Partition of an unstructured background mesh over ranks: host side of `phx_partition_cells`,
`phx_partition_layout` and `phx_submesh_create_from_flags`.

Every rank holds the whole mesh and calls these redundantly; the device code is deterministic to the bit, so all
ranks see the same partition without exchanging it.  Arrays go in and come out where they are handed over: numpy
on the host, torch tensors on the mesh's GPU.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .mesh import Mesh


def _on_device(a):
    return a is not None and hasattr(a, "data_ptr") and a.is_cuda


def _check_tensor(t, dtype, n, what):
    if t.dtype != dtype or not t.is_contiguous() or t.numel() != n:
        raise ValueError(f"{what}: a contiguous {dtype} tensor of {n} values is expected")


def partition_cells(mesh, nparts, weights=None):
    """Part (int32, 0 .. nparts - 1) of every cell: recursive coordinate bisection of the cell centroids, balanced by
    `weights` (non-negative int32 per cell, None = all ones).  The rules are spelled out at `phx_partition_cells`
    (include/phifem_hip.h) and restated in numpy in tests/partition_ref.py."""
    if mesh.cell_type not in ("triangle", "tetrahedron"):
        raise NotImplementedError("the partitioner serves triangles and tetrahedra")
    if _on_device(weights):
        import torch
        _check_tensor(weights, torch.int32, mesh.nc, "weights")
        out = torch.empty(mesh.nc, dtype=torch.int32, device=weights.device)
        L.check(L.lib.phx_partition_cells(mesh._h, int(nparts), L.ptr(weights)[0], C.c_void_p(out.data_ptr()), L.DEVICE))
        return out
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.int32)
        if w.shape != (mesh.nc,):
            raise ValueError(f"weights has shape {w.shape}, the mesh has {mesh.nc} cells")
    out = np.empty(mesh.nc, dtype=np.int32)
    L.check(L.lib.phx_partition_cells(mesh._h, int(nparts), None if w is None else w.ctypes.data_as(C.c_void_p),
                                      out.ctypes.data_as(C.c_void_p), L.HOST))
    return out


def partition_layout(mesh, nparts, part, rank):
    """(owner int32 [nv], flags uint8 [nc]) of `rank` on the TAGGED mesh: the owning part of every vertex (-1: none)
    and the local cells of the rank, flagged with the layer that takes them: 1 (a vertex is owned), 2 (facet neighbour
    of layer 1: the owned rows are complete), 3 / 4 (the same once more: the diagonals of the columns those rows refer
    to are complete), 0 = not local."""
    if _on_device(part):
        import torch
        _check_tensor(part, torch.int32, mesh.nc, "part")
        owner = torch.empty(mesh.nv, dtype=torch.int32, device=part.device)
        flags = torch.empty(mesh.nc, dtype=torch.uint8, device=part.device)
        L.check(L.lib.phx_partition_layout(mesh._h, int(nparts), L.ptr(part)[0], int(rank),
                                           C.c_void_p(owner.data_ptr()), C.c_void_p(flags.data_ptr()), L.DEVICE))
        return owner, flags
    p = np.ascontiguousarray(part, dtype=np.int32)
    if p.shape != (mesh.nc,):
        raise ValueError(f"part has shape {p.shape}, the mesh has {mesh.nc} cells")
    owner = np.empty(mesh.nv, dtype=np.int32)
    flags = np.empty(mesh.nc, dtype=np.uint8)
    L.check(L.lib.phx_partition_layout(mesh._h, int(nparts), p.ctypes.data_as(C.c_void_p), int(rank),
                                       owner.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p), L.HOST))
    return owner, flags


def local_mesh(mesh, flags):
    """(local Mesh, c_map, v_map) of the cells with flags != 0: a box-mode mesh that carries the parent's cell and facet
    tags; c_map / v_map (int32, ascending) give the parent cell / vertex of every local one."""
    h = C.c_void_p()
    if _on_device(flags):
        import torch
        _check_tensor(flags, torch.uint8, mesh.nc, "flags")
        L.check(L.lib.phx_submesh_create_from_flags(mesh._h, L.ptr(flags)[0], L.DEVICE, C.byref(h)))
    else:
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        if f.shape != (mesh.nc,):
            raise ValueError(f"flags has shape {f.shape}, the mesh has {mesh.nc} cells")
        L.check(L.lib.phx_submesh_create_from_flags(mesh._h, f.ctypes.data_as(C.c_void_p), L.HOST, C.byref(h)))
    sub = Mesh(h, device=mesh.device)
    c_map = np.empty(sub.nc, dtype=np.int32)
    v_map = np.empty(sub.nv, dtype=np.int32)
    L.check(L.lib.phx_submesh_maps(sub._h, c_map.ctypes.data_as(C.c_void_p), v_map.ctypes.data_as(C.c_void_p)))
    return sub, c_map, v_map
