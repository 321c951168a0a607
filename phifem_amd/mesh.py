"""Mesh handle resident in HBM + MeshTags view (host side of the C ABI)."""
import ctypes as C

import weakref

import numpy as np

from . import _lib as L


class MeshTags:
    """The part of dolfinx.mesh.MeshTags the reference relies on
    (src/phifem/mesh_scripts.py:386-388,425-427,562-567): `.indices` (int32, strictly
    increasing), `.values` (int32), `.dim`, `.find(v)`."""

    def __init__(self, dim, indices, values):
        self.dim = int(dim)
        self.indices = np.ascontiguousarray(indices, dtype=np.int32)
        self.values = np.ascontiguousarray(values, dtype=np.int32)
        if self.indices.size > 1 and np.any(np.diff(self.indices) <= 0):
            raise ValueError("MeshTags entities must be sorted and unique")

    def find(self, v):
        return self.indices[self.values == v]


class LazyMeshTags(MeshTags):
    """MeshTags whose host arrays are fetched from the device on first use.  The tags of a 256^3 box are 3e8 bytes
    on the device; `compute_tags_measures` must return MeshTags objects (src/phifem/mesh_scripts.py:647-653), but a
    caller that goes on to assemble and solve never looks at them.  The mesh flushes every outstanding object
    before its tags change again (`Mesh._flush_lazy_tags`), so what is read is always the state at creation."""

    def __init__(self, dim, mesh, facets):
        self.dim = int(dim)
        self._mesh, self._facets = mesh, facets
        self._idx = self._val = None
        mesh._lazy_tags.add(self)

    def _load(self):
        if self._idx is None:
            m = self._mesh
            vals = m.facet_tag_values() if self._facets else m.cell_tag_values()
            idx = np.flatnonzero(vals > 0).astype(np.int32)
            self._idx, self._val = idx, np.ascontiguousarray(vals[idx], dtype=np.int32)
            self._mesh = None

    @property
    def indices(self):
        self._load()
        return self._idx

    @property
    def values(self):
        self._load()
        return self._val


class Mesh:
    """Owns a `phx_mesh*`.  Arrays stay on the GPU; accessors copy on demand."""

    def __init__(self, handle, parent=None, device=None):
        self._h = C.c_void_p(handle) if not isinstance(handle, C.c_void_p) else handle
        self.parent = parent
        self._lazy_tags = weakref.WeakSet()
        self._tag_generation = 0        # bumped by every Python entry that changes the tags of this mesh
        self.device = int(device) if device is not None else (parent.device if parent is not None else 0)
        cnt = (C.c_int64 * 6)()
        L.check(L.lib.phx_mesh_counts(self._h, cnt))
        self.gdim, ct, self.nv, self.nc, self.nf, self.nbf = (int(v) for v in cnt)
        self.cell_type = L.CELL_NAMES[ct]
        self.tdim = self.gdim
        self.nvpc = {"triangle": 3, "quadrilateral": 4, "tetrahedron": 4}[self.cell_type]
        self.nfpc = self.nvpc

    # --- construction -------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, cell_type, x, cells, device=0):
        """Unstructured mesh (stands in for XDMFFile.read_mesh,
        tests/test_compute_meshtags.py:136-137).  Quadrilaterals in tensor-product order."""
        if cell_type not in L.CELL_TYPES:
            raise NotImplementedError(
                "Mesh tags computation does not support other cell types than "
                "'triangle', 'quadrilateral' or 'tetrahedron'")  # mesh_scripts.py:326-329
        x = np.ascontiguousarray(x, dtype=np.float64)
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        h = C.c_void_p()
        L.check(L.lib.phx_mesh_create(x.shape[1], L.CELL_TYPES[cell_type], x.shape[0],
                                      x.ctypes.data_as(C.c_void_p), cells.shape[0],
                                      cells.ctypes.data_as(C.c_void_p), device, C.byref(h)))
        return cls(h, device=device)

    def __del__(self):
        try:
            if self._h:
                L.lib.phx_mesh_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # --- accessors ----------------------------------------------------------------------
    def _flush_lazy_tags(self):
        """Materialise the MeshTags handed out so far.  Called by every Python entry that is about to change the
        tags of this mesh (`_tag_cells`, `_tag_facets`, the overwrite path), so a MeshTags object always shows
        the state it was created in; callers that change tags through the raw C ABI call it themselves."""
        self._tag_generation += 1
        for t in list(self._lazy_tags):
            t._load()

    def _get(self, which, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        L.check(L.lib.phx_mesh_get_array(self._h, which, out.ctypes.data_as(C.c_void_p), L.HOST))
        return out

    @property
    def x(self):
        return self._get(L.ARR_COORDS, (self.nv, self.gdim), np.float64)

    @property
    def cells(self):
        return self._get(L.ARR_CELLS, (self.nc, self.nvpc), np.int32)

    @property
    def c2f(self):
        return self._get(L.ARR_C2F, (self.nc, self.nfpc), np.int32)

    @property
    def f2c(self):
        return self._get(L.ARR_F2C, (self.nf, 2), np.int32)

    @property
    def boundary_facets(self):
        """(cell, local facet) of the background-boundary facets, ascending facet index."""
        return self._get(L.ARR_BFACETS, (self.nbf, 2), np.int32)

    @property
    def ne(self):
        n = C.c_int64(0)
        L.check(L.lib.phx_mesh_edge_count(self._h, C.byref(n)))
        return n.value

    @property
    def c2e(self):
        """cell -> edges (basix local edge order); builds the edge numbering on first use."""
        nepc = 6 if self.cell_type == "tetrahedron" else 3
        self.ne
        return self._get(L.ARR_C2E, (self.nc, nepc), np.int32)

    @property
    def edges(self):
        """(ne, 2) vertex pairs, ascending."""
        return self._get(L.ARR_EDGES, (self.ne, 2), np.int32)

    def p2_dof_points(self):
        """Coordinates of the P2 nodes: the vertices, then the edge midpoints."""
        x, e = self.x, self.edges
        return np.concatenate([x, 0.5 * (x[e[:, 0]] + x[e[:, 1]])], axis=0)

    def q2_dof_points(self):
        """Coordinates of the Q2 nodes of a quadrilateral mesh: the vertices, the edge midpoints in FACET order,
        the cell centres (the nodal layout `NeumannRobinSolver` and `NodalFunction(degree=2)` use on quadrilaterals)."""
        if self.cell_type != "quadrilateral":
            raise ValueError("q2_dof_points is for quadrilateral meshes")
        x, cells, c2f = self.x, self.cells, self.c2f
        fverts = np.empty((self.nf, 2), dtype=np.int64)
        lfv = np.array([[0, 1], [0, 2], [1, 3], [2, 3]])       # local facet -> local vertices (tensor-product order)
        for lf in range(4):
            fverts[c2f[:, lf]] = cells[:, lfv[lf]]
        return np.concatenate([x, 0.5 * (x[fverts[:, 0]] + x[fverts[:, 1]]), x[cells].mean(axis=1)], axis=0)

    def lagrange_ndofs(self, degree):
        """Number of global DoFs of a degree-1/2/3 Lagrange function in the library's layout (`NodalFunction`)."""
        if degree not in (1, 2, 3):
            raise NotImplementedError("Lagrange functions of degree 1, 2 and 3 are implemented")
        if degree == 1:
            return self.nv
        if self.cell_type == "quadrilateral":
            return self.nv + self.nf + self.nc if degree == 2 else self.nv + 2 * self.nf + 4 * self.nc
        if degree == 2:
            return self.nv + self.ne
        return self.nv + 2 * self.ne + (self.nc if self.cell_type == "triangle" else self.nf)

    def _facet_vertices(self):
        """(nf, nvpf) global vertices of every facet, ascending (read from the facet's first cell)."""
        from .mesh_scripts import _FACET_VERTS
        cells, c2f, f2c = self.cells, self.c2f, self.f2c
        c0 = f2c[:, 0]
        lf = np.argmax(c2f[c0] == np.arange(self.nf)[:, None], axis=1)
        return np.sort(cells[c0[:, None], _FACET_VERTS[self.cell_type][lf]], axis=1)

    def lagrange_dof_points(self, degree, device=False):
        """Coordinates (ndofs, gdim) of the global DoFs of a degree-1/2/3 Lagrange function, in the layout of
        `NodalFunction` -- the points `interpolate` evaluates at.  device=False: numpy, computed here (the readable
        statement of the formulas); device=True: a float64 tensor on the mesh's GPU from `phx_lagrange_dof_points`,
        bit for bit the same numbers.  Formulas (include/phifem_hip.h; A, B = (1 -+ 1/sqrt5)/2):
          edge / facet pair of (p < q):  B x_p + A x_q, then A x_p + B x_q  (degree 2: 0.5 x_p + 0.5 x_q)
          triangle centroid:             ((x_0 + x_1) + x_2) / 3, face centroid of (p < q < r): ((x_p + x_q) + x_r) / 3
          quadrilateral interior nodes:  bilinear map at (A,A), (B,A), (A,B), (B,B) (degree 2: at (1/2, 1/2))."""
        n = self.lagrange_ndofs(degree)
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            out = torch.empty((n, self.gdim), dtype=torch.float64, device=dev)
            L.sync_torch_stream(dev)
            L.check(L.lib.phx_lagrange_dof_points(self._h, degree, C.c_void_p(out.data_ptr())))
            return out
        x = self.x
        if degree == 1:
            return x
        A = (1.0 - 1.0 / np.sqrt(5.0)) / 2.0
        B = (1.0 + 1.0 / np.sqrt(5.0)) / 2.0
        quad = self.cell_type == "quadrilateral"
        pairs = self._facet_vertices() if quad else self.edges
        xp, xq = x[pairs[:, 0]], x[pairs[:, 1]]
        if degree == 2:
            edge_nodes = 0.5 * xp + 0.5 * xq
        else:
            edge_nodes = np.stack([B * xp + A * xq, A * xp + B * xq], axis=1).reshape(-1, self.gdim)
        parts = [x, edge_nodes]
        cells = self.cells
        if quad:
            xc = x[cells]                                   # (nc, 4, gdim)
            ts = [(0.5, 0.5)] if degree == 2 else [(B, A), (A, B)]      # 1-D weights (1 - xi, xi)
            nodes = []
            order = [(0, 0)] if degree == 2 else [(0, 0), (1, 0), (0, 1), (1, 1)]
            for i, j in order:
                u0, u1 = ts[i]
                w0, w1 = ts[j]
                n0, n1, n2, n3 = u0 * w0, u1 * w0, u0 * w1, u1 * w1
                nodes.append(((n0 * xc[:, 0] + n1 * xc[:, 1]) + n2 * xc[:, 2]) + n3 * xc[:, 3])
            parts.append(np.stack(nodes, axis=1).reshape(-1, self.gdim))
        elif degree == 3 and self.cell_type == "triangle":
            parts.append(((x[cells[:, 0]] + x[cells[:, 1]]) + x[cells[:, 2]]) / 3.0)
        elif degree == 3:
            fv = self._facet_vertices()
            parts.append(((x[fv[:, 0]] + x[fv[:, 1]]) + x[fv[:, 2]]) / 3.0)
        return np.ascontiguousarray(np.concatenate(parts, axis=0))

    def refine(self, marked=None, edges=None):
        """Uniform regular refinement, or marked refinement with a cell / edge mask (`phifem_amd.refine`)."""
        return refine(self, marked=marked, edges=edges)

    @property
    def parent_cells(self):
        """Meshes made by `refine(mesh, marked=..)`: (nc,) int32, the coarse cell every cell lies in."""
        return self._get(L.ARR_PARENT_CELLS, (self.nc,), np.int32)

    @property
    def child_nodes(self):
        """Meshes made by `refine(mesh, marked=..)`: (nc, nvpc) int8, every cell as local degree-2 nodes of its
        parent (0 .. nvpc-1 the parent's vertices, nvpc + k the midpoint of its local edge k)."""
        return self._get(L.ARR_CHILD_NODES, (self.nc, self.nvpc), np.int8)

    def cell_tag_values(self):
        return self._get(L.ARR_CELL_TAGS, (self.nc,), np.int32)

    def facet_tag_values(self):
        return self._get(L.ARR_FACET_TAGS, (self.nf,), np.int32)

    def synchronize(self):
        L.check(L.lib.phx_mesh_synchronize(self._h))

    def timings(self):
        t = (C.c_double * 8)()
        L.check(L.lib.phx_last_timings(self._h, t))
        tl = (C.c_double * 3)()      # point location and evaluation (phifem_amd.evaluate): wall seconds of the last calls
        L.check(L.lib.phx_locate_timings(self._h, tl))
        return {"tag_cells": t[0], "tag_facets": t[1], "assemble": t[2], "solve": t[3],
                "spmv_avg": t[4], "refine_kernels": t[6], "refine_create": t[7],
                "locate_build": tl[0], "locate": tl[1], "evaluate": tl[2]}


def create_box(lo, hi, n, device=0, offset=None, n_global=None):
    """Kuhn simplicial box generated on the device (dolfinx.mesh.create_box / create_rectangle,
    demo/weak-dirichlet/flower/main.py:45-46)."""
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    n = np.ascontiguousarray(n, dtype=np.int64)
    gdim = lo.size
    off = None if offset is None else np.ascontiguousarray(offset, dtype=np.int64)
    ng = None if n_global is None else np.ascontiguousarray(n_global, dtype=np.int64)
    h = C.c_void_p()
    L.check(L.lib.phx_mesh_create_box(
        gdim, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p),
        n.ctypes.data_as(C.c_void_p),
        None if off is None else off.ctypes.data_as(C.c_void_p),
        None if ng is None else ng.ctypes.data_as(C.c_void_p), device, C.byref(h)))
    return Mesh(h, device=device)


def create_rectangle(bbox, n, device=0, cell_type="triangle"):
    """dolfinx.mesh.create_rectangle(comm, [[x0,y0],[x1,y1]], [nx,ny], cell_type): triangles with diagonal
    'right' (the generated box), or quadrilaterals in dolfinx's tensor-product vertex and cell order
    (vertex j (nx + 1) + i at (x_i, y_j); cell vertices v0 (0,0), v1 (1,0), v2 (0,1), v3 (1,1))."""
    if cell_type == "triangle":
        return create_box(bbox[0], bbox[1], n, device=device)
    if cell_type != "quadrilateral":
        raise ValueError("cell_type can only be 'triangle' or 'quadrilateral'")
    (x0, y0), (x1, y1) = bbox
    nx, ny = int(n[0]), int(n[1])
    X, Y = np.meshgrid(np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1), indexing="xy")
    x = np.stack([X.reshape(-1), Y.reshape(-1)], axis=1)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    v0 = (j * (nx + 1) + i).reshape(-1)
    cells = np.stack([v0, v0 + 1, v0 + nx + 1, v0 + nx + 2], axis=1).astype(np.int32)
    return Mesh.from_arrays("quadrilateral", x, cells, device=device)


def _mask_u8(mask, n, mesh, what):
    """A cell / edge mask as contiguous uint8 of length n: numpy array or tensor on the mesh's GPU."""
    if hasattr(mask, "data_ptr"):
        import torch
        if not mask.is_cuda or mask.device.index != mesh.device:
            raise ValueError(f"refine: the {what} mask has to be a numpy array or a tensor on the mesh's GPU")
        m = (mask != 0).to(torch.uint8).contiguous()
    else:
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    if tuple(m.shape) != (n,):
        raise ValueError(f"refine: {what} mask of shape ({n},) expected, got {tuple(m.shape)}")
    return m


def _refine_marked(mesh, marked, edges):
    if mesh.cell_type == "quadrilateral":
        raise NotImplementedError("marked refinement of quadrilaterals is not implemented (it needs hanging nodes)")
    cm = None if marked is None else _mask_u8(marked, mesh.nc, mesh, "cell")
    em = None if edges is None else _mask_u8(edges, mesh.ne, mesh, "edge")
    kinds = {hasattr(a, "data_ptr") for a in (cm, em) if a is not None}
    if len(kinds) == 2:                         # one location flag crosses the C ABI: bring the numpy mask over
        import torch
        cm, em = (a if hasattr(a, "data_ptr") else torch.from_numpy(a).cuda(mesh.device) for a in (cm, em))
    pc, loc = L.ptr(cm)
    pe, loce = L.ptr(em)
    h = C.c_void_p()
    info = (C.c_int64 * 3)()
    L.check(L.lib.phx_mesh_refine_marked(mesh._h, pc, pe, loc if cm is not None else loce, C.byref(h), info))
    fine = Mesh(h, device=mesh.device)
    fine.coarse = mesh
    fine.nchild = None                          # the child count varies: see parent_cells
    fine.refine_info = (int(info[0]), int(info[1]), int(info[2]))
    return fine


def refine(mesh, marked=None, edges=None):
    """`refine(mesh)`: uniform regular refinement, as below.  `refine(mesh, marked=cell mask, edges=edge mask)`, either
    or both: marked refinement of a triangle or tetrahedron mesh by longest-edge bisection with closure (the rule of
    include/phifem_hip.h / DESIGN.md 7e; dolfinx.mesh.refine(mesh, edges)).  The masks are what `mark_dorfler` returns:
    numpy arrays or tensors on the mesh's GPU, (nc,) over the cells and (ne,) over `mesh.edges`, non-zero = marked.
    The result is an ordinary untagged mesh with `fine.coarse`, `fine.parent_cells`, `fine.child_nodes`,
    `fine.refine_info` = (marked edges after the closure, closure sweeps, fine cells) and `fine.nchild = None`;
    `prolongate` works on it.

    Uniform regular refinement on the device (dolfinx.mesh.refine(mesh)[0], demo/interface-elasticity/main.py:390):
    every triangle into 4, every tetrahedron into 8 (Bey's rule on the stored vertex order), every quadrilateral
    into 4.  The fine vertices are `mesh.lagrange_dof_points(2)` in that order, child k of cell c is fine cell
    nchild * c + k (include/phifem_hip.h states the child tables).  The result is an ordinary untagged mesh --
    `parent` stays None, it is no sub-mesh -- that carries `fine.coarse` (the mesh it came from, kept alive) and
    `fine.nchild`."""
    if marked is not None or edges is not None:
        return _refine_marked(mesh, marked, edges)
    h = C.c_void_p()
    L.check(L.lib.phx_mesh_refine(mesh._h, C.byref(h)))
    fine = Mesh(h, device=mesh.device)
    fine.coarse = mesh
    fine.nchild = fine.nc // mesh.nc
    return fine


def prolongate(fine, values, degree=1):
    """The Lagrange function of `degree` given by `values` on `fine.coarse`, expressed on `fine` (the spaces are nested:
    the same function).  `values`: a NodalFunction (its degree is used), a numpy array or a tensor on the mesh's GPU,
    of shape (ndofs,) or (ncomp, ndofs) in the layout `solve()` returns; the result is of the same kind and shape on
    the fine mesh.  Degree 1 on all cell types, degree 2 on simplices."""
    from .mesh_scripts import NodalFunction
    coarse = getattr(fine, "coarse", None)
    if coarse is None:
        raise ValueError("prolongate: the mesh was not produced by refine()")
    if isinstance(values, NodalFunction):
        return NodalFunction(prolongate(fine, values.values, values.degree), values.degree)
    if degree not in (1, 2) or (degree == 2 and coarse.cell_type == "quadrilateral"):
        raise NotImplementedError("prolongation: degree 1 on every cell type, degree 2 on simplices")
    nin, nout = coarse.lagrange_ndofs(degree), fine.lagrange_ndofs(degree)
    is_tensor = hasattr(values, "data_ptr")
    if is_tensor:
        import torch
        if not values.is_cuda or values.device.index != fine.device:
            raise ValueError("prolongate: a tensor has to live on the mesh's GPU")
        v = values.to(torch.float64).contiguous()
    else:
        v = np.ascontiguousarray(values, dtype=np.float64)
    shape = tuple(v.shape)
    if len(shape) not in (1, 2) or shape[-1] != nin:
        raise ValueError(f"prolongate: expected {nin} values per component, got shape {shape}")
    ncomp = 1 if len(shape) == 1 else shape[0]
    oshape = shape[:-1] + (nout,)
    if ncomp == 0:
        raise ValueError("prolongate: no component")
    out = torch.empty(oshape, dtype=torch.float64, device=v.device) if is_tensor else np.empty(oshape)
    pi, li = L.ptr(v)
    po, lo = L.ptr(out)
    L.check(L.lib.phx_prolongate(coarse._h, fine._h, degree, ncomp, pi, li, po, lo))
    return out


def restrict(fine, values, degree=1):
    """The transpose of `prolongate`: `values` on `fine` -> values on `fine.coarse`, with <restrict(r), x> =
    <r, prolongate(x)>.  It maps residuals (functionals), not functions.  `values`: a numpy array or a tensor on the
    mesh's GPU, of shape (nv,) or (ncomp, nv) of the fine mesh; the result is of the same kind on the coarse mesh.
    Degree 1 on triangles and tetrahedra, after uniform and after marked refinement.  The additions run in a stated
    order (include/phifem_hip.h): the same bits on every run."""
    coarse = getattr(fine, "coarse", None)
    if coarse is None:
        raise ValueError("restrict: the mesh was not produced by refine()")
    if degree != 1 or coarse.cell_type == "quadrilateral":
        raise NotImplementedError("restriction: degree 1 on triangles and tetrahedra")
    nin, nout = fine.nv, coarse.nv
    is_tensor = hasattr(values, "data_ptr")
    if is_tensor:
        import torch
        if not values.is_cuda or values.device.index != fine.device:
            raise ValueError("restrict: a tensor has to live on the mesh's GPU")
        v = values.to(torch.float64).contiguous()
    else:
        v = np.ascontiguousarray(values, dtype=np.float64)
    shape = tuple(v.shape)
    if len(shape) not in (1, 2) or shape[-1] != nin:
        raise ValueError(f"restrict: expected {nin} values per component, got shape {shape}")
    ncomp = 1 if len(shape) == 1 else shape[0]
    if ncomp == 0:
        raise ValueError("restrict: no component")
    oshape = shape[:-1] + (nout,)
    out = torch.empty(oshape, dtype=torch.float64, device=v.device) if is_tensor else np.empty(oshape)
    pi, li = L.ptr(v)
    po, lo = L.ptr(out)
    L.check(L.lib.phx_restrict(coarse._h, fine._h, degree, ncomp, pi, li, po, lo))
    return out
