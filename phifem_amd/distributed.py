"""Partitioned problem drivers: one process per GPU (torch.distributed over RCCL/xGMI).

Two layouts.  SLABS (`SlabProblem` and its subclasses) serve uniform Kuhn lattices and are described below; a GENERAL
PARTITION (`PartitionedProblem`, at the end of this file) serves any triangle or tetrahedron mesh.

The background box is cut into slabs of cube layers along the last axis; every rank generates
its slab plus GHOST cube layers on the device (same global coordinates bit for bit), tags and
assembles it redundantly -- no matrix contribution ever crosses a rank -- and owns the rows of
the vertex planes inside its slab.  The only data-path exchanges are the halo of vector entries
before each SpMV and the batched scalar all-reduce of the Krylov dot products.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .mesh import create_box
from .mesh_scripts import NodalFunction, _tag_cells, _tag_facets
from .solver import PhiFEMSolver

GHOST_LAYERS = 4  # see DESIGN.md "Multi-GPU": tags/active flags exact on every referenced plane


def slab_layout(n_per_rank, rank, world, ghost=GHOST_LAYERS):
    """Cube-layer bookkeeping of rank `rank`: owned layers [L0, L1), local box [k0, k1),
    owned vertex planes [L0, P1) (the last rank also owns the closing plane)."""
    nz = n_per_rank * world
    L0, L1 = rank * n_per_rank, (rank + 1) * n_per_rank
    k0, k1 = max(0, L0 - ghost), min(nz, L1 + ghost)
    P1 = L1 + 1 if rank == world - 1 else L1
    return {"nz": nz, "L0": L0, "L1": L1, "k0": k0, "k1": k1, "P0": L0, "P1": P1}


class SlabProblem:
    """BASELINE configs[1] per GPU, weak-scaled: n^3 cubes per rank of an n x n x (n*world) box on
    [-1.5,1.5]^2 x [-1.5*world, 1.5*world] around the capsule  x^2 + y^2 + max(|z| - c, 0)^2 = 1,
    c = 1.5 (world - 1): the unit sphere of configs[1] for one rank, a cylinder of radius 1 with
    hemispherical caps for more -- one connected domain with full cross-sections at every slab interface
    and the same work per unit length (an ellipsoid stretched with `world` gives the middle slabs 2.25 x
    the DoFs of the sphere and leaves the end slabs empty)."""

    def __init__(self, n_per_rank, rank=0, world=1, device=0, rtol=1e-8, max_iter=20000, nxy=None):
        """nxy = None: BASELINE configs[1] weak-scaled (n^3 cubes per rank, capsule).
        nxy = 1024, n_per_rank = 128: BASELINE configs[4] -- the 1024^3 box of [-1.5,1.5]^3 cut into
        eight 1024 x 1024 x 128 slabs; with `world` < 8 ranks the z-range shrinks to [-1.5 world/8, 1.5 world/8], around the UNIT SPHERE (same h)."""
        self.n, self.rank, self.world, self.device = n_per_rank, rank, world, device
        self.nxy = nxy or n_per_rank
        self.config5 = nxy is not None
        self.rtol, self.max_iter = rtol, max_iter
        self.lay = slab_layout(n_per_rank, rank, world)

    def setup(self):
        import torch
        n, w, lay = self.n, self.world, self.lay
        nxy = self.nxy
        zext = 1.5 * w * n / nxy if self.config5 else 1.5 * w   # same h in z as in x and y
        lo = [-1.5, -1.5, -zext]
        hi = [1.5, 1.5, zext]
        self.mesh = create_box(lo, hi, [nxy, nxy, lay["k1"] - lay["k0"]], device=self.device,
                               offset=[0, 0, lay["k0"]], n_global=[nxy, nxy, lay["nz"]])
        # the slab's end planes inside the global box are cuts, not background boundary
        L.check(L.lib.phx_mesh_set_slab_faces(self.mesh._h, 1 if lay["k0"] > 0 else 0,
                                              1 if lay["k1"] < lay["nz"] else 0))
        if w > 1:
            # a slab that does not touch the domain (ranks 0 and 7 of the 1024^3 box around the unit sphere)
            # gets an empty system and still joins every collective
            L.check(L.lib.phx_set_option(self.mesh._h, L.OPT_ALLOW_EMPTY, 1))
        dev = torch.device("cuda", self.device)
        x = torch.empty((self.mesh.nv, 3), dtype=torch.float64, device=dev)
        L.check(L.lib.phx_mesh_get_array(self.mesh._h, L.ARR_COORDS, C.c_void_p(x.data_ptr()), L.DEVICE))
        cyl = 0.0 if self.config5 else 1.5 * (w - 1)   # half length of the cylindrical part
        dz = torch.clamp(torch.abs(x[:, 2]) - cyl, min=0.0)
        self.phi = x[:, 0] ** 2 + x[:, 1] ** 2 + dz ** 2 - 1.0
        # manufactured solution u = sin x sin y sin z:  -Laplace(u) = 3 u
        self.u_ex = torch.sin(x[:, 0]) * torch.sin(x[:, 1]) * torch.sin(x[:, 2])
        self.f = 3.0 * self.u_ex
        self.out = torch.empty(2 * self.mesh.nv, dtype=torch.float64, device=dev)
        del x
        torch.cuda.synchronize()
        self.solver = PhiFEMSolver(self.mesh)
        if w > 1:
            from .dist_solver import DistributedKrylov
            self.dk = DistributedKrylov(self)

    # --- one step of the hot path; the subclasses only say how they tag and assemble -----------------
    single_layer_cut = True

    def _assemble(self):
        return self.solver.assemble(self.phi, self.f, self.u_ex)

    def _tag_levelset(self):
        return self.phi

    def step(self, profile_spmv=False):
        """tag -> assemble -> solve, everything resident on the device."""
        mesh = self.mesh
        staged = _tag_cells(mesh, NodalFunction(self._tag_levelset()), 1, single_layer_cut=self.single_layer_cut)
        if self.world > 1:
            self.dk.agree_on_exterior()
        _tag_facets(mesh, staged, 1)
        info = self._assemble()
        if self.world == 1:
            self.solver.solve(rtol=self.rtol, max_iter=self.max_iter, out=self.out,
                              profile_spmv=profile_spmv)
            st = self.solver.stats
            n_owned = info["n_active"]
        else:
            st = self.dk.solve(self.out, profile_spmv=profile_spmv)
            n_owned = st["n_owned"]
        return self._step_result(mesh.timings(), info, st, n_owned)

    def _step_result(self, t, info, st, n_owned):
        """The dict `step()` returns; t = stage timings of the mesh that was tagged."""
        pc = self.solver.precond_info()
        return {
            "n_active_owned": n_owned, "iterations": st["iterations"], "relres": st["relres"],
            "converged": bool(st.get("converged", st["relres"] <= self.rtol)),
            "precond_exact": bool(st.get("precond_exact", False)),
            "stage_s": {"tag": t["tag_cells"] + t["tag_facets"], "assemble": t["assemble"],
                        "solve": st["seconds"]},
            "spmv_avg_s": st.get("spmv_avg_s", 0.0), "spmv_count": st.get("spmv_timed", 0),
            "spmv_algorithmic_bytes": 12.0 * info["sell_nnz"] + 20.0 * info["n_active"],
            "spmv_stream_bytes": info["spmv_matrix_bytes"], "spmv_rows": info["n_active"],
            "system": {k: info[k] for k in ("n_active", "n_active_u", "stencil_rows", "stencil_runs", "n_slices",
                                            "sell_nnz", "sell_padded_nnz", "slot_capacity")},
            # sine-transform y pass of the preconditioner: reads and writes every lattice point once
            "precond": pc["precond"], "precond_L": pc["precond_L"], "precond_points": pc["precond_points"],
            "dst_avg_s": pc["dst_avg_s"], "dst_count": pc["dst_timed"],
            "dst_algorithmic_bytes": 2.0 * pc["precond_value_bytes"] * pc["precond_points"],
            "precond_value_bytes": pc["precond_value_bytes"],
        }


def detect_kuhn_lattice(x, rtol=64 * 2.220446049250313e-16):
    """Tensor lattice behind the vertices of a caller-supplied box mesh (any vertex order): (lo[3], hi[3], n[3], lat) with
    lat[v] = i + (nx + 1) (j + (ny + 1) k), or a ValueError naming what is not a lattice.  Host side, numpy."""
    x = np.asarray(x, dtype=np.float64)
    nv, gdim = x.shape
    if gdim != 3:
        raise ValueError("a 3-D box is partitioned into z-slabs")
    lo, hi, n, idx = [], [], [], []
    for a in range(3):
        vals = np.unique(x[:, a])
        ext = vals[-1] - vals[0]
        scale = max(abs(vals[0]), abs(vals[-1]), ext)
        # coordinates equal up to a few ulps of the box size are one lattice plane
        keep = np.concatenate(([True], np.diff(vals) > rtol * scale))
        planes = vals[keep]
        na = planes.size - 1
        if na < 1:
            raise ValueError(f"axis {a}: the vertices lie in one plane")
        q = (x[:, a] - planes[0]) / ext * na
        i = np.rint(q).astype(np.int64)
        gen = planes[0] + ext * (i / na)
        if np.any(np.abs(x[:, a] - gen) > rtol * scale):
            raise ValueError(f"axis {a}: the vertices are not on a uniform lattice (a graded or perturbed mesh cannot be "
                             f"served by generated slabs)")
        lo.append(planes[0]); hi.append(planes[-1]); n.append(na); idx.append(i)
    lat = idx[0] + (n[0] + 1) * (idx[1] + (n[1] + 1) * idx[2])
    if nv != (n[0] + 1) * (n[1] + 1) * (n[2] + 1) or np.unique(lat).size != nv:
        raise ValueError("the vertices do not fill a tensor lattice")
    return np.array(lo), np.array(hi), np.array(n, dtype=np.int64), lat


class ArraySlabProblem(SlabProblem):
    """A caller-supplied Kuhn box -- vertices `x` in ANY order, what dolfinx's create_box hands over --
    partitioned into z-slabs over the ranks (missing item 4; the reference is serial,
    src/phifem/mesh_scripts.py:264 "TODO ... parallel computing").  Every rank is given the WHOLE vertex array and the nodal
    data in the caller's numbering (as a dolfinx caller that read one mesh file has them), recognises the lattice,
    generates its slab + ghost layers on the device and runs the slab pipeline (tag, assemble redundantly, solve with halo
    exchange + slab-exact preconditioner); `solution()` hands the owned part back in the caller's vertex numbering.
    Only the lattice has to be uniform: a mesh that is not a tensor lattice raises ValueError (no silent fallback)."""

    def __init__(self, x, phi, f, u_D, rank=0, world=1, device=0, rtol=1e-8, max_iter=20000):
        self.lo_box, self.hi_box, self.n_box, self.lat = detect_kuhn_lattice(x)
        nz = int(self.n_box[2])
        if nz % world:
            raise ValueError(f"{nz} cube layers along z do not split into {world} equal slabs")
        super().__init__(nz // world, rank=rank, world=world, device=device, rtol=rtol, max_iter=max_iter)
        self.nxy = int(self.n_box[0])
        self.plane_vertices = int((self.n_box[0] + 1) * (self.n_box[1] + 1))
        self._phi, self._f, self._uD = (np.asarray(a, dtype=np.float64) for a in (phi, f, u_D))
        # caller vertex of a global lattice point
        self.lat2v = np.empty(self.lat.size, dtype=np.int64)
        self.lat2v[self.lat] = np.arange(self.lat.size)

    def setup(self):
        import torch
        lay, w = self.lay, self.world
        nx, ny = int(self.n_box[0]), int(self.n_box[1])
        self.mesh = create_box(self.lo_box, self.hi_box, [nx, ny, lay["k1"] - lay["k0"]], device=self.device,
                               offset=[0, 0, lay["k0"]], n_global=[nx, ny, lay["nz"]])
        L.check(L.lib.phx_mesh_set_slab_faces(self.mesh._h, 1 if lay["k0"] > 0 else 0, 1 if lay["k1"] < lay["nz"] else 0))
        if w > 1:
            L.check(L.lib.phx_set_option(self.mesh._h, L.OPT_ALLOW_EMPTY, 1))
        dev = torch.device("cuda", self.device)
        # the slab's vertices are lattice points k0 .. k1 of the global lattice, in lattice order
        g0 = lay["k0"] * self.plane_vertices
        self.caller_vertex = self.lat2v[g0:g0 + self.mesh.nv]
        take = torch.from_numpy(self.caller_vertex).to(dev)
        self.phi = torch.from_numpy(self._phi).to(dev)[take].contiguous()
        self.f = torch.from_numpy(self._f).to(dev)[take].contiguous()
        self.u_ex = torch.from_numpy(self._uD).to(dev)[take].contiguous()
        self.out = torch.empty(2 * self.mesh.nv, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        self.solver = PhiFEMSolver(self.mesh)
        if w > 1:
            from .dist_solver import DistributedKrylov
            self.dk = DistributedKrylov(self)

    def solution(self):
        """(caller vertex ids, u, p) of the vertices this rank OWNS (the planes P0 .. P1 of its slab)."""
        lay, nv = self.lay, self.mesh.nv
        w = self.out.cpu().numpy()
        plane = np.arange(nv) // self.plane_vertices + lay["k0"]
        own = (plane >= lay["P0"]) & (plane < lay["P1"])
        return self.caller_vertex[own], w[:nv][own], w[nv:][own]


class ElasticitySlabProblem(SlabProblem):
    """BASELINE configs[3]: 3-D interface elasticity (5-field mixed phi-FEM, P1 vector fields,
    E_in = 1, E_out = 1e-3, nu = 0.3, phi = 1 - r^2: demo/interface-elasticity/data.py:14-22,39-40)
    on an n x n x (nz_per_rank * world) Kuhn box of [-1.5,1.5]^3, slab-partitioned.  Tags without the
    single-layer rule and u_in = u_D on the box boundary, as in the demo (main.py:115-117,158-177)."""

    def __init__(self, nxy, nz_per_rank, rank=0, world=1, device=0, rtol=1e-8, max_iter=200000, coarse=-1):
        super().__init__(nz_per_rank, rank=rank, world=world, device=device, rtol=rtol,
                         max_iter=max_iter, nxy=nxy)
        self.n_blocks = 27
        self.coarse = coarse      # PHX_OPT_EL_COARSE: -1 automatic (on from 80 cubes per axis of the global box)

    def setup(self):
        import torch
        from .solver import InterfaceElasticitySolver
        lay, nxy = self.lay, self.nxy
        nzl = lay["k1"] - lay["k0"]
        self.mesh = create_box([-1.5] * 3, [1.5] * 3, [nxy, nxy, nzl], device=self.device,
                               offset=[0, 0, lay["k0"]], n_global=[nxy, nxy, lay["nz"]])
        L.check(L.lib.phx_mesh_set_slab_faces(self.mesh._h, 1 if lay["k0"] > 0 else 0,
                                              1 if lay["k1"] < lay["nz"] else 0))
        dev = torch.device("cuda", self.device)
        x = torch.empty((self.mesh.nv, 3), dtype=torch.float64, device=dev)
        L.check(L.lib.phx_mesh_get_array(self.mesh._h, L.ARR_COORDS, C.c_void_p(x.data_ptr()), L.DEVICE))
        self.phi = 1.0 - (x ** 2).sum(dim=1)
        self.f = torch.stack([torch.sin(x[:, 0]) + 0.2, torch.cos(x[:, 1]), 0.5 * x[:, 2]]).contiguous()
        self.u_D = (0.1 * torch.stack([x[:, 0] * x[:, 1], torch.sin(x[:, 2]), x[:, 0] - x[:, 1]])).contiguous()
        # Dirichlet vertices: the faces of the GLOBAL box this slab touches
        n1 = nxy + 1
        v = torch.arange(self.mesh.nv, device=dev)
        i, j, k = v % n1, (v // n1) % n1, v // (n1 * n1) + lay["k0"]
        on = (i == 0) | (i == nxy) | (j == 0) | (j == nxy) | (k == 0) | (k == lay["nz"])
        self.bc_vertices = torch.nonzero(on).flatten().to(torch.int32).contiguous()
        self.out = torch.empty(27 * self.mesh.nv, dtype=torch.float64, device=dev)
        del x
        torch.cuda.synchronize()
        # bit-reproducible assembly and dot products: the iteration count of this ill-conditioned system is then the
        # same on every run (it moved between 712 and 912 with atomics in arrival order)
        self.solver = InterfaceElasticitySolver(self.mesh, deterministic=True, coarse=self.coarse)
        if self.world > 1:
            from .dist_solver import DistributedKrylov
            self.dk = DistributedKrylov(self)

    single_layer_cut = False

    def _assemble(self):
        return self.solver.assemble(self.phi, self.f, self.u_D, self.bc_vertices)


class P2Problem(SlabProblem):
    """BASELINE configs[2] on one GPU: 3-D weak-Dirichlet Poisson, P2 x P2 with the div(grad) and ghost-penalty
    stabilisation terms, level-set in P2, spherical domain, n^3 Kuhn box.  The system is STRUCTURED: the interior rows
    are applied from eight translation-invariant stencils and never assembled or stored, which is what lets the
    512^3 box of the config (1.08e9 P2 entities per field, 1.7e8 active rows) fit one GPU."""

    def __init__(self, n, device=0, rtol=1e-8, max_iter=100000, coarse_space=None):
        """coarse_space: PhiFEMSolver's two-level option (None: off, "auto", or H / h >= 5)."""
        self.n, self.device, self.rtol, self.max_iter = n, device, rtol, max_iter
        self.coarse_space = coarse_space
        self.world, self.rank = 1, 0

    def setup(self):
        import torch
        self.mesh = create_box([-1.5] * 3, [1.5] * 3, [self.n] * 3, device=self.device)
        dev = torch.device("cuda", self.device)
        x = torch.empty((self.mesh.nv, 3), dtype=torch.float64, device=dev)
        L.check(L.lib.phx_mesh_get_array(self.mesh._h, L.ARR_COORDS, C.c_void_p(x.data_ptr()), L.DEVICE))
        self.phi1 = (x ** 2).sum(dim=1) - 1.0            # P1 nodal values drive the tagging
        # bit-reproducible assembly and dot products (the iteration count moved between 694 and 892 without)
        self.solver = PhiFEMSolver(self.mesh, degree=2, levelset_degree=2, deterministic=True,
                                   coarse_space=self.coarse_space)
        ne = self.mesh.ne                                 # builds the edge numbering
        e = torch.empty((ne, 2), dtype=torch.int32, device=dev)
        L.check(L.lib.phx_mesh_get_array(self.mesh._h, L.ARR_EDGES, C.c_void_p(e.data_ptr()), L.DEVICE))
        # nodal data at the P2 points (vertices, then edge midpoints), evaluated in chunks: at 512^3 there are 9.4e8
        # edges, and torch temporaries of that length (index tensors, gathered coordinates) would take > 100 GB
        nv = self.mesh.nv
        nd = nv + ne
        self.phi = torch.empty(nd, dtype=torch.float64, device=dev)
        self.u_ex = torch.empty(nd, dtype=torch.float64, device=dev)

        def fill(lo, pts):
            self.phi[lo:lo + pts.shape[0]] = (pts ** 2).sum(dim=1) - 1.0
            self.u_ex[lo:lo + pts.shape[0]] = torch.sin(pts[:, 0]) * torch.sin(pts[:, 1]) * torch.sin(pts[:, 2])

        chunk = 1 << 25
        for lo in range(0, nv, chunk):
            fill(lo, x[lo:lo + chunk])
        for lo in range(0, ne, chunk):
            ee = e[lo:lo + chunk].long()
            fill(nv + lo, 0.5 * (x[ee[:, 0]] + x[ee[:, 1]]))
            del ee
        self.f = 3.0 * self.u_ex
        self.out = torch.empty(2 * nd, dtype=torch.float64, device=dev)
        del x, e
        torch.cuda.synchronize()
        torch.cuda.empty_cache()    # the assembly's transient buffers need the room torch's allocator would keep

    def _tag_levelset(self):
        return self.phi1


class PartitionedProblem:
    """P1 x P1 weak-Dirichlet Poisson (box mode) on ANY triangle or tetrahedron background mesh -- graded, unstructured,
    vertices and cells in any order -- partitioned over the ranks (the reference is serial,
    src/phifem/mesh_scripts.py:264 "TODO ... parallel computing").

    Data model: every rank is handed the WHOLE mesh (`x`, `cells`) and the nodal data `phi`, `f`, `u_D` in the caller's
    numbering, as `ArraySlabProblem` is handed its vertex array, and tags the whole mesh itself, so no tag ever crosses
    a rank.  THE BACKGROUND MESH THEREFORE HAS TO FIT ONE GPU.  The cells are split by recursive coordinate bisection
    (`partition_cells`, weight 1 for cells tagged 1 / 2, 0 for the exterior); a vertex belongs to the part of the
    lowest-numbered cell of Omega_h that contains it; a rank works on four layers of cells around its vertices
    (`phx_partition_layout`), with the tags of the whole mesh transferred, and assembles every row it owns -- and the
    diagonal of every column those rows refer to -- completely from them: no matrix entry crosses a rank.  The solve is Jacobi-BiCGStab with a halo exchange with up to world - 1 peers.
    A rank that owns nothing holds an empty system and still joins every collective."""

    single_layer_cut = True   # as SlabProblem: one layer of cut cells

    def __init__(self, cell_type, x, cells, phi, f, u_D, rank=0, world=1, device=0, rtol=1e-8, max_iter=20000,
                 deterministic=False, balance="domain"):
        """balance = "domain" (default): the parts share the cells of Omega_h (weight 1 for tags 1 / 2, 0 outside);
        "cells": they share the background cells -- parts away from the domain then own nothing."""
        if cell_type not in ("triangle", "tetrahedron"):
            raise NotImplementedError("PartitionedProblem serves triangle and tetrahedron meshes")
        if balance not in ("domain", "cells"):
            raise ValueError("balance is 'domain' or 'cells'")
        self.balance = balance
        self.cell_type = cell_type
        self._x = np.ascontiguousarray(x, dtype=np.float64)
        self._cells = np.ascontiguousarray(cells, dtype=np.int32)
        nv = self._x.shape[0]
        self._phi, self._f, self._uD = (np.ascontiguousarray(a, dtype=np.float64) for a in (phi, f, u_D))
        for a, name in ((self._phi, "phi"), (self._f, "f"), (self._uD, "u_D")):
            if a.shape != (nv,):
                raise ValueError(f"{name} has shape {a.shape}, the mesh has {nv} vertices")
        self.rank, self.world, self.device = int(rank), int(world), int(device)
        self.rtol, self.max_iter, self.deterministic = rtol, max_iter, bool(deterministic)
        self.setup_s = {}

    def _tag_background(self):
        staged = _tag_cells(self.bg, NodalFunction(self.phi_g), 1, single_layer_cut=self.single_layer_cut)
        _tag_facets(self.bg, staged, 1)

    def _extract(self):
        """Local mesh with the tags of the background mesh, the nodal data on it and the solver."""
        import torch
        from .partition import local_mesh
        dev = torch.device("cuda", self.device)
        self.mesh, self.c_map, self.v_map = local_mesh(self.bg, self.flags)
        take = torch.from_numpy(self.v_map.astype(np.int64)).to(dev)
        self.phi, self.f, self.u_D = (g[take].contiguous() for g in (self.phi_g, self.f_g, self.uD_g))
        self.owner_v = self.owner[take]
        self.owned_v = self.owner_v == self.rank
        self.out = torch.empty(2 * self.mesh.nv, dtype=torch.float64, device=dev)
        pc = self.part[torch.from_numpy(self.c_map.astype(np.int64)).to(dev)]
        self.owned_cells = int((pc == self.rank).sum().item())
        self.ghost_cells = int(self.c_map.size) - self.owned_cells
        # a rank that owns nothing gets an empty system and still joins every collective
        L.check(L.lib.phx_set_option(self.mesh._h, L.OPT_ALLOW_EMPTY, 1))
        self.solver = PhiFEMSolver(self.mesh, deterministic=self.deterministic)

    def setup(self):
        import time
        import torch
        import warnings
        from .mesh import Mesh
        from .partition import partition_cells, partition_layout
        dev = torch.device("cuda", self.device)
        self.bg = Mesh.from_arrays(self.cell_type, self._x, self._cells, device=self.device)
        self.phi_g, self.f_g, self.uD_g = (torch.from_numpy(a).to(dev) for a in (self._phi, self._f, self._uD))
        torch.cuda.synchronize(dev)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self._tag_background()
        self.tag_timings = self.bg.timings()
        t0 = time.perf_counter()
        tags = torch.empty(self.bg.nc, dtype=torch.int32, device=dev)
        L.check(L.lib.phx_mesh_get_array(self.bg._h, L.ARR_CELL_TAGS, C.c_void_p(tags.data_ptr()), L.DEVICE))
        weights = ((tags == 1) | (tags == 2)).to(torch.int32).contiguous()
        self.part = partition_cells(self.bg, self.world, weights if self.balance == "domain" else None)
        if self.balance != "domain":   # (the all-ones weights are made inside the library; the result lives on the host)
            self.part = torch.from_numpy(self.part).to(dev)
        t1 = time.perf_counter()
        self.owner, self.flags = partition_layout(self.bg, self.world, self.part, self.rank)
        self._extract()
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        self.setup_s = {"partition": t1 - t0, "layout": t2 - t1}
        if self.world > 1:
            from .dist_solver import PartitionedKrylov
            self.dk = PartitionedKrylov(self)

    def step(self, profile_spmv=False):
        """assemble -> solve on the local mesh.  The level-set is fixed at construction, so tagging, partition and local
        mesh are the ones of `setup()` (the "tag" stage time reported is that tagging of the whole mesh)."""
        t = dict(self.tag_timings)
        info = self.solver.assemble(self.phi, self.f, self.u_D)
        t["assemble"] = self.mesh.timings()["assemble"]
        n_peers = halo_entries = 0
        if self.world == 1:
            self.solver.solve(rtol=self.rtol, max_iter=self.max_iter, out=self.out, profile_spmv=profile_spmv)
            st = self.solver.stats
            n_owned = info["n_active"]
        else:
            st = self.dk.solve(self.out, profile_spmv=profile_spmv)
            n_owned = st["n_owned"]
            halos = self.dk.last_solver.halos
            n_peers = len(halos)
            halo_entries = sum(int(h["recv"][0].numel()) for h in halos)
        res = self._step_result(t, info, st, n_owned)
        res.update({"n_peers": n_peers, "halo_entries": halo_entries, "ghost_cells": self.ghost_cells,
                    "owned_cells": self.owned_cells,
                    "ghost_cells_per_owned_cell": self.ghost_cells / max(self.owned_cells, 1)})
        return res

    _step_result = SlabProblem._step_result

    def solution(self):
        """(caller vertex ids, u, p) of the vertices this rank OWNS."""
        nv = self.mesh.nv
        w = self.out.cpu().numpy()
        own = self.owned_v.cpu().numpy()
        return self.v_map[own].astype(np.int64), w[:nv][own], w[nv:][own]
