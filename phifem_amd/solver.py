"""PhiFEMSolver: the assemble -> solve sequence of the weak-Dirichlet demo over the C ABI.

The reference writes this sequence out in each demo (demo/weak-dirichlet/flower/main.py:102-186:
UFL forms, dolfinx assemble_matrix/assemble_vector, PETSc KSP + MUMPS); ROADMAP.md:15 plans a
class-based interface for it.  This class is that interface for the P1 x P1 weak-Dirichlet
Poisson problem (Q1 x Q1 on quadrilateral meshes of rectangles), with the element integration,
scatter and Krylov solve in HIP.
"""
import ctypes as C
import warnings

import numpy as np

from . import _lib as L


class ConvergenceWarning(RuntimeWarning):
    """The Krylov solve stopped at max_iter with a relative residual above rtol.  The reference solves
    directly (MUMPS LU, demo/weak-dirichlet/flower/main.py:162-182), so its callers assume an accurate
    solution: an unconverged iterate must not pass silently."""


def check_converged(stats, rtol, strict=False):
    """Warn (or raise with strict=True) when `stats` describes an unconverged solve."""
    if stats.get("converged", True):
        return
    msg = (f"BiCGStab did not converge: relative residual {stats['relres']:.3e} > rtol {rtol:g} after "
           f"{stats['iterations']} iterations")
    if strict:
        raise ArithmeticError(msg)
    warnings.warn(msg, ConvergenceWarning, stacklevel=3)


_COARSE_REASONS = {
    1: "not a single-rank P2 system on a generated box with the lattice preconditioner",
    2: "the box is smaller than 2 H",
    3: "too many coarse DoFs for the dense inverse (20000)",
    4: "the Galerkin coarse matrix is singular",
    5: "the check |Ac Ac^-1 v - v| of the inverse failed",
    6: "automatic choice: the correction does not pay at this box size",
}


def _p2_coarse_option(coarse_space):
    """PHX_OPT_P2_COARSE value of the `coarse_space` argument."""
    if coarse_space is None:
        return 0
    if isinstance(coarse_space, str):
        if coarse_space == "auto":
            return -1
        raise ValueError(f"coarse_space={coarse_space!r}: None, 'auto' or an int >= 5")
    if isinstance(coarse_space, bool) or int(coarse_space) != coarse_space or int(coarse_space) < 5:
        raise ValueError(f"coarse_space={coarse_space!r}: None, 'auto' or an int >= 5 (H / h)")
    return int(coarse_space)


class PhiFEMSolver:
    def __init__(self, mesh, pen_coef=1.0, stab_coef=1.0, degree=1, levelset_degree=1, deterministic=False,
                 coarse_space=None, multilevel=False):
        """multilevel (PHX_OPT_MULTILEVEL, degree 1 on triangle / tetrahedron meshes that `refine` produced, one
        rank): the u block is preconditioned with one geometric-multigrid V-cycle over the refinement hierarchy the mesh
        carries (`mesh.coarse`, down to the first mesh whose parent is gone), the p block keeps Jacobi.
        False (default): nothing changes.  True: built by `assemble`; ValueError when the mesh has no living parent,
        when every boundary vertex is active (the level matrices would be singular) or on a slab / partitioned rank;
        NotImplementedError for degree 2, quadrilaterals, sub-meshes, `coarse_space`, and meshes the lattice
        preconditioner serves (Kuhn boxes).  "auto": as True where it can be built, quietly Jacobi (or the lattice
        preconditioner) elsewhere.  `stats["precond"]` reports "multilevel", `stats["precond_L"]` = [levels, vertices
        of level 0, coarse kind: 1 dense inverse, 0 smoothing sweeps].

        coarse_space (PHX_OPT_P2_COARSE, degree 2 on a generated Kuhn box, one rank): two-level preconditioner, the
        additive Galerkin correction R Ac^-1 R^T on multilinear functions of spacing H on top of the lattice sine
        transform.  None (default): off; "auto": the library picks H (and leaves it off where it does not pay);
        an int >= 5: H / h.  Built on the first solve; a correction that was asked for and could not be built is
        reported by a RuntimeWarning and `stats["coarse_reason"]`.

        deterministic=True (PHX_OPT_DETERMINISTIC): bit-reproducible assembly (degree 2, and degree 1 on meshes that
        are not GENERATED Kuhn boxes -- a caller-supplied Kuhn box is then assembled in its own numbering instead of on
        the generated box behind it: the element kernels run twice and accumulate exactly) and Krylov dot products -- the same matrix bits, iteration count and solution
        on every run; costs one more pass of the element kernels.

        mesh: a tagged `phifem_amd.Mesh` (box mode) or the sub-mesh returned by
        `compute_tags_measures(..., box_mode=False)`; coefficients as main.py:42-43;
        degree = primal_degree = auxiliary degree (main.py:38, 76-78), levelset_degree as main.py:40.
        Degree-2 nodal arrays list the vertex values first, then the edge-midpoint values
        (`mesh.p2_dof_points()`).

        Quadrilateral meshes (`create_rectangle(..., cell_type="quadrilateral")`, box mode or sub-mesh): Q1 x Q1 with
        Q1 nodal phi_h, f_h, u_D (degree = levelset_degree = 1) on axis-parallel rectangles in tensor-product vertex
        order; other quadrilaterals raise NotImplementedError at `assemble`.  Q2 spaces and `coarse_space` are not
        implemented there."""
        if degree not in (1, 2) or levelset_degree not in (1, 2):
            raise NotImplementedError("Lagrange degrees 1 and 2 are implemented")
        if getattr(mesh, "cell_type", None) == "quadrilateral":
            if degree != 1 or levelset_degree != 1:
                raise NotImplementedError("quadrilateral meshes: Q1 x Q1 with a Q1 level-set (degree = levelset_degree "
                                          "= 1) is implemented")
            if coarse_space is not None:
                raise NotImplementedError("quadrilateral meshes: Q1 x Q1 without coarse_space is implemented (the "
                                          "coarse-space correction is built for degree 2 on simplicial boxes)")
        if degree == 1 and levelset_degree != 1:
            raise NotImplementedError("a P2 level-set needs degree = 2")
        self.degree, self.levelset_degree = degree, levelset_degree
        self.mesh = mesh
        self.pen_coef = float(pen_coef)
        self.stab_coef = float(stab_coef)
        self._sys = None
        self.stats = {}
        self.deterministic = bool(deterministic)
        self.coarse_space = coarse_space
        self._p2_coarse = _p2_coarse_option(coarse_space)
        if multilevel not in (False, True, "auto"):
            raise ValueError(f"multilevel={multilevel!r}: False, True or 'auto'")
        self.multilevel = multilevel
        if multilevel is True:
            if degree != 1:
                raise NotImplementedError("multilevel is implemented for degree = 1")
            if getattr(mesh, "cell_type", None) == "quadrilateral":
                raise NotImplementedError("multilevel is implemented on triangles and tetrahedra")
            if getattr(mesh, "parent", None) is not None:
                raise NotImplementedError("multilevel needs the refined mesh itself (box_mode=True), not a sub-mesh")
            if coarse_space is not None:
                raise NotImplementedError("multilevel is not combined with coarse_space")
            if getattr(mesh, "coarse", None) is None:
                raise ValueError("multilevel=True: the mesh was not produced by refine() (no parent to coarsen to)")
        if self._p2_coarse != 0:
            if degree != 2:
                raise NotImplementedError("coarse_space is implemented for degree = 2")
            if getattr(mesh, "parent", None) is not None:
                raise NotImplementedError("coarse_space needs the box mesh (box_mode=True), not a sub-mesh")

    def _apply_options(self):
        L.check(L.lib.phx_set_option(self.mesh._h, L.OPT_DETERMINISTIC, int(getattr(self, "deterministic", False))))
        L.check(L.lib.phx_set_option(self.mesh._h, L.OPT_P2_COARSE, int(getattr(self, "_p2_coarse", 0))))
        L.check(L.lib.phx_set_option(self.mesh._h, L.OPT_MULTILEVEL, int(getattr(self, "_ml_on", False))))
        if hasattr(self, "coarse"):
            L.check(L.lib.phx_set_option(self.mesh._h, L.OPT_EL_COARSE, self.coarse))
        if hasattr(self, "_elwd_coarse"):     # ElasticitySolver: its own option, PHX_OPT_EL_COARSE is the sibling's
            L.check(L.lib.phx_set_option(self.mesh._h, L.OPT_ELWD_COARSE, self._elwd_coarse))

    def __del__(self):
        self._free()

    def _free(self):
        try:
            if self._sys is not None:
                L.lib.phx_system_destroy(self._sys)
                self._sys = None
        except Exception:
            pass

    def _arr(self, a, n):
        """Nodal array of the C ABI: numpy (converted) or a torch tensor, which is handed to the kernels as a
        raw `double*` and therefore has to BE one: float64, contiguous, n values, and -- on the device -- on
        the mesh's GPU."""
        if hasattr(a, "data_ptr"):
            import torch
            if a.dtype != torch.float64:
                raise ValueError(f"nodal tensor has dtype {a.dtype}, the C ABI takes float64")
            if not a.is_contiguous():
                raise ValueError("nodal tensor is not contiguous")
            if a.numel() != n:
                raise ValueError(f"nodal tensor has {a.numel()} values, the space has {n} DoFs")
            if a.is_cuda and a.device.index != self.mesh.device:
                raise ValueError(f"nodal tensor lives on cuda:{a.device.index}, the mesh on cuda:{self.mesh.device}")
            return a
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape[0] != n:
            raise ValueError(f"nodal array has {a.shape[0]} values, the space has {n} DoFs")
        return a

    def assemble(self, phi_h, f_h, u_D):
        """Bilinear + linear form of main.py:112-154 (nodal P1 data, numpy or device tensors)."""
        self._free()
        nd = self.ndofs
        nphi = self.mesh.nv if self.levelset_degree == 1 else nd
        phi_h = self._arr(phi_h, nphi)
        f_h, u_D = (self._arr(a, nd) for a in (f_h, u_D))
        locs = {L.ptr(a)[1] for a in (phi_h, f_h, u_D)}
        if len(locs) != 1:
            raise ValueError("phi_h, f_h and u_D must all live on the host or all on the device")
        self._keep = (phi_h, f_h, u_D)   # inputs stay alive as long as the system they were read for
        self._tag_generation = self.mesh._tag_generation
        self._sys = self._assemble_raw()
        self._setup_multilevel()
        return self.info()

    def _wants_multilevel(self):
        ml = getattr(self, "multilevel", False)
        if ml == "auto":
            m = self.mesh
            return (self.degree == 1 and getattr(m, "cell_type", None) in ("triangle", "tetrahedron")
                    and getattr(m, "parent", None) is None and getattr(m, "coarse", None) is not None
                    and getattr(self, "_p2_coarse", 0) == 0)
        return ml is True

    def _setup_multilevel(self):
        """Builds the multilevel preconditioner of the system just assembled, so that its refusals surface here."""
        self._ml_on = False
        if not self._wants_multilevel():
            return
        try:
            L.check(L.lib.phx_multilevel_setup(self._sys))
            self._ml_on = True
        except (ValueError, NotImplementedError):
            if self.multilevel is True:
                self._free()
                raise

    def _assemble_raw(self):
        phi_h, f_h, u_D = self._keep
        loc = L.ptr(phi_h)[1]
        h = C.c_void_p()
        self._apply_options()
        if self.degree == 1:
            L.check(L.lib.phx_assemble_poisson_wd(
                self.mesh._h, self.pen_coef, self.stab_coef, L.ptr(phi_h)[0], L.ptr(f_h)[0],
                L.ptr(u_D)[0], loc, C.byref(h)))
        else:
            L.check(L.lib.phx_assemble_poisson_wd_p2(
                self.mesh._h, self.pen_coef, self.stab_coef, L.ptr(phi_h)[0], self.levelset_degree,
                L.ptr(f_h)[0], L.ptr(u_D)[0], loc, C.byref(h)))
        return h

    @property
    def ndofs(self):
        """DoFs per field in the full numbering (vertices, plus edges at degree 2)."""
        return self.mesh.nv if self.degree == 1 else self.mesh.nv + self.mesh.ne

    def info(self):
        i = (C.c_int64 * 14)()
        L.check(L.lib.phx_system_info(self._sys, i))
        keys = ("n_active", "n_active_u", "nnz", "n_full", "sell_padded_nnz", "slot_capacity",
                "sell_nnz", "n_slices", "indexed_slices", "spmv_matrix_bytes", "indexed_slices_lds",
                "stencil_rows", "stencil_runs", "has_csr")
        return dict(zip(keys, (int(v) for v in i)))

    def export_csr(self):
        """(scipy-style rowptr, col, val, rhs, dof) of the active system, for inspection/tests.

        The CSR copy is LAZY: P1 systems on Kuhn boxes are assembled straight into the solver formats
        (stencil-coded interior rows + SELL, PHX_OPT_STRUCTURED) and never form it; the first export
        re-assembles the same inputs once with PHX_OPT_EXPORT_CSR set and reads the CSR of that system."""
        i = self.info()

        def buffers(n, nnz):
            arrs = (np.empty(n + 1, dtype=np.int64), np.empty(nnz, dtype=np.int32), np.empty(nnz, dtype=np.float64),
                    np.empty(n, dtype=np.float64), np.empty(n, dtype=np.int64))
            return arrs, [a.ctypes.data_as(C.c_void_p) for a in arrs]

        if i["has_csr"]:
            (rowptr, col, val, rhs, dof), args = buffers(i["n_active"], i["nnz"])
            L.check(L.lib.phx_system_export(self._sys, *args))
        elif getattr(self, "_keep", None) is not None and getattr(self, "_tag_generation", None) is not None:
            if self._tag_generation != self.mesh._tag_generation:
                warnings.warn("the mesh was tagged again after assemble(): the exported CSR is rebuilt from the CURRENT "
                              "tags and equals the solved system only if they are unchanged (set PHX_OPT_EXPORT_CSR "
                              "before assembling to keep the solved system's own copy)", RuntimeWarning, stacklevel=2)
            L.check(L.lib.phx_set_option(self.mesh._h, L.OPT_EXPORT_CSR, 1))
            try:
                h = self._assemble_raw()
            finally:
                L.check(L.lib.phx_set_option(self.mesh._h, L.OPT_EXPORT_CSR, 0))
            try:
                # sizes of the RE-ASSEMBLED system: a structured system only estimates its structural count
                j = (C.c_int64 * 14)()
                L.check(L.lib.phx_system_info(h, j))
                (rowptr, col, val, rhs, dof), args = buffers(int(j[0]), int(j[2]))
                L.check(L.lib.phx_system_export(h, *args))
            finally:
                L.lib.phx_system_destroy(h)
        else:
            (rowptr, col, val, rhs, dof), args = buffers(i["n_active"], i["nnz"])
            L.check(L.lib.phx_system_export(self._sys, *args))   # reports "assembled without its CSR copy"
        return rowptr, col, val, rhs, dof

    def export_rhs_dof(self):
        """(rhs, dof) of the active system without the matrix: right-hand side in active numbering and the map
        active row -> full DoF index (works at sizes where the CSR copy would not fit the host)."""
        n = self.info()["n_active"]
        rhs = np.empty(n, dtype=np.float64)
        dof = np.empty(n, dtype=np.int64)
        L.check(L.lib.phx_system_export(self._sys, None, None, None, rhs.ctypes.data_as(C.c_void_p),
                                        dof.ctypes.data_as(C.c_void_p)))
        return rhs, dof

    def solve(self, rtol=1e-8, max_iter=20000, out=None, profile_spmv=False, strict=False, x0=None):
        """Replaces the KSP/MUMPS block of main.py:162-182.  Returns the mixed solution in the
        full numbering [u (nv), p (nv)] with inactive DoFs at zero; `out` may be a device
        tensor of 2*nv doubles.  `stats["converged"]` says whether rtol was reached; if not, a
        `ConvergenceWarning` is issued (strict=True: ArithmeticError) -- the reference's direct solve
        never returns an inaccurate x silently.

        x0 (`phx_solve_from`): a starting vector in the full numbering, a numpy array or a device tensor of the kind
        of `out` (a new numpy array / a new tensor on x0's device when `out` is None).  The solve then runs on the
        correction b - A x0 and stops at ||b - A x|| <= rtol ||b||; an x0 that meets the tolerance already comes back
        unchanged with 0 iterations.  None: the solve from zero."""
        nfull = self.info()["n_full"]
        x0_dev = x0 is not None and hasattr(x0, "data_ptr") and x0.is_cuda
        if out is None:
            if x0_dev:
                import torch
                out = torch.empty(nfull, dtype=torch.float64, device=x0.device)
            else:
                out = np.empty(nfull, dtype=np.float64)
        elif hasattr(out, "data_ptr"):
            import torch
            if out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != nfull:
                raise ValueError(f"`out` must be a contiguous float64 tensor of {nfull} values")
        p, loc = L.ptr(out)
        st = (C.c_double * 8)()
        self._apply_options()
        L.check(L.lib.phx_set_option(self.mesh._h, L.OPT_PROFILE_SPMV, int(profile_spmv)))
        if x0 is None:
            L.check(L.lib.phx_solve(self._sys, 0, float(rtol), int(max_iter), p, loc, st))
        else:
            x0 = self._arr(x0, nfull)
            p0, loc0 = L.ptr(x0)
            if loc0 != loc:
                raise ValueError("x0 and out must both live on the host or both on the device")
            L.check(L.lib.phx_solve_from(self._sys, 0, float(rtol), int(max_iter), p0, p, loc, st))
        self.stats = {"iterations": int(st[0]), "relres": st[1], "seconds": st[2],
                      "spmv": int(st[3]), "spmv_avg_s": st[4], "spmv_timed": int(st[5]),
                      "converged": bool(st[6]), "restarts": int(st[7])}
        ident = C.c_int(0)
        L.check(L.lib.phx_krylov_identity_loop(self._sys, C.byref(ident)))
        self.stats["identity_loop"] = bool(ident.value)
        L.check(L.lib.phx_krylov_reduced_loop(self._sys, C.byref(ident)))
        self.stats["reduced_loop"] = bool(ident.value)
        self.stats.update(self.precond_info())
        if getattr(self, "_elwd_coarse", 0) != 0:
            self.stats.update(self.coarse_info())
            reason = self.stats["coarse_reason"]
            if reason and self._elwd_coarse > 0:
                warnings.warn(f"coarse={self._elwd_coarse}: no coarse correction was built ({reason}); the solve used the "
                              f"vertex blocks alone", RuntimeWarning, stacklevel=2)
        if getattr(self, "_p2_coarse", 0) != 0:
            self.stats.update(self.coarse_info())
            reason = self.stats["coarse_reason"]
            if reason:
                warnings.warn(f"coarse_space={self.coarse_space!r}: no coarse correction was built ({reason}); the solve "
                              f"used the plain preconditioner", RuntimeWarning, stacklevel=2)
        check_converged(self.stats, rtol, strict)
        return out

    def split(self, w):
        """solution_wh.split() (main.py:185): (u, p) views of the mixed vector."""
        nd = self.ndofs
        return w[:nd], w[nd:]

    def estimate(self, w, parts=False):
        """Residual error indicator per cell (`phifem_amd.estimate`) of the mixed solution `w` = [u, p] that `solve()`
        returned, with the phi_h, f_h, u_D handed to the last `assemble` and the tags the mesh holds now.  All five
        nodal functions have the solver's degree, so a degree-2 solver needs levelset_degree = 2."""
        if getattr(self, "_keep", None) is None:
            raise RuntimeError("estimate: call assemble() first")
        if self.levelset_degree != self.degree:
            raise NotImplementedError("estimate: phi_h must have the degree of u_h (levelset_degree = degree)")
        from .estimate import estimate
        # the data of assemble() on the side of w: the indicator is of the kind of the solution
        if hasattr(w, "data_ptr") and w.is_cuda:
            import torch
            data = [a if hasattr(a, "data_ptr") and a.is_cuda else torch.as_tensor(np.asarray(a), device=w.device)
                    for a in self._keep]
        else:
            w = np.asarray(w)
            data = [a.cpu().numpy() if hasattr(a, "data_ptr") else a for a in self._keep]
        u, p = self.split(w)
        return estimate(self.mesh, u, p, data[0], data[1], data[2], degree=self.degree, parts=parts)

    def precond_info(self):
        """State of the fictitious-domain preconditioner after a solve (phx_precond_info)."""
        o = (C.c_double * 8)()
        L.check(L.lib.phx_precond_info(self._sys, o))
        return {"precond": {1: "box-dst", 2: "vertex-block-jacobi", 3: "vertex-block-jacobi+coarse",
                            4: "box-dst+coarse", 5: "multilevel"}.get(int(o[0]), "jacobi"), "precond_L": [int(o[1]), int(o[2]), int(o[3])],
                "precond_points": int(o[4]), "dst_avg_s": o[5], "dst_timed": int(o[6]),
                "precond_value_bytes": int(o[7])}

    def coarse_info(self):
        """The coarse-space correction after a solve (phx_coarse_info): ratio H / h, coarse DoFs of u and p, build
        seconds, operator products of the probing, bytes of the dense apply; `coarse_reason` names why a requested
        correction was not built (None when it was, or when none was asked for)."""
        o = (C.c_double * 6)()
        L.check(L.lib.phx_coarse_info(self._sys, o))
        built = o[1] + o[2] > 0
        return {"coarse_ratio": int(o[0]) if built else 0, "coarse_dofs": int(o[1] + o[2]),
                "coarse_dofs_u": int(o[1]), "coarse_dofs_p": int(o[2]), "coarse_build_s": o[3],
                "coarse_probes": int(o[4]), "coarse_apply_bytes": int(o[5]),
                "coarse_reason": None if built else getattr(self, "_coarse_reasons", _COARSE_REASONS).get(int(-o[0]))}

    def coarse_export(self):
        """(node_of, Ac^-1) of the coarse correction (phx_coarse_export): node_of[i] = field * M + node of compact
        coarse DoF i, node = i + m0 (j + m1 k) at the lattice point (i, j, k) * H."""
        nc = self.coarse_info()["coarse_dofs"]
        node_of = np.empty(nc, dtype=np.int32)
        ainv = np.empty((nc, nc), dtype=np.float64)
        L.check(L.lib.phx_coarse_export(self._sys, node_of.ctypes.data_as(C.c_void_p), ainv.ctypes.data_as(C.c_void_p)))
        return node_of, ainv

    def coarse_apply(self, v, out0):
        """One application of the coarse correction (phx_coarse_apply): (out, gc, zc) with out = out0 + D R Ac^-1 R^T v,
        gc = R^T v and zc = Ac^-1 gc.  `v`, `out0` and `out` are numpy arrays in the solver's position order."""
        if self._sys is None:
            raise ValueError("coarse_apply: call assemble() and solve() first")
        nc = self.coarse_info()["coarse_dofs"]
        vp = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        out = None if out0 is None else np.array(out0, dtype=np.float64, order="C")
        n = self.info()["n_active"]
        for a in (vp, out):
            if a is not None and a.shape != (n,):
                raise ValueError(f"coarse_apply: vectors of {n} values (the active rows, in position order) are expected")
        gc, zc = np.empty(nc, dtype=np.float64), np.empty(nc, dtype=np.float64)
        L.check(L.lib.phx_coarse_apply(self._sys, L.ptr(vp)[0], L.ptr(out)[0], L.ptr(gc)[0], L.ptr(zc)[0], L.HOST))
        return out, gc, zc

    def spmv(self, x):
        y = np.empty_like(x)
        L.check(L.lib.phx_spmv(self._sys, x.ctypes.data_as(C.c_void_p),
                               y.ctypes.data_as(C.c_void_p), L.HOST))
        return y

    def spmv_bench(self, reps=50):
        o = (C.c_double * 3)()
        L.check(L.lib.phx_spmv_bench(self._sys, int(reps), o))
        return {"ms": o[0], "algorithmic_bytes": o[1], "padded_bytes": o[2]}


_OTHER_RESIDUALS = ("estimate: the residual indicator covers the weak-Dirichlet Poisson scheme of PhiFEMSolver; this "
                    "formulation has other residuals")


class StrongDirichletSolver(PhiFEMSolver):
    """Direct ("strong Dirichlet") phi-FEM: u_h = phi_h w_h with one scalar unknown w_h -- the
    assemble -> solve -> multiply sequence of demo/strong-dirichlet/flower/main.py:83-182 over the
    C ABI (`phx_assemble_poisson_sd`).  `degree` is fe_degree (main.py:39), `levelset_degree` as
    main.py:41; the mesh is the tagged background mesh (mesh_type "bg", main.py:60-65) or the
    sub-mesh (mesh_type "sub", main.py:66-70)."""

    def __init__(self, mesh, stab_coef=1.0, degree=1, levelset_degree=1):
        if degree not in (1, 2) or levelset_degree not in (1, 2):
            raise NotImplementedError("Lagrange degrees 1 and 2 are implemented")
        self.degree, self.levelset_degree = degree, levelset_degree
        self.mesh = mesh
        self.stab_coef = float(stab_coef)
        self._sys = None
        self.stats = {}

    def assemble(self, phi_h, f_h):
        """Bilinear + linear form of main.py:104-129 (nodal data, numpy or device tensors)."""
        self._free()
        nphi = self.mesh.nv if self.levelset_degree == 1 else self.mesh.nv + self.mesh.ne
        phi_h = self._arr(phi_h, nphi)
        f_h = self._arr(f_h, self.ndofs)
        locs = {L.ptr(a)[1] for a in (phi_h, f_h)}
        if len(locs) != 1:
            raise ValueError("phi_h and f_h must both live on the host or both on the device")
        h = C.c_void_p()
        L.check(L.lib.phx_assemble_poisson_sd(
            self.mesh._h, self.stab_coef, self.degree, L.ptr(phi_h)[0], self.levelset_degree,
            L.ptr(f_h)[0], locs.pop(), C.byref(h)))
        self._sys = h
        self._phi = phi_h
        return self.info()

    def split(self, w):
        raise NotImplementedError("one scalar field: solve() returns w_h itself")

    def estimate(self, w, parts=False):
        raise NotImplementedError(_OTHER_RESIDUALS)

    def solution(self, w, solution_degree=None):
        """u_h = w_h phi_h at the nodes of the solution space (main.py:172-182: both factors are
        interpolated into the space of degree `solution_degree`, then multiplied node by node).
        Implemented for solution_degree = degree = levelset_degree, where both interpolations
        are the identity."""
        k = self.degree if solution_degree is None else solution_degree
        if not (k == self.degree == self.levelset_degree):
            raise NotImplementedError("solution_degree must equal degree and levelset_degree")
        return w * self._phi


class NeumannRobinSolver(PhiFEMSolver):
    """Neumann / Robin phi-FEM, mixed (u, y, p) in P1 x P1^d x DG0 with a P2 level-set: the assemble ->
    solve sequence of demo/robin/square/main.py:98-190 over the C ABI (`phx_assemble_poisson_flux`), on
    triangles / tetrahedra.  `robin_coef = 0`, `facet_tag = 3` is the formulation of
    demo/neumann/square/main.py:113-158 (its quadrilateral cells are not covered).  Boundary condition:
    du/dn + robin_coef u = g on {phi = 0}."""

    def __init__(self, mesh, pen_coef=1.0, stab_coef=1.0, robin_coef=0.0, facet_tag=2, quadrature_degree=10):
        self.mesh = mesh
        self.params = np.array([pen_coef, stab_coef, robin_coef], dtype=np.float64)
        self.facet_tag, self.quadrature_degree = int(facet_tag), int(quadrature_degree)
        self.degree, self.levelset_degree = 1, 2
        self._sys = None
        self.stats = {}

    def assemble(self, phi_h, f_h, g_h):
        """phi_h: degree-2 nodal values -- simplices: vertices, then edges (`mesh.p2_dof_points()`);
        quadrilaterals (the cell type of demo/neumann/square/main.py:49-50, Q1 x Q1^2 x DG0 with a Q2 level-set):
        vertices, then edge midpoints by facet id, then cell centres (`mesh.q2_dof_points()`).
        f_h, g_h (u_N / u_R, main.py:103-110): degree-1 nodal values."""
        self._free()
        m = self.mesh
        nphi = m.nv + m.nf + m.nc if m.cell_type == "quadrilateral" else m.nv + m.ne
        phi_h = self._arr(phi_h, nphi)
        f_h, g_h = self._arr(f_h, m.nv), self._arr(g_h, m.nv)
        locs = {L.ptr(a)[1] for a in (phi_h, f_h, g_h)}
        if len(locs) != 1:
            raise ValueError("phi_h, f_h and g_h must all live on the host or all on the device")
        h = C.c_void_p()
        L.check(L.lib.phx_assemble_poisson_flux(
            m._h, self.params.ctypes.data_as(C.c_void_p), self.facet_tag, self.quadrature_degree,
            L.ptr(phi_h)[0], L.ptr(f_h)[0], L.ptr(g_h)[0], locs.pop(), C.byref(h)))
        self._sys = h
        return self.info()

    def split(self, w):
        """solution_wh.split() (main.py:186): u (nv,), y (nv, d), p (nc,)."""
        m = self.mesh
        d, nv = m.gdim, m.nv
        return w[:nv], w[nv:(1 + d) * nv].reshape(d, nv).T, w[(1 + d) * nv:]

    def estimate(self, w, parts=False):
        raise NotImplementedError(_OTHER_RESIDUALS)


class InterfaceElasticitySolver(PhiFEMSolver):
    """Two-material linear elasticity with a level-set interface, 5-field mixed phi-FEM
    (u_in, u_out, y_in, y_out, p), all first-order Lagrange: the assemble -> solve sequence of
    demo/interface-elasticity/main.py:145-289 over the C ABI (`phx_assemble_elasticity_if`).

    Cells: triangles, tetrahedra, or quadrilaterals that are axis-parallel rectangles in
    tensor-product vertex order (Q1 spaces, main.py:99-108; `create_rectangle(...,
    cell_type="quadrilateral")`); other quadrilaterals raise NotImplementedError at assembly.
    The mesh must be tagged in box mode (main.py:115-117).  Solution layout: component-major
    blocks of nv entries, see `blocks()`."""

    def __init__(self, mesh, E_in=1.0, nu_in=0.3, E_out=1.0e-3, nu_out=0.3,
                 penalization_coefficient=1.0, stabilization_coefficient=1.0, deterministic=False, coarse=-1):
        """coarse (PHX_OPT_EL_COARSE): spacing H / h of the coarse-space correction of the solve on generated boxes;
        -1 automatic (on from 80 cubes per axis), 0 off.  Quadrilateral meshes have no coarse space."""
        # material parameters demo/interface-elasticity/data.py:14-22, coefficients param1.yaml:16-17
        super().__init__(mesh, deterministic=deterministic)
        self.coarse = int(coarse)
        if self.coarse > 0 and mesh.cell_type == "quadrilateral":
            raise NotImplementedError("the coarse-space correction is built on generated simplicial boxes only")
        self.params = np.array([E_in, nu_in, E_out, nu_out, penalization_coefficient,
                                stabilization_coefficient], dtype=np.float64)

    def assemble(self, phi_h, f_h, u_D, bc_vertices):
        """phi_h: (nv,) nodal level-set; f_h, u_D: (nv, d) nodal vector fields; bc_vertices:
        vertices where u_in = u_D is imposed (the box boundary in the demo, main.py:158-177)."""
        self._free()
        self._apply_options()
        m = self.mesh
        d = m.gdim
        h = C.c_void_p()
        if hasattr(phi_h, "data_ptr") and phi_h.is_cuda:
            # device-resident inputs: f_h, u_D already component-major (d, nv); bc_vertices int32
            f_cm, u_cm, bcv = f_h.contiguous(), u_D.contiguous(), bc_vertices.contiguous()
            if tuple(f_cm.shape) != (d, m.nv) or tuple(u_cm.shape) != (d, m.nv):
                raise ValueError("device f_h and u_D must be component-major (d, nv)")
            self._keep = (phi_h, f_cm, u_cm, bcv)
            L.check(L.lib.phx_assemble_elasticity_if(
                m._h, self.params.ctypes.data_as(C.c_void_p), C.c_void_p(phi_h.data_ptr()),
                C.c_void_p(f_cm.data_ptr()), C.c_void_p(u_cm.data_ptr()), C.c_void_p(bcv.data_ptr()),
                bcv.numel(), L.DEVICE, C.byref(h)))
        else:
            phi_h = np.ascontiguousarray(phi_h, dtype=np.float64)
            f_cm = np.ascontiguousarray(np.asarray(f_h, dtype=np.float64).T)   # component-major
            u_cm = np.ascontiguousarray(np.asarray(u_D, dtype=np.float64).T)
            bcv = np.ascontiguousarray(bc_vertices, dtype=np.int32)
            if phi_h.shape[0] != m.nv or f_cm.shape != (d, m.nv) or u_cm.shape != (d, m.nv):
                raise ValueError("phi_h must be (nv,), f_h and u_D (nv, d)")
            if bcv.size and (bcv.min() < 0 or bcv.max() >= m.nv):
                raise ValueError("bc_vertices out of range")
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            L.check(L.lib.phx_assemble_elasticity_if(m._h, vp(self.params), vp(phi_h), vp(f_cm), vp(u_cm),
                                                     vp(bcv), bcv.size, L.HOST, C.byref(h)))
        self._sys = h
        return self.info()

    def estimate(self, w, parts=False):
        raise NotImplementedError(_OTHER_RESIDUALS)

    def blocks(self, w):
        """Split the solution: dict of (nv, d) / (nv, d, d) arrays (solution_wh.split(), main.py:291)."""
        m = self.mesh
        d, nv = m.gdim, m.nv
        w = np.asarray(w).reshape(-1, nv)
        return {"u_in": w[0:d].T, "u_out": w[d:2 * d].T,
                "y_in": w[2 * d:2 * d + d * d].T.reshape(nv, d, d),
                "y_out": w[2 * d + d * d:2 * d + 2 * d * d].T.reshape(nv, d, d),
                "p": w[2 * d + 2 * d * d:].T}


class ElasticitySolver(PhiFEMSolver):
    """One-material linear elasticity with the displacement prescribed on the immersed boundary {phi = 0}: mixed
    (u, p) in P1^d x P1^d on triangles / tetrahedra, the vector analogue of `PhiFEMSolver` (C ABI
    `phx_assemble_elasticity_wd`; forms in DESIGN.md 7h).

        a((u,p),(v,q)) = (sigma(u), eps(v))_{dx(1,2)} - ((sigma(u) n), v)_{ds}
                         + pen h^-2 (u - phi p / h, v - phi q / h)_{dx(2)} + stab avg(h) ([sigma(u) n], [sigma(v) n])_{dS(2,3)}
        L(v,q)         = (f, v)_{dx(1,2)} + pen h^-2 (u_D, v - phi q / h)_{dx(2)}

    sigma(u) = lam tr eps(u) I + 2 mu eps(u) with lam = E nu / ((1 + nu)(1 - 2 nu)), mu = E / (2 (1 + nu)): the law
    and plane-strain convention of `InterfaceElasticitySolver`.  The coefficients are NOT rescaled by E: pen_coef and
    stab_coef are the caller's to choose for the units of E (the demo works at E = 1, as the reference's interface
    demo does by dividing f by E_in).

    The mesh is a tagged generated box / rectangle with simplex cells, a `Mesh.from_arrays` mesh, or the sub-mesh of
    `compute_tags_measures(..., box_mode=False)`.  Solution layout: component-major blocks of nv entries, u_a -> a,
    p_a -> d + a (`split`); inactive DoFs are exactly 0.  The solve preconditions with the vertex blocks
    (`stats["precond"] == "vertex-block-jacobi"`), and on request with a Galerkin coarse space on top of them
    (`coarse=`, "vertex-block-jacobi+coarse"); there is no multilevel cycle for this system."""

    _coarse_reasons = {**_COARSE_REASONS,
                       1: "not a box: the correction needs a single-rank system on a generated simplicial box (not a "
                          "sub-mesh, a caller-supplied or a refined mesh) with its vertex blocks",
                       3: "too many coarse DoFs for the dense inverse (20000) or for the device memory left"}

    def __init__(self, mesh, E=1.0, nu=0.3, pen_coef=1.0, stab_coef=1.0, deterministic=False, degree=1,
                 coarse_space=None, multilevel=False, coarse=0):
        """coarse (PHX_OPT_ELWD_COARSE): spacing H / h of the coarse-space correction of the solve on generated boxes
        (2-D and 3-D, one rank): multilinear functions of spacing H per displacement component, Galerkin coarse matrix,
        added to the vertex blocks -- the iteration count then follows H / h instead of growing with the box.  0
        (default): off; -1: the library picks H and leaves the correction off where it does not pay;
        an int >= 5: this ratio.  Built on the first solve; `stats` then carries `coarse_info()`, and a ratio that was
        asked for and could not be served is reported by a RuntimeWarning and `stats["coarse_reason"]`.  Independent of
        `InterfaceElasticitySolver(coarse=)`: the two solvers may share a mesh.  `coarse_space=` and `multilevel=` are
        the spellings of `PhiFEMSolver` options that this system does not have."""
        if getattr(mesh, "cell_type", None) == "quadrilateral":
            raise NotImplementedError("weak-Dirichlet elasticity is assembled on triangles and tetrahedra (no Q1 spaces)")
        if degree != 1:
            raise NotImplementedError("weak-Dirichlet elasticity: P1 x P1 is implemented (degree = 1)")
        if coarse_space is not None:
            raise NotImplementedError("weak-Dirichlet elasticity: the coarse-space correction is asked for with coarse= "
                                      "(coarse_space is the P2 option of PhiFEMSolver)")
        if multilevel is not False:
            raise NotImplementedError("weak-Dirichlet elasticity has no multilevel preconditioner (vertex-block Jacobi only)")
        if isinstance(coarse, bool) or not isinstance(coarse, (int, np.integer)) or not (coarse in (0, -1) or 5 <= coarse <= 4096):
            raise ValueError(f"coarse={coarse!r}: 0 (off), -1 (automatic) or an int >= 5 (H / h)")
        if coarse > 0 and getattr(mesh, "parent", None) is not None:
            raise NotImplementedError("coarse needs the box mesh (box_mode=True), not a sub-mesh")
        super().__init__(mesh, pen_coef=pen_coef, stab_coef=stab_coef, deterministic=deterministic)
        self._elwd_coarse = int(coarse)
        self.params = np.array([E, nu, pen_coef, stab_coef], dtype=np.float64)

    def assemble(self, phi_h, f_h, u_D):
        """phi_h: (nv,) nodal level-set; f_h, u_D: (nv, d) nodal vector fields on the host, or device tensors (nv,) and
        component-major (d, nv).  All three on the host or all three on the device."""
        self._free()
        self._apply_options()
        m = self.mesh
        d = m.gdim
        on_dev = [hasattr(a, "data_ptr") and a.is_cuda for a in (phi_h, f_h, u_D)]
        if any(on_dev) and not all(on_dev):
            raise ValueError("phi_h, f_h and u_D must all live on the host or all on the device")
        h = C.c_void_p()
        if all(on_dev):
            if tuple(f_h.shape) != (d, m.nv) or tuple(u_D.shape) != (d, m.nv):
                raise ValueError("device f_h and u_D must be component-major (d, nv)")
            phi_h = self._arr(phi_h, m.nv)
            f_cm, u_cm = self._arr(f_h, d * m.nv), self._arr(u_D, d * m.nv)
            loc = L.DEVICE
        else:
            phi_h = np.ascontiguousarray(phi_h, dtype=np.float64)
            f_h, u_D = np.asarray(f_h, dtype=np.float64), np.asarray(u_D, dtype=np.float64)
            if phi_h.shape != (m.nv,) or f_h.shape != (m.nv, d) or u_D.shape != (m.nv, d):
                raise ValueError("phi_h must be (nv,), f_h and u_D (nv, d)")
            f_cm, u_cm = np.ascontiguousarray(f_h.T), np.ascontiguousarray(u_D.T)   # component-major
            loc = L.HOST
        self._keep = (phi_h, f_cm, u_cm)
        L.check(L.lib.phx_assemble_elasticity_wd(m._h, self.params.ctypes.data_as(C.c_void_p), L.ptr(phi_h)[0],
                                                 L.ptr(f_cm)[0], L.ptr(u_cm)[0], loc, C.byref(h)))
        self._sys = h
        return self.info()

    def split(self, w):
        """(u, p) of the mixed solution, each (nv, d)."""
        d, nv = self.mesh.gdim, self.mesh.nv
        w = w.reshape(2 * d, nv)
        return w[:d].T, w[d:].T

    def estimate(self, w, parts=False):
        raise NotImplementedError(_OTHER_RESIDUALS)


class ReactionSolver(PhiFEMSolver):
    """Reaction-diffusion c u - Lap u = f + c g on the level-set domain, u = u_D on {phi = 0}, c >= 0 a constant: the
    P1 x P1 weak-Dirichlet scheme of `PhiFEMSolver` with a mass term (C ABI `phx_assemble_reaction_wd`)

        a((u,p),(v,q)) = a_Poisson((u,p),(v,q)) + c (u, v)_{dx(1,2)} + stab c^2 h_T^2 (u, v)_{dx(2)}
        L(v,q)         = L_Poisson(f + c g; u_D)(v,q) + stab c h_T^2 (f + c g, v)_{dx(2)}

    on triangles and tetrahedra -- one implicit step of the heat equation (`HeatSolver`).  The mass is consistent.  DoF
    layout, active set and "inactive DoFs exactly 0" are those of `PhiFEMSolver`; every row is stored (no stencil-coded
    rows on a box), `solve`, `split`, `export_csr` and `spmv` work as in the base class.  `update_rhs` evaluates the
    linear form for new data on the device and leaves the matrix alone: the per-step call of a time loop, or of a sweep
    over load cases."""

    def __init__(self, mesh, reaction, pen_coef=1.0, stab_coef=1.0, deterministic=False, degree=1):
        if getattr(mesh, "cell_type", None) == "quadrilateral":
            raise NotImplementedError("the reaction term is assembled on triangles and tetrahedra (no Q1 spaces)")
        if degree != 1:
            raise NotImplementedError("the reaction term: P1 x P1 is implemented (degree = 1)")
        reaction = float(reaction)
        if not (0.0 <= reaction < np.inf):
            raise ValueError(f"reaction={reaction!r}: a finite value >= 0")
        super().__init__(mesh, pen_coef=pen_coef, stab_coef=stab_coef, deterministic=deterministic)
        self.reaction = reaction

    def _nodal(self, arrays):
        """The nodal arrays of one call as the C ABI takes them (None stays None), all on one side."""
        nv = self.mesh.nv
        arrays = [None if a is None else self._arr(a, nv) for a in arrays]
        if len({L.ptr(a)[1] for a in arrays if a is not None}) != 1:
            raise ValueError("the nodal arrays must all live on the host or all on the device")
        return arrays

    def assemble(self, phi_h, f_h, u_D, g_h=None):
        """Matrix and right-hand side for nodal P1 data (numpy or device tensors); g_h = None counts as 0."""
        self._free()
        phi_h, f_h, u_D, g_h = self._nodal((phi_h, f_h, u_D, g_h))
        self._keep = (phi_h, f_h, u_D, g_h)
        self._tag_generation = self.mesh._tag_generation
        self._apply_options()
        h = C.c_void_p()
        L.check(L.lib.phx_assemble_reaction_wd(self.mesh._h, self.pen_coef, self.stab_coef, self.reaction,
                                               L.ptr(phi_h)[0], L.ptr(f_h)[0], L.ptr(g_h)[0], L.ptr(u_D)[0],
                                               L.ptr(phi_h)[1], C.byref(h)))
        self._sys = h
        return self.info()

    def update_rhs(self, f_h, u_D, g_h=None):
        """Right-hand side for new f_h, u_D, g_h with the phi_h of `assemble` (`phx_system_update_rhs`): a gather per
        active vertex on the device, bit-reproducible; the matrix and every solver format stay as they are."""
        if self._sys is None:
            raise RuntimeError("update_rhs: call assemble() first")
        f_h, u_D, g_h = self._nodal((f_h, u_D, g_h))
        phi_h = self._keep[0]
        if L.ptr(phi_h)[1] != L.ptr(f_h)[1]:
            raise ValueError("update_rhs: the data must live where the phi_h of assemble() lives")
        self._keep = (phi_h, f_h, u_D, g_h)
        L.check(L.lib.phx_system_update_rhs(self._sys, L.ptr(phi_h)[0], L.ptr(f_h)[0], L.ptr(g_h)[0], L.ptr(u_D)[0],
                                            L.ptr(phi_h)[1]))

    def estimate(self, w, parts=False):
        raise NotImplementedError(_OTHER_RESIDUALS)


class DiffusionSolver(ReactionSolver):
    """Variable-coefficient diffusion c u - div(kappa grad u) = f + c g on the level-set domain, u = u_D on {phi = 0}:
    kappa_h a nodal P1 field, finite and > 0, c = `reaction` >= 0 a constant (C ABI `phx_assemble_diffusion_wd`;
    DESIGN.md 7j).  With F = f + c g and kb_T / kb_F the mean of kappa_h over the vertices of a cell / facet

        a((u,p),(v,q)) = (kappa grad u, grad v)_{dx(1,2)} + c (u, v)_{dx(1,2)} - (kappa d_n u, v)_{ds(100)}
                       + pen kb_T h_T^-2 (u - phi p / h_T, v - phi q / h_T)_{dx(2)}
                       + stab h_T^2 / kb_T (c u - grad kappa . grad u, c v - grad kappa . grad v)_{dx(2)}
                       + stab avg(h) (kappa [d_n u], [d_n v])_{dS(2,3)}
        L(v,q)         = (F, v)_{dx(1,2)} + pen kb_T h_T^-2 (u_D, v - phi q / h_T)_{dx(2)}
                       + stab h_T^2 / kb_T (F, c v - grad kappa . grad v)_{dx(2)}

    on triangles and tetrahedra (boxes, `Mesh.from_arrays` meshes, sub-meshes).  kappa_h = 1 is `ReactionSolver`'s
    system.  DoF layout, active set and "inactive DoFs exactly 0" are those of `PhiFEMSolver`; every row is stored;
    `solve`, `split`, `export_csr`, `spmv`, `info` come from the base class, `update_rhs` refreshes the right-hand side
    with the kappa_h of `assemble` (the system keeps its own device copy).  A kappa_h with an entry that is not finite
    and > 0 raises ValueError before anything is built.  `estimate` refuses; `estimate_zz` serves for marking.  On a
    lattice mesh `solve` uses the plain lattice preconditioner while max kappa_h / min kappa_h <= 50 and Jacobi above
    (measured: DESIGN.md 7j)."""

    def __init__(self, mesh, reaction=0.0, pen_coef=1.0, stab_coef=1.0, deterministic=False):
        if getattr(mesh, "cell_type", None) == "quadrilateral":
            raise NotImplementedError("variable-coefficient diffusion is assembled on triangles and tetrahedra (no Q1 "
                                      "spaces)")
        super().__init__(mesh, reaction, pen_coef=pen_coef, stab_coef=stab_coef, deterministic=deterministic)

    def assemble(self, kappa_h, phi_h, f_h, u_D, g_h=None):
        """Matrix and right-hand side for nodal P1 data (numpy arrays or device tensors, all on one side); g_h = None
        counts as 0."""
        self._free()
        kappa_h, phi_h, f_h, u_D, g_h = self._nodal((kappa_h, phi_h, f_h, u_D, g_h))
        self._keep = (phi_h, f_h, u_D, g_h)      # the library copies kappa_h
        self._tag_generation = self.mesh._tag_generation
        self._apply_options()
        h = C.c_void_p()
        L.check(L.lib.phx_assemble_diffusion_wd(self.mesh._h, self.pen_coef, self.stab_coef, self.reaction,
                                                L.ptr(kappa_h)[0], L.ptr(phi_h)[0], L.ptr(f_h)[0], L.ptr(g_h)[0],
                                                L.ptr(u_D)[0], L.ptr(phi_h)[1], C.byref(h)))
        self._sys = h
        return self.info()


class ConvectionDiffusionSolver(DiffusionSolver):
    """Convection-diffusion c u + beta . grad u - div(kappa grad u) = f + c g on the level-set domain, u = u_D on
    {phi = 0}: beta_h a nodal P1 vector field of shape (nv, d), finite; kappa_h as for `DiffusionSolver`; c = `reaction`
    >= 0 and `supg_coef` >= 0 constants (C ABI `phx_assemble_convection_wd`).  With F = f + c g,
    L u = c u + beta . grad u - grad kappa . grad u, bb_T / bb_F the mean of beta_h over the vertices of a cell / facet,
    ks_T = kb_T + h_T |bb_T|, ks_F = kb_F + avg(h) |bb_F| and tau_T = h_T^2 / ks_T

        a((u,p),(v,q)) = (kappa grad u, grad v)_{dx(1,2)} + c (u, v)_{dx(1,2)} + (beta . grad u, v)_{dx(1,2)}
                       - (kappa d_n u, v)_{ds(100)} + supg tau_T (L u, beta . grad v)_{dx(1,2)}
                       + pen ks_T h_T^-2 (u - phi p / h_T, v - phi q / h_T)_{dx(2)} + stab tau_T (L u, L v)_{dx(2)}
                       + stab avg(h) |F| ks_F ([d_n u], [d_n v])_{dS(2,3)}
        L(v,q)         = (F, v)_{dx(1,2)} + supg tau_T (F, beta . grad v)_{dx(1,2)}
                       + pen ks_T h_T^-2 (u_D, v - phi q / h_T)_{dx(2)} + stab tau_T (F, L v)_{dx(2)}

    on triangles and tetrahedra.  supg_coef > 0 adds streamline diffusion (SUPG) on all of Omega_h; 0.25 removes most of
    the overshoot at outflow layers.  Dirichlet data are imposed on all of {phi = 0}, inflow and outflow alike.  beta_h = 0
    is `DiffusionSolver`'s system.  The matrix is not symmetric; `solve` is BiCGStab as everywhere.  `update_rhs`, `solve`,
    `split`, `export_csr`, `spmv` come from the base classes; `info()` and `stats` carry `peclet_max` = max over the cells
    of Omega_h of h_T |bb_T| / kb_T.  On a lattice mesh `solve` uses the plain lattice preconditioner while the contrast
    of kappa_h is <= 50 and peclet_max is below the threshold of DESIGN.md 7k, and Jacobi above.  `estimate` refuses;
    `estimate_zz` serves for marking."""

    def __init__(self, mesh, reaction=0.0, pen_coef=1.0, stab_coef=1.0, supg_coef=0.0, deterministic=False):
        supg_coef = float(supg_coef)
        if not (0.0 <= supg_coef < np.inf):
            raise ValueError(f"supg_coef={supg_coef!r}: a finite value >= 0")
        super().__init__(mesh, reaction, pen_coef=pen_coef, stab_coef=stab_coef, deterministic=deterministic)
        self.supg_coef = supg_coef

    def _velocity(self, beta_h):
        """beta_h as the C ABI takes it: (nv, d), float64, contiguous."""
        nv, d = self.mesh.nv, self.mesh.gdim
        if not hasattr(beta_h, "data_ptr"):
            beta_h = np.ascontiguousarray(beta_h, dtype=np.float64)
        if tuple(beta_h.shape) != (nv, d):
            raise ValueError(f"beta_h has shape {tuple(beta_h.shape)}, the mesh needs ({nv}, {d})")
        return self._arr(beta_h, nv * d) if hasattr(beta_h, "data_ptr") else beta_h

    def assemble(self, beta_h, phi_h, f_h, u_D, g_h=None, kappa_h=None):
        """Matrix and right-hand side for nodal P1 data (numpy arrays or device tensors, all on one side); g_h = None
        counts as 0, kappa_h = None as ones."""
        self._free()
        beta_h = self._velocity(beta_h)
        if kappa_h is None:
            if hasattr(beta_h, "data_ptr"):
                import torch
                kappa_h = torch.ones(self.mesh.nv, dtype=torch.float64, device=beta_h.device)
            else:
                kappa_h = np.ones(self.mesh.nv)
        kappa_h, phi_h, f_h, u_D, g_h = self._nodal((kappa_h, phi_h, f_h, u_D, g_h))
        if L.ptr(beta_h)[1] != L.ptr(phi_h)[1]:
            raise ValueError("the nodal arrays must all live on the host or all on the device")
        self._keep = (phi_h, f_h, u_D, g_h)      # the library copies kappa_h and beta_h
        self._tag_generation = self.mesh._tag_generation
        self._apply_options()
        h = C.c_void_p()
        L.check(L.lib.phx_assemble_convection_wd(self.mesh._h, self.pen_coef, self.stab_coef, self.supg_coef, self.reaction,
                                                 L.ptr(kappa_h)[0], L.ptr(beta_h)[0], L.ptr(phi_h)[0], L.ptr(f_h)[0],
                                                 L.ptr(g_h)[0], L.ptr(u_D)[0], L.ptr(phi_h)[1], C.byref(h)))
        self._sys = h
        return self.info()

    def convection_info(self):
        """`peclet_max`, `beta_max` = max |beta_v| and `kappa_contrast` of the assembled system (phx_convection_info)."""
        o = (C.c_double * 4)()
        L.check(L.lib.phx_convection_info(self._sys, o))
        return {"peclet_max": o[0], "beta_max": o[1], "kappa_contrast": o[3]}

    def info(self):
        return dict(super().info(), **self.convection_info())

    def solve(self, *args, **kwargs):
        out = super().solve(*args, **kwargs)
        self.stats["peclet_max"] = self.convection_info()["peclet_max"]
        return out


class HeatSolver:
    """Heat equation du/dt - Lap u = f on the level-set domain, u = u_D on {phi = 0}, by implicit time stepping on
    `ReactionSolver`: backward Euler (scheme="bdf1": c = 1 / dt, g = u^n) or BDF2 (scheme="bdf2": c = 3 / (2 dt),
    g = (4 u^n - u^{n-1}) / 3, the first step by backward Euler).  The matrix is assembled once per value of c; a step
    refreshes the right-hand side on the device and solves, started from the previous solution.

        heat = HeatSolver(mesh, dt); heat.assemble(phi_h); heat.set_state(u0)
        for n in range(steps): w = heat.step(f_h(heat.t + dt), u_D(heat.t + dt))

    With device tensors (phi_h, u0, f_h, u_D) the loop makes no host copy of a nodal field.  `u` is the u half of the
    last w, `t` the time, `stats` the solve's stats plus `rhs_seconds`.

    kappa (a nodal P1 conductivity, finite and > 0, of the kind of phi_h): du/dt - div(kappa grad u) = f, stepped on
    `DiffusionSolver` instead; nothing else in the stepper changes.  None (default): the Laplacian, as above.

    velocity (a nodal P1 vector field of shape (nv, d), of the kind of phi_h): du/dt + beta . grad u - div(kappa grad u)
    = f, stepped on `ConvectionDiffusionSolver` with `supg_coef` (kappa = None: ones).  None (default): no transport,
    and `supg_coef` is not used."""

    def __init__(self, mesh, dt, scheme="bdf1", pen_coef=1.0, stab_coef=1.0, deterministic=False, kappa=None,
                 velocity=None, supg_coef=0.0):
        if getattr(mesh, "cell_type", None) == "quadrilateral":
            raise NotImplementedError("the heat solver runs on triangles and tetrahedra (no Q1 spaces)")
        dt = float(dt)
        if not (0.0 < dt < np.inf):
            raise ValueError(f"dt={dt!r}: a finite value > 0")
        if scheme not in ("bdf1", "bdf2"):
            raise ValueError(f"scheme={scheme!r}: 'bdf1' or 'bdf2'")
        self.mesh, self.dt, self.scheme = mesh, dt, scheme
        self._kw = dict(pen_coef=pen_coef, stab_coef=stab_coef, deterministic=deterministic)
        if kappa is not None:
            if hasattr(kappa, "data_ptr"):
                if kappa.numel() != mesh.nv:
                    raise ValueError(f"kappa has {kappa.numel()} values, the mesh {mesh.nv} vertices")
            else:
                kappa = np.ascontiguousarray(kappa, dtype=np.float64)
                if kappa.shape != (mesh.nv,):
                    raise ValueError(f"kappa has shape {kappa.shape}, the mesh {mesh.nv} vertices")
        self.kappa = kappa
        if velocity is not None:
            d = mesh.gdim
            if not hasattr(velocity, "data_ptr"):
                velocity = np.ascontiguousarray(velocity, dtype=np.float64)
            if tuple(velocity.shape) != (mesh.nv, d):
                raise ValueError(f"velocity has shape {tuple(velocity.shape)}, the mesh needs ({mesh.nv}, {d})")
            supg_coef = float(supg_coef)
            if not (0.0 <= supg_coef < np.inf):
                raise ValueError(f"supg_coef={supg_coef!r}: a finite value >= 0")
        self.velocity, self.supg_coef = velocity, supg_coef
        self._solver = None
        self._phi = None
        self.u = self._u_prev = self._w = None
        self.t = 0.0
        self.stats = {}

    def _zeros_like(self, a):
        if hasattr(a, "data_ptr"):
            import torch
            return torch.zeros_like(a)
        return np.zeros(self.mesh.nv)

    def _system(self, c):
        """The reaction (with kappa: diffusion) system at coefficient c on the current tags (assembled when c or the
        tags changed)."""
        if self._solver is None or self._solver.reaction != c:
            zero = self._zeros_like(self._phi)
            if self.velocity is not None:
                solver = ConvectionDiffusionSolver(self.mesh, c, supg_coef=self.supg_coef, **self._kw)
                solver.assemble(self.velocity, self._phi, zero, zero, kappa_h=self.kappa)
            elif self.kappa is None:
                solver = ReactionSolver(self.mesh, c, **self._kw)
                solver.assemble(self._phi, zero, zero)
            else:
                solver = DiffusionSolver(self.mesh, c, **self._kw)
                solver.assemble(self.kappa, self._phi, zero, zero)
            self._solver = solver
            self._w = None     # the previous solution belongs to another active set or system
        return self._solver

    def assemble(self, phi_h):
        """Builds the system of the next step on the tags the mesh holds now.  Calling it again after re-tagging is the
        moving-domain use: the state `u` is kept as it is, and its values on vertices that are newly active are the
        caller's responsibility (set them with `set_state` before the next step)."""
        self._solver = None
        nv = self.mesh.nv
        if hasattr(phi_h, "data_ptr"):
            if phi_h.numel() != nv:
                raise ValueError(f"phi_h has {phi_h.numel()} values, the mesh {nv} vertices")
        else:
            phi_h = np.ascontiguousarray(phi_h, dtype=np.float64)
            if phi_h.shape != (nv,):
                raise ValueError(f"phi_h has shape {phi_h.shape}, the mesh {nv} vertices")
        self._phi = phi_h
        bdf2 = self.scheme == "bdf2" and self._u_prev is not None
        return self._system((1.5 if bdf2 else 1.0) / self.dt).info()

    def set_state(self, u0, t=0.0):
        """Initial (or corrected) state: nodal values of u at time t, of the kind (numpy / device tensor) of phi_h.
        The multistep history starts again: the next BDF2 step is a backward Euler step."""
        nv = self.mesh.nv
        if hasattr(u0, "data_ptr"):
            if u0.numel() != nv:
                raise ValueError(f"u0 has {u0.numel()} values, the mesh {nv} vertices")
            u0 = u0.detach().clone().reshape(nv)
        else:
            u0 = np.array(u0, dtype=np.float64)
            if u0.shape != (nv,):
                raise ValueError(f"u0 has shape {u0.shape}, the mesh {nv} vertices")
        self.u, self._u_prev, self._w = u0, None, None
        self.t = float(t)

    def step(self, f_h, u_D, rtol=1e-8, max_iter=20000, warm_start=True):
        """One step from t to t + dt with f_h, u_D at t + dt.  Returns the mixed solution w = [u, p] of the step
        (full numbering, inactive DoFs 0; a tensor for tensor data) and advances `u`, `t`, `stats`."""
        if self._phi is None:
            raise RuntimeError("step: call assemble() first")
        if self.u is None:
            raise RuntimeError("step: call set_state() first")
        import time
        if self.scheme == "bdf2" and self._u_prev is not None:
            c, g = 1.5 / self.dt, (4.0 * self.u - self._u_prev) / 3.0
        else:
            c, g = 1.0 / self.dt, self.u
        solver = self._system(c)
        t0 = time.perf_counter()
        solver.update_rhs(f_h, u_D, g)
        rhs_seconds = time.perf_counter() - t0
        x0 = self._w if warm_start else None
        out = None
        if hasattr(self.u, "data_ptr") and self.u.is_cuda:
            import torch
            out = torch.empty(2 * self.mesh.nv, dtype=torch.float64, device=self.u.device)
        w = solver.solve(rtol=rtol, max_iter=max_iter, out=out, x0=x0)
        nv = self.mesh.nv
        self._u_prev = self.u if self.scheme == "bdf2" else None
        self.u, self._w = w[:nv], w
        self.t += self.dt
        self.stats = dict(solver.stats, rhs_seconds=rhs_seconds)
        return w
