"""Every preconditioner application of the Krylov loop against a float64 restatement of the operator it must be.

The phase API (`phx_krylov_phase` 7 / 8 / 9 / 10 through `phifem_amd.dist_solver.HipBackend`) applies the
preconditioner of an assembled system to vectors of the test's choice; `tests/precond_ref.py` restates the operator
(M^-1 = R K_box^-1 R^T on the u block, Jacobi elsewhere, the inverse vertex blocks for elasticity) and the placement
rule of the lattice box.  Per case: build, tag and assemble through the public API, attach a workspace, run KR_BEGIN /
KR_BEGIN2 (KR_BEGIN builds the preconditioner exactly as `phx_solve` does), ASSERT through `phx_precond_info` that
the kind and L0, L1, L2 are what `lattice_box` predicts (the case reaches its branch), overwrite p and s, run the
phases, read phat and shat.

What is compared is always x = C phat, C the column scaling of the SELL copy (1 on unscaled u columns, 1 / A_ii on
scaled ones): x must equal M^-1 p however a system stores its scaling.  C is not taken from the library: the test
applies KR_SPMV_P to a random phat and keeps the one of the two candidates for which v = A C phat holds row by row
against the exported CSR.

Vectors: a seeded standard normal in p and another one in s (a test cannot pass by reading the wrong buffer), then
unit impulses at the extreme active points, one per face of the bounding box (the Green's-function columns: an
off-by-one in `lo` or in the skipped-line intervals shows there most sharply), again different ones in p and s.  The
impulses come AFTER the dense vector, so lattice lines that the passes skip must not show what an earlier
application left there.  The u rows of phat are pre-set to NaN before every application.

The rows outside the u block are written by `RestOut` in the kernels that produce p (k_kr_begin, k_update_p,
k_update_s), not by phase 7: they are checked on the vectors the library produced itself, after KR_BEGIN
(x_i = b_i / A_ii) and after one real iteration up to KR_UPDATE_P (phat_i = p_i bit for bit, p no longer b).

Bounds.  Lattice kinds: max |x - x_ref| <= tol max |x_ref| over the u rows, tol = 1e-12 (f64 lattice) and 2e-5 (f32
lattice), the norm and numbers of test_hip_precond.py for the same transforms; the reference's own uncertainty is
below 1e-14 (test_precond_ref.py), a structural error is O(1).  The weighted (strong-Dirichlet) cases meet 1e-12 as
well (measured on an MI355X: 6.5e-16 .. 1.2e-15 of max |x_ref|); they print the difference of the reference evaluated
with float64 and with numpy.longdouble scalings (2.5e-16 .. 3.7e-16) next to their error.
Vertex blocks: |x_v - B_v^-1 p_v|_inf <= 8 k eps cond_inf(B_v) |B_v^-1 p_v|_inf per vertex, k the block size, cond
from the reference block: Gaussian elimination with partial pivoting on a k x k block.  k_jacobi_u: 2 ulp per entry.
Every case prints its worst ratio to its bound.

The coarse-space corrections (P2 with `coarse_space`, both elasticity solves with `coarse`) are applied through
`phx_coarse_apply` and compared stage by stage with float64 references in tests/test_hip_coarse_apply.py.
Not covered: the identity- and reduced-loop phases 52 - 63 (native loop only; the phase API refuses them).  `Applied.one_iteration`
runs a real iteration only to obtain a second p: the vector phases and scalar recurrences themselves are pinned one phase
at a time by tests/test_hip_krylov_phases.py, the native loops (the reduced application `box_precond_apply_red` among
them) through truncated solves by tests/test_hip_krylov_loops.py."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import precond_ref as R
from test_hip_precond import LEVELSETS

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TOL = {8: 1e-12, 4: 2e-5}      # by bytes per lattice value (phx_precond_info)


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


# ---- level-sets ---------------------------------------------------------------------------------------------------------
def _swap(fn, order):
    return lambda x: fn(x[:, order])


SETS = dict(LEVELSETS)
# two bodies separated in y / a torus around the x axis: planes whose active x lines leave a gap in y
SETS["two_balls_y"] = _swap(LEVELSETS["two_balls"], [1, 0, 2])
SETS["torus_x"] = _swap(LEVELSETS["torus"], [2, 1, 0])


def ball(centre, r=1.0):
    return lambda x: ((x - np.asarray(centre)[:x.shape[1]]) ** 2).sum(axis=1) - r * r


def bar(axis, half):
    """A brick of half-width `half` cells along `axis` in a box of unit cells (active extent 55 / 56: see the case)."""
    c = np.full(3, 4.0)
    c[axis] = 35.2
    w = np.full(3, 2.3)
    w[axis] = half
    return lambda x: np.max(np.abs(x - c) - w, axis=1)


# ---- one assembled system and what the reference needs to know about it ----------------------------------------------
class System:
    """solver, mesh, lattice coordinates of the u entities, lattice spacing, blocks of the backend."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def tag(P, mesh, phi_v, box_mode=True, single=True):
    from phifem_amd.mesh_scripts import NodalFunction
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kw = dict(single_layer_cut=True) if single else {}
        return P.compute_tags_measures(mesh, NodalFunction(phi_v), 1, box_mode=box_mode, **kw)


def lattice_coords(pts, lo, hl):
    """Integer lattice coordinates (k = 0 in 2-D) of points on the lattice of origin lo and spacing hl."""
    q = (pts - np.asarray(lo)) / np.asarray(hl)
    ijk = np.rint(q).astype(np.int64)
    assert np.abs(q - ijk).max() < 1e-6
    if ijk.shape[1] == 2:
        ijk = np.concatenate([ijk, np.zeros((ijk.shape[0], 1), dtype=np.int64)], axis=1)
    return ijk


def set_precond(P, mesh, value):
    from phifem_amd import _lib as L
    L.check(L.lib.phx_set_option(mesh._h, L.OPT_PRECOND, value))


def weak_system(P, lo, hi, n, phi_fn, degree=1, kphi=1, precond=1, deterministic=False, submesh=False, shuffle=False):
    """Weak-Dirichlet system (PhiFEMSolver) on the box lo .. hi of n cells; submesh: box_mode=False; shuffle: the box
    handed over as arrays in a random vertex, cell and local order."""
    from phifem_amd import _lib as L_
    lo, hi, n = np.asarray(lo, float), np.asarray(hi, float), np.asarray(n)
    d = lo.size
    mesh = P.create_box(lo, hi, n)
    if shuffle:
        x, cells = mesh.x, mesh.cells
        rng = np.random.default_rng(3)
        perm = rng.permutation(x.shape[0])
        inv = np.empty_like(perm)
        inv[perm] = np.arange(perm.size)
        cs = inv[cells][rng.permutation(cells.shape[0])]
        cs = np.take_along_axis(cs, rng.permuted(np.tile(np.arange(d + 1), (cs.shape[0], 1)), axis=1), axis=1)
        mesh = P.Mesh.from_arrays("tetrahedron" if d == 3 else "triangle", x[perm], cs.astype(np.int32))
    _, _, sub, _, _ = tag(P, mesh, phi_fn(mesh.x), box_mode=not submesh)
    work = sub if submesh else mesh
    set_precond(P, work, precond)
    pts = work.p2_dof_points() if degree == 2 else work.x
    phi = phi_fn(pts) if kphi == degree else phi_fn(work.x)
    uex = np.prod(np.sin(pts + 0.3), axis=1)
    s = P.PhiFEMSolver(work, degree=degree, levelset_degree=kphi, deterministic=deterministic)
    # P1: the system keeps its own CSR copy, so the exported diagonal is the solver's bit for bit (a second assembly
    # may sum the ghost penalty in another order).  P2 systems that keep the copy are not structured: they are
    # exported by the lazy re-assembly, which is bit-identical with deterministic=True
    L_.check(L_.lib.phx_set_option(work._h, L_.OPT_EXPORT_CSR, int(degree == 1)))
    try:
        info = s.assemble(phi, float(d) * uex, uex)
    finally:
        L_.check(L_.lib.phx_set_option(work._h, L_.OPT_EXPORT_CSR, 0))
    assert info["has_csr"] == 1 or degree == 2
    h = (hi - lo) / n
    hl = h / 2 if degree == 2 else h
    return System(solver=s, mesh=work, ijk=lattice_coords(pts, lo, hl), hl=hl, n=n, gdim=d, p2=degree == 2,
                  nfields=2, blocks=None, weighted=False)


def strong_system(P, lo, hi, n, phi_fn, det_fn=None, f_fn=None, submesh=False):
    """Strong-Dirichlet system (StrongDirichletSolver, P1): the weighted lattice preconditioner."""
    lo, hi, n = np.asarray(lo, float), np.asarray(hi, float), np.asarray(n)
    d = lo.size
    mesh = P.create_box(lo, hi, n)
    _, _, sub, _, _ = tag(P, mesh, (det_fn or phi_fn)(mesh.x), box_mode=not submesh, single=False)
    work = sub if submesh else mesh
    set_precond(P, work, 1)
    x = work.x
    f = f_fn(x) if f_fn else 1.0 + np.sin(x[:, 0])
    s = P.StrongDirichletSolver(work)
    s.assemble(phi_fn(x), f)
    h = (hi - lo) / n
    return System(solver=s, mesh=work, ijk=lattice_coords(x, lo, h), hl=h, n=n, gdim=d, p2=False, nfields=1,
                  blocks=1, weighted=True)


class Applied:
    """The phase API opened on a system: workspace attached, KR_BEGIN / KR_BEGIN2 run, the exported matrix at hand."""

    def __init__(self, P, c, own_fn=None, exact=False):
        import torch
        from phifem_amd import _lib as L
        from phifem_amd import dist_solver as D
        self.torch, self.L, self.D, self.c = torch, L, D, c
        s, mesh = c.solver, c.mesh
        self.info = s.info()
        n = self.n = self.info["n_active"]
        self.dev = torch.device("cuda", mesh.device)
        self.b = D.HipBackend(s, self.dev, blocks=c.blocks)
        self.perm = self.b.perm.cpu().numpy()
        rowptr, col, val, rhs, dof = s.export_csr()
        self.A = sp.csr_matrix((val, col, rowptr), shape=(n, n))
        rhs_own, dof_own = s.export_rhs_dof()          # the solved system's own right-hand side (the CSR may be a re-assembly)
        assert np.array_equal(dof_own, dof)
        self.dof, self.rhs = dof, rhs_own
        self.diag = self.A.diagonal()[self.perm]                      # solver order from here on
        assert np.all(self.diag != 0.0)
        self.As = self.A[self.perm][:, self.perm].tocsr()
        nent = self.info["n_full"] // c.nfields if c.nfields in (1, 2) else 0
        self.ent = dof[self.perm]                                      # full index of solver row i
        self.is_u = self.ent < nent
        if nent:
            assert self.is_u.sum() == self.info["n_active_u"]
            assert np.array_equal(self.is_u, self.perm < self.is_u.sum())
        own = np.ones(n, dtype=np.uint8) if own_fn is None else own_fn(self).astype(np.uint8)
        self.own_np = own.astype(bool)
        self.work = torch.zeros(10 * n, dtype=torch.float64, device=self.dev)
        self.scal = torch.zeros(D.SCAL_DOUBLES, dtype=torch.float64, device=self.dev)
        self.own = torch.from_numpy(own).to(self.dev)
        torch.cuda.synchronize(self.dev)
        self.b.attach(self.work, self.scal, self.own)
        s._apply_options()
        self.exact = False
        if exact:
            self.exact = self._setup_exact()
            assert self.exact
        self.b.phase(D.KR_BEGIN)
        self.b.phase(D.KR_BEGIN2)
        mesh.synchronize()
        o = (C.c_double * 8)()
        L.check(L.lib.phx_precond_info(s._sys, o))
        self.kind, self.L, self.vbytes = int(o[0]), [int(o[1]), int(o[2]), int(o[3])], int(o[7])
        self.hat = self.b.precond_active()

    def _setup_exact(self):
        """The slab-exact preconditioner on one rank (HipBackend.setup_exact_precond without the collectives): one
        slab that owns every vertex plane."""
        torch, L, b = self.torch, self.L, self.b
        bb = (C.c_int64 * 6)()
        L.check(L.lib.phx_precond_local_bbox(b.sys, bb))
        zb = (C.c_int64 * 2)(0, int(self.c.n[2]) + 1)
        ncol = C.c_int64(0)
        L.check(L.lib.phx_precond_setup_global(b.sys, bb, 1, 0, zb, C.byref(ncol)))
        if ncol.value <= 0:
            return False
        b.carry_send = torch.zeros(2 * ncol.value, dtype=torch.float64, device=self.dev)
        b.carry_recv = torch.zeros(2 * ncol.value, dtype=torch.float64, device=self.dev)
        torch.cuda.synchronize(self.dev)
        L.check(L.lib.phx_precond_set_carry_buffers(b.sys, C.c_void_p(b.carry_send.data_ptr()),
                                                    C.c_void_p(b.carry_recv.data_ptr())))
        b.exact = True
        di = (C.c_int64 * 4)()
        L.check(L.lib.phx_precond_dist_info(b.sys, di))
        assert di[0] == 1 and di[1] == 2 * ncol.value
        return True

    def vec(self, k):
        n = self.n
        return self.work[k * n:(k + 1) * n]

    def read(self):
        """The ten vectors of the workspace as numpy arrays."""
        self.c.mesh.synchronize()
        w = self.work.cpu().numpy().copy()
        n = self.n
        names = ("r", "rhat", "p", "v", "s", "t", "y", "b", "phat", "shat")
        return {k: w[i * n:(i + 1) * n] for i, k in enumerate(names)}

    def put(self, k, a):
        self.vec(k).copy_(self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev))

    def _carries(self):
        self.c.mesh.synchronize()
        self.b.carry_recv.copy_(self.b.carry_send)
        self.torch.cuda.synchronize(self.dev)

    def precond(self, which):
        """phat = P p (which = 0) or shat = P s (1), both halves of the slab-exact variant."""
        D = self.D
        self.b.phase(D.KR_PRECOND_S if which else D.KR_PRECOND_P)
        if self.exact:
            self._carries()
            self.b.phase(D.KR_EXACT_S if which else D.KR_EXACT_P)

    def apply(self, p, s, poison=None):
        """(phat, shat) for p and s of the test's choice; `poison`: rows of phat / shat pre-set to NaN."""
        assert self.hat
        pre = np.zeros(self.n)
        if poison is not None:
            pre[poison] = np.nan
        self.put(2, p)
        self.put(4, s)
        self.put(8, pre)
        self.put(9, pre)
        self.torch.cuda.synchronize(self.dev)
        self.precond(0)
        self.precond(1)
        w = self.read()
        return w["phat"], w["shat"]

    def one_iteration(self):
        """One real BiCGStab iteration up to KR_UPDATE_P, as DistributedSolver.solve runs it on one rank."""
        D = self.D
        if self.hat:
            self.precond(0)
        self.b.phase(D.KR_SPMV_P)
        self.b.phase(D.KR_UPDATE_S)
        if self.hat:
            self.precond(1)
        self.b.phase(D.KR_SPMV_S)
        self.b.phase(D.KR_UPDATE_XR)
        self.b.phase(D.KR_UPDATE_P)

    def column_scaling(self):
        """C of the SELL copy, found by experiment: v = A C phat for a random phat (KR_SPMV_P) must hold row by row,
        |v_i - (A C phat)_i| <= 4 k eps (|A| |C phat|)_i (test_hip_stencil_paths.py), for exactly one of
        C = 1 / diag everywhere and C = 1 on the u columns."""
        z = np.random.default_rng(77).standard_normal(self.n)
        self.put(8 if self.hat else 2, z)
        self.torch.cuda.synchronize(self.dev)
        self.b.phase(self.D.KR_SPMV_P)
        v = self.read()["v"]
        k = int(np.diff(self.As.indptr).max())
        absA = abs(self.As)
        fits = {}
        for name, cs in (("scaled", 1.0 / self.diag), ("unscaled", np.where(self.is_u, 1.0, 1.0 / self.diag))):
            ratio = np.abs(v - self.As @ (cs * z)) / (EPS * (absA @ np.abs(cs * z)))
            fits[name] = (float(ratio[self.own_np].max()), cs)
        good = [nm for nm, (r, _) in fits.items() if r <= 4 * k]
        assert good, {nm: r for nm, (r, _) in fits.items()}
        if not self.is_u.any():
            return "scaled", fits["scaled"][1]
        assert len(good) == 1, {nm: r for nm, (r, _) in fits.items()}
        return good[0], fits[good[0]][1]


def impulses(ijk_rows, rows, n):
    """Six unit vectors (fewer in 2-D): one at an active point of minimal and of maximal coordinate per axis."""
    out = []
    for a in range(3):
        if ijk_rows[:, a].min() == ijk_rows[:, a].max():
            continue
        for pick in (np.argmin, np.argmax):
            e = np.zeros(n)
            e[rows[pick(ijk_rows[:, a])]] = 1.0
            out.append(e)
    return out


def check_non_u_rows(ap, cs, stage, w):
    """RestOut: the rows outside the u block of phat hold the library's own p bit for bit, so x = C phat = p / A_ii."""
    rest = ~ap.is_u
    if not rest.any():
        return 0.0
    assert np.array_equal(w["phat"][rest], w["p"][rest]), f"{stage}: phat differs from p outside the u block"
    x, ref = (cs * w["phat"])[rest], w["p"][rest] / ap.diag[rest]
    err = np.abs(x - ref)
    assert np.all(err <= 2 * EPS * np.abs(ref)), f"{stage}: {np.flatnonzero(err > 2 * EPS * np.abs(ref))[:8]}"
    return float((err / np.maximum(2 * EPS * np.abs(ref), 1e-300)).max())


def run_lattice_case(P, name, c, own_fn=None, exact=False, expect=None, twice=False):
    """The whole check of a lattice-preconditioned system; `expect(active_ijk, L, lo)`: the branch assertions."""
    ap = Applied(P, c, own_fn=own_fn, exact=exact)
    n, is_u, own = ap.n, ap.is_u, ap.own_np
    rows = np.flatnonzero(is_u & own)                     # solver rows the lattice serves
    act = c.ijk[ap.ent[rows]]
    box = R.lattice_box(act, c.n, c.gdim, p2=c.p2)
    assert box is not None
    Lref, lo = box
    assert ap.kind == 1 and ap.L == Lref, (name, ap.kind, ap.L, Lref, lo)
    assert ap.hat and ap.vbytes in TOL
    if expect:
        expect(act, Lref, lo)
    w0 = ap.read()
    # after KR_BEGIN: p = b on owned rows
    bvec = np.where(own, ap.rhs[ap.perm], 0.0)
    assert np.array_equal(w0["p"], bvec)
    ap.one_iteration()
    w1 = ap.read()
    assert np.any(w1["p"][~is_u & own] != bvec[~is_u & own]) or not (~is_u).any()
    kind, cs = ap.column_scaling()
    q_rest = max(check_non_u_rows(ap, cs, "after KR_BEGIN", w0), check_non_u_rows(ap, cs, "after KR_UPDATE_P", w1))
    weights = ap.diag[rows] if c.weighted else None
    tol = TOL[ap.vbytes]
    rng = np.random.default_rng(5)
    vecs = [rng.standard_normal(n), rng.standard_normal(n)] + impulses(act, rows, n)
    if len(vecs) % 2:
        vecs.append(vecs[2])
    worst, selfdiff, first = 0.0, 0.0, None
    for k in range(0, len(vecs), 2):
        p, s = vecs[k], vecs[k + 1]
        phat, shat = ap.apply(p, s, poison=rows)
        if first is None:
            first = phat.copy()
        for what, v, hat in ((f"p[{k}]", p, phat), (f"s[{k + 1}]", s, shat)):
            ref = R.apply_minv_u(v[rows], act, Lref, lo, c.hl if c.gdim == 3 else list(c.hl) + [0.0],
                                 weights=weights, gdim=c.gdim)
            x = (cs * hat)[rows]
            assert np.all(np.isfinite(x)), f"{name} {what}: {np.flatnonzero(~np.isfinite(x))[:8]} not written"
            err = np.abs(x - ref).max() / np.abs(ref).max()
            if c.weighted:
                ref_ld = R.apply_minv_u(v[rows], act, Lref, lo, c.hl if c.gdim == 3 else list(c.hl) + [0.0],
                                        weights=weights, gdim=c.gdim, scalings=np.longdouble)
                selfdiff = max(selfdiff, float(np.abs(ref_ld - ref).max() / np.abs(ref).max()))
            at = int(np.abs(x - ref).argmax())
            assert err <= tol, (f"{name} {what}: {err:.3e} of max|x_ref| (tol {tol:g}), worst at lattice point "
                                f"{act[at].tolist()} (L {Lref}, lo {lo}, C {kind})")
            worst = max(worst, err / tol)
            # u rows this rank does not own are never written
            assert np.all(hat[is_u & ~own] == 0.0)
    if twice:
        again, _ = ap.apply(vecs[0], vecs[1], poison=rows)
        assert np.array_equal(again[rows], first[rows]), "two applications to the same vector differ"
    bbox = np.stack([act.min(axis=0), act.max(axis=0)]).tolist()
    print(f"[{name}] n={ap.n} u rows={rows.size} bbox={bbox} L={Lref} lo={lo} C={kind} f{8 * ap.vbytes} "
          f"exact={ap.exact} vectors={len(vecs)}: worst {worst:.2e} of the bound {tol:g}; non-u rows {q_rest:.2f} of "
          f"2 ulp" + (f"; reference f64 vs longdouble scalings {selfdiff:.2e}" if c.weighted else ""))
    return ap, act, Lref, lo


def y_gap(act, L, lo):
    """Some z plane whose active x lines leave a gap in y (k_line_intervals fills the hull)."""
    for z in np.unique(act[:, 2]):
        ys = np.unique(act[act[:, 2] == z, 1])
        if ys.size and ys.max() - ys.min() + 1 > ys.size:
            return True
    return False


BOX = ([-1.5] * 3, [1.5] * 3)

# name -> (lo, hi, n, level-set, keyword arguments of weak_system, branch assertion)
P1_CASES = {
    "sphere": (*BOX, [32] * 3, SETS["sphere"], {}, None),
    "sphere_anisotropic": ([-1.5, -1.4, -1.3], [1.5, 1.6, 1.2], [32, 40, 24], SETS["sphere"], {}, None),
    "two_balls": (*BOX, [32] * 3, SETS["two_balls"], {}, None),
    "torus": (*BOX, [32] * 3, SETS["torus"], {}, None),
    "two_balls_y": (*BOX, [32] * 3, SETS["two_balls_y"], {}, lambda a, L, lo: y_gap(a, L, lo) or pytest.fail("no gap")),
    "torus_x": (*BOX, [32] * 3, SETS["torus_x"], {}, lambda a, L, lo: y_gap(a, L, lo) or pytest.fail("no gap")),
    # the lattice box reaches past the x = 1.5 face of the mesh (32 cells): gmap = -1 out there
    "boundary_crossing": (*BOX, [32] * 3, SETS["boundary_crossing"], {},
                          lambda a, L, lo: (a[:, 0].max() == 32 and lo[0] + L[0] > 32) or pytest.fail("inside the mesh")),
    # open z margins: ball cut by the z = 0 face, by the top face, by both
    "cut_bottom": (*BOX, [24] * 3, ball([0.0, 0.0, -1.1]), {},
                   lambda a, L, lo: (a[:, 2].min() == 0 and a[:, 2].max() < 24
                                     and L[2] == a[:, 2].max() + 1 + 32 + 4 + 1 and lo[2] == -33) or pytest.fail("margins")),
    "cut_top": (*BOX, [24] * 3, ball([0.0, 0.0, 1.1]), {},
                lambda a, L, lo: (a[:, 2].min() > 0 and a[:, 2].max() == 24
                                  and L[2] == 24 - a[:, 2].min() + 1 + 4 + 32 + 1 and lo[2] == a[:, 2].min() - 5)
                or pytest.fail("margins")),
    "cut_both": ([-1.5, -1.5, -0.6], [1.5, 1.5, 0.6], [24, 24, 10], SETS["sphere"], {},
                 lambda a, L, lo: (a[:, 2].min() == 0 and a[:, 2].max() == 10 and L[2] == 11 + 64 + 1 and lo[2] == -33)
                 or pytest.fail("margins")),
    # both sides of a pick-length boundary: extent 55 -> L = 64 ((L - 1 - extent) = 8, even), 56 -> 128 (71, odd)
    "extent55_x": ([0.0] * 3, [70.0, 8.0, 8.0], [70, 8, 8], bar(0, 26.3), {},
                   lambda a, L, lo: (np.ptp(a[:, 0]) + 1 == 55 and L[0] == 64) or pytest.fail("extent")),
    "extent56_x": ([0.0] * 3, [70.0, 8.0, 8.0], [70, 8, 8], bar(0, 26.8), {},
                   lambda a, L, lo: (np.ptp(a[:, 0]) + 1 == 56 and L[0] == 128) or pytest.fail("extent")),
    "extent55_y": ([0.0] * 3, [8.0, 70.0, 8.0], [8, 70, 8], bar(1, 26.3), {},
                   lambda a, L, lo: (np.ptp(a[:, 1]) + 1 == 55 and L[1] == 64) or pytest.fail("extent")),
    "extent56_y": ([0.0] * 3, [8.0, 70.0, 8.0], [8, 70, 8], bar(1, 26.8), {},
                   lambda a, L, lo: (np.ptp(a[:, 1]) + 1 == 56 and L[1] == 128) or pytest.fail("extent")),
    "disk_2d": ([-1.5] * 2, [1.5] * 2, [48] * 2, SETS["sphere"], {},
                lambda a, L, lo: (L[2] == 2 and lo[2] == -1) or pytest.fail("2-D")),
    # f32 lattice
    "sphere_f32": (*BOX, [32] * 3, SETS["sphere"], dict(precond=2), None),
    "torus_x_f32": (*BOX, [32] * 3, SETS["torus_x"], dict(precond=2), None),
    # sub-mesh of a box (on_box_lattice, lat2v) and a box handed over as shuffled arrays (v2lat)
    "submesh_3d": (*BOX, [16] * 3, SETS["offset_ellipsoid"], dict(submesh=True), None),
    "submesh_2d": ([-1.5] * 2, [1.5] * 2, [40] * 2, ball([0.1, -0.05]), dict(submesh=True), None),
    "shuffled_arrays_3d": (*BOX, [12] * 3, SETS["sphere"], dict(shuffle=True), None),
    "shuffled_arrays_2d": ([-1.5] * 2, [1.5] * 2, [40] * 2, SETS["sphere"], dict(shuffle=True), None),
}


@pytest.mark.parametrize("name", list(P1_CASES))
def test_p1_weak_dirichlet(P, name):
    lo, hi, n, phi, kw, expect = P1_CASES[name]
    c = weak_system(P, lo, hi, n, phi, **kw)
    ap, act, L, lo_ = run_lattice_case(P, name, c, expect=expect)
    assert ap.vbytes == (4 if kw.get("precond") == 2 else 8)


def test_deterministic_application_is_bit_reproducible(P):
    c = weak_system(P, *BOX, [32] * 3, SETS["offset_ellipsoid"], deterministic=True)
    run_lattice_case(P, "deterministic", c, twice=True)


# P2: k_active_bbox_p2, k_box_gmap_p2, the h / 2 lattice
P2_CASES = {
    "p2_2d_kphi1": ([-1.5] * 2, [1.5] * 2, [20] * 2, ball([0.03, -0.02]), dict(kphi=1), None),
    "p2_2d_kphi2": ([-1.5] * 2, [1.5] * 2, [20] * 2, ball([0.03, -0.02]), dict(kphi=2), None),
    "p2_3d_kphi1": (*BOX, [10] * 3, ball([0.03, -0.02, 0.01]), dict(kphi=1), None),
    "p2_3d_kphi2": (*BOX, [10] * 3, ball([0.03, -0.02, 0.01]), dict(kphi=2), None),
    # the top face of the h / 2 lattice is its plane 2 n2
    "p2_3d_cut_top": (*BOX, [10] * 3, ball([0.0, 0.0, 1.0]), dict(kphi=2),
                      lambda a, L, lo: (a[:, 2].max() == 20 and a[:, 2].min() > 0
                                        and L[2] == 20 - a[:, 2].min() + 1 + 4 + 32 + 1) or pytest.fail("margins")),
}


@pytest.mark.parametrize("name", list(P2_CASES))
def test_p2_weak_dirichlet(P, name):
    lo, hi, n, phi, kw, expect = P2_CASES[name]
    c = weak_system(P, lo, hi, n, phi, degree=2, **kw)
    ap, act, L, lo_ = run_lattice_case(P, name, c, expect=expect)
    assert (act % 2 == 1).any()          # edge midpoints among the active points


def flower_system(P, submesh=False):
    import flower_data as F
    return strong_system(P, [-4.5] * 2, [4.5] * 2, [64] * 2, lambda x: F.levelset(x.T),
                         det_fn=lambda x: F.detection_levelset(x.T), f_fn=lambda x: F.source_term(x.T), submesh=submesh)


SD_CASES = {
    "sd_box_2d": lambda P: strong_system(P, [-1.5] * 2, [1.5] * 2, [32] * 2, ball([0.03, -0.02])),
    "sd_flower_2d": lambda P: flower_system(P),
    "sd_flower_2d_submesh": lambda P: flower_system(P, submesh=True),
    "sd_ball_3d": lambda P: strong_system(P, *BOX, [16] * 3, ball([0.03, -0.02, 0.01])),
}


@pytest.mark.parametrize("name", list(SD_CASES))
def test_strong_dirichlet_weighted(P, name):
    """S^-1 K_box^-1 S^-1 with S^2 = |diag A| / kd (k_dscale_weighted)."""
    c = SD_CASES[name](P)
    ap, act, L, lo = run_lattice_case(P, name, c)
    assert not (~ap.is_u).any()


@pytest.mark.parametrize("name", ["sphere", "cut_bottom"])
def test_slab_exact_on_one_rank(P, name):
    """phx_precond_setup_global with nranks = 1 and zb = [0, nz + 1]: box_middle_A, the copy of the carries,
    box_middle_B; the same operator and the same bound as the one-piece application."""
    lo, hi, n, phi, kw, expect = P1_CASES[name]
    c = weak_system(P, lo, hi, n, phi, **kw)
    ap, act, L, lo_ = run_lattice_case(P, name + "_exact", c, exact=True, expect=expect)
    assert ap.exact


def test_rank_local_with_the_upper_half_unowned(P):
    """`own` mask of a slab solve: bounding box and gmap over the owned rows only; the unowned u rows of phat stay 0."""
    lo, hi, n, phi, kw, _ = P1_CASES["sphere"]
    c = weak_system(P, lo, hi, n, phi)

    def own_fn(ap):
        nent = ap.info["n_full"] // 2
        return c.ijk[ap.ent % nent][:, 2] < n[2] // 2

    def expect(act, L, lo_):
        if not (act[:, 2].max() == n[2] // 2 - 1 and L[2] == act[:, 2].max() - act[:, 2].min() + 1 + 9):
            pytest.fail("the box is not the owned half")

    ap, act, L, lo_ = run_lattice_case(P, "upper_half_unowned", c, own_fn=own_fn, expect=expect)
    assert (ap.is_u & ~ap.own_np).sum() > 100


# ---- vertex-block Jacobi of the elasticity system ----------------------------------------------------------------------
def elasticity_system(P, d, n, E_out, quad):
    from oracle import elasticity as EL
    if quad:
        mesh = P.create_rectangle([[-1.5, -1.5], [1.5, 1.5]], [n, n], cell_type="quadrilateral")
    else:
        mesh = P.create_box([-1.5] * d, [1.5] * d, [n] * d)
    x = mesh.x
    phi = 1.0 - ((x - np.array([0.04, -0.03, 0.02])[:d]) ** 2).sum(axis=1)
    tag(P, mesh, phi, single=False)
    ijk = lattice_coords(x, [-1.5] * d, [3.0 / n] * d)
    bcv = np.flatnonzero(np.any((ijk[:, :d] == 0) | (ijk[:, :d] == n), axis=1))
    rng = np.random.default_rng(5)
    f = np.sin(x @ rng.standard_normal((d, d))) + 0.3
    uD = np.cos(x @ rng.standard_normal((d, d)))
    set_precond(P, mesh, 1)
    s = P.InterfaceElasticitySolver(mesh, E_in=1.0, E_out=E_out, coarse=0)
    s.assemble(phi, f, uD, bcv)
    return System(solver=s, mesh=mesh, ijk=ijk, n=np.array([n] * d), gdim=d, nfields=0, blocks=EL.Blocks(d).C,
                  weighted=False, p2=False)


@pytest.mark.parametrize("E_out", [1.0, 1.0e-3])
@pytest.mark.parametrize("d,n,quad", [(2, 16, False), (3, 6, False), (2, 16, True)])
def test_elasticity_vertex_blocks(P, d, n, quad, E_out):
    """k_bj_build / k_bj_apply: x_v = B_v^-1 p_v per vertex, B_v the diagonal block of the exported CSR."""
    c = elasticity_system(P, d, n, E_out, quad)
    ap = Applied(P, c)
    assert ap.kind == 2 and ap.hat, ap.kind
    kind, cs = ap.column_scaling()
    nv = c.mesh.nv
    assert ap.info["n_full"] == c.blocks * nv
    rng = np.random.default_rng(6)
    vert = ap.ent % nv                                     # vertex of solver row i
    act_v = np.unique(vert)
    vij = c.ijk[act_v]
    ext = np.unique([act_v[f(vij[:, a])] for a in range(d) for f in (np.argmin, np.argmax)])
    e_first, e_last = np.zeros(ap.n), np.zeros(ap.n)
    for v in ext:                                          # blocks are independent: one impulse per extreme vertex
        r = np.flatnonzero(vert == v)
        r = r[np.argsort(ap.ent[r])]
        e_first[r[0]] = 1.0
        e_last[r[-1]] = 1.0
    vecs = [rng.standard_normal(ap.n), rng.standard_normal(ap.n), e_last, e_first]
    iperm = np.empty(ap.n, dtype=np.int64)
    iperm[ap.perm] = np.arange(ap.n)
    worst, kmax, cmax = 0.0, 0, 0.0
    for k in (0, 2):
        hats = ap.apply(vecs[k], vecs[k + 1], poison=np.arange(ap.n))
        for v, hat in zip(vecs[k:k + 2], hats):
            x = cs * hat
            assert np.all(np.isfinite(x))
            # reference in active numbering
            ref_a, groups, conds = R.apply_block_jacobi(v[iperm], ap.A, ap.dof, nv)
            xa = x[iperm]
            for rows, cnd in zip(groups, conds):
                kk = rows.size
                scale = np.abs(ref_a[rows]).max()
                err = np.abs(xa[rows] - ref_a[rows]).max()
                bound = 8 * kk * EPS * cnd * scale
                assert err <= bound, (f"vertex {int(ap.dof[rows[0]] % nv)} (k = {kk}, cond {cnd:.2e}): {err:.3e} > "
                                      f"{bound:.3e}; x {xa[rows]} ref {ref_a[rows]}")
                if scale > 0.0:
                    worst = max(worst, err / bound)
                kmax, cmax = max(kmax, kk), max(cmax, cnd)
    print(f"[elasticity d={d} n={n} quad={quad} E_out={E_out}] n={ap.n} vertices={act_v.size} largest block {kmax} "
          f"largest cond {cmax:.2e} C={kind}: worst {worst:.2e} of the bound 8 k eps cond")


# ---- k_jacobi_u: structured systems with the lattice preconditioner configured out ------------------------------------
@pytest.mark.parametrize("degree,n", [(1, 16), (2, 8)])
def test_jacobi_u_of_structured_systems(P, degree, n):
    """OPT_PRECOND = 0 on a Kuhn box: u columns are unscaled and phase 7 divides the u rows by the diagonal; x = C phat
    = p / A_ii on every row, to 2 ulp."""
    c = weak_system(P, *BOX, [n] * 3, SETS["sphere"], degree=degree, kphi=degree, precond=0, deterministic=degree == 2)
    try:
        ap = Applied(P, c)
        assert ap.kind == 0 and ap.hat, (ap.kind, ap.hat)      # phat / shat apart from p / s: k_jacobi_u runs
        kind, cs = ap.column_scaling()
        assert kind == "unscaled"
        rng = np.random.default_rng(9)
        p, s = rng.standard_normal(ap.n), rng.standard_normal(ap.n)
        phat, shat = ap.apply(p, s, poison=np.arange(ap.n))
        worst = 0.0
        for v, hat in ((p, phat), (s, shat)):
            ref = R.apply_minv(v, ap.diag, ap.is_u)
            err = np.abs(cs * hat - ref)
            assert np.all(err <= 2 * EPS * np.abs(ref)), np.flatnonzero(err > 2 * EPS * np.abs(ref))[:8]
            worst = max(worst, float((err / (2 * EPS * np.abs(ref))).max()))
        print(f"[jacobi_u degree={degree} n={n}] rows={ap.n} u rows={ap.is_u.sum()}: worst {worst:.2f} of 2 ulp")
    finally:
        set_precond(P, c.mesh, 1)
