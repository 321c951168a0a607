"""Restriction (`phifem_amd.restrict`) and the multilevel preconditioner (`PhiFEMSolver(..., multilevel=True)`) on the
GPU against the numpy specification tests/multilevel_ref.py.

Hierarchies (the smallest that reach every branch):
  disk3        `disk` (212 triangles), 3 marked rounds on the 10 % of cells nearest a point: three index chains, vertex
               counts that are no multiples of 64
  disk_empty   `disk`, one such round, then one round with an EMPTY mask: zero new vertices.  The level is KEPT (a copy of
               the level below with an empty transfer), not skipped: the V-cycle smooths on it like on any other
  graded_tet   `graded_tet_box`, 2 marked rounds: 3-D, high valence
  kuhn3        3^3 Kuhn box, uniformly refined once (the fine mesh is re-created as a lattice mesh), then one marked
               round: lattice base; coarse kind 1 (the lattice solve of level 0, kind 2, is not built)
  box8         8^3 Kuhn box with 2 Doerfler rounds of its own sphere solve: a whole solve in 3-D
  rect_big     51 x 51 rectangle of triangles (2704 vertices > 2048) with one marked round: coarse kind 0

Bounds: the restriction equals the reference bit for bit; <restrict(r), x> = <r, prolongate(x)> to 1e-13 relative;
the operator meets max |x - x_ref| <= 1e-12 max |x_ref| (the bound of test_hip_precond_operator.py for f64 lattice
kinds); solutions agree with the Jacobi solve's to 100 rtol; strictly fewer iterations than Jacobi.

The solves run with deterministic=True, so their figures are the same on every run (measured on an MI355X: disk
level 5 |w_multilevel - w_jacobi| = 4.5e-7 of max |w|, 66 iterations against 176; box8 1.0e-7, 114 against 256).  The
100 rtol margin on the disk is thin for a reason that is the system's, not the preconditioner's: either solve alone is
70 - 130 relres away from the direct solve of the exported matrix (cond(A D^-1) ~ 5e3 on level 0 already), and without
deterministic dot products the difference of the two was seen between 6.5e-7 and 1.7e-6 from run to run."""
import ctypes as C
import functools
import gc
import warnings

import numpy as np
import pytest

import multilevel_ref as ML
import partition_ref as PR
import refine_marked_ref as RM
from datasets import load_mesh
from test_hip_precond_operator import Applied, System, check_non_u_rows

pytestmark = pytest.mark.gpu
RTOL = 1e-8


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def live_bytes():
    from phifem_amd import _lib as L
    a, b = C.c_int64(0), C.c_int64(0)
    L.check(L.lib.phx_pool_stats(C.byref(a), C.byref(b)))
    return a.value


def _point(x):
    lo, hi = x.min(axis=0), x.max(axis=0)
    return lo + (hi - lo) * np.array([0.37, 0.58, 0.44][:x.shape[1]])


def _ctype(mesh):
    return mesh.cell_type


def level_of(mesh, pairs):
    return dict(ctype=_ctype(mesh), x=mesh.x, cells=mesh.cells.astype(np.int64), pairs=pairs)


def refine_marked(P, mesh, mask):
    """(fine mesh, pairs): the library's refinement, its transfer pairs from the specification on the library's own
    edge numbering (tests/test_hip_refine_marked.py pins the two to each other)."""
    fine = P.refine(mesh, marked=mask)
    ref = RM.refine_marked_ref(_ctype(mesh), mesh.x, mesh.cells.astype(np.int64), cell_marks=np.asarray(mask),
                               edges=mesh.edges)
    assert np.array_equal(fine.x, ref["x"]) and np.array_equal(fine.cells, ref["cells"])
    return fine, ML.pairs_marked(ref)


def refine_uniform(P, mesh):
    fine = P.refine(mesh)
    return fine, np.asarray(mesh.edges, dtype=np.int64)


def nearest_rounds(P, mesh, rounds):
    meshes, levels = [mesh], [level_of(mesh, None)]
    for _ in range(rounds):
        m = meshes[-1]
        fine, pairs = refine_marked(P, m, RM.nearest_mask(m.x, m.cells, _point(m.x)))
        meshes.append(fine)
        levels.append(level_of(fine, pairs))
    return meshes, levels


def build_hierarchy(P, name):
    """-> (meshes, levels) of levels 0 .. L"""
    if name in ("disk3", "disk_empty"):
        ctype, x, cells = load_mesh("disk")
        meshes, levels = nearest_rounds(P, P.Mesh.from_arrays(ctype, x, cells), 3 if name == "disk3" else 1)
        if name == "disk_empty":
            fine, pairs = refine_marked(P, meshes[-1], np.zeros(meshes[-1].nc, dtype=np.uint8))
            assert fine.nv == meshes[-1].nv and pairs.shape[0] == 0
            meshes.append(fine)
            levels.append(level_of(fine, pairs))
        return meshes, levels
    if name == "graded_tet":
        x, cells = PR.graded_tet_box()
        return nearest_rounds(P, P.Mesh.from_arrays("tetrahedron", x, cells), 2)
    if name == "kuhn3":
        box = P.create_box([-1.5] * 3, [1.5] * 3, [3] * 3)
        fine, pairs = refine_uniform(P, box)
        meshes, levels = [box, fine], [level_of(box, None), level_of(fine, pairs)]
        m2, l2 = nearest_rounds(P, fine, 1)
        return meshes + m2[1:], levels + l2[1:]
    if name == "rect_big":
        rect = P.create_rectangle([[-1.5, -1.5], [1.5, 1.5]], [51, 51])
        assert rect.nv > ML.DENSE_CAP
        return nearest_rounds(P, rect, 1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _hier(name):
    import phifem_amd
    return build_hierarchy(phifem_amd, name)


def levelset(name, x):
    if name.startswith("disk"):
        _, x0, _ = load_mesh("disk")
        cen = x0.mean(axis=0) + np.array([0.013, -0.007])
        r = 0.62 * 0.5 * (x0.max(axis=0) - x0.min(axis=0)).min()
        return ((x - cen) ** 2).sum(axis=1) - r ** 2
    return (x ** 2).sum(axis=1) - 1.1 ** 2


def tagged_solver(P, name, mesh, **kw):
    from phifem_amd.mesh_scripts import NodalFunction
    x = mesh.x
    phi = levelset(name, x)
    uD = np.sin(x[:, 0]) * np.cos(x[:, 1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=True, single_layer_cut=True)
    s = P.PhiFEMSolver(mesh, **kw)
    return s, (phi, 2.0 * uD, uD)


# ---- 1. restriction -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["disk3", "disk_empty", "graded_tet", "kuhn3"])
def test_restrict_equals_reference_bit_for_bit(P, name):
    import torch
    meshes, levels = _hier(name)
    rng = np.random.default_rng(4)
    for l in range(1, len(meshes)):
        coarse, fine = meshes[l - 1], meshes[l]
        assert fine.coarse is coarse
        for ncomp in (1, 3):
            r = rng.standard_normal((ncomp, fine.nv)) if ncomp > 1 else rng.standard_normal(fine.nv)
            xc = rng.standard_normal((ncomp, coarse.nv)) if ncomp > 1 else rng.standard_normal(coarse.nv)
            got = P.restrict(fine, r)
            assert got.shape == xc.shape
            want = ML.restrict_ref(coarse.nv, levels[l]["pairs"], r)
            assert np.array_equal(got, want), f"{name} level {l} ncomp {ncomp}: restriction differs from the reference"
            assert np.array_equal(P.restrict(fine, r), got)                     # the same bits on every run
            gd = P.restrict(fine, torch.from_numpy(r).cuda())
            assert gd.is_cuda and np.array_equal(gd.cpu().numpy(), got)
            px = P.prolongate(fine, xc)
            lhs, rhs = float((got * xc).sum()), float((r * px).sum())
            scale = float(np.abs(got * xc).sum() + np.abs(r * px).sum())
            print(f"[{name} level {l} ncomp {ncomp}] nv {coarse.nv} -> {fine.nv}: |<Rr, x> - <r, Px>| = "
                  f"{abs(lhs - rhs) / scale:.2e} of the scale")
            assert abs(lhs - rhs) <= 1e-13 * scale
        # a row that tells left-to-right from any other order of the additions
        ptr, idx = ML.restriction_csr(coarse.nv, levels[l]["pairs"])
        rows = np.flatnonzero(np.diff(ptr) >= 2)
        if rows.size:
            p = rows[-1]
            v = np.zeros(fine.nv)
            v[p], v[idx[ptr[p]]], v[idx[ptr[p] + 1]] = 1.0, 2.0 ** 61, -2.0 ** 61
            assert P.restrict(fine, v)[p] == 0.0


def test_restrict_refusals(P):
    from phifem_amd import _lib as L
    meshes, _ = _hier("disk3")
    coarse, fine, finer = meshes[0], meshes[1], meshes[2]
    with pytest.raises(NotImplementedError):
        P.restrict(fine, np.zeros(fine.lagrange_ndofs(2)), degree=2)
    quad = P.create_rectangle([[0.0, 0.0], [1.0, 1.0]], [3, 2], cell_type="quadrilateral")
    qf = P.refine(quad)
    with pytest.raises(NotImplementedError):
        P.restrict(qf, np.zeros(qf.nv))
    with pytest.raises(ValueError):
        P.restrict(coarse, np.zeros(coarse.nv))                  # not produced by refine
    with pytest.raises(ValueError):
        P.restrict(fine, np.zeros(fine.nv + 1))                  # wrong length
    buf, out = np.zeros(finer.nv), np.zeros(coarse.nv)
    args = (buf.ctypes.data_as(C.c_void_p), L.HOST, out.ctypes.data_as(C.c_void_p), L.HOST)
    assert L.lib.phx_restrict(coarse._h, finer._h, 1, 1, *args) == L.ERR_VALUE          # a grandchild
    assert L.lib.phx_restrict(coarse._h, fine._h, 2, 1, *args) == L.ERR_NOT_IMPLEMENTED
    assert L.lib.phx_restrict(quad._h, qf._h, 1, 1, *args) == L.ERR_NOT_IMPLEMENTED


# ---- 2. the operator ----------------------------------------------------------------------------------------------------
def multilevel_system(P, name):
    from phifem_amd import _lib as L
    meshes, levels = _hier(name)
    mesh = meshes[-1]
    s, data = tagged_solver(P, name, mesh, multilevel=True)
    L.check(L.lib.phx_set_option(mesh._h, L.OPT_EXPORT_CSR, 1))
    try:
        info = s.assemble(*data)
    finally:
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_EXPORT_CSR, 0))
    assert info["has_csr"] == 1
    return System(solver=s, mesh=mesh, nfields=2, blocks=None), levels


@pytest.mark.parametrize("name,kind", [("disk3", 1), ("disk_empty", 1), ("graded_tet", 1), ("kuhn3", 1), ("rect_big", 0)])
def test_operator_equals_reference(P, name, kind):
    c, levels = multilevel_system(P, name)
    ap = Applied(P, c)
    n, is_u = ap.n, ap.is_u
    assert ap.hat and ap.kind == 5, (name, ap.kind)
    assert ap.L == [len(levels), levels[0]["x"].shape[0], kind], (name, ap.L)
    assert c.solver.precond_info()["precond"] == "multilevel"
    nv = c.mesh.nv
    rows = np.flatnonzero(is_u)
    vert = ap.ent[rows]                                          # vertex of u row i
    active_u = np.zeros(nv, dtype=bool)
    active_u[vert] = True
    ref = ML.Multilevel(levels, active_u)
    assert ref.coarse == kind
    w0 = ap.read()
    assert np.array_equal(w0["p"], ap.rhs[ap.perm])
    ap.one_iteration()
    w1 = ap.read()
    cname, cs = ap.column_scaling()
    q_rest = max(check_non_u_rows(ap, cs, "after KR_BEGIN", w0), check_non_u_rows(ap, cs, "after KR_UPDATE_P", w1))
    rng = np.random.default_rng(5)
    vecs = [rng.standard_normal(n), rng.standard_normal(n)]
    xv = c.mesh.x[vert]
    for a in range(xv.shape[1]):                                 # unit impulses at the extreme active vertices
        for pick in (np.argmin, np.argmax):
            e = np.zeros(n)
            e[rows[pick(xv[:, a])]] = 1.0
            vecs.append(e)
    worst, first = 0.0, None
    for k in range(0, len(vecs), 2):
        p, s = vecs[k], vecs[k + 1]
        phat, shat = ap.apply(p, s, poison=rows)
        if first is None:
            first = phat.copy()
        for what, v, hat in ((f"p[{k}]", p, phat), (f"s[{k + 1}]", s, shat)):
            g = np.zeros(nv)
            g[vert] = v[rows]
            xref = ref.apply(g)[vert]
            x = (cs * hat)[rows]
            assert np.all(np.isfinite(x)), f"{name} {what}: {np.flatnonzero(~np.isfinite(x))[:8]} not written"
            err = np.abs(x - xref).max() / np.abs(xref).max()
            worst = max(worst, err / 1e-12)
            assert err <= 1e-12, f"{name} {what}: {err:.3e} of max|x_ref|, worst at vertex {vert[np.abs(x - xref).argmax()]}"
    again, _ = ap.apply(vecs[0], vecs[1], poison=rows)
    assert np.array_equal(again[rows], first[rows]), "two applications to the same vector differ"
    print(f"[{name}] levels {[lv['x'].shape[0] for lv in levels]} coarse kind {kind} C={cname} n={n} u rows={rows.size} "
          f"vectors={len(vecs)}: worst {worst:.2e} of the bound 1e-12; non-u rows {q_rest:.2f} of 2 ulp")


# ---- 3. solves ----------------------------------------------------------------------------------------------------------
def dorfler_loop(P, name, mesh, rounds):
    """-> list of (iterations Jacobi, iterations multilevel or None, w_jacobi, w_multilevel) per level"""
    out = []
    for rnd in range(rounds + 1):
        sj, data = tagged_solver(P, name, mesh, deterministic=True)
        sj.assemble(*data)
        wj = sj.solve(rtol=RTOL)
        assert sj.stats["converged"]
        itm, wm = None, None
        if rnd > 0:
            sm, _ = tagged_solver(P, name, mesh, multilevel=True, deterministic=True)
            sm.assemble(*data)
            wm = sm.solve(rtol=RTOL)
            assert sm.stats["converged"] and sm.stats["precond"] == "multilevel", sm.stats
            assert sm.stats["precond_L"][0] == rnd + 1
            itm = sm.stats["iterations"]
        else:
            assert sj.stats["precond"] == ("box-dst" if name == "box8" else "jacobi")
        out.append((sj.stats["iterations"], itm, wj, wm))
        if rnd < rounds:
            mesh = P.refine(mesh, marked=P.mark_dorfler(mesh, sj.estimate(wj), theta=0.5))
    return out


@pytest.mark.parametrize("name,rounds", [("disk", 5), ("box8", 2)])
def test_solve_takes_fewer_iterations_than_jacobi(P, name, rounds):
    if name == "disk":
        mesh = P.Mesh.from_arrays(*load_mesh("disk"))
    else:
        mesh = P.create_box([-1.5] * 3, [1.5] * 3, [8] * 3)
    res = dorfler_loop(P, name, mesh, rounds)
    print(f"[{name}] iterations per level: Jacobi {[r[0] for r in res]}, multilevel {[r[1] for r in res]}")
    itj, itm, wj, wm = res[-1]
    diff = np.abs(wm - wj).max() / np.abs(wj).max()
    print(f"[{name}] last level: |w_multilevel - w_jacobi| = {diff:.2e} of max|w|")
    assert diff <= 100 * RTOL
    assert itm < itj, (itm, itj)


def test_auto_on_a_parentless_mesh_keeps_jacobi(P):
    mesh = P.Mesh.from_arrays(*load_mesh("disk"))
    # (deterministic=True: two solves of one system give the same bits and the same count only with it)
    s0, data = tagged_solver(P, "disk", mesh, deterministic=True)
    s0.assemble(*data)
    w0 = s0.solve(rtol=RTOL)
    s1, _ = tagged_solver(P, "disk", mesh, multilevel="auto", deterministic=True)
    s1.assemble(*data)
    w1 = s1.solve(rtol=RTOL)
    assert s1.stats["precond"] == "jacobi" and s1.stats["iterations"] == s0.stats["iterations"]
    assert np.array_equal(w0, w1)
    meshes, _ = _hier("disk3")                                    # ... and builds it where there is a parent
    s2, data2 = tagged_solver(P, "disk", meshes[-1], multilevel="auto")
    s2.assemble(*data2)
    s2.solve(rtol=RTOL)
    assert s2.stats["precond"] == "multilevel"


# ---- 4. housekeeping ----------------------------------------------------------------------------------------------------
def _build_and_drop(P):
    ctype, x, cells = load_mesh("disk")
    meshes, _ = nearest_rounds(P, P.Mesh.from_arrays(ctype, x, cells), 2)
    s, data = tagged_solver(P, "disk", meshes[-1], multilevel=True)
    s.assemble(*data)
    s.solve(rtol=RTOL)
    assert s.stats["precond"] == "multilevel"
    P.restrict(meshes[-1], np.ones(meshes[-1].nv))
    del s, meshes
    gc.collect()


def test_pool_returns_to_its_starting_figures(P):
    _build_and_drop(P)                                            # (first use of every staging buffer)
    before = live_bytes()
    _build_and_drop(P)
    assert live_bytes() == before


def test_refusals(P):
    from phifem_amd import _lib as L
    ctype, x, cells = load_mesh("disk")
    coarse = P.Mesh.from_arrays(ctype, x, cells)
    with pytest.raises(ValueError):
        P.PhiFEMSolver(coarse, multilevel=True)                  # no parent
    fine = P.refine(coarse, marked=RM.nearest_mask(x, cells, _point(x)))
    # every boundary vertex active (the level-set is negative everywhere): no constraint, K singular
    from phifem_amd.mesh_scripts import NodalFunction
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(fine, NodalFunction(-np.ones(fine.nv)), 1, box_mode=True, single_layer_cut=True)
    s = P.PhiFEMSolver(fine, multilevel=True)
    with pytest.raises(ValueError, match="singular"):
        s.assemble(-np.ones(fine.nv), np.ones(fine.nv), np.zeros(fine.nv))
    with pytest.raises(NotImplementedError):
        P.PhiFEMSolver(fine, degree=2, levelset_degree=2, multilevel=True)
    quad = P.refine(P.create_rectangle([[0.0, 0.0], [1.0, 1.0]], [4, 4], cell_type="quadrilateral"))
    with pytest.raises(NotImplementedError):
        P.PhiFEMSolver(quad, multilevel=True)
    with pytest.raises(NotImplementedError):
        P.PhiFEMSolver(fine, degree=2, levelset_degree=2, coarse_space="auto", multilevel=True)
    # a mesh the lattice preconditioner serves
    boxf = P.refine(P.create_box([-1.5] * 3, [1.5] * 3, [4] * 3))
    sb, data = tagged_solver(P, "box", boxf, multilevel=True)
    with pytest.raises(NotImplementedError):
        sb.assemble(*data)
    # a sub-mesh
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, sub, _, _ = P.compute_tags_measures(fine, NodalFunction(levelset("disk", fine.x)), 1, box_mode=False,
                                                  single_layer_cut=True)
    with pytest.raises(NotImplementedError):
        P.PhiFEMSolver(sub, multilevel=True)
    # a slab of a partitioned box: the C entry refuses the system (no refined slab exists for the keyword to meet:
    # refinement re-creates a slab as a whole box, and a slab itself has no parent)
    slab = P.create_box([-1.5, -1.5, -0.375], [1.5, 1.5, 0.375], [8, 8, 2], offset=[0, 0, 3], n_global=[8, 8, 8])
    ss, sdata = tagged_solver(P, "box", slab)
    ss.assemble(*sdata)
    assert L.lib.phx_multilevel_setup(ss._sys) == L.ERR_VALUE
    assert b"slab" in L.lib.phx_last_error()
    with pytest.raises(ValueError):
        P.PhiFEMSolver(slab, multilevel=True)
    # the coarse mesh is destroyed before assembling: refused, no fault
    s2, data2 = tagged_solver(P, "disk", fine, multilevel=True)
    L.check(L.lib.phx_mesh_destroy(coarse._h))
    coarse._h = None
    with pytest.raises(ValueError, match="no living parent"):
        s2.assemble(*data2)
