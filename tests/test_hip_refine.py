"""Uniform refinement and the nested P1 / P2 transfer on the GPU (`phifem_amd.refine`, `phifem_amd.prolongate`) against
the numpy specification tests/refine_ref.py: meshes and the degree-1 transfer bit for bit, degree 2 to round-off."""
import ctypes as C
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import hub_meshes as HM
import partition_ref as PR
import refine_ref as RR
from datasets import load_mesh
from oracle import assembly as OA
from oracle.topology import Topology

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
MESHES = ["single_triangle", "single_tetrahedron", "single_quadrilateral", "disk", "square_tri", "square_quad",
          "graded_tet_box", "hub_3d", "box_3x4x5"]
HUB_3D = min((k for k, c in HM.CASES.items() if c["d"] == 3), key=lambda k: (HM.CASES[k]["nbg"] + sum(h[1] for h in HM.CASES[k]["hubs"]), k))


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


@functools.lru_cache(maxsize=None)
def arrays(name):
    """(cell type, x, cells) of a caller-supplied test mesh; None for the generated box."""
    if name == "box_3x4x5":
        return None
    if name == "graded_tet_box":
        return ("tetrahedron",) + PR.graded_tet_box()
    if name == "hub_3d":
        x, cells, _ = HM.case_mesh(HUB_3D)
        return "tetrahedron", np.ascontiguousarray(x, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    if name.startswith("single_"):
        return (name[7:],) + RR.single_cell(name[7:])
    return load_mesh(name)


def coarse_mesh(P, name):
    """-> (mesh, cell type, x, cells, edges): `edges` is the library's edge numbering where it is not the ascending
    sorted pair (generated boxes number edges in closed form), else None."""
    a = arrays(name)
    if a is None:
        mesh = P.create_box([-1.0, 0.0, 0.5], [1.0, 1.5, 2.0], [3, 4, 5])
        return mesh, "tetrahedron", mesh.x, mesh.cells.astype(np.int64), mesh.edges
    ctype, x, cells = a
    return P.Mesh.from_arrays(ctype, x, cells), ctype, x, cells, None


@functools.lru_cache(maxsize=None)
def reference(name):
    """(fine x, fine cells) of the specification, computed once per caller-supplied mesh."""
    ctype, x, cells = arrays(name)
    return RR.refine_ref(ctype, x, cells)


def live_bytes():
    from phifem_amd import _lib as L
    a, b = C.c_int64(0), C.c_int64(0)
    L.check(L.lib.phx_pool_stats(C.byref(a), C.byref(b)))
    return a.value


# ---- 1. refine == refine_ref ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_refine_equals_reference(P, name):
    mesh, ctype, x, cells, edges = coarse_mesh(P, name)
    if edges is None and ctype != "quadrilateral":
        assert np.array_equal(mesh.edges, RR.edge_numbering(ctype, cells)[1])     # the documented numbering
    fine = P.refine(mesh)
    xf, cf = RR.refine_ref(ctype, x, cells, edges) if edges is not None else reference(name)
    gx, gc = fine.x, fine.cells
    assert gx.shape == xf.shape and gc.shape == cf.shape
    assert np.array_equal(gx, xf), "fine coordinates differ from the specification"
    assert np.array_equal(gc, cf), "fine cells differ from the specification"
    assert np.array_equal(gx, mesh.lagrange_dof_points(2))
    assert fine.parent is None and fine.coarse is mesh and fine.cell_type == ctype
    nchild = 8 if ctype == "tetrahedron" else 4
    assert fine.nchild == nchild and fine.nc == nchild * mesh.nc
    # the library's own topology of the fine mesh
    nv, nc, nf, nbf = mesh.nv, mesh.nc, mesh.nf, mesh.nbf
    if ctype == "quadrilateral":
        assert fine.nv == nv + nf + nc and fine.nf == 2 * nf + 4 * nc and fine.nbf == 2 * nbf
    elif ctype == "triangle":
        assert fine.nv == nv + mesh.ne and fine.nf == 2 * nf + 3 * nc and fine.nbf == 2 * nbf
    else:
        assert fine.nv == nv + mesh.ne and fine.nf == 4 * nf + 8 * nc and fine.nbf == 4 * nbf
    topo = Topology(ctype, cf, xf.shape[0])
    assert np.array_equal(fine.c2f, topo.c2f) and np.array_equal(fine.f2c, topo.f2c)
    assert fine.refine().nc == nchild * fine.nc          # Mesh.refine, and a refined mesh refines again


# ---- 2. two levels ----------------------------------------------------------------------------------------------------
def test_two_levels_coarse_square(P):
    ctype, x, cells = load_mesh("coarse_square")
    m2 = P.refine(P.refine(P.Mesh.from_arrays(ctype, x, cells)))
    x2, c2 = RR.refine_ref(ctype, *RR.refine_ref(ctype, x, cells))
    assert np.array_equal(m2.x, x2) and np.array_equal(m2.cells, c2)
    assert m2.coarse.coarse.nc * 16 == m2.nc


def test_two_levels_generated_box(P):
    m0 = P.create_box([0.0] * 3, [1.0, 2.0, 3.0], [2, 2, 2])
    m2 = P.refine(P.refine(m0))
    x1, c1 = RR.refine_ref("tetrahedron", m0.x, m0.cells, m0.edges)   # level 0 numbers its edges in closed form
    x2, c2 = RR.refine_ref("tetrahedron", x1, c1)
    assert np.array_equal(m2.x, x2) and np.array_equal(m2.cells, c2)


# ---- 3. the lattice behind a refined lattice mesh ---------------------------------------------------------------------
def _solve(P, mesh, phi, f, uD, rtol=1e-10):
    from phifem_amd.mesh_scripts import NodalFunction
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=True, single_layer_cut=True)
        s = P.PhiFEMSolver(mesh, deterministic=True)
        s.assemble(phi, f, uD)
        w = s.solve(rtol=rtol)
    return s, w


@pytest.mark.parametrize("kind", ["tetrahedron", "quadrilateral"])
def test_lattice_is_kept(P, kind):
    if kind == "tetrahedron":
        fine = P.refine(P.create_box([-1.5] * 3, [1.5] * 3, [6] * 3))
    else:
        fine = P.refine(P.create_rectangle([[-1.5, -1.5], [1.5, 1.5]], [8, 6], cell_type="quadrilateral"))
    x, cells = fine.x, fine.cells
    twin = P.Mesh.from_arrays(kind, x, cells)
    phi = (x ** 2).sum(axis=1) - 1.0
    uex = np.prod(np.sin(x), axis=1)
    f = x.shape[1] * uex
    s1, w1 = _solve(P, fine, phi, f, uex)
    s2, w2 = _solve(P, twin, phi, f, uex)
    assert s1.stats["precond"] == s2.stats["precond"] == "box-dst"      # the sine-transform preconditioner
    assert s1.stats["precond_L"] == s2.stats["precond_L"]
    assert s1.stats["iterations"] == s2.stats["iterations"] and s1.stats["converged"]
    assert np.array_equal(w1, w2)
    if kind == "quadrilateral":       # children are axis-parallel rectangles in tensor-product order
        xc = x[cells]
        assert np.all(xc[:, 0, 1] == xc[:, 1, 1]) and np.all(xc[:, 2, 1] == xc[:, 3, 1])
        assert np.all(xc[:, 0, 0] == xc[:, 2, 0]) and np.all(xc[:, 1, 0] == xc[:, 3, 0])
        assert np.all(xc[:, 1, 0] > xc[:, 0, 0]) and np.all(xc[:, 2, 1] > xc[:, 0, 1])


# ---- 4. unstructured solve on a refined mesh --------------------------------------------------------------------------
def _case_data(name, x):
    """phi, f, u_D of partition_ref.case(name), evaluated at the points x."""
    if name == "tetbox":
        phi = ((x - np.array([0.05, -0.03, 0.02])) ** 2).sum(axis=1) - 1.0
        uD = np.sin(x[:, 0]) * np.cos(x[:, 1]) + 0.3 * x[:, 2]
    else:
        _, x0, _ = load_mesh(name)
        cen = x0.mean(axis=0) + np.array([0.013, -0.007])
        r = 0.62 * 0.5 * (x0.max(axis=0) - x0.min(axis=0)).min()
        phi = ((x - cen) ** 2).sum(axis=1) - r ** 2
        uD = np.sin(x[:, 0]) * np.cos(x[:, 1])
    return phi, 2.0 * np.sin(x[:, 0]) * np.cos(x[:, 1]), uD


@pytest.mark.parametrize("name", ["disk", "tetbox"])
def test_unstructured_assembly_on_refined_mesh(P, name):
    from phifem_amd.mesh_scripts import NodalFunction
    ctype, x, cells, phi0, f0, uD0 = PR.case(name)
    p0, f0r, u0 = _case_data(name, x)
    assert np.array_equal(p0, phi0) and np.array_equal(f0r, f0) and np.array_equal(u0, uD0)   # the same formulas
    fine = P.refine(P.Mesh.from_arrays(ctype, x, cells))
    xf, cf = fine.x, fine.cells
    twin = P.Mesh.from_arrays(ctype, xf, cf)
    phi, f, uD = _case_data(name, xf)
    out = []
    for mesh in (fine, twin):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, _, _, meas, _ = P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=True, single_layer_cut=True)
        s = P.PhiFEMSolver(mesh, deterministic=True)
        s.assemble(phi, f, uD)
        out.append(s.export_csr())
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    rowptr, col, val, rhs, dof = out[0]
    topo = Topology(ctype, cf.astype(np.int64), xf.shape[0])
    assert np.array_equal(topo.c2f, fine.c2f)
    A, b, act = OA.assemble_poisson_wd(topo, xf, fine.cell_tag_values(), fine.facet_tag_values(), meas(100), phi, f, uD)
    idx = np.flatnonzero(act)
    assert np.array_equal(dof, idx)
    Ao = A[idx][:, idx].tocsr()
    Ao.sort_indices()
    assert np.array_equal(rowptr, Ao.indptr) and np.array_equal(col, Ao.indices)
    assert np.abs(val - Ao.data).max() <= 1e-12 * np.abs(Ao.data).max()
    assert np.abs(rhs - b[idx]).max() <= 1e-12 * np.abs(b).max()


# ---- 5. prolongation, degree 1 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_prolongate_p1_bit_exact(P, name):
    import torch
    mesh, ctype, x, cells, edges = coarse_mesh(P, name)
    fine = P.refine(mesh)
    rng = np.random.default_rng(11)
    for shape in [(mesh.nv,), (3, mesh.nv)]:
        v = rng.standard_normal(shape)
        ref = RR.prolongate_ref(ctype, x, cells, v, 1, edges)
        got = P.prolongate(fine, v)
        assert isinstance(got, np.ndarray) and got.shape == ref.shape and np.array_equal(got, ref)
        gd = P.prolongate(fine, torch.from_numpy(v).cuda(), degree=1)
        assert gd.is_cuda and tuple(gd.shape) == ref.shape and np.array_equal(gd.cpu().numpy(), ref)
    assert np.array_equal(P.prolongate(fine, np.ascontiguousarray(mesh.x.T)), fine.x.T)
    from phifem_amd.mesh_scripts import NodalFunction
    nf = P.prolongate(fine, NodalFunction(v[0], 1))
    assert isinstance(nf, NodalFunction) and nf.degree == 1 and np.array_equal(nf.values, ref[0])


# ---- 6. prolongation, degree 2 ----------------------------------------------------------------------------------------
def _quadratic(p):
    return 0.2 + p[:, 0] * p[:, -1] - 0.7 * p[:, 0] ** 2 + 0.4 * p[:, -1] ** 2 + p.sum(axis=1)


@pytest.mark.parametrize("name", ["disk", "graded_tet_box", "box_3x4x5"])
def test_prolongate_p2(P, name):
    import torch
    mesh, ctype, x, cells, edges = coarse_mesh(P, name)
    fine = P.refine(mesh)
    n2 = mesh.lagrange_ndofs(2)
    rng = np.random.default_rng(12)
    v = rng.standard_normal((3, n2))
    # |got - ref| <= 64 eps max|u|: at most 10 terms with sum |w| <= 2 give 22 eps max|u| per side, both sides round
    ref = RR.prolongate_ref(ctype, x, cells, v, 2, edges)
    got = P.prolongate(fine, v, degree=2)
    assert got.shape == ref.shape == (3, fine.lagrange_ndofs(2))
    err = np.abs(got - ref).max()
    print(f"{name}: P2 prolongation |got - ref| = {err:.3e} ({err / (EPS * np.abs(v).max()):.2f} eps max|u|)")
    assert err <= 64 * EPS * np.abs(v).max()
    assert np.array_equal(got[:, :n2], v)                       # fine vertex DoFs are copies
    assert np.array_equal(P.prolongate(fine, v, degree=2), got)  # the same bits on every run
    gd = P.prolongate(fine, torch.from_numpy(v[1]).cuda(), degree=2)
    assert gd.is_cuda and np.array_equal(gd.cpu().numpy(), got[1])
    # the interpolant of a quadratic prolongs to its interpolant on the fine mesh
    q, qf = _quadratic(mesh.lagrange_dof_points(2)), _quadratic(fine.lagrange_dof_points(2))
    errq = np.abs(P.prolongate(fine, q, degree=2) - qf).max()
    print(f"{name}: quadratic |got - interpolant| = {errq:.3e} ({errq / (EPS * np.abs(q).max()):.2f} eps max|u|)")
    assert errq <= 64 * EPS * np.abs(q).max()


def test_prolongate_not_implemented(P):
    ctype, x, cells = arrays("single_quadrilateral")
    qf = P.refine(P.Mesh.from_arrays(ctype, x, cells))
    with pytest.raises(NotImplementedError):
        P.prolongate(qf, np.zeros(qf.coarse.lagrange_ndofs(2)), degree=2)
    ctype, x, cells = arrays("single_triangle")
    tf = P.refine(P.Mesh.from_arrays(ctype, x, cells))
    with pytest.raises(NotImplementedError):
        P.prolongate(tf, np.zeros(tf.coarse.lagrange_ndofs(3)), degree=3)
    from phifem_amd import _lib as L
    for fine, deg in ((qf, 2), (tf, 3), (qf, 3)):                   # the C entry refuses as well
        buf = np.zeros(64)
        rc = L.lib.phx_prolongate(fine.coarse._h, fine._h, deg, 1, buf.ctypes.data_as(C.c_void_p), L.HOST,
                                  buf.ctypes.data_as(C.c_void_p), L.HOST)
        with pytest.raises(NotImplementedError):
            L.check(rc)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind(P):
    from phifem_amd import _lib as L
    P.create_box([0.0] * 3, [1.0] * 3, [2, 2, 2]).ne         # (first use of the pool and of the read-back staging)
    start = live_bytes()
    ctype, x, cells = arrays("disk")
    coarse = P.Mesh.from_arrays(ctype, x, cells)
    other = P.Mesh.from_arrays(ctype, x, cells)
    fine = P.refine(coarse)
    assert coarse.ne + other.ne + fine.ne > 0                # (edge arrays are built on first use and stay with their mesh)
    before = live_bytes()
    v = np.zeros(coarse.nv)
    with pytest.raises(ValueError):
        P.prolongate(other, v)                                # not produced by refine
    fine.coarse = other                                       # refined, but from another mesh
    with pytest.raises(ValueError):
        P.prolongate(fine, v)
    with pytest.raises(ValueError):
        P.prolongate(fine, v, degree=2)
    fine.coarse = coarse
    with pytest.raises(ValueError):
        P.prolongate(fine, np.zeros(coarse.nv + 1))           # wrong length
    slab = P.create_box([0.0] * 3, [1.0] * 3, [2, 2, 2], offset=[0, 0, 2], n_global=[2, 2, 6])
    in_slab = live_bytes()
    L.check(L.lib.phx_mesh_set_slab_faces(slab._h, 1, 1))
    exempt = live_bytes() - in_slab
    with pytest.raises(ValueError):
        P.refine(slab)
    assert live_bytes() == in_slab + exempt
    L.check(L.lib.phx_mesh_set_slab_faces(slab._h, 0, 0))     # no cut face declared any more
    assert P.refine(slab).nc == 8 * slab.nc
    del slab
    with pytest.raises(NotImplementedError):
        L.check(L.lib.phx_refine_tables(5, None, None, None))     # not one of the three cell types
    assert live_bytes() == before
    del fine, coarse, other
    assert live_bytes() == start


# ---- 8. the demo ------------------------------------------------------------------------------------------------------
def test_refine_demo_errors_decrease():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo", "weak-dirichlet", "refine.py"), "--levels", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    errs = [float(line.split("L2=")[1].split()[0]) for line in r.stdout.splitlines() if "L2=" in line]
    assert len(errs) == 2 and errs[1] < errs[0], r.stdout
