"""GPU checks of weak-Dirichlet Poisson on QUADRILATERALS (`phx_assemble_poisson_wd` on a mesh of axis-parallel
rectangles: Q1 x Q1, `PhiFEMSolver` on `create_rectangle(..., cell_type="quadrilateral")`) against the numpy
restatement `tests/poisson_quad_ref.py`, of the lattice preconditioner on rectangular lattices, and of the
convergence orders next to the triangle path.  Tolerance of the matrix / rhs: 1e-11 relative to the largest entry
(atomic accumulation order, FMA); solution 1e-6 at solver rtol 1e-10 (the project's SOL_TOL)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import poisson_quad_ref as PQ

pytestmark = pytest.mark.gpu
MAT_TOL = 1e-11
SOL_TOL = 1e-6
BBOX = [[-1.5, -1.5], [1.5, 1.5]]


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def tag(P, mesh, centre=(0.0, 0.0), box_mode=True):
    """Tags the unit disc around `centre`; -> (work mesh, phi on it, arguments of PQ.assemble)."""
    from phifem_amd.mesh_scripts import NodalFunction
    phi = ((mesh.x - np.asarray(centre)) ** 2).sum(axis=1) - 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, sub, meas, _ = P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=box_mode,
                                                     single_layer_cut=True)
    work = mesh if box_mode else sub
    xw = work.x
    phiw = ((xw - np.asarray(centre)) ** 2).sum(axis=1) - 1.0
    geo = dict(cells=work.cells.astype(np.int64), x=xw, c2f=work.c2f.astype(np.int64), f2c=work.f2c.astype(np.int64),
               cell_tags=work.cell_tag_values(), facet_tags=work.facet_tag_values(),
               ds=meas(100) if box_mode else work.boundary_facets.reshape(-1), phi=phiw)
    return work, phiw, geo


def quad(P, n):
    return P.create_rectangle(BBOX, [n, n], cell_type="quadrilateral")


def hip_matrix(solver):
    rowptr, col, val, rhs, dof = solver.export_csr()
    n = rowptr.size - 1
    return sp.csr_matrix((val, col, rowptr), shape=(n, n)), rhs, dof


@pytest.mark.parametrize("n,box", [(12, True), (24, True), (40, True), (24, False)])
def test_matrix_rhs_pattern_numbering_vs_restatement(P, n, box):
    work, phi, geo = tag(P, quad(P, n), centre=(0.03, -0.02), box_mode=box)
    rng = np.random.default_rng(5)
    f = np.sin(work.x @ rng.standard_normal(2)) + 0.3
    uD = np.cos(work.x @ rng.standard_normal(2))
    A, b, act = PQ.assemble(**geo, f=f, uD=uD, gamma=1.3, sigma=0.7)
    s = P.PhiFEMSolver(work, pen_coef=1.3, stab_coef=0.7)
    info = s.assemble(phi, f, uD)
    H, rhs, dof = hip_matrix(s)
    idx = np.flatnonzero(act)
    nv = work.nv
    assert info["n_active"] == idx.size and info["n_active_u"] == act[:nv].sum() and info["n_full"] == 2 * nv
    assert np.array_equal(dof, idx), "active DoF numbering differs"
    Ao = A[idx][:, idx].tocsr()
    Ao.sort_indices()
    assert np.array_equal(H.indptr, Ao.indptr) and np.array_equal(H.indices, Ao.indices)
    scale = np.abs(Ao.data).max()
    err_a = np.abs(H.data - Ao.data).max() / scale
    err_b = np.abs(rhs - b[idx]).max() / np.abs(b).max()
    print(f"quad wd n={n} box={box}: n_active={idx.size} nnz={H.nnz} matrix err {err_a:.2e} rhs err {err_b:.2e}")
    assert err_a <= MAT_TOL and err_b <= MAT_TOL
    xv = rng.standard_normal(idx.size)
    y, yo = s.spmv(xv), Ao @ xv
    assert np.abs(y - yo).max() <= MAT_TOL * np.abs(yo).max()
    # phx_system_get_perm: the vertex -> active row maps behave as for triangles
    import ctypes as C
    from phifem_amd import _lib as L
    du, dp = np.empty(nv, dtype=np.int32), np.empty(nv, dtype=np.int32)
    L.check(L.lib.phx_system_get_perm(s._sys, None, du.ctypes.data_as(C.c_void_p), dp.ctypes.data_as(C.c_void_p), L.HOST))
    assert np.array_equal(np.flatnonzero(du >= 0), np.flatnonzero(act[:nv]))
    assert np.array_equal(np.flatnonzero(dp >= 0), np.flatnonzero(act[nv:]))
    assert np.array_equal(du[du >= 0], np.arange(act[:nv].sum()))
    assert np.array_equal(dp[dp >= 0], act[:nv].sum() + np.arange(act[nv:].sum()))


def test_patch_test_through_hip(P):
    """f = 0, u_D = u linear: Q1 reproduces u exactly and p = 0 (consistency of main.py:112-151)."""
    work, phi, geo = tag(P, quad(P, 32))
    ulin = work.x @ np.array([1.0, 2.0]) + 0.5
    _, _, act = PQ.assemble(**geo, f=np.zeros(work.nv), uD=ulin)
    s = P.PhiFEMSolver(work)
    s.assemble(phi, np.zeros(work.nv), ulin)
    w = s.solve(rtol=1e-13, max_iter=5000)
    u, p = s.split(w)
    ua = act[:work.nv]
    assert np.abs(u[ua] - ulin[ua]).max() < 1e-8
    assert np.abs(p).max() < 1e-6
    assert np.all(w[~act] == 0.0)


@pytest.mark.parametrize("n,box", [(48, True), (32, False)])
def test_solve_vs_direct(P, n, box):
    work, phi, geo = tag(P, quad(P, n), box_mode=box)
    uex = np.prod(np.sin(work.x), axis=1)
    A, b, act = PQ.assemble(**geo, f=2.0 * uex, uD=uex)
    s = P.PhiFEMSolver(work)
    s.assemble(phi, 2.0 * uex, uex)
    w = s.solve(rtol=1e-10)
    assert s.stats["relres"] <= 1e-10 and s.stats["iterations"] > 0
    wo = PQ.solve_direct(A, b, act)
    assert np.abs(w - wo).max() <= SOL_TOL * np.abs(wo).max()
    assert np.all(w[~act] == 0.0)
    r = A @ w - b
    assert np.linalg.norm(r[act]) <= 1e-8 * np.linalg.norm(b)


def test_deterministic(P):
    work, phi, geo = tag(P, quad(P, 40), centre=(0.03, -0.02))
    uex = np.prod(np.sin(work.x), axis=1)
    out = []
    for _ in range(2):
        s = P.PhiFEMSolver(work, deterministic=True)
        s.assemble(phi, 2.0 * uex, uex)
        rowptr, col, val, rhs, dof = s.export_csr()
        w = s.solve(rtol=1e-10)
        assert s.stats["converged"]
        out.append((rowptr, col, val, rhs, dof, s.stats["iterations"], w))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def solve_disc(P, mesh, precond=1, deterministic=False, rtol=1e-10):
    from phifem_amd import _lib as L
    L.check(L.lib.phx_set_option(mesh._h, L.OPT_PRECOND, precond))
    work, phi, _ = tag(P, mesh)
    uex = np.prod(np.sin(work.x), axis=1)
    s = P.PhiFEMSolver(work, deterministic=deterministic)
    s.assemble(phi, 2.0 * uex, uex)
    w = s.solve(rtol=rtol, max_iter=200000)
    assert s.stats["converged"]
    return w, dict(s.stats)


@pytest.mark.parametrize("n", [64, 128])
def test_lattice_preconditioner_beats_jacobi(P, n):
    """The sine-transform solve of the 5-point lattice Laplacian preconditions the 9-point Q1 stiffness (spectrally
    equivalent, not equal): in force on a rectangular lattice, in the standard loop -- the identity / reduced loops
    need stencil rows equal to the lattice row -- and strictly fewer iterations than Jacobi (measured: 62 against 72 at
    n = 64, 70 against 104 at n = 128)."""
    w1, st1 = solve_disc(P, quad(P, n), precond=1)
    w0, st0 = solve_disc(P, quad(P, n), precond=0)
    print(f"quad wd n={n}: box-dst {st1['iterations']} iterations, jacobi {st0['iterations']}")
    assert st1["precond"] == "box-dst" and st0["precond"] == "jacobi"
    assert not st1["identity_loop"] and not st1["reduced_loop"]
    assert st1["precond_points"] > 0
    assert st0["iterations"] > st1["iterations"]
    assert np.abs(w1 - w0).max() <= SOL_TOL * np.abs(w0).max()


def test_preconditioner_on_submesh(P):
    from phifem_amd.mesh_scripts import NodalFunction
    mesh = quad(P, 64)
    phi = (mesh.x ** 2).sum(axis=1) - 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, sub, _, _ = P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=False, single_layer_cut=True)
    uex = np.prod(np.sin(sub.x), axis=1)
    s = P.PhiFEMSolver(sub)
    s.assemble((sub.x ** 2).sum(axis=1) - 1.0, 2.0 * uex, uex)
    s.solve(rtol=1e-10)
    assert s.stats["converged"] and s.stats["precond"] == "box-dst"


def test_shuffled_vertices_get_the_same_preconditioner(P):
    """A caller's copy of the mesh with its vertices in any order (`Mesh.from_arrays`) is recognised as a lattice:
    the same preconditioner, in deterministic mode the same iteration count, the same solution (the system is
    assembled on a copy of the mesh in lattice vertex order: 54 and 54 iterations; 54 and 60 without it)."""
    n = 64
    mesh = quad(P, n)
    x, cells = mesh.x, mesh.cells
    rng = np.random.default_rng(3)
    perm = rng.permutation(x.shape[0])          # new vertex id -> old vertex id
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    shuffled = P.Mesh.from_arrays("quadrilateral", x[perm], inv[cells].astype(np.int32))
    w0, st0 = solve_disc(P, mesh, deterministic=True)
    w1, st1 = solve_disc(P, shuffled, deterministic=True)
    print(f"quad wd shuffled n={n}: {st0['iterations']} / {st1['iterations']} iterations")
    assert st0["precond"] == "box-dst" and st1["precond"] == "box-dst"
    assert st0["precond_L"] == st1["precond_L"] and st0["precond_points"] == st1["precond_points"]
    assert st1["iterations"] == st0["iterations"]
    nv = x.shape[0]
    assert np.abs(w1[:nv] - w0[:nv][perm]).max() <= SOL_TOL * np.abs(w0).max()
    assert np.abs(w1[nv:] - w0[nv:][perm]).max() <= SOL_TOL * np.abs(w0).max()


def test_convergence_orders_next_to_triangles(P):
    """u = sin x sin y on the unit disc, n = 32, 64, 128: relative L2 and H10 errors over the inside cells
    (`postprocess.cell_errors`) and their observed orders (least-squares slope over the three meshes), for Q1 on
    squares and -- the yardstick -- P1 on the triangles of `create_rectangle`.  The quadrilateral orders must reach
    the triangle orders minus 0.3 (the scatter of a three-point fit)."""
    from phifem_amd.postprocess import cell_errors
    exact = lambda p: np.sin(p[0]) * np.sin(p[1])    # noqa: E731
    ns = (32, 64, 128)
    errs = {}
    for ctype in ("triangle", "quadrilateral"):
        for n in ns:
            mesh = P.create_rectangle(BBOX, [n, n], cell_type=ctype)
            work, phi, _ = tag(P, mesh)
            uex = exact(work.x.T)
            s = P.PhiFEMSolver(work)
            s.assemble(phi, 2.0 * uex, uex)
            w = s.solve(rtol=1e-11, max_iter=100000)
            assert s.stats["converged"]
            inside = np.flatnonzero(work.cell_tag_values() == 1).astype(np.int32)
            e = cell_errors(work, s.split(w)[0], exact, degree=1, cells=inside)
            errs[ctype, n] = (e["l2_relative"], e["h10_relative"])
    logh = np.log(3.0 / np.asarray(ns, dtype=float))
    order = {(c, k): np.polyfit(logh, np.log([errs[c, n][k] for n in ns]), 1)[0]
             for c in ("triangle", "quadrilateral") for k in (0, 1)}
    for c in ("triangle", "quadrilateral"):
        print(f"{c}: L2 " + " ".join(f"{errs[c, n][0]:.3e}" for n in ns) + f" (order {order[c, 0]:.2f}); H10 "
              + " ".join(f"{errs[c, n][1]:.3e}" for n in ns) + f" (order {order[c, 1]:.2f})")
    assert order["quadrilateral", 0] >= order["triangle", 0] - 0.3
    assert order["quadrilateral", 1] >= order["triangle", 1] - 0.3


def test_rejections(P):
    from phifem_amd.mesh_scripts import NodalFunction
    from test_oracle_flux_quad import quad_mesh
    x0, cells0 = quad_mesh(8)
    xs = x0.copy()
    xs[:, 0] += 0.2 * xs[:, 1]
    sheared = P.Mesh.from_arrays("quadrilateral", xs, cells0.astype(np.int32))
    phi = (xs ** 2).sum(axis=1) - 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(sheared, NodalFunction(phi), 1, box_mode=True, single_layer_cut=True)
    s = P.PhiFEMSolver(sheared)
    with pytest.raises(NotImplementedError):
        s.assemble(phi, np.zeros(sheared.nv), np.zeros(sheared.nv))
    mesh = quad(P, 8)
    with pytest.raises(NotImplementedError, match="Q1"):
        P.PhiFEMSolver(mesh, degree=2)
    with pytest.raises(NotImplementedError, match="Q1"):
        P.PhiFEMSolver(mesh, degree=2, levelset_degree=2)
    with pytest.raises(NotImplementedError, match="Q1"):
        P.PhiFEMSolver(mesh, coarse_space=5)
    with pytest.raises(ValueError):
        P.PhiFEMSolver(mesh).assemble(np.zeros(mesh.nv), np.zeros(mesh.nv), np.zeros(mesh.nv))   # untagged


def test_device_resident_inputs_and_outputs(P):
    import torch
    work, phi, geo = tag(P, quad(P, 40))
    uex = np.prod(np.sin(work.x), axis=1)
    A, b, act = PQ.assemble(**geo, f=2.0 * uex, uD=uex)
    s = P.PhiFEMSolver(work)
    dev = torch.device("cuda:0")
    tphi, tf, tu = (torch.from_numpy(a).to(dev) for a in (phi, 2.0 * uex, uex))
    s.assemble(tphi, tf, tu)
    out = torch.empty(2 * work.nv, dtype=torch.float64, device=dev)
    s.solve(rtol=1e-10, out=out)
    torch.cuda.synchronize()
    wo = PQ.solve_direct(A, b, act)
    assert np.abs(out.cpu().numpy() - wo).max() <= SOL_TOL * np.abs(wo).max()
