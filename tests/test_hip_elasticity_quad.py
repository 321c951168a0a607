"""GPU checks of interface elasticity on QUADRILATERALS (`phx_assemble_elasticity_if` on a mesh of axis-parallel
rectangles: Q1 spaces, the cell_type "quadrilateral" of demo/interface-elasticity/main.py:99-108) against the numpy
restatement `tests/elasticity_quad_ref.py`, and of `phx_cell_errors` on quadrilaterals (Q3 reference space, 4 x 4
Gauss).  Tolerance of the matrix / rhs: 1e-11 relative to the largest entry (atomic accumulation order, FMA)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from elasticity_quad_ref import assemble_elasticity_quad
from oracle import elasticity as EL
from oracle.topology import Topology
from test_elasticity_quad_ref import demo_data
from test_oracle_flux_quad import quad_mesh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def setup(P, n, centre=(0.0, 0.0)):
    from phifem_amd.mesh_scripts import NodalFunction
    mesh = P.create_rectangle([[-1.5, -1.5], [1.5, 1.5]], [n, n], cell_type="quadrilateral")
    x = mesh.x
    phi = 1.0 - ((x - np.asarray(centre)) ** 2).sum(axis=1)            # data.py:39-40
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=True)   # main.py:115-117
    topo = Topology("quadrilateral", mesh.cells.astype(np.int64), mesh.nv)
    topo.c2f, topo.f2c, topo.nf = mesh.c2f.astype(np.int64), mesh.f2c.astype(np.int64), mesh.nf
    i, j = np.arange(mesh.nv) % (n + 1), np.arange(mesh.nv) // (n + 1)
    bcv = np.flatnonzero((i == 0) | (i == n) | (j == 0) | (j == n))
    return mesh, topo, x, phi, bcv


def reference(P, mesh, topo, x, phi, f, uD, bcv, **kw):
    from phifem_amd.mesh_scripts import BoundaryMeasure
    meas = BoundaryMeasure(mesh, True)
    return assemble_elasticity_quad(topo, x, mesh.cell_tag_values(), mesh.facet_tag_values(), meas(100), meas(101),
                                    phi, f, uD, bcv, **kw)


def test_create_rectangle_quadrilateral(P):
    x0, cells0 = quad_mesh(7)
    mesh = P.create_rectangle([[-1.5, -1.5], [1.5, 1.5]], [7, 7], cell_type="quadrilateral")
    assert mesh.cell_type == "quadrilateral"
    assert np.array_equal(mesh.x, x0) and np.array_equal(mesh.cells, cells0)
    m2 = P.create_rectangle([[0.0, 0.0], [2.0, 1.0]], [4, 2], cell_type="quadrilateral")
    assert m2.nv == 15 and m2.nc == 8
    assert np.array_equal(m2.cells[5], [6, 7, 11, 12]) and np.allclose(m2.x[7], [1.0, 0.5])
    with pytest.raises(ValueError):
        P.create_rectangle([[0.0, 0.0], [1.0, 1.0]], [2, 2], cell_type="hexagon")


@pytest.mark.parametrize("n,E_out", [(12, 1.0e-3), (16, 1.0)])
def test_matrix_rhs_spmv_vs_reference(P, n, E_out):
    mesh, topo, x, phi, bcv = setup(P, n, centre=(0.04, -0.03))
    rng = np.random.default_rng(5)
    f = np.sin(x @ rng.standard_normal((2, 2))) + 0.3
    uD = np.cos(x @ rng.standard_normal((2, 2)))
    A, b, act = reference(P, mesh, topo, x, phi, f, uD, bcv, E_in=1.0, E_out=E_out)
    s = P.InterfaceElasticitySolver(mesh, E_in=1.0, E_out=E_out)
    info = s.assemble(phi, f, uD, bcv)
    rowptr, col, val, rhs, dof = s.export_csr()
    idx = np.flatnonzero(act)
    assert info["n_active"] == idx.size and np.array_equal(dof, idx)
    H = sp.csr_matrix((val, col, rowptr), shape=(idx.size, idx.size))
    Ao = A[idx][:, idx].tocsr()
    scale = np.abs(Ao.data).max()
    assert abs(H - Ao).max() <= 1e-11 * scale
    assert np.abs(rhs - b[idx]).max() <= 1e-11 * np.abs(b).max()
    xv = rng.standard_normal(idx.size)
    y = s.spmv(xv)
    assert np.abs(y - Ao @ xv).max() <= 1e-11 * np.abs(Ao @ xv).max()


def linear_field(x):
    G = np.array([[0.3, -0.2], [0.15, 0.25]])
    lam, mu = EL.lame(1.0, 0.3)
    return x @ G.T + 0.1, lam * np.trace(G) * np.eye(2) + mu * (G + G.T)


def test_patch_test_through_hip(P):
    """Same material, linear displacement: the exact nodal vector satisfies the HIP system."""
    mesh, topo, x, phi, bcv = setup(P, 16, centre=(0.04, -0.03))
    ulin, sig = linear_field(x)
    s = P.InterfaceElasticitySolver(mesh, E_in=1.0, E_out=1.0)
    s.assemble(phi, np.zeros((mesh.nv, 2)), ulin, bcv)
    rowptr, col, val, rhs, dof = s.export_csr()
    B, nv = EL.Blocks(2), mesh.nv
    w = np.zeros(B.C * nv)
    for a in range(2):
        for side in (0, 1):
            w[B.u(side, a) * nv:(B.u(side, a) + 1) * nv] = ulin[:, a]
            for bb in range(2):
                w[B.y(side, a, bb) * nv:(B.y(side, a, bb) + 1) * nv] = -sig[a, bb]
    r = s.spmv(w[dof]) - rhs
    assert np.abs(r).max() <= 1e-10 * np.abs(val).max()


def test_deterministic(P):
    mesh, topo, x, phi, bcv = setup(P, 16, centre=(0.04, -0.03))
    f, uex = demo_data()
    ue = uex(x, 1e-3)
    out = []
    for _ in range(2):
        s = P.InterfaceElasticitySolver(mesh, E_out=1e-3, deterministic=True)
        s.assemble(phi, f(x), ue, bcv)
        rowptr, col, val, rhs, dof = s.export_csr()
        s.solve(rtol=1e-10, max_iter=200000)
        out.append((rowptr, col, val, rhs, dof, s.stats["iterations"]))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def test_solve_same_material(P):
    mesh, topo, x, phi, bcv = setup(P, 16)
    ulin, _ = linear_field(x)
    s = P.InterfaceElasticitySolver(mesh, E_in=1.0, E_out=1.0)
    s.assemble(phi, np.zeros((mesh.nv, 2)), ulin, bcv)
    w = s.solve(rtol=1e-12, max_iter=50000)
    assert s.stats["relres"] <= 1e-12
    vin = np.unique(mesh.cells[mesh.cell_tag_values() != 3])
    assert np.abs(s.blocks(w)["u_in"][vin] - ulin[vin]).max() < 1e-7


def test_demo_problem(P):
    """E_in = 1, E_out = 1e-3, nu = 0.3, phi = 1 - r^2 (data.py): the u_in error at the inside vertices falls > 2.5x
    from n = 15 to 30; the solve runs with the vertex blocks."""
    E_out = 1e-3
    f, uex = demo_data()
    errs, its = [], []
    for n in (15, 30):
        mesh, topo, x, phi, bcv = setup(P, n)
        ue = uex(x, E_out)
        s = P.InterfaceElasticitySolver(mesh, E_out=E_out)
        s.assemble(phi, f(x), ue, bcv)
        w = s.solve(rtol=1e-10, max_iter=200000)
        assert s.stats["relres"] <= 1e-10
        assert s.stats["precond"] == "vertex-block-jacobi", s.stats
        its.append(s.stats["iterations"])
        vin = np.unique(mesh.cells[mesh.cell_tag_values() == 1])
        errs.append(np.abs(s.blocks(w)["u_in"][vin] - ue[vin]).max() / np.abs(ue[vin]).max())
    print("quadrilateral elasticity demo: iterations", its, "errors", errs)
    assert errs[0] / errs[1] > 2.5, errs


def test_rejections(P):
    from phifem_amd.mesh_scripts import NodalFunction
    x0, cells0 = quad_mesh(8)
    xs = x0.copy()
    xs[:, 0] += 0.2 * xs[:, 1]
    sheared = P.Mesh.from_arrays("quadrilateral", xs, cells0.astype(np.int32))
    phi = 1.0 - (xs ** 2).sum(axis=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(sheared, NodalFunction(phi), 1, box_mode=True)
    s = P.InterfaceElasticitySolver(sheared)
    bcv = np.unique(cells0[:2].reshape(-1))
    with pytest.raises(NotImplementedError):
        s.assemble(phi, np.zeros((sheared.nv, 2)), np.zeros((sheared.nv, 2)), bcv)
    mesh = P.create_rectangle([[-1.5, -1.5], [1.5, 1.5]], [8, 8], cell_type="quadrilateral")
    with pytest.raises(NotImplementedError):
        P.InterfaceElasticitySolver(mesh, coarse=4)
    P.InterfaceElasticitySolver(mesh, coarse=0)
    P.InterfaceElasticitySolver(mesh, coarse=-1)


# --- cell_errors on quadrilaterals ----------------------------------------------------------------------------------
def q3_errors_ref(mesh, u_h, exact):
    """numpy restatement: Q3 on the GLL-warped nodes, I(u_h) = u_h, 4 x 4 Gauss."""
    t = np.array([0.0, 0.5 * (1 - 5 ** -0.5), 0.5 * (1 + 5 ** -0.5), 1.0])
    gq, gw = np.polynomial.legendre.leggauss(4)
    gq, gw = 0.5 * (gq + 1.0), 0.5 * gw

    def lag(z):
        L = np.ones((z.size, 4))
        dL = np.zeros((z.size, 4))
        for k in range(4):
            for m in range(4):
                if m == k:
                    continue
                dprod = np.ones(z.size) / (t[k] - t[m])
                for r in range(4):
                    if r not in (k, m):
                        dprod = dprod * (z - t[r]) / (t[k] - t[r])
                dL[:, k] += dprod
                L[:, k] *= (z - t[m]) / (t[k] - t[m])
        return L, dL
    Lq, dLq = lag(gq)
    X = mesh.x[mesh.cells]
    o, hx, hy = X[:, 0], X[:, 1, 0] - X[:, 0, 0], X[:, 2, 1] - X[:, 0, 1]
    nx, ny = np.tile(t, 4), np.repeat(t, 4)                              # node iy * 4 + ix
    pts = o[:, None, :] + np.stack([nx[None] * hx[:, None], ny[None] * hy[:, None]], axis=2)
    ue = np.asarray(exact(pts.reshape(-1, 2).T)).reshape(-1, mesh.nc, 16)     # (ncomp, cell, node)
    uh = np.asarray(u_h).reshape(mesh.nv, -1).T
    bil = np.stack([(1 - nx) * (1 - ny), nx * (1 - ny), (1 - nx) * ny, nx * ny], axis=1)   # (16, 4)
    Ih = np.einsum("jk,pck->pcj", bil, uh[:, mesh.cells])
    Nq = np.einsum("ax,by->abyx", Lq, Lq).reshape(4, 4, 16)            # [qx, qy, j]
    Nx = np.einsum("ax,by->abyx", dLq, Lq).reshape(4, 4, 16)
    Ny = np.einsum("ax,by->abyx", Lq, dLq).reshape(4, 4, 16)
    W = np.outer(gw, gw)

    def integrals(v):
        val = np.einsum("abj,pcj->pcab", Nq, v)
        gx = np.einsum("abj,pcj->pcab", Nx, v) / hx[None, :, None, None]
        gy = np.einsum("abj,pcj->pcab", Ny, v) / hy[None, :, None, None]
        det = (hx * hy)[:, None, None]
        return (np.einsum("ab,cab->c", W, det * (val ** 2).sum(axis=0)),
                np.einsum("ab,cab->c", W, det * (gx ** 2 + gy ** 2).sum(axis=0)))
    l2, h10 = integrals(ue - Ih)
    nl2, nh10 = integrals(ue)
    return l2, h10, nl2.sum(), nh10.sum()


def nonuniform_quads(n):
    tx = np.cumsum(np.r_[0.0, 0.5 + np.random.default_rng(1).random(n)])
    ty = np.cumsum(np.r_[0.0, 0.5 + np.random.default_rng(2).random(n)])
    X, Y = np.meshgrid(tx / tx[-1] * 2.0 - 0.7, ty / ty[-1] * 1.6 - 0.4, indexing="xy")
    x = np.stack([X.reshape(-1), Y.reshape(-1)], axis=1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    v0 = (j * (n + 1) + i).reshape(-1)
    return x, np.stack([v0, v0 + 1, v0 + n + 1, v0 + n + 2], axis=1).astype(np.int32)


@pytest.mark.parametrize("ncomp", [1, 2])
def test_cell_errors_quad_vs_reference(P, ncomp):
    from phifem_amd.postprocess import cell_errors
    x, cells = nonuniform_quads(9)
    mesh = P.Mesh.from_arrays("quadrilateral", x, cells)
    if ncomp == 1:
        exact = lambda p: np.sin(2.0 * p[0]) * np.cos(p[1]) + p[0] ** 2          # noqa: E731
    else:
        exact = lambda p: np.stack([np.sin(2.0 * p[0]) * np.cos(p[1]), np.exp(0.5 * p[0] - p[1])])  # noqa: E731
    uh = exact(x.T).T
    noise = 0.05 * np.cos(3.0 * x[:, 0] + x[:, 1])
    uh = uh + (noise if uh.ndim == 1 else noise[:, None])
    e = cell_errors(mesh, uh, exact, degree=1)
    l2, h10, nl2, nh10 = q3_errors_ref(mesh, uh, exact)
    assert np.abs(e["l2_local"] - l2).max() <= 1e-12 * np.abs(l2).max()
    assert np.abs(e["h10_local"] - h10).max() <= 1e-12 * np.abs(h10).max()
    assert e["l2_norm_exact"] == pytest.approx(nl2, rel=1e-12)
    assert e["h10_norm_exact"] == pytest.approx(nh10, rel=1e-12)
    sel = np.array([3, 0, 40, 17], dtype=np.int32)
    es = cell_errors(mesh, uh, exact, degree=1, cells=sel)
    assert np.allclose(es["l2_local"], e["l2_local"][sel], rtol=1e-14, atol=0.0)


def test_cell_errors_quad_exact_cases(P):
    from phifem_amd.postprocess import cell_errors
    x, cells = nonuniform_quads(6)
    mesh = P.Mesh.from_arrays("quadrilateral", x, cells)
    # a bilinear exact solution lies in Q1: the error vanishes
    bil = lambda p: np.stack([1.0 + 2.0 * p[0] - p[1] + 0.7 * p[0] * p[1], -0.3 * p[0] * p[1] + p[1]])  # noqa: E731
    e = cell_errors(mesh, bil(x.T).T, bil, degree=1)
    assert e["l2_sum"] <= 1e-28 * e["l2_norm_exact"] and e["h10_sum"] <= 1e-28 * e["h10_norm_exact"]
    assert e["l2_relative"] <= 1e-14 and e["h10_relative"] <= 1e-14
    # the norms of a Q3 polynomial are its closed-form integrals over [x0, x1] x [y0, y1]
    q3 = lambda p: p[0] ** 3 * p[1] ** 3        # noqa: E731
    e = cell_errors(mesh, np.zeros(mesh.nv), q3, degree=1)
    x0, x1, y0, y1 = x[:, 0].min(), x[:, 0].max(), x[:, 1].min(), x[:, 1].max()
    i7 = lambda a, b: (b ** 7 - a ** 7) / 7.0   # noqa: E731
    i5 = lambda a, b: (b ** 5 - a ** 5) / 5.0   # noqa: E731
    assert e["l2_norm_exact"] == pytest.approx(i7(x0, x1) * i7(y0, y1), rel=1e-12)
    assert e["h10_norm_exact"] == pytest.approx(9.0 * (i5(x0, x1) * i7(y0, y1) + i7(x0, x1) * i5(y0, y1)), rel=1e-12)
    assert e["l2_sum"] == pytest.approx(e["l2_norm_exact"], rel=1e-12)
