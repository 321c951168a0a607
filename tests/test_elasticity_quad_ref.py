"""CPU checks of the quadrilateral interface-elasticity restatement (`tests/elasticity_quad_ref.py`, the forms of
demo/interface-elasticity/main.py:179-269 with Q1 spaces on rectangles): the 3 x 3 / 2-point rules are exact, the
bulk stiffness is symmetric with the rigid-body modes in its kernel, the same-material patch test, and convergence
to the demo's exact solution."""
import warnings

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from elasticity_quad_ref import _features, _sigma, assemble_elasticity_quad
from oracle import elasticity as EL
from oracle import tagging as T
from oracle.assembly_flux_quad import gauss01
from oracle.topology import Topology

from test_oracle_flux_quad import quad_mesh


def setup(n, centre=(0.0, 0.0)):
    x, cells = quad_mesh(n)
    topo = Topology("quadrilateral", cells, x.shape[0])
    phi = 1.0 - ((x - np.asarray(centre)) ** 2).sum(axis=1)          # data.py:39-40
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ct, ft, _, meas, _, _ = T.compute_tags_measures("quadrilateral", x, topo, T.NodalP1(phi), 1, box_mode=True)
    cv = np.zeros(topo.nc, dtype=np.int64)
    cv[ct.indices] = ct.values
    bcv = np.unique(topo.facet_vertices[topo.boundary_facets])
    return x, topo, cv, ft.values, meas, phi, bcv


def test_tags_cover_every_form():
    x, topo, cv, fv, meas, phi, bcv = setup(12, (0.04, -0.03))
    assert set(np.unique(cv)) == {1, 2, 3}
    assert (fv == 3).any() and (fv == 4).any()
    assert np.asarray(meas(100)).size > 0 and np.asarray(meas(101)).size > 0


@pytest.mark.parametrize("E_out", [1e-3, 1.0])
def test_rules_are_exact(E_out):
    """3 x 3 cell / 2-point facet Gauss rules give the matrix of the 5 x 5 / 4-point rules to round-off."""
    x, topo, cv, fv, meas, phi, bcv = setup(12, (0.04, -0.03))
    rng = np.random.default_rng(3)
    f = np.sin(x @ rng.standard_normal((2, 2))) + 0.3
    uD = np.cos(x @ rng.standard_normal((2, 2)))
    args = (topo, x, cv, fv, meas(100), meas(101), phi, f, uD, bcv)
    A3, b3, a3 = assemble_elasticity_quad(*args, E_out=E_out, nq=3, nqf=2)
    A5, b5, a5 = assemble_elasticity_quad(*args, E_out=E_out, nq=5, nqf=4)
    assert np.array_equal(a3, a5)
    assert abs(A3 - A5).max() <= 1e-13 * abs(A5).max()
    assert np.abs(b3 - b5).max() <= 1e-13 * np.abs(b5).max()


def test_bulk_stiffness_symmetric_with_rigid_modes():
    hx, hy = np.array([0.3]), np.array([0.2])
    g1, w1 = gauss01(3)
    xi, eta = (a.reshape(-1) for a in np.meshgrid(g1, g1, indexing="ij"))
    wq = (w1[:, None] * w1[None, :]).reshape(-1) * hx[0] * hy[0]
    N, dN, U, Y, P, G, DY = _features(hx, hy, xi, eta)
    lam, mu = EL.lame(1.0, 0.3)
    S = _sigma(G[:, :, :, 0], lam, mu)
    Eps = 0.5 * (G[:, :, :, 0] + np.swapaxes(G[:, :, :, 0], -1, -2))
    K = np.einsum("q,cqjab,cqiab->cij", wq, S, Eps)[0]
    B = EL.Blocks(2)
    iu = np.array([B.u(0, a) * 4 + i for a in range(2) for i in range(4)])
    Ku = K[np.ix_(iu, iu)]
    assert np.abs(Ku - Ku.T).max() <= 1e-14 * np.abs(Ku).max()
    assert np.abs(K).sum() == pytest.approx(np.abs(Ku).sum())            # nothing outside the u_in block
    X = np.array([[0.0, 0.0], [hx[0], 0.0], [0.0, hy[0]], [hx[0], hy[0]]])
    for mode in (np.array([[1.0, 0.0]] * 4), np.array([[0.0, 1.0]] * 4), np.stack([-X[:, 1], X[:, 0]], axis=1)):
        assert np.abs(Ku @ mode.T.reshape(-1)).max() <= 1e-13 * np.abs(Ku).max()
    assert np.linalg.matrix_rank(Ku) == 8 - 3


@pytest.mark.parametrize("n", [12, 16])
def test_same_material_patch_test(n):
    """E_out = E_in, f = 0, u linear: u_in = u_out = u, y_in = y_out = -sigma(u), p = 0 solves the system."""
    x, topo, cv, fv, meas, phi, bcv = setup(n, (0.04, -0.03))
    G = np.array([[0.3, -0.2], [0.15, 0.25]])
    ulin = x @ G.T + 0.1
    lam, mu = EL.lame(1.0, 0.3)
    sig = lam * np.trace(G) * np.eye(2) + mu * (G + G.T)
    A, b, act = assemble_elasticity_quad(topo, x, cv, fv, meas(100), meas(101), phi, np.zeros((topo.nv, 2)), ulin,
                                         bcv, E_in=1.0, E_out=1.0)
    B, nv = EL.Blocks(2), topo.nv
    w = np.zeros(B.C * nv)
    for a in range(2):
        for side in (0, 1):
            w[B.u(side, a) * nv:(B.u(side, a) + 1) * nv] = ulin[:, a]
            for bb in range(2):
                w[B.y(side, a, bb) * nv:(B.y(side, a, bb) + 1) * nv] = -sig[a, bb]
    w[~act] = 0.0
    r = (A @ w - b)[act]
    assert np.abs(r).max() <= 1e-10 * max(np.abs(b).max(), np.abs(A.data).max() * np.abs(w).max())
    idx = np.flatnonzero(act)
    xs = spla.spsolve(A[idx][:, idx].tocsc(), b[idx])
    assert np.abs(xs - w[idx]).max() < 1e-8


def demo_data():
    import sympy as sy
    E_in, nu = 1.0, 0.3
    X, Y = sy.symbols("x y")
    r = sy.sqrt(X ** 2 + Y ** 2)
    u = sy.Matrix([sy.cos(r), sy.cos(r)])
    lam, mu = EL.lame(E_in, nu)
    grad = u.jacobian([X, Y])
    sig = lam * (grad[0, 0] + grad[1, 1]) * sy.eye(2) + mu * (grad + grad.T)
    f_sym = -sy.Matrix([sy.diff(sig[0, 0], X) + sy.diff(sig[0, 1], Y),
                        sy.diff(sig[1, 0], X) + sy.diff(sig[1, 1], Y)]) / E_in
    ffun = sy.lambdify((X, Y), f_sym, "numpy")

    def f(x):
        xs = np.where(np.abs(x) < 1e-12, 1e-9, x)
        return np.array(ffun(xs[:, 0], xs[:, 1])).reshape(2, -1).T

    def uex(x, E_out):
        rr = np.sqrt((x ** 2).sum(axis=1))
        v = np.cos(rr) - np.cos(1.0) / E_in
        v = np.where(rr < 1.0, v * (E_in / E_out), v)
        return np.stack([v, v], axis=1)
    return f, uex


def test_convergence_to_the_demo_solution():
    """E_in = 1, E_out = 1e-3, phi = 1 - r^2: the u_in error at the inside vertices falls > 2.5x from n = 15 to 30."""
    E_out = 1e-3
    f, uex = demo_data()
    errs = []
    for n in (15, 30):
        x, topo, cv, fv, meas, phi, bcv = setup(n)
        ue = uex(x, E_out)
        A, b, act = assemble_elasticity_quad(topo, x, cv, fv, meas(100), meas(101), phi, f(x), ue, bcv, E_out=E_out)
        idx = np.flatnonzero(act)
        w = np.zeros(b.size)
        w[idx] = spla.spsolve(A[idx][:, idx].tocsc(), b[idx])
        nv = topo.nv
        vin = np.unique(topo.cells[cv == 1])
        u_in = np.stack([w[0:nv], w[nv:2 * nv]], axis=1)
        errs.append(np.abs(u_in[vin] - ue[vin]).max() / np.abs(ue[vin]).max())
    assert errs[0] / errs[1] > 2.5, errs
