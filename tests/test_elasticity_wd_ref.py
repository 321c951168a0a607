"""The numpy specification of weak-Dirichlet elasticity (tests/elasticity_wd_ref.py) against what the scheme has to
satisfy on its own: patch test, rigid-body kernel, the scalar penalty blocks of the Poisson oracle, an independent
quadrature of the same integrands, and the convergence rate of a manufactured solution.  No GPU use."""
import functools

import numpy as np
import pytest

import elasticity_wd_ref as R
from oracle import assembly as OA
from oracle.assembly_quad import simplex_rule
from oracle.elasticity import lame
from oracle.points import FACET_VERTS

CENTRE = (0.03, -0.02, 0.01)
GRAD = np.array([[0.3, -0.2, 0.1], [0.15, 0.25, -0.05], [0.05, 0.1, -0.3]])


@functools.lru_cache(maxsize=None)
def problem(d, n):
    return R.box_problem(d, n, CENTRE)


def smooth_data(x, seed=5):
    d = x.shape[1]
    rng = np.random.default_rng(seed)
    return np.sin(x @ rng.standard_normal((d, d))) + 0.3, np.cos(x @ rng.standard_normal((d, d)))


@pytest.mark.parametrize("d,n", [(2, 16), (3, 6)])
def test_patch_test(d, n):
    """A linear displacement with f = 0, u_D = u_lin: (u_lin, 0) satisfies the system."""
    topo, x, ct, ft, ds, phi = problem(d, n)
    ulin = x @ GRAD[:d, :d].T + 0.1
    A, b, act = R.assemble_elasticity_wd(topo, x, ct, ft, ds, phi, np.zeros_like(x), ulin)
    w = np.concatenate([ulin.T.reshape(-1), np.zeros(d * topo.nv)])
    r = A @ w - b
    print(f"patch test d={d} n={n}: residual {np.abs(r[act]).max():.3e}, max|A| {np.abs(A.data).max():.3e}")
    assert np.abs(r[act]).max() <= 1e-12 * np.abs(A.data).max()
    assert np.all(r[~act] == 0.0)
    wd = R.solve_direct(A, b, act)
    assert np.abs(wd - np.where(act, w, 0.0)).max() <= 1e-9
    assert np.all(wd[~act] == 0.0)


@pytest.mark.parametrize("d,n", [(2, 16), (3, 6)])
def test_rigid_body_fields_in_the_kernel(d, n):
    """Translations and infinitesimal rotations carry no stress: stiffness + jump terms (pen = 0) annihilate them on
    the rows of vertices that touch no ds facet (the one-sided boundary term has rows on the ds vertices only)."""
    topo, x, ct, ft, ds, phi = problem(d, n)
    A, _, act = R.assemble_elasticity_wd(topo, x, ct, ft, ds, phi, np.zeros_like(x), np.zeros_like(x), pen_coef=0.0)
    ents = np.asarray(ds).reshape(-1, 2)
    on_ds = np.zeros(topo.nv, dtype=bool)
    on_ds[np.take_along_axis(topo.cells[ents[:, 0]], FACET_VERTS[topo.cell_type][ents[:, 1]], axis=1)] = True
    rows = act.copy()
    for a in range(2 * d):
        rows[a * topo.nv:(a + 1) * topo.nv] &= ~on_ds
    assert rows[:d * topo.nv].sum() > 0
    fields = [np.tile(np.eye(d)[a], (topo.nv, 1)) for a in range(d)]
    for a in range(d):
        for c in range(a + 1, d):
            W = np.zeros((d, d))
            W[a, c], W[c, a] = 1.0, -1.0
            fields.append(x @ W.T)
    scale = np.abs(A.data).max()
    for u in fields:
        w = np.concatenate([u.T.reshape(-1), np.zeros(d * topo.nv)])
        assert np.abs((A @ w)[rows]).max() <= 1e-12 * scale * max(np.abs(u).max(), 1.0)
    # and a field whose stress has a divergence is not in it
    w = np.concatenate([(x ** 2 * np.arange(1, d + 1)).T.reshape(-1), np.zeros(d * topo.nv)])
    assert np.abs((A @ w)[rows]).max() > 1e-3 * scale


@pytest.mark.parametrize("d,n", [(2, 16), (3, 6)])
def test_penalty_blocks_are_the_scalar_ones(d, n):
    """pen h^-2 (u - phi p / h) . (v - phi q / h) is the scalar penalty block once per component."""
    topo, x, ct, ft, ds, phi = problem(d, n)
    nv = topo.nv
    f, uD = smooth_data(x)
    zero = np.zeros_like(x)
    kw = dict(stab_coef=0.0)
    A1, b1, _ = R.assemble_elasticity_wd(topo, x, ct, ft, ds, phi, zero, uD, pen_coef=1.3, **kw)
    A0, b0, _ = R.assemble_elasticity_wd(topo, x, ct, ft, ds, phi, zero, uD, pen_coef=0.0, **kw)
    P, bp = (A1 - A0).tocsr(), b1 - b0
    cutv = np.unique(topo.cells[ct == 2])
    assert cutv.size > 0
    for a in range(d):
        S1, s1, _ = OA.assemble_poisson_wd(topo, x, ct, ft, ds, phi, np.zeros(nv), uD[:, a], pen_coef=1.3, stab_coef=0.0)
        S0, s0, _ = OA.assemble_poisson_wd(topo, x, ct, ft, ds, phi, np.zeros(nv), uD[:, a], pen_coef=0.0, stab_coef=0.0)
        Q, bq = (S1 - S0).tocsr(), s1 - s0
        el = np.concatenate([a * nv + cutv, (d + a) * nv + cutv])
        sc = np.concatenate([cutv, nv + cutv])
        # both sides are differences of two assemblies: each entry carries the rounding of the sums it was taken from
        # (a handful of terms of the size of the largest entry), not of the penalty term alone
        eps = np.finfo(np.float64).eps
        assert abs(P[el][:, el] - Q[sc][:, sc]).max() <= 16 * eps * (np.abs(A1.data).max() + np.abs(S1.data).max())
        assert np.abs(bp[el] - bq[sc]).max() <= 16 * eps * (np.abs(b1).max() + np.abs(s1).max())
        assert np.abs(Q[sc][:, sc].data).max() > 1e-3 * np.abs(A1.data).max()      # the blocks are there to compare
        # nothing couples different components
        other = np.setdiff1d(np.arange(2 * d * nv), np.concatenate([a * nv + np.arange(nv), (d + a) * nv + np.arange(nv)]))
        assert abs(P[el][:, other]).max() == 0.0


def assemble_by_quadrature(topo, x, ct, ft, ds, phi, f, uD, E, nu, pen, stab, degree=8):
    """The same integrands, integrated numerically: strain and stress tensors written out (no symmetry shortcut), P1
    functions evaluated at the points of a Stroud rule exact for `degree`, facet measures from the vertex coordinates."""
    import scipy.sparse as sp
    cells, nv = topo.cells, topo.nv
    d = x.shape[1]
    n = d + 1
    lam_, mu_ = lame(E, nu)
    g, vol, h = OA.simplex_geometry(x, cells)
    L, wq = simplex_rule(d, degree)
    Lf, wf = simplex_rule(d - 1, degree)
    eye = np.eye(d)

    def stress(c):
        """eps, sig [i, a] (d x d) of the basis N_i e_a on cell c."""
        eps = np.zeros((n, d, d, d))
        for i in range(n):
            for a in range(d):
                G = np.outer(eye[a], g[c, i])
                eps[i, a] = 0.5 * (G + G.T)
        sig = lam_ * np.trace(eps, axis1=2, axis2=3)[..., None, None] * eye + 2.0 * mu_ * eps
        return eps, sig

    def facet_measure(c, lf):
        p = x[cells[c, FACET_VERTS[topo.cell_type][lf]]]
        if d == 2:
            return np.linalg.norm(p[1] - p[0])
        return 0.5 * np.linalg.norm(np.cross(p[1] - p[0], p[2] - p[0]))

    def outward_normal(c, lf):
        p = x[cells[c, FACET_VERTS[topo.cell_type][lf]]]
        if d == 2:
            t = p[1] - p[0]
            nrm = np.array([t[1], -t[0]])
        else:
            nrm = np.cross(p[1] - p[0], p[2] - p[0])
        nrm /= np.linalg.norm(nrm)
        return nrm if nrm @ (p[0] - x[cells[c, lf]]) > 0 else -nrm

    R_, C_, V_ = [], [], []
    b = np.zeros(2 * d * nv)
    for c in np.flatnonzero((ct == 1) | (ct == 2)):
        eps, sig = stress(c)
        K = vol[c] * wq.sum() * np.einsum("iapq,jcpq->iajc", eps, sig)
        for i in range(n):
            for a in range(d):
                for j in range(n):
                    for cc in range(d):
                        R_.append(a * nv + cells[c, i]); C_.append(cc * nv + cells[c, j]); V_.append(K[i, a, j, cc])
                b[a * nv + cells[c, i]] += vol[c] * np.sum(wq * (L @ f[cells[c], a]) * L[:, i])
    for c, lf in np.asarray(ds).reshape(-1, 2):
        _, sig = stress(c)
        nrm, area = outward_normal(c, lf), facet_measure(c, lf)
        Lc = np.insert(Lf, lf, 0.0, axis=1)             # facet points in the barycentric coordinates of the cell
        for i in range(n):
            Ni = np.sum(wf * Lc[:, i])
            for a in range(d):
                for j in range(n):
                    for cc in range(d):
                        R_.append(a * nv + cells[c, i]); C_.append(cc * nv + cells[c, j])
                        V_.append(-area * Ni * (sig[j, cc] @ nrm)[a])
    for c in np.flatnonzero(ct == 2):
        ph, hc = L @ phi[cells[c]], h[c]
        B = np.concatenate([L, -(ph / hc)[:, None] * L], axis=1)       # v = N_i e_a -> N_i;  q = N_i e_a -> -phi N_i / h
        Mq = pen * hc ** -2 * vol[c] * np.einsum("q,qr,qs->rs", wq, B, B)
        for a in range(d):
            rq = pen * hc ** -2 * vol[c] * np.einsum("q,q,qr->r", wq, L @ uD[cells[c], a], B)
            for r in range(2 * n):
                row = ((d + a) if r >= n else a) * nv + cells[c, r % n]
                b[row] += rq[r]
                for s in range(2 * n):
                    R_.append(row); C_.append(((d + a) if s >= n else a) * nv + cells[c, s % n]); V_.append(Mq[r, s])
    for fct in np.flatnonzero(((ft == 2) | (ft == 3)) & (topo.f2c[:, 1] >= 0)):
        cp, cm = topo.f2c[fct]
        lfp = int(np.argmax(topo.c2f[cp] == fct))
        nrm, area = outward_normal(cp, lfp), facet_measure(cp, lfp)
        tr = [np.einsum("iapq,q->iap", stress(cp)[1], nrm), -np.einsum("iapq,q->iap", stress(cm)[1], nrm)]   # jump
        wgt = stab * 0.5 * (h[cp] + h[cm]) * area * wf.sum()
        for cr, Tr in zip((cp, cm), tr):
            for ccol, Tc in zip((cp, cm), tr):
                Kf = wgt * np.einsum("iap,jcp->iajc", Tr, Tc)
                for i in range(n):
                    for a in range(d):
                        for j in range(n):
                            for cc in range(d):
                                R_.append(a * nv + cells[cr, i]); C_.append(cc * nv + cells[ccol, j]); V_.append(Kf[i, a, j, cc])
    A = sp.coo_matrix((V_, (R_, C_)), shape=(2 * d * nv, 2 * d * nv)).tocsr()
    A.sum_duplicates()
    return A, b


@pytest.mark.parametrize("d,n", [(2, 8), (3, 5)])
def test_closed_forms_against_quadrature(d, n):
    topo, x, ct, ft, ds, phi = problem(d, n)
    f, uD = smooth_data(x)
    par = dict(E=1.7, nu=0.35, pen_coef=1.3, stab_coef=0.7)
    A, b, _ = R.assemble_elasticity_wd(topo, x, ct, ft, ds, phi, f, uD, **par)
    Aq, bq = assemble_by_quadrature(topo, x, ct, ft, ds, phi, f, uD, par["E"], par["nu"], par["pen_coef"],
                                    par["stab_coef"])
    ea, eb = abs(A - Aq).max() / np.abs(A.data).max(), np.abs(b - bq).max() / np.abs(b).max()
    print(f"closed forms vs quadrature d={d}: matrix {ea:.2e}, rhs {eb:.2e}")
    assert ea <= 1e-13 and eb <= 1e-13


def manufactured(x, E=1.0, nu=0.3):
    """u = (sin x cos y, cos(x + y/2)) and f = -div sigma(u)."""
    lam_, mu_ = lame(E, nu)
    X, Y = x[:, 0], x[:, 1]
    s = X + 0.5 * Y
    u = np.stack([np.sin(X) * np.cos(Y), np.cos(s)], axis=1)
    lap = np.stack([-2.0 * np.sin(X) * np.cos(Y), -1.25 * np.cos(s)], axis=1)
    gdiv = np.stack([-np.sin(X) * np.cos(Y) - 0.5 * np.cos(s), -np.cos(X) * np.sin(Y) - 0.25 * np.cos(s)], axis=1)
    return u, -(mu_ * lap + (lam_ + mu_) * gdiv)


def test_convergence_of_the_manufactured_solution():
    """Unit circle in [-1.5, 1.5]^2, E = 1, nu = 0.3, direct solve: the RMS error at the vertices of the cells tagged 1
    falls by more than 3 from n = 32 to n = 64 (the bound of the scalar scheme; the prototype gave 2.75e-2, 6.81e-3)."""
    errs = []
    for n in (32, 64):
        topo, x, ct, ft, ds, phi = R.box_problem(2, n, (0.0, 0.0))
        u, f = manufactured(x)
        A, b, act = R.assemble_elasticity_wd(topo, x, ct, ft, ds, phi, f, u)
        w = R.solve_direct(A, b, act)
        uh = w[:2 * topo.nv].reshape(2, topo.nv).T
        vin = np.unique(topo.cells[ct == 1])
        errs.append(np.sqrt(np.mean((uh[vin] - u[vin]) ** 2)))
    print("weak-Dirichlet elasticity: RMS errors", errs, "ratio", errs[0] / errs[1])
    assert errs[0] / errs[1] > 3.0
