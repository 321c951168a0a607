"""The numpy specification of the variable-coefficient diffusion scheme (tests/diffusion_ref.py) against what it has to
satisfy on its own: the reaction specification at kappa = 1, homogeneity in (kappa, c, f), an independent quadrature of
every kappa-weighted integral, the patch test, second-order convergence on a manufactured problem, and exactness in
space of the time stepper.  No GPU use."""
import functools

import numpy as np
import pytest

import diffusion_ref as D
import heat_ref as R
from elasticity_wd_ref import box_problem
from oracle import assembly as OA

CENTRE = (0.03, -0.02, 0.01)
CASES = [(2, 16), (3, 6)]
PAR = dict(pen_coef=1.2, stab_coef=0.8)


@functools.lru_cache(maxsize=None)
def problem(d, n, centre=CENTRE):
    return box_problem(d, n, centre)


def smooth_data(x, seed=7):
    d = x.shape[1]
    rng = np.random.default_rng(seed)
    return [np.sin(x @ rng.standard_normal(d)) + 0.3 * k for k in range(3)]


def linear(x):
    return 1.0 + x @ np.arange(1.0, x.shape[1] + 1.0)      # 1 + x + 2 y (+ 3 z)


def linear_kappa(x):
    return 4.0 + 0.3 * (x @ np.arange(1.0, x.shape[1] + 1.0))      # positive on [-1.5, 1.5]^d


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("d,n", CASES)
def test_unit_conductivity_is_the_reaction_specification(d, n):
    topo, x, ct, ft, ds, phi = problem(d, n)
    f, uD, g = smooth_data(x)
    h = 3.0 / n
    one = np.ones(topo.nv)
    for c in (0.0, 1.0 / h, 1.0 / h ** 2):
        A0, b0, act0 = R.assemble_reaction_wd(topo, x, ct, ft, ds, phi, f, uD, c, g, **PAR)
        A, b, act = D.assemble_diffusion_wd(topo, x, ct, ft, ds, one, phi, f, uD, c, g, **PAR)
        assert np.array_equal(act, act0)
        assert np.array_equal(A.indptr, A0.indptr) and np.array_equal(A.indices, A0.indices)
        em, ev = rel(A.data, A0.data), rel(b, b0)
        print(f"kappa = 1 d={d} n={n} c={c:g}: matrix {em:.2e}, vector {ev:.2e} relative to the reaction specification")
        assert em <= 1e-13 and ev <= 1e-13
    # c = 0: the pattern is the Poisson oracle's
    Ap, _, actp = OA.assemble_poisson_wd(topo, x, ct, ft, ds, phi, f, uD, **PAR)
    A, _, act = D.assemble_diffusion_wd(topo, x, ct, ft, ds, D.smooth_kappa(x), phi, f, uD, 0.0, None, **PAR)
    assert np.array_equal(act, actp) and np.array_equal(A.indptr, Ap.indptr) and np.array_equal(A.indices, Ap.indices)


@pytest.mark.parametrize("d,n", CASES)
def test_homogeneity(d, n):
    """(kappa, c, f) -> (alpha kappa, alpha c, alpha f) gives (alpha A, alpha b)."""
    topo, x, ct, ft, ds, phi = problem(d, n)
    f, uD, g = smooth_data(x)
    kap = D.smooth_kappa(x)
    alpha = 3.7
    for c in (0.0, n / 3.0, (n / 3.0) ** 2):
        A, b, act = D.assemble_diffusion_wd(topo, x, ct, ft, ds, kap, phi, f, uD, c, g, **PAR)
        A2, b2, act2 = D.assemble_diffusion_wd(topo, x, ct, ft, ds, alpha * kap, phi, alpha * f, uD, alpha * c, g, **PAR)
        assert np.array_equal(act, act2) and np.array_equal(A.indices, A2.indices)
        em, ev = rel(A2.data, alpha * A.data), rel(b2, alpha * b)
        print(f"homogeneity d={d} n={n} c={c:g}: matrix {em:.2e}, vector {ev:.2e}")
        assert em <= 1e-13 and ev <= 1e-13


@pytest.mark.parametrize("d,n", CASES)
def test_weighted_terms_vs_quadrature(d, n):
    topo, x, ct, ft, ds, phi = problem(d, n)
    f, uD, g = smooth_data(x)
    kap = D.smooth_kappa(x)
    gg, vol, _ = OA.simplex_geometry(x, topo.cells)
    kc, Fc = kap[topo.cells], f[topo.cells]
    rng = np.random.default_rng(2)
    area = rng.uniform(0.5, 2.0, topo.nc)
    kf = kc[:, :d]
    for c in (0.0, n / 3.0, (n / 3.0) ** 2):
        pairs = [(D.stiffness_closed(gg, vol, kc), D.stiffness_quadrature(gg, vol, kc))]
        pairs += list(zip(D.residual_closed(gg, vol, kc, c, Fc), D.residual_quadrature(gg, vol, kc, c, Fc)))
        pairs += list(zip(D.facet_kappa_closed(d, area, kf), D.facet_kappa_quadrature(d, area, kf)))
        errs = [rel(a, b) for a, b in pairs]
        print(f"kappa-weighted terms d={d} n={n} c={c:g}: stiffness, residual block, residual vector, int_F kappa N_i, "
              f"int_F kappa: " + " ".join(f"{e:.2e}" for e in errs))
        assert max(errs) <= 1e-13
        # and the whole system from the quadrature
        A, b, _ = D.assemble_diffusion_wd(topo, x, ct, ft, ds, kap, phi, f, uD, c, g, **PAR)
        Aq, bq, _ = D.assemble_diffusion_wd(topo, x, ct, ft, ds, kap, phi, f, uD, c, g, quadrature=True, **PAR)
        assert np.array_equal(A.indices, Aq.indices) and rel(A.data, Aq.data) <= 1e-13 and rel(b, bq) <= 1e-13


@pytest.mark.parametrize("d,n", CASES)
def test_patch_test(d, n):
    """kappa and u linear, f = c u - grad kappa . grad u (P1), u_D = u: the scheme returns u, with p = 0.  Bound 1e-8
    max|u|, the bound of the heat exactness test (direct solves; values of order 10)."""
    topo, x, ct, ft, ds, phi = problem(d, n)
    kap, u = linear_kappa(x), linear(x)
    gkgu = 0.3 * (np.arange(1.0, d + 1.0) ** 2).sum()
    nv = topo.nv
    for c in (0.0, n / 3.0):
        A, b, act = D.assemble_diffusion_wd(topo, x, ct, ft, ds, kap, phi, c * u - gkgu, u, c, None, **PAR)
        w = OA.solve_direct(A, b, act)
        au = act[:nv]
        err, perr, umax = np.abs(w[:nv][au] - u[au]).max(), np.abs(w[nv:]).max(), np.abs(u[au]).max()
        print(f"patch test d={d} n={n} c={c:g}: |u_h - u| {err:.2e}, |p| {perr:.2e}, max|u| {umax:.2f}")
        assert err <= 1e-8 * umax and perr <= 1e-8 * umax


def test_convergence_on_the_manufactured_problem():
    """Unit disk in [-1.5, 1.5]^2, smooth kappa of contrast 10, c = 0: the root-mean-square nodal error over the vertices
    of inside cells falls by a factor >= 3 per halving (second order would be 4; the margin is for the pre-asymptotic
    range)."""
    errs = []
    for n in (16, 32, 64):
        topo, x, ct, ft, ds, phi = problem(2, n, (0.0, 0.0, 0.0))
        kap, u, f = D.manufactured(x, 0.0)
        A, b, act = D.assemble_diffusion_wd(topo, x, ct, ft, ds, kap, phi, f, u, 0.0)
        w = OA.solve_direct(A, b, act)
        inside = np.unique(topo.cells[ct == 1])
        errs.append(np.sqrt(np.mean((w[inside] - u[inside]) ** 2)))
    print("manufactured problem, rms nodal error n = 16, 32, 64: " + " ".join(f"{e:.3e}" for e in errs)
          + f" | factors {errs[0] / errs[1]:.2f} {errs[1] / errs[2]:.2f}")
    assert errs[0] >= 3.0 * errs[1] and errs[1] >= 3.0 * errs[2]


@pytest.mark.parametrize("scheme", ["bdf1", "bdf2"])
@pytest.mark.parametrize("d,n", CASES)
def test_stepper_is_exact_in_space_for_p1_data(d, n, scheme):
    """u = l(x) gamma(t) with l and kappa linear: du/dt - div(kappa grad u) = l gamma' - gamma grad kappa . grad l, so
    with f = l gamma'(t_n) - gamma_n (grad kappa . grad l) and u_D = l gamma_n (gamma_n the scheme's own scalar
    recurrence) the stepper returns l gamma_n, p = 0.  Bound 1e-8 max|u|."""
    topo, x, ct, ft, ds, phi = problem(d, n)
    dt, nsteps = 3.0 / n, 4
    ell, kap = linear(x), linear_kappa(x)
    gkgl = 0.3 * (np.arange(1.0, d + 1.0) ** 2).sum()
    dgamma = lambda t: 3.0 * t * t
    gam = R.scalar_recurrence(1.0, dgamma, dt, scheme, nsteps)
    k_of = lambda t: int(round(t / dt)) - 1
    ws = D.diffusion_steps(topo, x, ct, ft, ds, kap, phi, dt, scheme, ell, lambda t: ell * dgamma(t) - gam[k_of(t)] * gkgl,
                           lambda t: ell * gam[k_of(t)], nsteps)
    nv = topo.nv
    au = np.flatnonzero(ws[0][:nv] != 0.0)
    err = max(np.abs(w[:nv][au] - gk * ell[au]).max() for w, gk in zip(ws, gam))
    perr = max(np.abs(w[nv:]).max() for w in ws)
    umax = max(np.abs(w[:nv]).max() for w in ws)
    print(f"exactness d={d} n={n} {scheme}: |u - gamma_n l| {err:.2e}, |p| {perr:.2e}, max|u| {umax:.2f}")
    assert err <= 1e-8 * umax and perr <= 1e-8 * umax
