"""The numpy specification of the convection-diffusion scheme (tests/convection_ref.py) against what it has to satisfy on
its own: the diffusion specification at beta = 0, the pattern and the loss of symmetry with beta != 0, homogeneity in
(kappa, beta, c, f), an independent quadrature of every new integral, the patch test, convergence on a manufactured
problem, the effect of SUPG on an outflow layer, and exactness in space of the time stepper.  No GPU use."""
import functools

import numpy as np
import pytest

import convection_ref as V
import diffusion_ref as D
import heat_ref as R
from elasticity_wd_ref import box_problem
from oracle import assembly as OA

CENTRE = (0.03, -0.02, 0.01)
CASES = [(2, 16), (3, 6)]
PAR = dict(pen_coef=1.2, stab_coef=0.8, supg_coef=0.3)
DPAR = dict(pen_coef=1.2, stab_coef=0.8)


@functools.lru_cache(maxsize=None)
def problem(d, n, centre=CENTRE):
    return box_problem(d, n, centre)


def smooth_data(x, seed=7):
    d = x.shape[1]
    rng = np.random.default_rng(seed)
    return [np.sin(x @ rng.standard_normal(d)) + 0.3 * k for k in range(3)]


def rotating_field(x, scale=3.0):
    """A smooth field of magnitude about `scale`: a rotation in the (x, y) plane plus a drift, wavy in the last axis."""
    b = np.zeros_like(x)
    b[:, 0] = -x[:, 1] + 0.4
    b[:, 1] = x[:, 0] + 0.2 * np.sin(2.0 * x[:, -1])
    if x.shape[1] == 3:
        b[:, 2] = 0.5 * np.cos(x[:, 0])
    return scale * b


def linear(x):
    return 1.0 + x @ np.arange(1.0, x.shape[1] + 1.0)      # 1 + x + 2 y (+ 3 z)


def linear_kappa(x):
    return 4.0 + 0.3 * (x @ np.arange(1.0, x.shape[1] + 1.0))      # positive on [-1.5, 1.5]^d


def linear_beta(x):
    """5 (0.5 + x - 0.4 x_d, -1 + 0.7 y, 0.2 + x): linear in x, divergence 5 * 1.7 (2-D: x_d = y, divergence 5 * 0.7 +
    5)."""
    d = x.shape[1]
    b = np.stack([0.5 + x[:, 0] - 0.4 * x[:, d - 1], -1.0 + 0.7 * x[:, 1], 0.2 + x[:, 0]], axis=1)
    return 5.0 * b[:, :d]


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("d,n", CASES)
def test_zero_velocity_is_the_diffusion_specification(d, n):
    topo, x, ct, ft, ds, phi = problem(d, n)
    f, uD, g = smooth_data(x)
    kap = D.smooth_kappa(x)
    zero = np.zeros((topo.nv, d))
    for c in (0.0, n / 3.0):
        A0, b0, act0 = D.assemble_diffusion_wd(topo, x, ct, ft, ds, kap, phi, f, uD, c, g, **DPAR)
        A, b, act = V.assemble_convection_wd(topo, x, ct, ft, ds, kap, zero, phi, f, uD, c, g, **PAR)
        assert np.array_equal(act, act0)
        assert np.array_equal(A.indptr, A0.indptr) and np.array_equal(A.indices, A0.indices)
        em, ev = rel(A.data, A0.data), rel(b, b0)
        print(f"beta = 0 d={d} n={n} c={c:g}: matrix {em:.2e}, vector {ev:.2e} relative to the diffusion specification")
        assert em <= 1e-13 and ev <= 1e-13


@pytest.mark.parametrize("d,n", CASES)
def test_pattern_is_the_poisson_oracles_and_the_matrix_is_not_symmetric(d, n):
    topo, x, ct, ft, ds, phi = problem(d, n)
    f, uD, g = smooth_data(x)
    for c in (0.0, n / 3.0):
        Ap, _, actp = OA.assemble_poisson_wd(topo, x, ct, ft, ds, phi, f, uD, **DPAR)
        A, _, act = V.assemble_convection_wd(topo, x, ct, ft, ds, D.smooth_kappa(x), rotating_field(x), phi, f, uD, c, g,
                                             **PAR)
        assert np.array_equal(act, actp) and np.array_equal(A.indptr, Ap.indptr) and np.array_equal(A.indices, Ap.indices)
        Au = A[:topo.nv][:, :topo.nv]
        asym = np.abs((Au - Au.T).data).max() / np.abs(Au.data).max()
        print(f"beta != 0 d={d} n={n} c={c:g}: |A - A^T| / |A| on the (u,u) block {asym:.2e}")
        assert asym > 1e-3


@pytest.mark.parametrize("d,n", CASES)
def test_homogeneity(d, n):
    """(kappa, beta, c, f) -> alpha (kappa, beta, c, f) gives (alpha A, alpha b)."""
    topo, x, ct, ft, ds, phi = problem(d, n)
    f, uD, g = smooth_data(x)
    kap, beta = D.smooth_kappa(x), rotating_field(x)
    alpha = 3.7
    for c in (0.0, n / 3.0):
        A, b, act = V.assemble_convection_wd(topo, x, ct, ft, ds, kap, beta, phi, f, uD, c, g, **PAR)
        A2, b2, act2 = V.assemble_convection_wd(topo, x, ct, ft, ds, alpha * kap, alpha * beta, phi, alpha * f, uD,
                                                alpha * c, g, **PAR)
        assert np.array_equal(act, act2) and np.array_equal(A.indices, A2.indices)
        em, ev = rel(A2.data, alpha * A.data), rel(b2, alpha * b)
        print(f"homogeneity d={d} n={n} c={c:g}: matrix {em:.2e}, vector {ev:.2e}")
        assert em <= 1e-13 and ev <= 1e-13


@pytest.mark.parametrize("d,n", CASES)
def test_closed_forms_vs_quadrature(d, n):
    topo, x, ct, ft, ds, phi = problem(d, n)
    f, uD, g = smooth_data(x)
    kap, beta = D.smooth_kappa(x), rotating_field(x)
    gg, vol, _ = OA.simplex_geometry(x, topo.cells)
    kc, bc, Fc = kap[topo.cells], beta[topo.cells], f[topo.cells]
    for c in (0.0, n / 3.0):
        pairs = [(V.advection_closed(gg, vol, bc), V.advection_quadrature(gg, vol, bc))]
        pairs += list(zip(V.supg_closed(gg, vol, kc, bc, c, Fc), V.supg_quadrature(gg, vol, kc, bc, c, Fc)))
        pairs += list(zip(V.residual_closed(gg, vol, kc, bc, c, Fc), V.residual_quadrature(gg, vol, kc, bc, c, Fc)))
        errs = [rel(a, b) for a, b in pairs]
        print(f"closed forms d={d} n={n} c={c:g}: advection, SUPG block, SUPG vector, residual block, residual vector: "
              + " ".join(f"{e:.2e}" for e in errs))
        assert max(errs) <= 1e-13
        # at beta = 0 the residual pair is diffusion_ref's
        B0, r0 = D.residual_closed(gg, vol, kc, c, Fc)
        B, r = V.residual_closed(gg, vol, kc, 0.0 * bc, c, Fc)
        assert rel(B, B0) <= 1e-13 and rel(r, r0) <= 1e-13
        # and the whole system from the quadrature
        A, b, _ = V.assemble_convection_wd(topo, x, ct, ft, ds, kap, beta, phi, f, uD, c, g, **PAR)
        Aq, bq, _ = V.assemble_convection_wd(topo, x, ct, ft, ds, kap, beta, phi, f, uD, c, g, quadrature=True, **PAR)
        em, ev = rel(A.data, Aq.data), rel(b, bq)
        print(f"  whole system from the quadrature: matrix {em:.2e}, vector {ev:.2e}")
        assert np.array_equal(A.indices, Aq.indices) and em <= 1e-13 and ev <= 1e-13


@pytest.mark.parametrize("d,n", CASES)
def test_patch_test(d, n):
    """kappa, beta and u linear, f = c u + beta . grad u - grad kappa . grad u (P1), u_D = u: the scheme returns u, with
    p = 0.  Bound 1e-8 max|u| (direct solves; values of order 10)."""
    topo, x, ct, ft, ds, phi = problem(d, n)
    kap, beta, u = linear_kappa(x), linear_beta(x), linear(x)
    wts = np.arange(1.0, d + 1.0)
    gkgu = 0.3 * (wts ** 2).sum()
    nv = topo.nv
    for c in (0.0, n / 3.0):
        fh = c * u + beta @ wts - gkgu
        A, b, act = V.assemble_convection_wd(topo, x, ct, ft, ds, kap, beta, phi, fh, u, c, None, **PAR)
        w = OA.solve_direct(A, b, act)
        au = act[:nv]
        err, perr, umax = np.abs(w[:nv][au] - u[au]).max(), np.abs(w[nv:]).max(), np.abs(u[au]).max()
        print(f"patch test d={d} n={n} c={c:g}: |u_h - u| {err:.2e}, |p| {perr:.2e}, max|u| {umax:.2f}")
        assert err <= 1e-8 * umax and perr <= 1e-8 * umax


@pytest.mark.parametrize("supg", [0.0, 0.25])
def test_convergence_on_the_manufactured_problem(supg):
    """Unit disk in [-1.5, 1.5]^2, `manufactured` with kscale 0.01, bscale 1 (cell Peclet numbers of order 10 at n = 16),
    c = 0, pen = stab = 1: the root-mean-square nodal error over the vertices of inside cells falls by a factor >= 3 per
    halving."""
    errs = []
    for n in (16, 32, 64):
        topo, x, ct, ft, ds, phi = problem(2, n, (0.0, 0.0, 0.0))
        kap, beta, u, f = V.manufactured(x, 0.0, 0.01, 1.0)
        A, b, act = V.assemble_convection_wd(topo, x, ct, ft, ds, kap, beta, phi, f, u, 0.0, supg_coef=supg)
        w = OA.solve_direct(A, b, act)
        inside = np.unique(topo.cells[ct == 1])
        errs.append(np.sqrt(np.mean((w[inside] - u[inside]) ** 2)))
    print(f"manufactured problem supg={supg}, rms nodal error n = 16, 32, 64: " + " ".join(f"{e:.3e}" for e in errs)
          + f" | factors {errs[0] / errs[1]:.2f} {errs[1] / errs[2]:.2f}")
    assert errs[0] >= 3.0 * errs[1] and errs[1] >= 3.0 * errs[2]


def test_supg_removes_the_overshoot_at_the_outflow_layer():
    """Unit disk, kappa = 0.01, beta = (1, 0), f = 1, u_D = 0, c = 0, n = 16: the reduced solution is x + sqrt(1 - y^2);
    the overshoot max(u_h - (x + sqrt(1 - y^2))) over the vertices of inside cells with supg 0.25 is at most half of
    what it is with supg 0."""
    topo, x, ct, ft, ds, phi = problem(2, 16, (0.0, 0.0, 0.0))
    nv = topo.nv
    beta = np.zeros((nv, 2))
    beta[:, 0] = 1.0
    inside = np.unique(topo.cells[ct == 1])
    reduced = x[inside, 0] + np.sqrt(np.maximum(1.0 - x[inside, 1] ** 2, 0.0))
    over = []
    for supg in (0.0, 0.25):
        A, b, act = V.assemble_convection_wd(topo, x, ct, ft, ds, np.full(nv, 0.01), beta, phi, np.ones(nv), np.zeros(nv),
                                             0.0, supg_coef=supg)
        w = OA.solve_direct(A, b, act)
        over.append((w[inside] - reduced).max())
    print(f"overshoot at kappa = 0.01, n = 16: supg 0 {over[0]:.3f}, supg 0.25 {over[1]:.3f}")
    assert over[0] > 0.0 and over[1] <= 0.5 * over[0]


@pytest.mark.parametrize("scheme", ["bdf1", "bdf2"])
@pytest.mark.parametrize("d,n", CASES)
def test_stepper_is_exact_in_space_for_p1_data(d, n, scheme):
    """u = l(x) gamma(t) with l, kappa and beta linear: du/dt + beta . grad u - div(kappa grad u) = l gamma' + gamma
    (beta . grad l - grad kappa . grad l), which is P1 in space; with that f at t_n (gamma_n the scheme's own scalar
    recurrence) and u_D = l gamma_n the stepper returns l gamma_n, p = 0.  Bound 1e-8 max|u|."""
    topo, x, ct, ft, ds, phi = problem(d, n)
    dt, nsteps = 3.0 / n, 4
    ell, kap, beta = linear(x), linear_kappa(x), linear_beta(x)
    wts = np.arange(1.0, d + 1.0)
    space = beta @ wts - 0.3 * (wts ** 2).sum()
    dgamma = lambda t: 3.0 * t * t
    gam = R.scalar_recurrence(1.0, dgamma, dt, scheme, nsteps)
    k_of = lambda t: int(round(t / dt)) - 1
    ws = V.convection_steps(topo, x, ct, ft, ds, kap, beta, phi, dt, scheme, ell,
                            lambda t: ell * dgamma(t) + gam[k_of(t)] * space, lambda t: ell * gam[k_of(t)], nsteps, **PAR)
    nv = topo.nv
    au = np.flatnonzero(ws[0][:nv] != 0.0)
    err = max(np.abs(w[:nv][au] - gk * ell[au]).max() for w, gk in zip(ws, gam))
    perr = max(np.abs(w[nv:]).max() for w in ws)
    umax = max(np.abs(w[:nv]).max() for w in ws)
    print(f"exactness d={d} n={n} {scheme}: |u - gamma_n l| {err:.2e}, |p| {perr:.2e}, max|u| {umax:.2f}")
    assert err <= 1e-8 * umax and perr <= 1e-8 * umax
