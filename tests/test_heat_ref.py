"""The numpy specification of the reaction / heat scheme (tests/heat_ref.py) against what it has to satisfy on its own:
the Poisson oracle at c = 0, an independent quadrature of the mass terms, and exactness in space of the time stepper
for data that is P1 in space.  No GPU use."""
import functools

import numpy as np
import pytest

import heat_ref as R
from elasticity_wd_ref import box_problem
from oracle import assembly as OA

CENTRE = (0.03, -0.02, 0.01)
CASES = [(2, 16), (3, 6)]


@functools.lru_cache(maxsize=None)
def problem(d, n):
    return box_problem(d, n, CENTRE)


def smooth_data(x, seed=7):
    d = x.shape[1]
    rng = np.random.default_rng(seed)
    return [np.sin(x @ rng.standard_normal(d)) + 0.3 * k for k in range(3)]


def linear(x):
    return 1.0 + x @ np.arange(1.0, x.shape[1] + 1.0)      # 1 + x + 2 y (+ 3 z)


@pytest.mark.parametrize("d,n", CASES)
def test_no_reaction_is_the_poisson_oracle(d, n):
    topo, x, ct, ft, ds, phi = problem(d, n)
    f, uD, g = smooth_data(x)
    A0, b0, act0 = OA.assemble_poisson_wd(topo, x, ct, ft, ds, phi, f, uD, pen_coef=1.2, stab_coef=0.8)
    for gh in (None, g, np.zeros_like(g)):
        A, b, act = R.assemble_reaction_wd(topo, x, ct, ft, ds, phi, f, uD, 0.0, gh, pen_coef=1.2, stab_coef=0.8)
        assert np.array_equal(act, act0) and np.array_equal(b, b0)
        assert np.array_equal(A.indptr, A0.indptr) and np.array_equal(A.indices, A0.indices)
        assert np.array_equal(A.data, A0.data)


@pytest.mark.parametrize("d,n", CASES)
def test_mass_terms_vs_quadrature(d, n):
    topo, x, ct, ft, ds, phi = problem(d, n)
    F = smooth_data(x)[0]
    h = 3.0 / n
    for c in (1.0 / h, 1.0 / h ** 2):
        M, l = R.mass_terms(x, topo.cells, ct, c, 0.8, F)
        Mq, lq = R.mass_quadrature(x, topo.cells, ct, c, 0.8, F)
        em = abs(M - Mq).max() / abs(Mq).max()
        el = np.abs(l - lq).max() / np.abs(lq).max()
        print(f"mass terms d={d} n={n} c={c:g}: matrix {em:.2e}, vector {el:.2e} relative to the quadrature")
        assert em <= 1e-13 and el <= 1e-13
        # symmetric, supported on the vertices of Omega_h, and the whole mass of Omega_h (plus the cut-cell weight)
        assert abs(M - M.T).max() <= 1e-15 * abs(M).max()      # duplicates are summed in another order in M.T
        vol, hh = R.cell_volume_diameter(x, topo.cells)
        wa, _ = R.cell_weights(ct, hh, c, 0.8)
        assert abs(M.sum() - (wa * vol).sum()) <= 1e-12 * (wa * vol).sum()


def run_exactness(d, n, scheme, nsteps=4):
    topo, x, ct, ft, ds, phi = problem(d, n)
    dt = 3.0 / n
    ell = linear(x)
    dgamma = lambda t: 3.0 * t * t
    gam = R.scalar_recurrence(1.0, dgamma, dt, scheme, nsteps)
    times = [dt * (k + 1) for k in range(nsteps)]
    step_of = lambda t: int(round(t / dt)) - 1
    ws = R.heat_steps(topo, x, ct, ft, ds, phi, dt, scheme, ell * 1.0, lambda t: ell * dgamma(t),
                      lambda t: ell * gam[step_of(t)], nsteps)
    nv = topo.nv
    au = np.flatnonzero(ws[0][:nv] != 0.0)
    err = max(np.abs(w[:nv][au] - g * ell[au]).max() for w, g in zip(ws, gam))
    perr = max(np.abs(w[nv:]).max() for w in ws)
    umax = max(np.abs(w[:nv]).max() for w in ws)
    assert times[-1] == pytest.approx(nsteps * dt)
    return err, perr, umax


@pytest.mark.parametrize("scheme", ["bdf1", "bdf2"])
@pytest.mark.parametrize("d,n", [(2, 16), (2, 32), (3, 6), (3, 12)])
def test_stepper_is_exact_in_space_for_p1_data(d, n, scheme):
    """u = (1 + x + 2 y [+ 3 z]) gamma(t), gamma' = 3 t^2, f = (1 + x + 2 y [+ 3 z]) gamma', dt = h, 4 steps from
    gamma(0) = 1.  u_D is the discrete solution itself: the linear function times the scheme's own scalar recurrence
    (gamma_{n+1} = gamma_n + dt gamma'(t_{n+1}); BDF2: gamma_{n+1} = (4 gamma_n - gamma_{n-1}) / 3 + (2 dt / 3)
    gamma'(t_{n+1}) after one backward Euler step), so that the stepper has to return exactly that, with p = 0.
    Bound: 1e-8 max|u| (direct solves; measured 2e-13 .. 4e-10 for backward Euler, values of order 5)."""
    err, perr, umax = run_exactness(d, n, scheme)
    print(f"exactness d={d} n={n} {scheme}: |u - gamma_n l| {err:.2e}, |p| {perr:.2e}, max|u| {umax:.2f}")
    assert err <= 1e-8 * umax and perr <= 1e-8 * umax
