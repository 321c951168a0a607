"""tests/krylov_ref.py pinned without a GPU: phase by phase against the numpy stand-in of the distributed CPU tests
(tests/cpu_backend.py, written independently), the iteration against a direct solve, both restart causes, and the
reduced loop's starting point."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl
import torch

import krylov_ref as K
from cpu_backend import CpuBackend, assemble_local
from phifem_amd import dist_solver as D

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def slab():
    x, topo, cv, A, b, act = assemble_local(8, 1, 0, 8)
    return A, b, act, topo.nv


def _own(kind, n):
    if kind == "all":
        return np.ones(n, dtype=np.uint8)
    return (np.random.default_rng(4).random(n) < 0.5).astype(np.uint8)


# The ONE difference in layout between the two statements.  CpuBackend keeps a single rho: KR_UPDATE_P / KR_BEGIN2 /
# KR_RESTART write S_RHO and KR_UPDATE_S reads it.  The device (and krylov_ref) write S_RHO_NEXT there, and KR_UPDATE_S
# copies it to S_RHO, which is the "old" rho of beta.  So CpuBackend's S_RHO is the reference's S_RHO_NEXT at all times;
# S_RESTARTS and S_MODE do not exist in CpuBackend, and its KR_BEGIN always vetoes (R_RR = 1).
SCALARS = [(K.S_RHO, K.S_RHO_NEXT), (K.S_ALPHA, K.S_ALPHA), (K.S_OMEGA, K.S_OMEGA), (K.S_BB, K.S_BB), (K.S_RR, K.S_RR)] + \
          [(K.R_OFF + q, K.R_OFF + q) for q in (K.R_RV, K.R_TS, K.R_TT, K.R_RHO, K.R_RR)]


@pytest.mark.parametrize("owned", ["all", "half"])
def test_phases_match_the_cpu_backend(slab, owned):
    A, b, act, nv = slab
    be = CpuBackend(A, b, act, nv)
    n = be.n
    own = _own(owned, n)
    work = torch.zeros(10 * n, dtype=torch.float64)
    scal = torch.zeros(D.SCAL_DOUBLES, dtype=torch.float64)
    be.attach(work, scal, torch.from_numpy(own))
    ownb = own.astype(bool)
    V = {k: np.zeros(n) for k in K.NAMES}
    S = np.zeros(K.HEAD)

    def compare(what):
        w = work.numpy()
        for i, k in enumerate(K.NAMES[:8]):
            assert np.array_equal(w[i * n:(i + 1) * n], V[k]), (what, k)
        sc = scal.numpy()
        for cpu, ref in SCALARS:
            assert sc[cpu] == S[ref] or abs(sc[cpu] - S[ref]) <= 4 * EPS * abs(S[ref]), (what, cpu, sc[cpu], S[ref])

    def spmv(src, dst, dots):
        """The SpMV phases are the backend's own business: the same product into the reference state."""
        V[dst] = np.where(ownb, be.As @ V[src], 0.0)
        for q, (a, c) in dots.items():
            S[K.R_OFF + q] = V[a] @ V[c]

    be.phase(D.KR_BEGIN)
    V, S = K.phase_begin(V, S, ownb, None, False, be.rhs, veto=1.0)
    compare("begin")
    be.phase(D.KR_BEGIN2)
    V, S = K.phase_begin2(V, S)
    assert S[K.S_MODE] == 1.0
    compare("begin2")
    for it in range(4):
        be.phase(D.KR_SPMV_P)
        spmv("p", "v", {K.R_RV: ("v", "rhat")})
        be.phase(D.KR_UPDATE_S)
        V, S = K.phase_update_s(V, S, ownb, None, False)
        compare(f"update_s {it}")
        be.phase(D.KR_SPMV_S)
        spmv("s", "t", {K.R_TS: ("t", "s"), K.R_TT: ("t", "t")})
        be.phase(D.KR_UPDATE_XR)
        V, S = K.phase_update_xr(V, S, ownb, None, False)
        compare(f"update_xr {it}")
        be.phase(D.KR_UPDATE_P)
        V, S = K.phase_update_p(V, S, ownb, None, False)
        compare(f"update_p {it}")
    assert S[K.S_RESTARTS] == 0.0
    be.phase(D.KR_TRUE_SPMV)
    spmv("y", "t", {})
    be.phase(D.KR_TRUE_RESIDUAL)
    V, S = K.phase_true_residual(V, S, ownb)
    compare("true residual")
    be.phase(D.KR_RESTART)
    V, S = K.phase_restart(V, S, ownb, None, False)
    compare("restart")
    assert S[K.S_RESTARTS] == 1.0 and S[K.S_RHO] == S[K.S_RHO_NEXT] == S[K.R_OFF + K.R_RR]
    # a forced breakdown: both statements copy r to p and rhat and take (r, r) for rho
    scal.numpy()[K.S_OMEGA] = 0.0
    S[K.S_OMEGA] = 0.0
    be.phase(D.KR_UPDATE_P)
    V, S = K.phase_update_p(V, S, ownb, None, False)
    compare("update_p, omega = 0")
    assert S[K.S_RESTARTS] == 2.0
    out = torch.zeros(2 * nv, dtype=torch.float64)
    be.finish(out)
    ref = K.finish(V["y"], np.arange(n), be.idx, 1.0 / be.d, 2 * nv)
    assert np.all(np.abs(out.numpy() - ref) <= EPS * np.abs(ref))


def test_bicgstab_with_jacobi_reaches_the_direct_solve(slab):
    A, b, act, nv = slab
    idx = np.flatnonzero(act)
    Aa = A[idx][:, idx].tocsr()
    d = Aa.diagonal()
    rhs = b[idx]
    xd = spl.spsolve(Aa.tocsc(), rhs)
    it = K.bicgstab(Aa, rhs, lambda p: p / d, k=300)
    rel = np.array(it.rnorm) / np.linalg.norm(rhs)
    j = int(np.argmin(rel))
    assert rel[j] <= 1e-11, rel.min()
    assert not any(it.restart[:j + 1])
    # the recursive residual is the true one while the iteration is young
    assert abs(np.linalg.norm(rhs - Aa @ it.x[4]) - it.rnorm[4]) <= 1e-12 * np.linalg.norm(rhs)
    assert np.abs(it.x[j] - xd).max() <= 1e-8 * np.abs(xd).max()
    # from a starting point: the same limit
    x0 = np.random.default_rng(0).standard_normal(rhs.size) * np.abs(xd).max()
    it0 = K.bicgstab(Aa, rhs, lambda p: p / d, x0=x0, k=300)
    j0 = int(np.argmin(it0.rnorm))
    assert np.abs(it0.x[j0] - xd).max() <= 1e-8 * np.abs(xd).max()


def _state(n, seed):
    rng = np.random.default_rng(seed)
    V = {k: rng.standard_normal(n) for k in K.NAMES}
    S = np.zeros(K.HEAD)
    S[K.S_MODE] = 1.0
    S[K.S_RHO], S[K.S_ALPHA], S[K.S_OMEGA], S[K.S_RESTARTS] = 1.7, 0.6, 0.8, 3.0
    S[K.R_OFF + K.R_RR] = 2.5
    S[K.R_OFF + K.R_RHO] = -0.9
    return V, S


def test_both_restart_causes():
    n = 37
    own = np.arange(n) % 3 != 0
    rest = np.arange(n) >= 20
    V0, S0 = _state(n, 1)
    # no restart: owned rows get the recurrence, the others 0, rho_next = (rhat, r)
    V, S = K.phase_update_p(V0, S0, own, rest, True)
    beta = (-0.9 / 1.7) * (0.6 / 0.8)
    assert K.written(V0, V) == ["p", "phat"]
    assert np.array_equal(V["p"], np.where(own, V0["r"] + beta * (V0["p"] - 0.8 * V0["v"]), 0.0))
    assert np.array_equal(V["phat"][rest], V["p"][rest]) and np.array_equal(V["phat"][~rest], V0["phat"][~rest])
    assert S[K.S_RHO_NEXT] == -0.9 and S[K.S_RR] == 2.5 and S[K.S_RESTARTS] == 3.0 and S[K.S_RHO] == 1.7
    # cause 2, collapse: |(rhat, r)| <= 1e-14 (r, r) restarts, twice that does not
    for factor, expect in ((0.5e-14, True), (2e-14, False)):
        S1 = S0.copy()
        S1[K.R_OFF + K.R_RHO] = factor * S1[K.R_OFF + K.R_RR]
        assert K.kr_restart(S1, S1[K.R_OFF + K.R_RHO], S1[K.R_OFF + K.R_RR])[0] is expect
        V, S = K.phase_update_p(V0, S1, own, rest, True)
        assert S[K.S_RESTARTS] == (4.0 if expect else 3.0)
        if expect:
            # r is copied on EVERY row, owned or not, and RestOut follows
            assert K.written(V0, V) == ["rhat", "p", "phat"]
            assert np.array_equal(V["p"], V0["r"]) and np.array_equal(V["rhat"], V0["r"])
            assert np.array_equal(V["phat"][rest], V0["r"][rest])
            assert S[K.S_RHO_NEXT] == S1[K.R_OFF + K.R_RR]
        else:
            assert S[K.S_RHO_NEXT] == S1[K.R_OFF + K.R_RHO]
    # cause 1, a beta that is not finite: omega = 0 (inf), rho = 0 with rho_new = 0 (nan)
    for idx, rho_new in ((K.S_OMEGA, -0.9), (K.S_RHO, 0.0)):
        S1 = S0.copy()
        S1[idx] = 0.0
        S1[K.R_OFF + K.R_RHO] = rho_new
        V, S = K.phase_update_p(V0, S1, own, rest, True)
        assert S[K.S_RESTARTS] == 4.0 and S[K.S_RHO_NEXT] == 2.5 and np.array_equal(V["rhat"], V0["r"])
    # without phat of its own nothing but p (and rhat) is written
    V, S = K.phase_update_p(V0, S0, own, None, False)
    assert K.written(V0, V) == ["p"]


def test_iteration_restarts_on_a_collapse():
    """This 3 x 3 system with b = e_1 ends its first iteration with r orthogonal to rhat: the iteration restarts from r
    (p = rhat = r, rho = (r, r)) and reaches the solution three iterations later."""
    A = sp.csr_matrix(np.array([[2.0, 2.0, -1.0], [1.0, 2.0, 1.0], [2.0, 1.0, 1.0]]))
    b = np.array([1.0, 0.0, 0.0])
    it = K.bicgstab(A, b, lambda p: p, k=4, keep=True)
    assert it.restart == [True, False, False, False], it.restart
    assert np.array_equal(it.vectors[0]["p"], it.vectors[0]["r"]) and np.array_equal(it.vectors[0]["rhat"], it.vectors[0]["r"])
    assert np.abs(A @ it.x[3] - b).max() <= 1e-14


def test_reduced_start_keeps_the_krylov_vectors_zero_on_C():
    """B = A M^-1 with B[C, :] = I[C, :]: from x0 = M^-1 E_C b_C the residual vanishes on C and stays there."""
    rng = np.random.default_rng(8)
    n = 60
    C = np.sort(rng.choice(n, 25, replace=False))
    B = np.eye(n) * 4.0 + 0.3 * rng.standard_normal((n, n))
    B[C] = np.eye(n)[C]
    M = np.diag(1.0 + rng.random(n)) + 0.05 * rng.standard_normal((n, n))      # the preconditioner's matrix
    Minv = np.linalg.inv(M)
    A = B @ M
    b = rng.standard_normal(n)
    minv = lambda p: Minv @ p
    x0 = K.reduced_start(A, b, minv, C)
    assert np.abs((b - A @ x0)[C]).max() <= 1e-13
    it = K.bicgstab(A, b, minv, x0=x0, k=6, keep=True)
    for j, vec in enumerate(it.vectors):
        for k in ("r", "s", "p", "v", "t"):
            assert np.abs(vec[k][C]).max() <= 1e-12 * max(1.0, np.abs(vec[k]).max()), (j, k)
    assert it.rnorm[-1] < it.rnorm[0]
    # ... while a start from zero does not
    plain = K.bicgstab(A, b, minv, k=1, keep=True)
    assert np.abs(plain.vectors[0]["p"][C]).max() > 1e-3
