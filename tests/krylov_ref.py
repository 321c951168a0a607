"""The vector phases and scalar recurrences of the BiCGStab loop (test infrastructure): a float64 numpy statement of
what the kernels of `phifem_amd/csrc/phx_solve.hip` write, phase by phase, as the phase API (`phx_krylov_phase`, mode 1)
runs them, and of the iteration `kr_drive` makes of them.

State.  Ten vectors in solver order, named as in `KrVecs`: r, rhat, p, v, s, t, y, b, phat, shat (a dict), and the 16
head scalars S: S[0 .. 7] the solver state, S[R_OFF + q] the dot products of the running iteration (in mode 1 `dotv`
returns S[R_OFF + q]).  `own` is the ownership mask (None: every row), `hat` says whether phat / shat are vectors of
their own (False: the kernels are handed p / s in their place and entries 8, 9 of the workspace are never touched),
`rest` the rows `RestOut` writes (None: no RestOut; the rows outside the u block where the lattice preconditioner is
in force).

Every phase function returns a NEW (V, S): vectors the phase does not write are the very arrays that came in, written
ones are fresh arrays, so `written(V0, V1)` names what a phase wrote.  Dot products are plain numpy sums; a test that
needs them exactly sums the terms itself.
"""
import numpy as np

NAMES = ("r", "rhat", "p", "v", "s", "t", "y", "b", "phat", "shat")
S_RHO, S_ALPHA, S_OMEGA, S_BB, S_RR, S_RESTARTS, S_RHO_NEXT, S_MODE = range(8)
R_OFF = 8
R_RV, R_TS, R_TT, R_SS, R_RHO, R_RR = range(6)
HEAD = 16
RESTART_COLLAPSE = 1.0e-14      # kr_restart: |(rhat, r)| <= 1e-14 (r, r)
RESTART_HUGE = 1.0e300          # kr_restart: |beta| beyond this, or not a number

KR_BEGIN, KR_BEGIN2, KR_UPDATE_S, KR_UPDATE_XR, KR_UPDATE_P, KR_TRUE_RESIDUAL, KR_RESTART = 0, 1, 3, 5, 6, 12, 13


def _mine(own, n):
    return np.ones(n, dtype=bool) if own is None else np.asarray(own, dtype=bool)


def _put_rest(V, name, src, rest, hat):
    """RestOut::put: hat[i] = src[i] on the rows of `rest` (phat or shat apart from p / s only)."""
    if hat and rest is not None and np.any(rest):
        out = V[name].copy()
        out[rest] = src[rest]
        V[name] = out


def written(V0, V1):
    return [k for k in NAMES if V1[k] is not V0[k]]


def kr_restart(S, rho_new, rr):
    """The breakdown rule of `kr_restart`: (restart?, beta).  Cause 1: beta is not finite or beyond 1e300 (omega = 0,
    rho = 0); cause 2: (rhat, r) has collapsed relative to (r, r)."""
    with np.errstate(all="ignore"):
        beta = (np.float64(rho_new) / np.float64(S[S_RHO])) * (np.float64(S[S_ALPHA]) / np.float64(S[S_OMEGA]))
        huge = not (abs(beta) <= RESTART_HUGE)
        collapse = not (abs(rho_new) > RESTART_COLLAPSE * rr)
    return bool(huge or collapse), beta


def phase_begin(V, S, own, rest, hat, rhs, veto=0.0):
    """Phase 0 (k_kr_begin, mode 1).  `rhs`: the right-hand side in solver order (rhs[perm]).  The whole scalar block is
    cleared, b = r = rhat = p = own ? rhs : 0, y = 0, R_RHO = (b, b), R_RR = the veto of this rank."""
    V, S = dict(V), np.zeros_like(S)
    bi = np.where(_mine(own, rhs.size), rhs, 0.0)
    for k in ("b", "r", "rhat", "p"):
        V[k] = bi.copy()
    V["y"] = np.zeros_like(bi)
    _put_rest(V, "phat", bi, rest, hat)
    S[R_OFF + R_RHO] = bi @ bi
    S[R_OFF + R_RR] = veto
    return V, S


def phase_begin2(V, S, own=None, rest=None, hat=False):
    """Phase 1 (k_kr_begin2, mode 1): rho = rho_next = bb = rr = R_RHO."""
    S = S.copy()
    S[S_MODE] = 1.0
    S[S_RHO] = S[S_RHO_NEXT] = S[S_BB] = S[S_RR] = S[R_OFF + R_RHO]
    return V, S


def phase_update_s(V, S, own, rest, hat):
    """Phase 3 (k_update_s): alpha = rho_next / (rhat, v), s = own ? r - alpha v : 0; hands rho_next over to rho."""
    V, S = dict(V), S.copy()
    rho = S[S_RHO_NEXT]
    with np.errstate(all="ignore"):
        alpha = rho / S[R_OFF + R_RV]
        V["s"] = np.where(_mine(own, V["r"].size), V["r"] - alpha * V["v"], 0.0)
    _put_rest(V, "shat", V["s"], rest, hat)
    S[S_ALPHA] = alpha
    S[S_RHO] = rho
    return V, S


def phase_update_xr(V, S, own, rest, hat):
    """Phase 5 (k_update_xr): omega = (t, s) / (t, t); y += alpha phat + omega shat on owned rows, r = own ? s - omega t
    : 0; R_RHO = (rhat, r), R_RR = (r, r)."""
    V, S = dict(V), S.copy()
    mine = _mine(own, V["r"].size)
    phat, shat = (V["phat"], V["shat"]) if hat else (V["p"], V["s"])
    alpha = S[S_ALPHA]
    with np.errstate(all="ignore"):
        omega = S[R_OFF + R_TS] / S[R_OFF + R_TT]
        V["y"] = np.where(mine, V["y"] + (alpha * phat + omega * shat), V["y"])
        V["r"] = np.where(mine, V["s"] - omega * V["t"], 0.0)
    S[R_OFF + R_RHO] = V["rhat"] @ V["r"]
    S[R_OFF + R_RR] = V["r"] @ V["r"]
    S[S_OMEGA] = omega
    return V, S


def phase_update_p(V, S, own, rest, hat):
    """Phase 6 (k_update_p): beta = (rho_new / rho)(alpha / omega), p = own ? r + beta (p - omega v) : 0, rho_next =
    rho_new.  On a restart (kr_restart) p = rhat = r on EVERY row, rho_next = (r, r) and S_RESTARTS goes up by one."""
    V, S = dict(V), S.copy()
    rho_new, rr = S[R_OFF + R_RHO], S[R_OFF + R_RR]
    restart, beta = kr_restart(S, rho_new, rr)
    S[S_RHO_NEXT] = rr if restart else rho_new
    S[S_RR] = rr
    if restart:
        S[S_RESTARTS] += 1.0
        V["p"] = V["r"].copy()
        V["rhat"] = V["r"].copy()
    else:
        V["p"] = np.where(_mine(own, V["r"].size), V["r"] + beta * (V["p"] - S[S_OMEGA] * V["v"]), 0.0)
    _put_rest(V, "phat", V["p"], rest, hat)
    return V, S


def phase_true_residual(V, S, own, rest=None, hat=False):
    """Phase 12 (k_true_residual): r = own ? b - t : 0, R_RR = (r, r)."""
    V, S = dict(V), S.copy()
    V["r"] = np.where(_mine(own, V["b"].size), V["b"] - V["t"], 0.0)
    S[R_OFF + R_RR] = V["r"] @ V["r"]
    return V, S


def phase_restart(V, S, own, rest, hat):
    """Phase 13 (k_restart_from_r): rhat = p = r on every row, rho = rho_next = rr = R_RR, alpha = omega = 1."""
    V, S = dict(V), S.copy()
    V["rhat"] = V["r"].copy()
    V["p"] = V["r"].copy()
    _put_rest(V, "phat", V["r"], rest, hat)
    S[S_RHO] = S[S_RHO_NEXT] = S[S_RR] = S[R_OFF + R_RR]
    S[S_ALPHA] = S[S_OMEGA] = 1.0
    S[S_RESTARTS] += 1.0
    return V, S


PHASES = {KR_BEGIN: phase_begin, KR_BEGIN2: phase_begin2, KR_UPDATE_S: phase_update_s, KR_UPDATE_XR: phase_update_xr,
          KR_UPDATE_P: phase_update_p, KR_TRUE_RESIDUAL: phase_true_residual, KR_RESTART: phase_restart}


def finish(y, perm, dof, cscale, nfull):
    """phx_krylov_finish (k_scatter_solution): x_full[dof[perm[i]]] = C_i y_i, zero elsewhere; `cscale` the column
    scaling of the stored values in solver order."""
    x = np.zeros(nfull, dtype=np.result_type(y, cscale))
    x[np.asarray(dof)[np.asarray(perm)]] = y * cscale
    return x


class Iterates:
    """x_1 .. x_k, |r_j|_2 (the recursive residual of iteration j), whether iteration j ended in a restart, and, when
    asked for, the vectors r, s, p after every iteration."""

    def __init__(self):
        self.x, self.rnorm, self.restart, self.vectors = [], [], [], []


def bicgstab(A, b, minv, x0=None, k=1, keep=False):
    """Right-preconditioned BiCGStab as `kr_drive` runs it, k iterations without convergence logic.  `minv(p)` is the
    whole M^-1 in x-space (the column scaling of the device's stored values times its preconditioner), so the
    device's y and this x are related by x = C y.  From x0 (None: 0): r = rhat = p = b - A x0, rho = (r, r)."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b.copy() if x0 is None else b - A @ x
    rhat, p = r.copy(), r.copy()
    S = np.zeros(HEAD)
    S[S_RHO] = S[S_RHO_NEXT] = S[S_RR] = r @ r
    S[S_ALPHA] = S[S_OMEGA] = 1.0
    out = Iterates()
    for _ in range(k):
        with np.errstate(all="ignore"):
            phat = minv(p)
            v = A @ phat
            rho = S[S_RHO_NEXT]
            alpha = rho / (rhat @ v)
            S[S_ALPHA], S[S_RHO] = alpha, rho
            s = r - alpha * v
            shat = minv(s)
            t = A @ shat
            omega = (t @ s) / (t @ t)
            S[S_OMEGA] = omega
            x = x + (alpha * phat + omega * shat)
            r = s - omega * t
            rho_new, rr = rhat @ r, r @ r
            restart, beta = kr_restart(S, rho_new, rr)
            S[S_RHO_NEXT] = rr if restart else rho_new
            S[S_RR] = rr
            if restart:
                S[S_RESTARTS] += 1.0
                p, rhat = r.copy(), r.copy()
            else:
                p = r + beta * (p - omega * v)
        out.x.append(x.copy())
        out.rnorm.append(float(np.sqrt(rr)))
        out.restart.append(restart)
        if keep:
            out.vectors.append(dict(r=r.copy(), s=s.copy(), p=p.copy(), v=v.copy(), t=t.copy(), rhat=rhat.copy()))
    return out


def reduced_start(A, b, minv, C):
    """x0 = M^-1 E_C b_C of the reduced loop (KR_BEGIN2 with kr_reduced): u0 = b on the rows C, 0 elsewhere.  Where A M^-1
    is the identity on C the residual b - A x0 vanishes there, and with it every later Krylov vector."""
    u0 = np.zeros_like(np.asarray(b, dtype=np.float64))
    u0[C] = np.asarray(b)[C]
    return minv(u0)
