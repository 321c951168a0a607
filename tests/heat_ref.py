"""numpy specification of the reaction / heat scheme (`phifem_amd.ReactionSolver`, `phifem_amd.HeatSolver`,
`phx_assemble_reaction_wd`, `phx_system_update_rhs`); test infrastructure only, no GPU use.

    c u - Lap u = f + c g  on Omega_h,  u = u_D on {phi = 0},  c >= 0 constant, (u, p) in P1 x P1:

    a((u,p),(v,q)) = a_Poisson((u,p),(v,q)) + c (u, v)_{dx(1,2)} + stab c^2 h_T^2 (u, v)_{dx(2)}
    L(v,q)         = L_Poisson(f + c g; u_D)(v,q) + stab c h_T^2 (f + c g, v)_{dx(2)}

The Poisson part IS `oracle.assembly.assemble_poisson_wd`, called with f + c g.  The two mass terms and the one
right-hand-side term are written out here on their own, from the consistent P1 mass matrix
(1 + delta_ij) |T| / ((d+1)(d+2)) -- `mass_quadrature` integrates the same products with the collapsed Gauss-Legendre
rule of tests/estimate_ref.py as a check of that closed form.  `heat_steps` is a direct-solve time stepper for backward
Euler (c = 1/dt, g = u^n) and BDF2 (c = 3/(2 dt), g = (4 u^n - u^{n-1}) / 3, first step by backward Euler)."""
import math

import numpy as np
import scipy.sparse as sp

from oracle import assembly as OA


def cell_volume_diameter(x, cells):
    xc = x[cells]
    d = x.shape[1]
    vol = np.abs(np.linalg.det(xc[:, 1:] - xc[:, :1])) / math.factorial(d)
    n = cells.shape[1]
    h = np.sqrt(np.max([((xc[:, i] - xc[:, j]) ** 2).sum(axis=1) for i in range(n) for j in range(i + 1, n)], axis=0))
    return vol, h


def p1_mass(d):
    """(1/|T|) int N_i N_j = (1 + delta_ij) / ((d+1)(d+2))."""
    return (np.ones((d + 1, d + 1)) + np.eye(d + 1)) / ((d + 1) * (d + 2))


def cell_weights(cell_tags, h, reaction, stab_coef):
    """Per cell: the factor in front of (u, v)_T in a, and the factor in front of (f + c g, v)_T that L adds to the
    Poisson source term.  Zero outside Omega_h."""
    cell_tags = np.asarray(cell_tags)
    om = (cell_tags == 1) | (cell_tags == 2)
    cut = cell_tags == 2
    wa = np.where(om, reaction, 0.0) + np.where(cut, stab_coef * reaction ** 2 * h ** 2, 0.0)
    wl = np.where(cut, stab_coef * reaction * h ** 2, 0.0)
    return wa, wl


def mass_terms(x, cells, cell_tags, reaction, stab_coef, F):
    """(M, l): the matrix c (u,v)_{dx(1,2)} + stab c^2 h^2 (u,v)_{dx(2)} on the u block (nv x nv) and the vector
    stab c h^2 (F, v)_{dx(2)} (nv), from the closed-form mass matrix."""
    x = np.asarray(x, dtype=np.float64)
    nv, d = x.shape
    vol, h = cell_volume_diameter(x, cells)
    wa, wl = cell_weights(cell_tags, h, reaction, stab_coef)
    M2 = p1_mass(d)
    Me = (wa * vol)[:, None, None] * M2[None]
    rows = np.broadcast_to(cells[:, :, None], Me.shape).reshape(-1)
    cols = np.broadcast_to(cells[:, None, :], Me.shape).reshape(-1)
    keep = np.broadcast_to((wa != 0.0)[:, None, None], Me.shape).reshape(-1)
    M = sp.coo_matrix((Me.reshape(-1)[keep], (rows[keep], cols[keep])), shape=(nv, nv)).tocsr()
    l = np.zeros(nv)
    np.add.at(l, cells, (wl * vol)[:, None] * (F[cells] @ M2.T))
    return M, l


def mass_quadrature(x, cells, cell_tags, reaction, stab_coef, F):
    """The same (M, l) with every product N_i N_j integrated by the Duffy Gauss-Legendre rule of tests/estimate_ref.py."""
    import estimate_ref as E
    x = np.asarray(x, dtype=np.float64)
    nv, d = x.shape
    lam, w = E.simplex_rule(d)                        # P1 basis at the points = the barycentric coordinates
    vol, h = cell_volume_diameter(x, cells)
    wa, wl = cell_weights(cell_tags, h, reaction, stab_coef)
    NN = np.einsum("q,qi,qj->ij", w, lam, lam)        # (1/|T|) int N_i N_j
    Me = (wa * vol)[:, None, None] * NN[None]
    rows = np.broadcast_to(cells[:, :, None], Me.shape).reshape(-1)
    cols = np.broadcast_to(cells[:, None, :], Me.shape).reshape(-1)
    M = sp.coo_matrix((Me.reshape(-1), (rows, cols)), shape=(nv, nv)).tocsr()
    Fq = F[cells] @ lam.T                             # (nc, nq)
    l = np.zeros(nv)
    np.add.at(l, cells, (wl * vol)[:, None] * np.einsum("q,cq,qi->ci", w, Fq, lam))
    return M, l


def assemble_reaction_wd(topo, x, cell_tags, facet_tags, ds100, phi_h, f_h, u_D, reaction, g_h=None,
                         pen_coef=1.0, stab_coef=1.0):
    """(A csr (2nv x 2nv), b (2nv), active bool (2nv)) in the layout of `oracle.assembly.assemble_poisson_wd`."""
    nv = topo.nv
    F = np.asarray(f_h, dtype=np.float64) + (0.0 if g_h is None else reaction * np.asarray(g_h, dtype=np.float64))
    A, b, act = OA.assemble_poisson_wd(topo, x, cell_tags, facet_tags, ds100, phi_h, F, u_D,
                                       pen_coef=pen_coef, stab_coef=stab_coef)
    M, l = mass_terms(x, topo.cells, cell_tags, reaction, stab_coef, F)
    # entries appended in COO form: the structural pattern of the oracle (explicit zeros included) is kept
    Ac, Mc = A.tocoo(), M.tocoo()
    A = sp.coo_matrix((np.concatenate([Ac.data, Mc.data]), (np.concatenate([Ac.row, Mc.row]), np.concatenate([Ac.col, Mc.col]))),
                      shape=(2 * nv, 2 * nv)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    b = b.copy()
    b[:nv] += l
    return A, b, act


def heat_steps(topo, x, cell_tags, facet_tags, ds100, phi_h, dt, scheme, u0, f_of_t, uD_of_t, nsteps, t0=0.0,
               pen_coef=1.0, stab_coef=1.0):
    """Direct-solve time stepper: the list of the mixed solutions w^1 .. w^nsteps (full numbering, inactive DoFs 0)."""
    nv = topo.nv
    u, uprev, t, out = np.asarray(u0, dtype=np.float64), None, float(t0), []
    for _ in range(nsteps):
        if scheme == "bdf2" and uprev is not None:
            c, g = 1.5 / dt, (4.0 * u - uprev) / 3.0
        else:
            c, g = 1.0 / dt, u
        t += dt
        A, b, act = assemble_reaction_wd(topo, x, cell_tags, facet_tags, ds100, phi_h, f_of_t(t), uD_of_t(t), c, g,
                                         pen_coef=pen_coef, stab_coef=stab_coef)
        w = OA.solve_direct(A, b, act)
        uprev, u = u, w[:nv]
        out.append(w)
    return out


def scalar_recurrence(gamma0, dgamma, dt, scheme, nsteps, t0=0.0):
    """gamma_1 .. gamma_nsteps of gamma' = dgamma(t) under the scheme (what the stepper does to data that is P1 in space)."""
    g, gprev, t, out = float(gamma0), None, float(t0), []
    for _ in range(nsteps):
        t += dt
        if scheme == "bdf2" and gprev is not None:
            new = (4.0 * g - gprev) / 3.0 + (2.0 * dt / 3.0) * dgamma(t)
        else:
            new = g + dt * dgamma(t)
        gprev, g = g, new
        out.append(new)
    return out
