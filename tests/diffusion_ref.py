"""numpy specification of the variable-coefficient diffusion scheme (`phifem_amd.DiffusionSolver`,
`phifem_amd.HeatSolver(kappa=...)`, `phx_assemble_diffusion_wd`, `phx_system_update_rhs`); test infrastructure only, no
GPU use.

    c u - div(kappa grad u) = f + c g  on Omega_h,  u = u_D on {phi = 0},  kappa_h nodal P1 > 0, c >= 0 constant,
    (u, p) in P1 x P1, F = f + c g, kb_T / kb_F the mean of kappa_h over the vertices of a cell / facet:

    a((u,p),(v,q)) = (kappa grad u, grad v)_{dx(1,2)} + c (u, v)_{dx(1,2)} - (kappa d_n u, v)_{ds(100)}
                   + pen kb_T h_T^-2 (u - phi p / h_T, v - phi q / h_T)_{dx(2)}
                   + stab h_T^2 / kb_T (c u - grad kappa . grad u, c v - grad kappa . grad v)_{dx(2)}
                   + stab avg(h) (kappa [d_n u], [d_n v])_{dS(2,3)}
    L(v,q)         = (F, v)_{dx(1,2)} + pen kb_T h_T^-2 (u_D, v - phi q / h_T)_{dx(2)}
                   + stab h_T^2 / kb_T (F, c v - grad kappa . grad v)_{dx(2)}

Every integrand is a polynomial on an affine simplex; the closed forms are the functions `*_closed` below, and
`*_quadrature` integrates the same products with the collapsed Gauss-Legendre rule of tests/estimate_ref.py as a check.
Geometry and barycentric tensors are `oracle.assembly.simplex_geometry` / `_bary_tensor`.  Layout (u_v -> v, p_v ->
nv + v), active set and structural pattern are those of `oracle.assembly.assemble_poisson_wd`.  `diffusion_steps` is
the direct-solve time stepper (backward Euler and BDF2, as `heat_ref.heat_steps`) with a conductivity."""
import numpy as np
import scipy.sparse as sp

from oracle import assembly as OA
from oracle.points import FACET_VERTS


# ---- the kappa-weighted element terms, closed form and quadrature -------------------------------------------------------
def kappa_slopes(g, kc):
    """s[c][j] = grad kappa . grad N_j with grad kappa = sum_k kappa_k grad N_k (constant per cell)."""
    gk = np.einsum("ck,ckd->cd", kc, g)
    return np.einsum("cd,cjd->cj", gk, g)


def stiffness_closed(g, vol, kc):
    """(kappa grad N_j, grad N_i)_T = kb_T |T| grad N_i . grad N_j."""
    return (kc.mean(axis=1) * vol)[:, None, None] * np.einsum("cid,cjd->cij", g, g)


def stiffness_quadrature(g, vol, kc):
    import estimate_ref as E
    lam, w = E.simplex_rule(g.shape[2])
    kq = kc @ lam.T                                               # kappa at the points (nc, nq)
    return (vol * (kq @ w))[:, None, None] * np.einsum("cid,cjd->cij", g, g)


def residual_closed(g, vol, kc, c, Fc):
    """Without the factor stab h^2 / kb: the block (c N_j - s_j, c N_i - s_i)_T = |T| (c^2 M2 - c (s_i + s_j) / (d+1)
    + s_i s_j) and the vector (F, c N_i - s_i)_T = |T| (c sum_j M2[i,j] F_j - s_i mean F)."""
    d = g.shape[2]
    M2 = OA._bary_tensor(d, 2)
    s = kappa_slopes(g, kc)
    B = c * c * M2[None] - c * (s[:, :, None] + s[:, None, :]) / (d + 1) + s[:, :, None] * s[:, None, :]
    r = c * (Fc @ M2.T) - s * Fc.mean(axis=1)[:, None]
    return vol[:, None, None] * B, vol[:, None] * r


def residual_quadrature(g, vol, kc, c, Fc):
    import estimate_ref as E
    lam, w = E.simplex_rule(g.shape[2])
    s = kappa_slopes(g, kc)
    R = c * lam[None, :, :] - s[:, None, :]                       # (c N_i - s_i) at the points (nc, nq, n)
    B = np.einsum("q,cqi,cqj->cij", w, R, R)
    r = np.einsum("q,cq,cqi->ci", w, Fc @ lam.T, R)
    return vol[:, None, None] * B, vol[:, None] * r


def facet_kappa_closed(d, area, kf):
    """(int_F kappa N_i for the d vertices of F, int_F kappa): |F| (sum_F kappa + kappa_i) / (d (d+1)), |F| kb_F."""
    return area[:, None] * (kf.sum(axis=1)[:, None] + kf) / (d * (d + 1)), area * kf.mean(axis=1)


def facet_kappa_quadrature(d, area, kf):
    import estimate_ref as E
    lam, w = E.simplex_rule(d - 1)
    kq = kf @ lam.T
    return area[:, None] * np.einsum("q,fq,qi->fi", w, kq, lam), area * (kq @ w)


# ---- the system ---------------------------------------------------------------------------------------------------------
def assemble_diffusion_wd(topo, x, cell_tags, facet_tags, ds100, kappa_h, phi_h, f_h, u_D, reaction, g_h=None,
                          pen_coef=1.0, stab_coef=1.0, quadrature=False):
    """(A csr (2nv x 2nv), b (2nv), active bool (2nv)) in the layout of `oracle.assembly.assemble_poisson_wd`;
    quadrature=True takes the kappa-weighted integrals from the Gauss-Legendre rules instead of the closed forms."""
    x = np.asarray(x, dtype=np.float64)
    cells = topo.cells
    nv = topo.nv
    d = x.shape[1]
    n = d + 1
    c = float(reaction)
    kap = np.asarray(kappa_h, dtype=np.float64)
    phi_h, u_D = np.asarray(phi_h, dtype=np.float64), np.asarray(u_D, dtype=np.float64)
    F = np.asarray(f_h, dtype=np.float64) + (0.0 if g_h is None else c * np.asarray(g_h, dtype=np.float64))
    stiff = stiffness_quadrature if quadrature else stiffness_closed
    resid = residual_quadrature if quadrature else residual_closed
    fkap = facet_kappa_quadrature if quadrature else facet_kappa_closed
    g, vol, h = OA.simplex_geometry(x, cells)
    M2, M3, M4 = OA._bary_tensor(d, 2), OA._bary_tensor(d, 3), OA._bary_tensor(d, 4)
    fv = np.asarray(FACET_VERTS["triangle" if d == 2 else "tetrahedron"])      # local facet -> its local vertices
    rows, cols, vals = [], [], []
    b = np.zeros(2 * nv)

    def add(r, cc_, v):
        rows.append(np.broadcast_to(r, v.shape).reshape(-1))
        cols.append(np.broadcast_to(cc_, v.shape).reshape(-1))
        vals.append(v.reshape(-1))

    # (kappa grad u, grad v) + c (u, v) over dx(1,2); (F, v) over dx(1,2)
    om = np.flatnonzero((cell_tags == 1) | (cell_tags == 2))
    cv = cells[om]
    add(cv[:, :, None], cv[:, None, :], stiff(g[om], vol[om], kap[cv]) + c * vol[om, None, None] * M2[None])
    np.add.at(b, cv, vol[om, None] * (F[cv] @ M2.T))

    # -(kappa d_n u, v) over ds(100): n = -g_lf / |g_lf|, |F| = d |T| |g_lf|, so the entry of row i on F, column j is
    # (g_j . g_lf) / |g_lf| int_F kappa N_i
    ents = np.asarray(ds100, dtype=np.int64).reshape(-1, 2)
    if ents.size:
        ce, lf = ents[:, 0], ents[:, 1]
        gn = np.sqrt((g[ce, lf] ** 2).sum(axis=1))
        on = fv[lf]                                                # (ne, d) local vertices of the facet
        kN, _ = fkap(d, d * vol[ce] * gn, kap[cells[ce[:, None], on]])
        coef = np.einsum("cjd,cd->cj", g[ce], g[ce, lf]) / gn[:, None]
        for k in range(d):
            add(cells[ce, on[:, k]][:, None], cells[ce], kN[:, k][:, None] * coef)

    # penalisation on cut cells, weighted by kb_T; residual stabilisation on cut cells
    cut = np.flatnonzero(cell_tags == 2)
    cc = cells[cut]
    hc, vc = h[cut], vol[cut]
    kb = kap[cc].mean(axis=1)
    ph = phi_h[cc]
    gam = pen_coef * kb
    uu = (gam * hc ** -2 * vc)[:, None, None] * M2[None]
    up = -(gam * hc ** -3 * vc)[:, None, None] * np.einsum("ijk,ck->cij", M3, ph)
    pp = (gam * hc ** -4 * vc)[:, None, None] * np.einsum("ijkl,ck,cl->cij", M4, ph, ph)
    B, r = resid(g[cut], vc, kap[cc], c, F[cc])
    ws = stab_coef * hc ** 2 / kb
    add(cc[:, :, None], cc[:, None, :], uu + ws[:, None, None] * B)
    add(cc[:, :, None], nv + cc[:, None, :], up)
    add(nv + cc[:, :, None], cc[:, None, :], up)
    add(nv + cc[:, :, None], nv + cc[:, None, :], pp)
    ud = u_D[cc]
    np.add.at(b, cc, (gam * hc ** -2 * vc)[:, None] * (ud @ M2.T) + ws[:, None] * r)
    np.add.at(b, nv + cc, -(gam * hc ** -3 * vc)[:, None] * np.einsum("ijk,cj,ck->ci", M3, ud, ph))

    # ghost penalty stab avg(h) (kappa [d_n u], [d_n v]) over dS(2,3): kappa_h is continuous across F
    fs = np.flatnonzero(((facet_tags == 2) | (facet_tags == 3)) & (topo.f2c[:, 1] >= 0))
    if fs.size:
        cp, cm = topo.f2c[fs, 0], topo.f2c[fs, 1]
        lfp = np.argmax(topo.c2f[cp] == fs[:, None], axis=1)
        lfm = np.argmax(topo.c2f[cm] == fs[:, None], axis=1)
        gnp = np.sqrt((g[cp, lfp] ** 2).sum(axis=1))
        gnm = np.sqrt((g[cm, lfm] ** 2).sum(axis=1))
        Jp = np.einsum("cjd,cd->cj", g[cp], -g[cp, lfp] / gnp[:, None])
        Jm = np.einsum("cjd,cd->cj", g[cm], -g[cm, lfm] / gnm[:, None])
        Jall = np.concatenate([Jp, Jm], axis=1)
        dofs = np.concatenate([cells[cp], cells[cm]], axis=1)
        _, kint = fkap(d, d * vol[cp] * gnp, kap[cells[cp[:, None], fv[lfp]]])
        w = stab_coef * 0.5 * (h[cp] + h[cm]) * kint
        add(dofs[:, :, None], dofs[:, None, :], w[:, None, None] * Jall[:, :, None] * Jall[:, None, :])

    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * nv, 2 * nv)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    active = np.zeros(2 * nv, dtype=bool)
    active[cv.reshape(-1)] = True
    active[nv + cc.reshape(-1)] = True
    return A, b, active


def diffusion_steps(topo, x, cell_tags, facet_tags, ds100, kappa_h, phi_h, dt, scheme, u0, f_of_t, uD_of_t, nsteps,
                    t0=0.0, pen_coef=1.0, stab_coef=1.0):
    """Direct-solve time stepper of du/dt - div(kappa grad u) = f: the mixed solutions w^1 .. w^nsteps."""
    nv = topo.nv
    u, uprev, t, out = np.asarray(u0, dtype=np.float64), None, float(t0), []
    for _ in range(nsteps):
        if scheme == "bdf2" and uprev is not None:
            c, gg = 1.5 / dt, (4.0 * u - uprev) / 3.0
        else:
            c, gg = 1.0 / dt, u
        t += dt
        A, b, act = assemble_diffusion_wd(topo, x, cell_tags, facet_tags, ds100, kappa_h, phi_h, f_of_t(t), uD_of_t(t),
                                          c, gg, pen_coef=pen_coef, stab_coef=stab_coef)
        w = OA.solve_direct(A, b, act)
        uprev, u = u, w[:nv]
        out.append(w)
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------
def smooth_kappa(x, contrast=10.0):
    """exp(ln(contrast) / 2 sin 2x cos 1.5y): max / min -> contrast on a domain that holds the extrema."""
    return np.exp(0.5 * np.log(contrast) * np.sin(2.0 * x[:, 0]) * np.cos(1.5 * x[:, 1]))


def manufactured(x, reaction, contrast=10.0):
    """(kappa, u, f) at the points x: kappa = smooth_kappa, u = 0.5 + prod_a sin(w_a x_a + s_a) and
    f = c u - kappa Lap u - grad kappa . grad u."""
    d = x.shape[1]
    a = 0.5 * np.log(contrast)
    wv, sv = np.array([1.3, 0.9, 0.7])[:d], np.array([0.4, 1.2, 0.9])[:d]
    S, Cc = np.sin(x * wv + sv), np.cos(x * wv + sv)
    u = 0.5 + S.prod(axis=1)
    grad = np.stack([wv[k] * Cc[:, k] * np.delete(S, k, axis=1).prod(axis=1) for k in range(d)], axis=1)
    lap = -(wv ** 2).sum() * S.prod(axis=1)
    kap = smooth_kappa(x, contrast)
    gk = np.zeros_like(x)
    gk[:, 0] = a * kap * 2.0 * np.cos(2.0 * x[:, 0]) * np.cos(1.5 * x[:, 1])
    gk[:, 1] = -a * kap * 1.5 * np.sin(2.0 * x[:, 0]) * np.sin(1.5 * x[:, 1])
    return kap, u, reaction * u - kap * lap - (gk * grad).sum(axis=1)
