"""numpy specification of the convection-diffusion scheme (`phifem_amd.ConvectionDiffusionSolver`,
`phifem_amd.HeatSolver(velocity=...)`, `phx_assemble_convection_wd`, `phx_system_update_rhs`); test infrastructure only,
no GPU use.

    c u + beta . grad u - div(kappa grad u) = f + c g  on Omega_h,  u = u_D on {phi = 0},
    kappa_h nodal P1 > 0, beta_h a nodal P1 vector field [nv][d], c >= 0 constant, (u, p) in P1 x P1, F = f + c g.

Per cell T with vertices k = 0..d and g_j = grad N_j: T_kj = beta_k . g_j (beta . grad N_j = sum_k lambda_k T_kj),
s_j = grad kappa . g_j, Q_kj = c delta_kj + T_kj - s_j (the strong operator applied to N_j is sum_k lambda_k Q_kj),
bb_T the mean of beta_k, ks_T = kb_T + h_T |bb_T| the effective diffusivity, ks_F = kb_F + avg(h) |bb_F|,
tau_T = h_T^2 / ks_T:

    a((u,p),(v,q)) = (kappa grad u, grad v)_{dx(1,2)} + c (u, v)_{dx(1,2)} + (beta . grad u, v)_{dx(1,2)}
                   - (kappa d_n u, v)_{ds(100)}
                   + supg tau_T (c u + beta . grad u - grad kappa . grad u, beta . grad v)_{dx(1,2)}
                   + pen ks_T h_T^-2 (u - phi p / h_T, v - phi q / h_T)_{dx(2)}
                   + stab tau_T (c u + beta . grad u - grad kappa . grad u, c v + beta . grad v - grad kappa . grad v)_{dx(2)}
                   + stab avg(h) |F| ks_F ([d_n u], [d_n v])_{dS(2,3)}
    L(v,q)         = (F, v)_{dx(1,2)} + supg tau_T (F, beta . grad v)_{dx(1,2)}
                   + pen ks_T h_T^-2 (u_D, v - phi q / h_T)_{dx(2)}
                   + stab tau_T (F, c v + beta . grad v - grad kappa . grad v)_{dx(2)}

The closed forms are |T| times products with M2 = (1 + delta) / ((d+1)(d+2)); `*_quadrature` integrates the same
products with the collapsed Gauss-Legendre rule of tests/estimate_ref.py from beta and grad kappa at the points.  The
kappa pieces (stiffness, boundary term, facet integrals) are those of tests/diffusion_ref.py; with beta = 0 the system is
`diffusion_ref.assemble_diffusion_wd`'s for any supg.  Layout, active set and pattern are those of
`oracle.assembly.assemble_poisson_wd`."""
import numpy as np
import scipy.sparse as sp

import diffusion_ref as D
from oracle import assembly as OA
from oracle.points import FACET_VERTS


# ---- element tables -----------------------------------------------------------------------------------------------------
def advection_table(g, bc):
    """T[c][k][j] = beta_k . grad N_j."""
    return np.einsum("ckd,cjd->ckj", bc, g)


def operator_table(g, kc, bc, c):
    """Q[c][k][j] = c delta_kj + T_kj - s_j."""
    n = g.shape[1]
    return c * np.eye(n)[None] + advection_table(g, bc) - D.kappa_slopes(g, kc)[:, None, :]


def _tables_at_points(g, kc, bc, c, lam):
    """(beta . grad N_j, c N_j + beta . grad N_j - grad kappa . grad N_j) at the points: (nc, nq, n) each."""
    bq = np.einsum("qk,ckd->cqd", lam, bc)
    Tq = np.einsum("cqd,cjd->cqj", bq, g)
    return Tq, c * lam[None, :, :] + Tq - D.kappa_slopes(g, kc)[:, None, :]


def effective_diffusivity(h, kc, bc):
    """ks_T = kb_T + h_T |bb_T|."""
    return kc.mean(axis=1) + h * np.sqrt((bc.mean(axis=1) ** 2).sum(axis=1))


# ---- the new element terms, closed form and quadrature (all without their coefficient) ----------------------------------
def advection_closed(g, vol, bc):
    """(beta . grad N_j, N_i)_T = |T| (M2 T)_ij = |T| (col_j(T) + T_ij) / ((d+1)(d+2))."""
    d = g.shape[2]
    T = advection_table(g, bc)
    return vol[:, None, None] * (T.sum(axis=1)[:, None, :] + T) / ((d + 1) * (d + 2))


def advection_quadrature(g, vol, bc):
    import estimate_ref as E
    lam, w = E.simplex_rule(g.shape[2])
    Tq = np.einsum("cqd,cjd->cqj", np.einsum("qk,ckd->cqd", lam, bc), g)      # beta . grad N_j at the points
    return vol[:, None, None] * np.einsum("q,qi,cqj->cij", w, lam, Tq)


def _product_closed(X, Y, Fc, vol, d):
    """|T| X^T M2 Y and |T| X^T M2 F in the col / sum form."""
    cx, cy = X.sum(axis=1), Y.sum(axis=1)
    B = cx[:, :, None] * cy[:, None, :] + np.einsum("cki,ckj->cij", X, Y)
    r = cx * Fc.sum(axis=1)[:, None] + np.einsum("cki,ck->ci", X, Fc)
    return vol[:, None, None] * B / ((d + 1) * (d + 2)), vol[:, None] * r / ((d + 1) * (d + 2))


def supg_closed(g, vol, kc, bc, c, Fc):
    """Block (L N_j, beta . grad N_i)_T = |T| (T^T M2 Q)_ij and vector (F, beta . grad N_i)_T = |T| (T^T M2 F)_i."""
    return _product_closed(advection_table(g, bc), operator_table(g, kc, bc, c), Fc, vol, g.shape[2])


def supg_quadrature(g, vol, kc, bc, c, Fc):
    import estimate_ref as E
    lam, w = E.simplex_rule(g.shape[2])
    Tq, Qq = _tables_at_points(g, kc, bc, c, lam)
    B = np.einsum("q,cqi,cqj->cij", w, Tq, Qq)
    r = np.einsum("q,cq,cqi->ci", w, Fc @ lam.T, Tq)
    return vol[:, None, None] * B, vol[:, None] * r


def residual_closed(g, vol, kc, bc, c, Fc):
    """Block (L N_j, L N_i)_T = |T| (Q^T M2 Q)_ij and vector (F, L N_i)_T = |T| (Q^T M2 F)_i; at beta = 0
    `diffusion_ref.residual_closed`."""
    Q = operator_table(g, kc, bc, c)
    return _product_closed(Q, Q, Fc, vol, g.shape[2])


def residual_quadrature(g, vol, kc, bc, c, Fc):
    import estimate_ref as E
    lam, w = E.simplex_rule(g.shape[2])
    _, Qq = _tables_at_points(g, kc, bc, c, lam)
    B = np.einsum("q,cqi,cqj->cij", w, Qq, Qq)
    r = np.einsum("q,cq,cqi->ci", w, Fc @ lam.T, Qq)
    return vol[:, None, None] * B, vol[:, None] * r


# ---- the system ---------------------------------------------------------------------------------------------------------
def assemble_convection_wd(topo, x, cell_tags, facet_tags, ds100, kappa_h, beta_h, phi_h, f_h, u_D, reaction, g_h=None,
                           pen_coef=1.0, stab_coef=1.0, supg_coef=0.0, quadrature=False):
    """(A csr (2nv x 2nv), b (2nv), active bool (2nv)) in the layout of `oracle.assembly.assemble_poisson_wd`;
    quadrature=True takes every integral from the Gauss-Legendre rules instead of the closed forms."""
    x = np.asarray(x, dtype=np.float64)
    cells = topo.cells
    nv = topo.nv
    d = x.shape[1]
    c = float(reaction)
    kap = np.asarray(kappa_h, dtype=np.float64)
    beta = np.asarray(beta_h, dtype=np.float64).reshape(nv, d)
    phi_h, u_D = np.asarray(phi_h, dtype=np.float64), np.asarray(u_D, dtype=np.float64)
    F = np.asarray(f_h, dtype=np.float64) + (0.0 if g_h is None else c * np.asarray(g_h, dtype=np.float64))
    stiff = D.stiffness_quadrature if quadrature else D.stiffness_closed
    adv = advection_quadrature if quadrature else advection_closed
    supg = supg_quadrature if quadrature else supg_closed
    resid = residual_quadrature if quadrature else residual_closed
    fkap = D.facet_kappa_quadrature if quadrature else D.facet_kappa_closed
    g, vol, h = OA.simplex_geometry(x, cells)
    M2, M3, M4 = OA._bary_tensor(d, 2), OA._bary_tensor(d, 3), OA._bary_tensor(d, 4)
    fv = np.asarray(FACET_VERTS["triangle" if d == 2 else "tetrahedron"])      # local facet -> its local vertices
    rows, cols, vals = [], [], []
    b = np.zeros(2 * nv)

    def add(r, cc_, v):
        rows.append(np.broadcast_to(r, v.shape).reshape(-1))
        cols.append(np.broadcast_to(cc_, v.shape).reshape(-1))
        vals.append(v.reshape(-1))

    # (kappa grad u, grad v) + c (u, v) + (beta . grad u, v) + supg tau (L u, beta . grad v) over dx(1,2);
    # (F, v) + supg tau (F, beta . grad v) over dx(1,2)
    om = np.flatnonzero((cell_tags == 1) | (cell_tags == 2))
    cv = cells[om]
    tau = h[om] ** 2 / effective_diffusivity(h[om], kap[cv], beta[cv])
    S, sv = supg(g[om], vol[om], kap[cv], beta[cv], c, F[cv])
    add(cv[:, :, None], cv[:, None, :], stiff(g[om], vol[om], kap[cv]) + c * vol[om, None, None] * M2[None]
        + adv(g[om], vol[om], beta[cv]) + (supg_coef * tau)[:, None, None] * S)
    np.add.at(b, cv, vol[om, None] * (F[cv] @ M2.T) + (supg_coef * tau)[:, None] * sv)

    # -(kappa d_n u, v) over ds(100), as in diffusion_ref: the advection term is not integrated by parts
    ents = np.asarray(ds100, dtype=np.int64).reshape(-1, 2)
    if ents.size:
        ce, lf = ents[:, 0], ents[:, 1]
        gn = np.sqrt((g[ce, lf] ** 2).sum(axis=1))
        on = fv[lf]
        kN, _ = fkap(d, d * vol[ce] * gn, kap[cells[ce[:, None], on]])
        coef = np.einsum("cjd,cd->cj", g[ce], g[ce, lf]) / gn[:, None]
        for k in range(d):
            add(cells[ce, on[:, k]][:, None], cells[ce], kN[:, k][:, None] * coef)

    # penalisation on cut cells, weighted by ks_T; residual stabilisation on cut cells with tau_T
    cut = np.flatnonzero(cell_tags == 2)
    cc = cells[cut]
    hc, vc = h[cut], vol[cut]
    ks = effective_diffusivity(hc, kap[cc], beta[cc])
    ph = phi_h[cc]
    gam = pen_coef * ks
    uu = (gam * hc ** -2 * vc)[:, None, None] * M2[None]
    up = -(gam * hc ** -3 * vc)[:, None, None] * np.einsum("ijk,ck->cij", M3, ph)
    pp = (gam * hc ** -4 * vc)[:, None, None] * np.einsum("ijkl,ck,cl->cij", M4, ph, ph)
    B, r = resid(g[cut], vc, kap[cc], beta[cc], c, F[cc])
    ws = stab_coef * hc ** 2 / ks
    add(cc[:, :, None], cc[:, None, :], uu + ws[:, None, None] * B)
    add(cc[:, :, None], nv + cc[:, None, :], up)
    add(nv + cc[:, :, None], cc[:, None, :], up)
    add(nv + cc[:, :, None], nv + cc[:, None, :], pp)
    ud = u_D[cc]
    np.add.at(b, cc, (gam * hc ** -2 * vc)[:, None] * (ud @ M2.T) + ws[:, None] * r)
    np.add.at(b, nv + cc, -(gam * hc ** -3 * vc)[:, None] * np.einsum("ijk,cj,ck->ci", M3, ud, ph))

    # ghost penalty stab avg(h) |F| ks_F ([d_n u], [d_n v]) over dS(2,3), ks_F = kb_F + avg(h) |bb_F|
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
        fverts = cells[cp[:, None], fv[lfp]]
        area = d * vol[cp] * gnp
        _, kint = fkap(d, area, kap[fverts])
        hav = 0.5 * (h[cp] + h[cm])
        bF = np.sqrt((beta[fverts].mean(axis=1) ** 2).sum(axis=1))
        w = stab_coef * hav * (kint + area * hav * bF)
        add(dofs[:, :, None], dofs[:, None, :], w[:, None, None] * Jall[:, :, None] * Jall[:, None, :])

    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * nv, 2 * nv)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    active = np.zeros(2 * nv, dtype=bool)
    active[cv.reshape(-1)] = True
    active[nv + cc.reshape(-1)] = True
    return A, b, active


def peclet_max(topo, x, cell_tags, kappa_h, beta_h):
    """max over the cells of Omega_h of h_T |bb_T| / kb_T."""
    _, _, h = OA.simplex_geometry(np.asarray(x, dtype=np.float64), topo.cells)
    om = np.flatnonzero((cell_tags == 1) | (cell_tags == 2))
    cv = topo.cells[om]
    bT = np.sqrt((np.asarray(beta_h)[cv].mean(axis=1) ** 2).sum(axis=1))
    return float((h[om] * bT / np.asarray(kappa_h)[cv].mean(axis=1)).max())


def convection_steps(topo, x, cell_tags, facet_tags, ds100, kappa_h, beta_h, phi_h, dt, scheme, u0, f_of_t, uD_of_t,
                     nsteps, t0=0.0, pen_coef=1.0, stab_coef=1.0, supg_coef=0.0):
    """Direct-solve time stepper of du/dt + beta . grad u - div(kappa grad u) = f (backward Euler and BDF2, as
    `diffusion_ref.diffusion_steps`): the mixed solutions w^1 .. w^nsteps."""
    nv = topo.nv
    u, uprev, t, out = np.asarray(u0, dtype=np.float64), None, float(t0), []
    for _ in range(nsteps):
        if scheme == "bdf2" and uprev is not None:
            c, gg = 1.5 / dt, (4.0 * u - uprev) / 3.0
        else:
            c, gg = 1.0 / dt, u
        t += dt
        A, b, act = assemble_convection_wd(topo, x, cell_tags, facet_tags, ds100, kappa_h, beta_h, phi_h, f_of_t(t),
                                           uD_of_t(t), c, gg, pen_coef=pen_coef, stab_coef=stab_coef, supg_coef=supg_coef)
        w = OA.solve_direct(A, b, act)
        uprev, u = u, w[:nv]
        out.append(w)
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------
def manufactured(x, reaction, kscale=1.0, bscale=1.0):
    """(kappa, beta, u, f) at the points x: kappa = kscale smooth_kappa(x, 10), u the u of `diffusion_ref.manufactured`,
    beta = bscale (1 - 0.8 y, 0.5 + 0.8 x [, 0]) and f = c u - div(kappa grad u) + beta . grad u."""
    d = x.shape[1]
    kap, u, f0 = D.manufactured(x, 0.0, 10.0)                      # f0 = -div(kappa grad u) at kscale = 1
    wv, sv = np.array([1.3, 0.9, 0.7])[:d], np.array([0.4, 1.2, 0.9])[:d]
    S, Cc = np.sin(x * wv + sv), np.cos(x * wv + sv)
    grad = np.stack([wv[k] * Cc[:, k] * np.delete(S, k, axis=1).prod(axis=1) for k in range(d)], axis=1)
    beta = np.zeros_like(x)
    beta[:, 0] = bscale * (1.0 - 0.8 * x[:, 1])
    beta[:, 1] = bscale * (0.5 + 0.8 * x[:, 0])
    return kscale * kap, beta, u, reaction * u + kscale * f0 + (beta * grad).sum(axis=1)
