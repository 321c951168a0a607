"""Interface elasticity on QUADRILATERALS (test infrastructure): a numpy restatement of the 5-field mixed
phi-FEM of demo/interface-elasticity/main.py:179-235 (bilinear), :255-269 (linear) and the Dirichlet rows of
u_in :158-177,237-239,271-277 in Q1^2 x Q1^2 x Q1^{2x2} x Q1^{2x2} x Q1^2 with a Q1 nodal level-set, on
axis-parallel rectangles in tensor-product vertex order (v0 (0,0), v1 (1,0), v2 (0,1), v3 (1,1); basix facets
f0 (v0,v1), f1 (v0,v2), f2 (v1,v3), f3 (v2,v3)); h_T = the diagonal.  f_h and u_D are Q1 nodal vector fields.

Dense element matrices are built from the forms themselves (values, sigma, eps, div of each local function at
every quadrature point) with a tensor Gauss rule of `nq` points per direction on the cells and `nqf` points on the
facets; the interior-facet points of the second cell are located from the physical coordinates.  The DoF layout
and the Dirichlet treatment are those of oracle/elasticity.py: component-major blocks of nv entries.
"""
import numpy as np
import scipy.sparse as sp

from oracle.assembly_flux_quad import FACET_FIXED_Q, FACET_NORMAL_Q, gauss01, q1_tab, rect_geometry
from oracle.elasticity import Blocks, lame

NLOC = 56   # 14 blocks x 4 vertices; local function k = block * 4 + vertex


def _features(hx, hy, xi, eta):
    """Per cell (c) and point (q): for each of the 56 local functions its displacement value on each side
    U (c,q,56,2,2) [side, comp], its y tensor on each side Y (c,q,56,2,2,2), its p value P (c,q,56,2), and the
    physical gradients of the 4 vertex functions dN (c,q,4,2)."""
    N, dNr = q1_tab(xi, eta)
    nc, nq = hx.size, xi.size
    dN = dNr[None] / np.stack([hx, hy], axis=1)[:, None, None, :]
    B = Blocks(2)
    U = np.zeros((nc, nq, NLOC, 2, 2))
    Y = np.zeros((nc, nq, NLOC, 2, 2, 2))
    P = np.zeros((nc, nq, NLOC, 2))
    G = np.zeros((nc, nq, NLOC, 2, 2, 2))   # grad of the displacement [side, comp, dir]
    DY = np.zeros((nc, nq, NLOC, 2, 2))     # div of y [side, comp]
    for i in range(4):
        for s in range(2):
            for a in range(2):
                k = B.u(s, a) * 4 + i
                U[:, :, k, s, a] = N[None, :, i]
                G[:, :, k, s, a, :] = dN[:, :, i, :]
                for b in range(2):
                    k = B.y(s, a, b) * 4 + i
                    Y[:, :, k, s, a, b] = N[None, :, i]
                    DY[:, :, k, s, a] = dN[:, :, i, b]
        for a in range(2):
            P[:, :, (B.p + a) * 4 + i, a] = N[None, :, i]
    return N, dN, U, Y, P, G, DY


def _sigma(G, lam, mu):
    """sigma of displacement gradients G (..., 2, 2) [comp, dir]."""
    eps = 0.5 * (G + np.swapaxes(G, -1, -2))
    return lam * np.trace(eps, axis1=-2, axis2=-1)[..., None, None] * np.eye(2) + 2.0 * mu * eps


def assemble_elasticity_quad(topo, x, cell_tags, facet_tags, ds100, ds101, phi_h, f_h, uD, bc_vertices,
                             E_in=1.0, nu_in=0.3, E_out=1.0e-3, nu_out=0.3, pen_coef=1.0, stab_coef=1.0,
                             nq=3, nqf=2):
    """phi_h: (nv,) Q1 nodal; f_h, uD: (nv, 2) Q1 nodal; returns (A csr, b, active) over 14 nv DoFs."""
    x = np.asarray(x, dtype=np.float64)
    cells = topo.cells
    nv = topo.nv
    B = Blocks(2)
    ndof = B.C * nv
    o, hx, hy = rect_geometry(x, cells)
    hT = np.sqrt(hx ** 2 + hy ** 2)
    lam = [lame(E_in, nu_in)[0], lame(E_out, nu_out)[0]]
    mu = [lame(E_in, nu_in)[1], lame(E_out, nu_out)[1]]
    coef_in = (E_in / (E_in + E_out)) ** 2
    coef_out = (E_out / (E_in + E_out)) ** 2
    W = (coef_out, coef_in)     # main.py:191-192: the "in" term carries coef_out
    rows, cols, vals = [], [], []
    b = np.zeros(ndof)
    gdof = lambda cs: (np.arange(14)[None, :, None] * nv + cells[cs][:, None, :]).reshape(len(cs), NLOC)  # noqa: E731

    def add(rd, cd, E):
        rows.append(np.broadcast_to(rd[:, :, None], E.shape).reshape(-1))
        cols.append(np.broadcast_to(cd[:, None, :], E.shape).reshape(-1))
        vals.append(E.reshape(-1))

    g1, w1 = gauss01(nq)
    xi, eta = (a.reshape(-1) for a in np.meshgrid(g1, g1, indexing="ij"))
    wq = (w1[:, None] * w1[None, :]).reshape(-1)

    # ---- cells: stiffness on dx((1,2)) / dx((2,3)), source; cut cells dx(2)
    for kind in ("bulk", "cut"):
        sel = np.flatnonzero(np.isin(cell_tags, (1, 2, 3)) if kind == "bulk" else cell_tags == 2)
        if sel.size == 0:
            continue
        N, dN, U, Y, P, G, DY = _features(hx[sel], hy[sel], xi, eta)
        wd = wq[None, :] * (hx[sel] * hy[sel])[:, None]                        # (c, q)
        cd = gdof(sel)
        fq = np.einsum("qi,cia->cqa", N, f_h[cells[sel]])
        E = np.zeros((sel.size, NLOC, NLOC))
        if kind == "bulk":
            for s, tags in ((0, (1, 2)), (1, (2, 3))):
                on = np.isin(cell_tags[sel], tags).astype(float)
                S = _sigma(G[:, :, :, s], lam[s], mu[s])
                Eps = 0.5 * (G[:, :, :, s] + np.swapaxes(G[:, :, :, s], -1, -2))
                E += np.einsum("c,cq,cqjab,cqiab->cij", on, wd, S, Eps)
                r = np.einsum("c,cq,cqa,cqia->ci", on, wd, fq, U[:, :, :, s])
                np.add.at(b, cd, r)
        else:
            h = hT[sel]
            ph = np.einsum("qi,ci->cq", N, phi_h[cells[sel]])
            gph = np.einsum("cqid,ci->cqd", dN, phi_h[cells[sel]])
            for s in range(2):
                T1 = Y[:, :, :, s] + _sigma(G[:, :, :, s], lam[s], mu[s])          # y + sigma(u)
                E += pen_coef * W[s] * np.einsum("cq,cqiab,cqjab->cij", wd, T1, T1)
                E += stab_coef * np.einsum("c,cq,cqia,cqja->cij", h ** 2, wd, DY[:, :, :, s], DY[:, :, :, s])
                r = stab_coef * np.einsum("c,cq,cqa,cqia->ci", h ** 2, wd, fq, DY[:, :, :, s])
                np.add.at(b, cd, r)
            Yg = np.einsum("cqiab,cqb->cqia", Y[:, :, :, 0] - Y[:, :, :, 1], gph)
            E += pen_coef * np.einsum("c,cq,cqia,cqja->cij", h ** -2, wd, Yg, Yg)
            Pp = U[:, :, :, 0] - U[:, :, :, 1] + (h[:, None, None, None] ** -1) * ph[:, :, None, None] * P
            E += pen_coef * np.einsum("c,cq,cqia,cqja->cij", h ** -2, wd, Pp, Pp)
        add(cd, cd, E)

    # ---- one-sided boundary terms main.py:182-183: (y_s n, v_s) on d_bdry(100) / d_bdry(101)
    e1, ew = gauss01(nqf)
    for s, ents in ((0, ds100), (1, ds101)):
        ents = np.asarray(ents, dtype=np.int64).reshape(-1, 2)
        for lf in range(4):
            sel = ents[ents[:, 1] == lf, 0]
            if sel.size == 0:
                continue
            ax, val = FACET_FIXED_Q[lf]
            xe = np.full(nqf, val) if ax == 0 else e1
            ye = np.full(nqf, val) if ax == 1 else e1
            _, _, U, Y, _, _, _ = _features(hx[sel], hy[sel], xe, ye)
            length = hy[sel] if ax == 0 else hx[sel]
            Yn = np.einsum("cqiab,b->cqia", Y[:, :, :, s], FACET_NORMAL_Q[lf])
            E = np.einsum("q,c,cqia,cqja->cij", ew, length, U[:, :, :, s], Yn)
            cd = gdof(sel)
            add(cd, cd, E)

    # ---- facet stabilisation main.py:205-209 (dS(3), in) and :219-223 (dS(4), out)
    for s, ftag in ((0, 3), (1, 4)):
        fs = np.flatnonzero((facet_tags == ftag) & (topo.f2c[:, 1] >= 0))
        if fs.size == 0:
            continue
        cp, cm = topo.f2c[fs, 0], topo.f2c[fs, 1]
        J = np.zeros((fs.size, nqf, 2 * NLOC, 2))
        length = np.zeros(fs.size)
        pts = np.zeros((fs.size, nqf, 2))
        for side, cs in enumerate((cp, cm)):
            lfs = np.argmax(topo.c2f[cs] == fs[:, None], axis=1)
            for lf in range(4):
                m = np.flatnonzero(lfs == lf)
                if m.size == 0:
                    continue
                c_ = cs[m]
                ax, val = FACET_FIXED_Q[lf]
                if side == 0:
                    xe = np.full((m.size, nqf), val) if ax == 0 else np.broadcast_to(e1, (m.size, nqf))
                    ye = np.full((m.size, nqf), val) if ax == 1 else np.broadcast_to(e1, (m.size, nqf))
                    pts[m] = o[c_][:, None, :] + np.stack([xe * hx[c_][:, None], ye * hy[c_][:, None]], axis=2)
                    length[m] = hy[c_] if ax == 0 else hx[c_]
                # reference coordinates of the (physical) facet points in this cell
                xr = (pts[m] - o[c_][:, None, :]) / np.stack([hx[c_], hy[c_]], axis=1)[:, None, :]
                for q in range(nqf):
                    _, dNr = q1_tab(xr[:, q, 0], xr[:, q, 1])                     # one point per cell
                    dN = dNr / np.stack([hx[c_], hy[c_]], axis=1)[:, None, :]
                    Gq = np.zeros((m.size, NLOC, 2, 2))
                    for i in range(4):
                        for a in range(2):
                            Gq[:, B.u(s, a) * 4 + i, a, :] = dN[:, i, :]
                    J[m, q, side * NLOC:(side + 1) * NLOC] = np.einsum(
                        "ciab,b->cia", _sigma(Gq, lam[s], mu[s]), FACET_NORMAL_Q[lf])
        wgt = stab_coef * 0.5 * (hT[cp] + hT[cm]) * length
        E = np.einsum("q,c,cqia,cqja->cij", ew, wgt, J, J)
        dofs = np.concatenate([gdof(cp), gdof(cm)], axis=1)
        add(dofs, dofs, E)

    R, Cc, Vv = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    keepnz = Vv != 0.0
    R, Cc, Vv = R[keepnz], Cc[keepnz], Vv[keepnz]

    # ---- active set (oracle/elasticity.py)
    active = np.zeros(ndof, dtype=bool)
    v_in = np.unique(cells[np.isin(cell_tags, (1, 2))])
    v_out = np.unique(cells[np.isin(cell_tags, (2, 3))])
    v_cut = np.unique(cells[cell_tags == 2])
    for a in range(2):
        active[B.u(0, a) * nv + v_in] = True
        active[B.u(1, a) * nv + v_out] = True
        active[(B.p + a) * nv + v_cut] = True
        for bb in range(2):
            active[B.y(0, a, bb) * nv + v_cut] = True
            active[B.y(1, a, bb) * nv + v_cut] = True

    # ---- Dirichlet condition on u_in: unit rows, lifting, bc.set
    bc_vertices = np.asarray(bc_vertices, dtype=np.int64)
    bc_dofs = np.concatenate([B.u(0, a) * nv + bc_vertices for a in range(2)])
    bc_vals = np.concatenate([uD[bc_vertices, a] for a in range(2)])
    is_bc = np.zeros(ndof, dtype=bool)
    is_bc[bc_dofs] = True
    ubc = np.zeros(ndof)
    ubc[bc_dofs] = bc_vals
    lift = is_bc[Cc] & ~is_bc[R]
    np.subtract.at(b, R[lift], Vv[lift] * ubc[Cc[lift]])
    keep = ~is_bc[R] & ~is_bc[Cc]
    A = sp.coo_matrix((np.concatenate([Vv[keep], np.ones(bc_dofs.size)]),
                       (np.concatenate([R[keep], bc_dofs]), np.concatenate([Cc[keep], bc_dofs]))),
                      shape=(ndof, ndof)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    b[bc_dofs] = bc_vals
    active[bc_dofs] = True
    return A, b, active
