"""Weak-Dirichlet phi-FEM Poisson on QUADRILATERALS (test infrastructure): a numpy restatement of the mixed (u, p)
formulation of demo/weak-dirichlet/flower/main.py:112-135 (bilinear) and :142-151 (linear) in Q1 x Q1 with Q1 nodal
phi_h, f_h, u_D, on axis-parallel rectangles in tensor-product vertex order (v0 (0,0), v1 (1,0), v2 (0,1), v3 (1,1);
basix facets f0 (v0,v1), f1 (v0,v2), f2 (v1,v3), f3 (v2,v3)); h_T = the diagonal (CellDiameter).

Written from the UFL form, not from the kernels: every term is integrated numerically from the values, gradients and
Laplacians of the local basis functions at tensor Gauss points -- `nq` points per direction on the cells, `nqf` on
the facets, by default of a deliberately higher order (5 x 5, 4) than the minimal exact rules (3 x 3, 2); the
interior-facet points of the second cell are located from the physical coordinates.  COO assembly, duplicates summed.

DoF layout (shared with the HIP library): u at vertex v -> v, p at vertex v -> nv + v.  Active: u on the vertices of
cells tagged 1 or 2, p on the vertices of cells tagged 2.
"""
import numpy as np
import scipy.sparse as sp

FACET_VERTS = np.array([[0, 1], [0, 2], [1, 3], [2, 3]])
# outward normal of local facet lf, and (reference axis that is fixed on it, its value)
FACET_NORMAL = np.array([[0.0, -1.0], [-1.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
FACET_FIXED = [(1, 0.0), (0, 0.0), (0, 1.0), (1, 1.0)]


def gauss01(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def _lin(t):
    """1-D linear basis on [0, 1]: values, first and second derivatives, (npts, 2) each."""
    t = np.asarray(t, dtype=np.float64)
    return np.stack([1.0 - t, t], axis=-1), np.stack([-np.ones_like(t), np.ones_like(t)], axis=-1), \
        np.zeros(t.shape + (2,))


def q1_basis(xi, eta):
    """Bilinear basis at reference points: N (..., 4), reference gradient (..., 4, 2), reference second derivatives
    d2/dxi2 and d2/deta2 (..., 4, 2); vertex i = ix + 2 iy."""
    Lx, dLx, d2Lx = _lin(xi)
    Ly, dLy, d2Ly = _lin(eta)
    ix, iy = np.array([0, 1, 0, 1]), np.array([0, 0, 1, 1])
    N = Lx[..., ix] * Ly[..., iy]
    dN = np.stack([dLx[..., ix] * Ly[..., iy], Lx[..., ix] * dLy[..., iy]], axis=-1)
    d2N = np.stack([d2Lx[..., ix] * Ly[..., iy], Lx[..., ix] * d2Ly[..., iy]], axis=-1)
    return N, dN, d2N


def rect_geometry(x, cells):
    """origin, hx, hy of axis-parallel rectangles in tensor-product order; raises if a cell is not one."""
    X = x[cells]
    o = X[:, 0]
    hx = X[:, 1, 0] - o[:, 0]
    hy = X[:, 2, 1] - o[:, 1]
    ok = (hx > 0) & (hy > 0) & (np.abs(X[:, 1, 1] - o[:, 1]) <= 1e-12 * np.abs(hx)) \
        & (np.abs(X[:, 2, 0] - o[:, 0]) <= 1e-12 * np.abs(hy)) \
        & (np.abs(X[:, 3, 0] - X[:, 1, 0]) <= 1e-12 * np.abs(hx)) & (np.abs(X[:, 3, 1] - X[:, 2, 1]) <= 1e-12 * np.abs(hy))
    if not ok.all():
        raise NotImplementedError("quadrilateral assembly covers axis-parallel rectangles in tensor-product vertex order")
    return o, hx, hy


def assemble(cells, x, c2f, f2c, cell_tags, facet_tags, ds, phi, f, uD, gamma=1.0, sigma=1.0, nq=5, nqf=4,
             with_laplacian=False):
    """cells (nc, 4), x (nv, 2), c2f (nc, 4), f2c (nf, 2; -1: none), dense cell_tags (nc) / facet_tags (nf),
    ds: flat or (n, 2) [cell, local facet] entities of the one-sided boundary term (ds(100) in box mode, every
    exterior facet on a sub-mesh), phi / f / uD: Q1 nodal (nv,).  Returns (A csr (2 nv x 2 nv), b (2 nv), act bool).
    with_laplacian: also integrate sigma h^2 lap(u) lap(v) and -sigma h^2 f_h lap(v) on dx(2) (main.py:123-128,150)."""
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    c2f, f2c = np.asarray(c2f, dtype=np.int64), np.asarray(f2c, dtype=np.int64)
    cell_tags, facet_tags = np.asarray(cell_tags), np.asarray(facet_tags)
    nv = x.shape[0]
    o, hx, hy = rect_geometry(x, cells)
    hT = np.sqrt(hx ** 2 + hy ** 2)
    hxy = np.stack([hx, hy], axis=1)
    rows, cols, vals = [], [], []
    b = np.zeros(2 * nv)

    def add(rd, cd, E):
        rows.append(np.broadcast_to(rd[:, :, None], E.shape).reshape(-1))
        cols.append(np.broadcast_to(cd[:, None, :], E.shape).reshape(-1))
        vals.append(E.reshape(-1))

    g1, w1 = gauss01(nq)
    xi, eta = (a.reshape(-1) for a in np.meshgrid(g1, g1, indexing="ij"))
    wq = (w1[:, None] * w1[None, :]).reshape(-1)
    N, dNr, d2Nr = q1_basis(xi, eta)                                          # (q, 4), (q, 4, 2), (q, 4, 2)

    # ---- main.py:113 inner(grad u, grad v) dx((1,2)); main.py:143 inner(f_h, v) dx((1,2))
    om = np.flatnonzero((cell_tags == 1) | (cell_tags == 2))
    cv = cells[om]
    wd = wq[None, :] * (hx[om] * hy[om])[:, None]                             # (c, q)
    dN = dNr[None] / hxy[om][:, None, None, :]                                # (c, q, 4, 2)
    add(cv, cv, np.einsum("cq,cqid,cqjd->cij", wd, dN, dN))
    fq = np.einsum("qi,ci->cq", N, f[cv])
    np.add.at(b, cv, np.einsum("cq,cq,qi->ci", wd, fq, N))

    # ---- main.py:115-122 penalisation on dx(2), its right-hand side :144-149 (and the Laplacian terms :123-128,150)
    cut = np.flatnonzero(cell_tags == 2)
    cc = cells[cut]
    if cut.size:
        h = hT[cut]
        wd = wq[None, :] * (hx[cut] * hy[cut])[:, None]
        phq = np.einsum("qi,ci->cq", N, phi[cc])
        udq = np.einsum("qi,ci->cq", N, uD[cc])
        # B(u, p) = u - h^-1 phi_h p of the 8 local functions (u_0..3, p_0..3)
        Bf = np.concatenate([np.broadcast_to(N[None], (cut.size,) + N.shape),
                             -(phq / h[:, None])[:, :, None] * N[None]], axis=2)               # (c, q, 8)
        E = gamma * np.einsum("c,cq,cqa,cqb->cab", h ** -2, wd, Bf, Bf)
        r = gamma * np.einsum("c,cq,cq,cqa->ca", h ** -2, wd, udq, Bf)
        if with_laplacian:
            lap = (d2Nr[None] / (hxy[cut] ** 2)[:, None, None, :]).sum(axis=3)                 # (c, q, 4)
            Lf = np.concatenate([lap, np.zeros_like(lap)], axis=2)
            E = E + sigma * np.einsum("c,cq,cqa,cqb->cab", h ** 2, wd, Lf, Lf)
            fq = np.einsum("qi,ci->cq", N, f[cc])
            r = r - sigma * np.einsum("c,cq,cq,cqa->ca", h ** 2, wd, fq, Lf)
        cd = np.concatenate([cc, nv + cc], axis=1)
        add(cd, cd, E)
        np.add.at(b, cd, r)

    # ---- main.py:114  -inner(inner(grad u, n), v) ds
    e1, ew = gauss01(nqf)
    ents = np.asarray(ds, dtype=np.int64).reshape(-1, 2)
    for lf in range(4):
        sel = ents[ents[:, 1] == lf, 0]
        if sel.size == 0:
            continue
        ax, val = FACET_FIXED[lf]
        xe = np.full(nqf, val) if ax == 0 else e1
        ye = np.full(nqf, val) if ax == 1 else e1
        Nf, dNf, _ = q1_basis(xe, ye)
        dn = np.einsum("cqjd,d->cqj", dNf[None] / hxy[sel][:, None, None, :], FACET_NORMAL[lf])
        length = hy[sel] if ax == 0 else hx[sel]
        add(cells[sel], cells[sel], -np.einsum("q,c,qi,cqj->cij", ew, length, Nf, dn))

    # ---- main.py:129-134  avg(h_T) inner(jump(grad u, n), jump(grad v, n)) dS((2,3))
    fs = np.flatnonzero(((facet_tags == 2) | (facet_tags == 3)) & (f2c[:, 1] >= 0))
    if fs.size:
        cp, cm = f2c[fs, 0], f2c[fs, 1]
        J = np.zeros((fs.size, nqf, 8))
        length = np.zeros(fs.size)
        pts = np.zeros((fs.size, nqf, 2))
        for side, cs in enumerate((cp, cm)):
            lfs = np.argmax(c2f[cs] == fs[:, None], axis=1)
            for lf in range(4):
                m = np.flatnonzero(lfs == lf)
                if m.size == 0:
                    continue
                c_ = cs[m]
                ax, val = FACET_FIXED[lf]
                if side == 0:
                    xe = np.full((m.size, nqf), val) if ax == 0 else np.broadcast_to(e1, (m.size, nqf))
                    ye = np.full((m.size, nqf), val) if ax == 1 else np.broadcast_to(e1, (m.size, nqf))
                    pts[m] = o[c_][:, None, :] + np.stack([xe * hx[c_][:, None], ye * hy[c_][:, None]], axis=2)
                    length[m] = hy[c_] if ax == 0 else hx[c_]
                xr = (pts[m] - o[c_][:, None, :]) / hxy[c_][:, None, :]          # the facet points in this cell
                _, dNf, _ = q1_basis(xr[:, :, 0], xr[:, :, 1])                   # (c, q, 4, 2)
                J[m, :, side * 4:(side + 1) * 4] = np.einsum("cqjd,d->cqj", dNf / hxy[c_][:, None, None, :],
                                                             FACET_NORMAL[lf])
        wgt = sigma * 0.5 * (hT[cp] + hT[cm]) * length
        dofs = np.concatenate([cells[cp], cells[cm]], axis=1)
        add(dofs, dofs, np.einsum("q,c,cqa,cqb->cab", ew, wgt, J, J))

    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(2 * nv, 2 * nv)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    act = np.zeros(2 * nv, dtype=bool)
    act[cv.reshape(-1)] = True
    act[nv + cc.reshape(-1)] = True
    return A, b, act


def solve_direct(A, b, act):
    """main.py:162-182 (MUMPS with null-pivot detection): the solve on the active DoFs, zero elsewhere."""
    import scipy.sparse.linalg as spla
    idx = np.flatnonzero(act)
    w = np.zeros_like(b)
    w[idx] = spla.spsolve(A[idx][:, idx].tocsc(), b[idx])
    return w
