"""Specification of the recovered gradient and of the recovery-based (Zienkiewicz-Zhu) indicator (TEST INFRASTRUCTURE,
pure numpy in float64): what phifem_amd/csrc/phx_recover.inc.hip has to agree with.  Nothing here is taken from the
kernels.

Inputs: a mesh, nodal values u_h of degree k with ncomp >= 1 components ((ndofs,) or (ncomp, ndofs), vertices first,
then at degree 2 the edges of `c2e`), and a set S of selected cells (a mask; `omega_mask` gives the cells tagged 1 or 2).

    G(v) = ( sum_{T in S_v} |T| grad u_h|_T (x_v) ) / ( sum_{T in S_v} |T| ),   S_v = the cells of S that contain v,
    G(v) = 0 exactly where S_v is empty;

|T| = |det J| / d! on simplices, hx hy on rectangles; grad u_h|_T (x_v) the gradient of T's own polynomial at its
corner v (P1: one constant per cell; P2: the P1 gradient field at the corner; Q1: the bilinear's gradient at the
corner).  G_h is the P1 / Q1 interpolant of the vertex values, per component and direction, and for T in S

    eta_T^2 = sum over the components c of int_T |G_h,c - grad u_h,c|^2,       0 for T not in S.

Both closed forms are exact.  Simplices: the integrand is P1 for k = 1 and k = 2; with d_i = G(v_i) - grad u_h|_T(x_v_i)
    int_T = |T| / ((d + 1)(d + 2)) ( sum_i d_i . d_i + (sum_i d_i) . (sum_i d_i) ).
Rectangles: the difference is bilinear, int_T = hx hy sum_ij d_i (M1 (x) M1)_ij d_j, M1 = [[1/3, 1/6], [1/6, 1/3]].
`eta2_quadrature` integrates the same G_h - grad u_h with Gauss-Legendre rules instead (the independent rule).

Next to each number its SCALE: the same formula with every product of a nodal value and a basis gradient replaced by its
absolute value (direction by direction).  Round-off of any evaluation order is a small multiple of eps times the scale.

    recover_ref(ctype, x, cells, degree, u, mask, c2e=None) -> Recovered(G, G_scale, eta2, eta2_scale)
"""
import collections

import numpy as np

import estimate_ref as ER

Recovered = collections.namedtuple("Recovered", "G G_scale eta2 eta2_scale")
M1 = np.array([[1.0 / 3.0, 1.0 / 6.0], [1.0 / 6.0, 1.0 / 3.0]])


def omega_mask(tags):
    """The default S: the cells tagged 1 or 2 (tag & 0x7f, as estimate_ref reads them)."""
    t = np.asarray(tags) & 0x7f
    return ((t == 1) | (t == 2)).astype(np.uint8)


def check_space(ctype, degree):
    if ctype not in ("triangle", "tetrahedron", "quadrilateral"):
        raise NotImplementedError(ctype)
    if degree not in (1, 2) or (degree == 2 and ctype == "quadrilateral"):
        raise NotImplementedError("degree 1 on triangles, tetrahedra and rectangles, degree 2 on simplices")


def corner_basis_gradients(ctype, x, cells, degree):
    """(gN (nc, ncorner, nb, d): physical gradient of basis function b of the cell at its corner i, vol (nc,))."""
    if ctype == "quadrilateral":
        hx, hy, vol, _ = ER.rect_geometry(x, cells)
        xi = np.array([0.0, 1.0, 0.0, 1.0])
        eta = np.array([0.0, 0.0, 1.0, 1.0])
        _, dN = ER.q1_basis(xi, eta)                                   # (corner, b, 2) reference derivatives
        gN = dN[None] / np.stack([hx, hy], axis=1)[:, None, None, :]
        return gN, vol
    g, vol, _ = ER.simplex_geometry(x, cells)                          # g (nc, n, d)
    n = cells.shape[1]
    _, dN = ER.simplex_basis(ctype, degree, np.eye(n))                 # (corner, nb, n)
    return np.einsum("ibm,cmd->cibd", dN, g), vol


def corner_gradients(ctype, x, cells, degree, u, c2e=None):
    """(cg, cg_abs (nc, ncorner, ncomp, d), vol): gradient of each cell's own polynomial at its corners, and the same
    sums with |u_b| |grad N_b|."""
    check_space(ctype, degree)
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    dofs = ER.cell_dofs(ctype, cells, degree, x.shape[0], c2e)
    gN, vol = corner_basis_gradients(ctype, x, cells, degree)
    U = u[:, dofs]                                                     # (ncomp, nc, nb)
    cg = np.einsum("kcb,cibd->cikd", U, gN)
    cga = np.einsum("kcb,cibd->cikd", np.abs(U), np.abs(gN))
    return cg, cga, vol


def _vertex_average(nv, cells, sel, vol, cg):
    """sum_{T in S_v} |T| cg / sum |T| per vertex (0 where the star is empty), and the flag `has a star`."""
    num = np.zeros((nv,) + cg.shape[2:])
    den = np.zeros(nv)
    c = np.flatnonzero(sel)
    for i in range(cells.shape[1]):
        np.add.at(num, cells[c, i], vol[c, None, None] * cg[c, i])
        np.add.at(den, cells[c, i], vol[c])
    has = den > 0.0
    out = np.zeros_like(num)
    out[has] = num[has] / den[has, None, None]
    return out, has


def _closed_form(ctype, vol, dd):
    """int_T |D|^2 for the P1 / Q1 function D with corner values dd (nc, ncorner, ncomp, d), summed over components."""
    if ctype == "quadrilateral":
        MM = np.kron(M1, M1)                                           # corner i = 2 iy + ix: (M1 (x) M1)[i][j]
        return vol * np.einsum("cikd,ij,cjkd->c", dd, MM, dd)
    n = dd.shape[1]
    s = dd.sum(axis=1)
    return vol / (n * (n + 1)) * ((dd * dd).sum(axis=(1, 2, 3)) + (s * s).sum(axis=(1, 2)))


def recover_ref(ctype, x, cells, degree, u, mask, c2e=None):
    """Recovered(G, G_scale, eta2, eta2_scale): G of shape (nv, d) for u of shape (ndofs,), else (ncomp, nv, d)."""
    cells = np.asarray(cells, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    sel = np.asarray(mask).astype(bool)
    assert sel.shape == (cells.shape[0],)
    cg, cga, vol = corner_gradients(ctype, x, cells, degree, u, c2e)
    nv = x.shape[0]
    G, _ = _vertex_average(nv, cells, sel, vol, cg)                    # (nv, ncomp, d)
    Ga, _ = _vertex_average(nv, cells, sel, vol, cga)
    eta2 = np.where(sel, _closed_form(ctype, vol, G[cells] - cg), 0.0)
    eta2s = np.where(sel, _closed_form(ctype, vol, Ga[cells] + cga), 0.0)
    G, Ga = np.transpose(G, (1, 0, 2)), np.transpose(Ga, (1, 0, 2))
    if np.ndim(u) == 1:
        G, Ga = G[0], Ga[0]
    return Recovered(np.ascontiguousarray(G), np.ascontiguousarray(Ga), eta2, eta2s)


def star_lengths(nv, cells, mask):
    """(selected cells per vertex, all cells per vertex)."""
    cells = np.asarray(cells, dtype=np.int64)
    sel = np.asarray(mask).astype(bool)
    return np.bincount(cells[sel].reshape(-1), minlength=nv), np.bincount(cells.reshape(-1), minlength=nv)


def eta2_quadrature(ctype, x, cells, degree, u, mask, G, c2e=None, ngauss=4):
    """eta2 with Gauss-Legendre rules applied to G_h - grad u_h at the rule's points (G as recover_ref returns it): the
    rule is exact to degree 2 ngauss - 1 per variable, the integrand has degree 2 (+ 2 of the collapsed coordinates)."""
    check_space(ctype, degree)
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    sel = np.asarray(mask).astype(bool)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    G = np.asarray(G, dtype=np.float64)
    G = G[None] if G.ndim == 2 else G                                  # (ncomp, nv, d)
    dofs = ER.cell_dofs(ctype, cells, degree, x.shape[0], c2e)
    U = u[:, dofs]                                                     # (ncomp, nc, nb)
    Gc = G[:, cells]                                                   # (ncomp, nc, ncorner, d)
    if ctype == "quadrilateral":
        hx, hy, vol, _ = ER.rect_geometry(x, cells)
        t, w1 = ER.gauss01(ngauss)
        xi, eta = (a.reshape(-1) for a in np.meshgrid(t, t, indexing="ij"))
        w = np.outer(w1, w1).reshape(-1)
        N, dN = ER.q1_basis(xi, eta)                                   # (nq, 4), (nq, 4, 2)
        gu = np.einsum("kcb,qbd->kcqd", U, dN) / np.stack([hx, hy], axis=1)[None, :, None, :]
    else:
        g, vol, _ = ER.simplex_geometry(x, cells)
        lam, w = ER.simplex_rule(x.shape[1], ngauss)
        N = lam                                                        # the P1 basis
        _, dN = ER.simplex_basis(ctype, degree, lam)                   # (nq, nb, n)
        gu = np.einsum("kcb,qbm,cmd->kcqd", U, dN, g)
    Gh = np.einsum("qi,kcid->kcqd", N, Gc)
    diff = Gh - gu
    return np.where(sel, vol * np.einsum("q,kcqd->c", w, diff * diff), 0.0)
