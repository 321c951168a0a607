"""Weak-Dirichlet linear elasticity, mixed (u, p) in P1^d x P1^d on affine simplices: numpy specification of
`phx_assemble_elasticity_wd` (test infrastructure only; no GPU use).

The vector analogue of the weak-Dirichlet Poisson scheme (oracle/assembly.py; reference
demo/weak-dirichlet/flower/main.py:112-135 bilinear, :142-151 linear), with the material law of the interface demo
(demo/interface-elasticity/data.py:5-36): sigma(u) = lam tr eps(u) I + 2 mu eps(u), plane strain in 2-D.

  a((u,p),(v,q)) =  int_{dx(1,2)} sigma(u) : eps(v)
                  - int_{ds} (sigma(u) n) . v
                  + pen h_T^-2 int_{dx(2)} (u - h_T^-1 phi_h p) . (v - h_T^-1 phi_h q)
                  + stab avg(h_T) int_{dS(2,3)} [sigma(u) n] . [sigma(v) n]
  L(v,q)         =  int_{dx(1,2)} f_h . v  +  pen h_T^-2 int_{dx(2)} u_D . (v - h_T^-1 phi_h q)

ds: ds(100) in box mode, every exterior facet of a sub-mesh otherwise; h_T the cell diameter; n the outward normal of
the + cell.  The cell stabilisation stab h_T^2 (div sigma(u), div sigma(v)) and its right-hand-side partner vanish
identically for P1 (as oracle/assembly.py:110 notes for the scalar form).  Every integrand is a polynomial on an affine
cell: the closed forms with the barycentric tensors are exact.  The coefficients are NOT rescaled by E.

DoF layout: component-major blocks of nv entries, u_a at vertex v -> a nv + v, p_a at vertex v -> (d + a) nv + v.
Active set: u_a on the vertices of cells tagged 1 or 2, p_a on the vertices of cells tagged 2.
"""
import numpy as np
import scipy.sparse as sp

from oracle.assembly import _bary_tensor, simplex_geometry
from oracle.elasticity import lame, sigma_basis


def facet_sides(topo, g, fs):
    """The two cells of the interior facets fs -> [(cells, outward unit normal, |grad N_lf|)] * 2."""
    out = []
    for side in (0, 1):
        cs = topo.f2c[fs, side]
        lf = np.argmax(topo.c2f[cs] == fs[:, None], axis=1)
        gn = np.sqrt((g[cs, lf] ** 2).sum(axis=1))
        out.append((cs, -g[cs, lf] / gn[:, None], gn))
    return out


def assemble_elasticity_wd(topo, x, cell_tags, facet_tags, ds, phi_h, f_h, u_D, E=1.0, nu=0.3, pen_coef=1.0,
                           stab_coef=1.0):
    """cell_tags / facet_tags: dense int arrays; ds: flat [cell, local facet, ...]; phi_h (nv,); f_h, u_D (nv, d).
    Returns (A csr (2 d nv)^2, b, active bool)."""
    x = np.asarray(x, dtype=np.float64)
    cells = topo.cells
    nv = topo.nv
    d = x.shape[1]
    n = d + 1
    cell_tags = np.asarray(cell_tags)
    facet_tags = np.asarray(facet_tags)
    f_h = np.asarray(f_h, dtype=np.float64).reshape(nv, d)
    u_D = np.asarray(u_D, dtype=np.float64).reshape(nv, d)
    g, vol, h = simplex_geometry(x, cells)
    M2, M3, M4 = _bary_tensor(d, 2), _bary_tensor(d, 3), _bary_tensor(d, 4)
    lam, mu = lame(E, nu)
    rows, cols, vals = [], [], []
    b = np.zeros(2 * d * nv)

    def add(blk_r, vr, blk_c, vc, v):
        """v (ne, nr, ncol): rows on the vertices vr (ne, nr) of block blk_r, columns on vc (ne, ncol) of blk_c."""
        r = blk_r * nv + vr[:, :, None]
        c = blk_c * nv + vc[:, None, :]
        rows.append(np.broadcast_to(r, v.shape).reshape(-1))
        cols.append(np.broadcast_to(c, v.shape).reshape(-1))
        vals.append(np.ascontiguousarray(v).reshape(-1))

    # ---- sigma(u) : eps(v) and f_h . v on dx((1,2))
    om = np.flatnonzero((cell_tags == 1) | (cell_tags == 2))
    cv = cells[om]
    S = sigma_basis(g[om], lam, mu)                       # S[c, j, b] = sigma(N_j e_b)
    for a in range(d):
        for c in range(d):
            # eps(N_i e_a) : S[j, c] = S[j, c, a, :] . g_i  (S symmetric)
            add(a, cv, c, cv, vol[om, None, None] * np.einsum("cjq,ciq->cij", S[:, :, c, a, :], g[om]))
        np.add.at(b, a * nv + cv, vol[om, None] * np.einsum("ij,cj->ci", M2, f_h[cv, a]))

    # ---- -(sigma(u) n) . v on ds: n = -g_lf / |g_lf|, |F| = d vol |g_lf|, int_F N_i = |F| / d for i on F
    ents = np.asarray(ds, dtype=np.int64).reshape(-1, 2)
    if ents.size:
        ce, lf = ents[:, 0], ents[:, 1]
        Se = sigma_basis(g[ce], lam, mu)
        t = vol[ce, None, None, None] * np.einsum("cjbpq,cq->cjbp", Se, g[ce, lf])   # (ne, j, col comp, row comp)
        for i in range(n):
            on_f = lf != i
            if not on_f.any():
                continue
            ci = ce[on_f]
            for a in range(d):
                for c in range(d):
                    add(a, cells[ci, i][:, None], c, cells[ci], t[on_f][:, None, :, c, a])

    # ---- penalisation on the cut cells: the scalar blocks of oracle/assembly.py:93-109, once per component
    cut = np.flatnonzero(cell_tags == 2)
    cc = cells[cut]
    hc, vc = h[cut], vol[cut]
    ph = np.asarray(phi_h, dtype=np.float64)[cc]
    gam = pen_coef
    uu = gam * (hc ** -2 * vc)[:, None, None] * M2[None]
    up = -gam * (hc ** -3 * vc)[:, None, None] * np.einsum("ijk,ck->cij", M3, ph)
    pp = gam * (hc ** -4 * vc)[:, None, None] * np.einsum("ijkl,ck,cl->cij", M4, ph, ph)
    for a in range(d):
        add(a, cc, a, cc, uu)
        add(a, cc, d + a, cc, up)
        add(d + a, cc, a, cc, up)
        add(d + a, cc, d + a, cc, pp)
        ud = u_D[cc, a]
        np.add.at(b, a * nv + cc, gam * (hc ** -2 * vc)[:, None] * np.einsum("ij,cj->ci", M2, ud))
        np.add.at(b, (d + a) * nv + cc, -gam * (hc ** -3 * vc)[:, None] * np.einsum("ijk,cj,ck->ci", M3, ud, ph))
    # stab h_T^2 (div sigma(u), div sigma(v)) on dx(2) and its right-hand side: div sigma of a P1 field vanishes.

    # ---- stab avg(h) [sigma(u) n] . [sigma(v) n] on dS((2,3))
    fs = np.flatnonzero(((facet_tags == 2) | (facet_tags == 3)) & (topo.f2c[:, 1] >= 0))
    if fs.size:
        sides = facet_sides(topo, g, fs)
        (cp, _, gnp), (cm, _, _) = sides
        area = d * vol[cp] * gnp
        wgt = stab_coef * 0.5 * (h[cp] + h[cm]) * area
        J = [np.einsum("cjbpq,cq->cjbp", sigma_basis(g[cs], lam, mu), nrm) for cs, nrm, _ in sides]   # sigma(N_j e_b) n
        for (cr, _, _), Jr in zip(sides, J):
            for (ccol, _, _), Jc in zip(sides, J):
                for a in range(d):
                    for c in range(d):
                        add(a, cells[cr], c, cells[ccol],
                            wgt[:, None, None] * np.einsum("cip,cjp->cij", Jr[:, :, a], Jc[:, :, c]))

    ndof = 2 * d * nv
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(ndof, ndof)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    active = np.zeros(ndof, dtype=bool)
    for a in range(d):
        active[a * nv + cv.reshape(-1)] = True
        active[(d + a) * nv + cc.reshape(-1)] = True
    return A, b, active


def solve_direct(A, b, active):
    """Solution in the full numbering: direct solve on the active DoFs, exactly 0 elsewhere."""
    import scipy.sparse.linalg as spla
    idx = np.flatnonzero(active)
    w = np.zeros_like(b)
    w[idx] = spla.spsolve(A[idx][:, idx].tocsc(), b[idx])
    return w


def box_problem(d, n, centre=(0.03, -0.02, 0.01), lo=-1.5, hi=1.5, single_layer_cut=True):
    """Kuhn box [lo, hi]^d with n cubes per axis, tagged by the oracle with the unit sphere about `centre`
    -> (topo, x, cell_tags, facet_tags, ds100, phi)."""
    import warnings

    from oracle import meshgen
    from oracle import tagging as T
    from oracle.topology import Topology
    ctype = "triangle" if d == 2 else "tetrahedron"
    x, cells = meshgen.create_box([lo] * d, [hi] * d, [n] * d)
    topo = Topology(ctype, cells, x.shape[0])
    phi = ((x - np.asarray(centre)[:d]) ** 2).sum(axis=1) - 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ct, ft, _, meas, _, _ = T.compute_tags_measures(ctype, x, topo, T.NodalP1(phi), 1, box_mode=True,
                                                        single_layer_cut=single_layer_cut)
    cv = np.zeros(topo.nc, dtype=np.int64)
    cv[ct.indices] = ct.values
    return topo, x, cv, np.asarray(ft.values), meas(100), phi
