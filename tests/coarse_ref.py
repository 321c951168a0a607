"""numpy specification of the coarse-space correction  out += D R Ac^-1 R^T in  of phifem_amd/csrc/phx_coarse.inc.hip
(test infrastructure only; no GPU use).

R: multilinear hats on a coarse lattice of spacing H = ratio_h h over the box [-1.5, 1.5]^d, node c = (c_0, c_1, c_2)
at the point c * H, c_a = 0 .. ceil(n_a / ratio_h), one set per coarse block.  Three layouts (DoF index = block * nent +
entity, `dof` maps an active row to it):

  "elwd"       weak-Dirichlet elasticity: blocks u_a, a < d, on the vertex lattice; every active u row is eligible,
               the p blocks carry nothing;
  "p2"         P2 weak Dirichlet: the fields u and p on the h/2 lattice (vertices and edge midpoints), every active
               row eligible; the kernels count h/2 steps, their ratio is 2 ratio_h;
  "interface"  interface elasticity: 2 d blocks u_in[a], u_out[a]; the y and p blocks carry nothing and the u_in rows
               of the caller's bc_vertices (Dirichlet rows) are left out.

Columns are the COMPACT coarse DoFs: node_of[i] = block * M + node, node = c_0 + m_0 (c_1 + m_1 c_2) -- the nodes whose
hat is positive on an eligible row, in ascending order (`used_nodes`).
D: the inverse of the column scaling C of the operator A C the loop iterates on.  diag A for both elasticity layouts.
P2 (k_p2c_dpos): a structured system (generated 3-D box) keeps its u columns unscaled, D = 1 on the u rows and diag A on
the p rows; every other P2 system (2-D boxes are assembled row by row) scales all columns, D = diag A on every row.
Ac = R^T A R with the unscaled matrix.  Everything here is in the ACTIVE-ROW order of the exported CSR."""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble          # float64 where numpy offers nothing wider
LO, HI = -1.5, 1.5
EPS = float(np.finfo(np.float64).eps)


def blocks_with_hats(layout, d):
    return {"elwd": d, "p2": 2, "interface": 2 * d}[layout]


def steps_per_cube(layout):
    return 2 if layout == "p2" else 1


def coarse_dims(ncubes, ratio_h, d):
    """(m[3], M): coarse nodes per axis and per block."""
    m = [-(-int(ncubes[a]) // ratio_h) + 1 if a < d else 1 for a in range(3)]
    return m, m[0] * m[1] * m[2]


def lattice_index(pts, ncubes, d, steps=1):
    """Integer index of every point on the lattice of `steps` points per cube edge, (npts, d)."""
    cnt = np.asarray([int(ncubes[a]) * steps for a in range(d)], dtype=np.float64)
    t = (np.asarray(pts, dtype=np.float64)[:, :d] - LO) / (HI - LO) * cnt
    i = np.rint(t).astype(np.int64)
    assert np.abs(t - i).max() <= 1e-9, "a point off the lattice"
    return i


def eligible(dof, nent, d, layout, bc_vertices=None):
    """Mask of the active rows that carry coarse functions."""
    blk = np.asarray(dof) // nent
    ok = blk < blocks_with_hats(layout, d)
    if layout == "interface" and bc_vertices is not None:
        ok &= ~((blk < d) & np.isin(np.asarray(dof) % nent, np.asarray(bc_vertices)))
    return ok


def axis_nodes(i, ratio, m):
    """Restatement of cc_axis: the two coarse nodes and weights that cover the fine index i along an axis with m coarse
    nodes -> (c (n, 2), w (n, 2))."""
    i = np.asarray(i, dtype=np.int64)
    c0 = i // ratio
    c0 = np.where(c0 > m - 2, max(m - 2, 0), c0)
    t = i.astype(np.float64) / float(ratio) - c0.astype(np.float64)
    has1 = c0 + 1 < m
    c1 = np.where(has1, c0 + 1, c0)
    return np.stack([c0, c1], axis=1), np.stack([1.0 - t, np.where(has1, t, 0.0)], axis=1)


def _full_restriction(idx, blk, ok, m, M, nblk, ratio, d, form):
    """R over ALL nblk * M nodes (columns block * M + node), csr without explicit zeros."""
    n = idx.shape[0]
    rows = np.flatnonzero(ok)
    if form == "hat":
        # the hat of node c along an axis: 1 - |i - c ratio| / ratio on |i - c ratio| < ratio
        w = np.ones((rows.size, M))
        node = np.arange(M)
        cn = [node % m[0], (node // m[0]) % m[1], node // (m[0] * m[1])]
        for a in range(d):
            w *= np.clip(1.0 - np.abs(idx[rows, a:a + 1] - cn[a][None, :] * ratio) / float(ratio), 0.0, None)
        r, c = np.nonzero(w)
        Rm = sp.csr_matrix((w[r, c], (rows[r], blk[rows][r] * M + c)), shape=(n, nblk * M))
    elif form == "axis":
        cs, ws = zip(*[axis_nodes(idx[rows, a], ratio, m[a]) for a in range(d)])
        rr, cc, ww = [], [], []
        for q in range(2 ** d):
            node = np.zeros(rows.size, dtype=np.int64)
            w = np.ones(rows.size)
            stride = 1
            for a in range(d):
                b = (q >> a) & 1
                node += stride * cs[a][:, b]
                w = w * ws[a][:, b]
                stride *= m[a]
            # the clamped last node returns (c0, c0) with weights (1 - t, 0): the zero-weight twin is dropped
            keep = w != 0.0
            rr.append(rows[keep]); cc.append((blk[rows] * M + node)[keep]); ww.append(w[keep])
        Rm = sp.coo_matrix((np.concatenate(ww), (np.concatenate(rr), np.concatenate(cc))), shape=(n, nblk * M)).tocsr()
        Rm.sum_duplicates()
    else:
        raise ValueError(form)
    Rm.eliminate_zeros()
    Rm.sort_indices()
    return Rm


def _full(pts, dof, nent, ncubes, ratio_h, d, layout, bc_vertices, form):
    """R over all nodes of the blocks that carry hats."""
    dof = np.asarray(dof, dtype=np.int64)
    steps = steps_per_cube(layout)
    idx = lattice_index(np.asarray(pts)[dof % nent], ncubes, d, steps)
    m, M = coarse_dims(ncubes, ratio_h, d)
    ok = eligible(dof, nent, d, layout, bc_vertices)
    return _full_restriction(idx, dof // nent, ok, m, M, blocks_with_hats(layout, d), ratio_h * steps, d, form)


def used_nodes(pts, dof, nent, ncubes, ratio_h, d, layout="elwd", bc_vertices=None):
    """node_of of the compact coarse space: the nodes whose hat is positive on an eligible row, ascending."""
    full = _full(pts, dof, nent, ncubes, ratio_h, d, layout, bc_vertices, "hat")
    return np.flatnonzero(np.asarray(full.sum(axis=0)).ravel() > 0.0).astype(np.int32)


def restriction(pts, dof, nent, node_of, ncubes, ratio_h, d, layout="elwd", bc_vertices=None, form="hat"):
    """R (active rows x compact coarse DoFs) as csr, from the coordinates `pts` of the entities (vertices; P2: vertices
    and edge midpoints), the exported `dof` and the exported `node_of` (None: the nodes of `used_nodes`).
    form "hat": the hat formula per node; "axis": two nodes and weights per axis, as cc_axis states them."""
    if node_of is None:
        node_of = used_nodes(pts, dof, nent, ncubes, ratio_h, d, layout, bc_vertices)
    full = _full(pts, dof, nent, ncubes, ratio_h, d, layout, bc_vertices, form)
    return full[:, np.asarray(node_of, dtype=np.int64)].tocsr()


def scaling(A, dof, nent, layout, u_unscaled=True):
    """D by active row; u_unscaled: the P2 system keeps its u columns unscaled (structured, 3-D box)."""
    diag = np.asarray(A.diagonal(), dtype=np.float64)
    if layout == "p2" and u_unscaled:
        return np.where(np.asarray(dof) < nent, 1.0, diag)
    return diag


def rt_dot(Rm, v):
    """R^T v, accumulated in longdouble."""
    Rc = Rm.tocoo()
    out = np.zeros(Rm.shape[1], dtype=LD)
    np.add.at(out, Rc.col, Rc.data.astype(LD) * np.asarray(v, dtype=LD)[Rc.row])
    return out


def r_dot(Rm, z):
    """R z, accumulated in longdouble."""
    Rc = Rm.tocoo()
    out = np.zeros(Rm.shape[0], dtype=LD)
    np.add.at(out, Rc.row, Rc.data.astype(LD) * np.asarray(z, dtype=LD)[Rc.col])
    return out


def dense_dot(Am, x):
    """A x for a dense A, accumulated in longdouble."""
    return np.asarray(Am, dtype=LD) @ np.asarray(x, dtype=LD)


def galerkin(A, Rm):
    """Ac = R^T A R, dense float64."""
    return np.asarray((Rm.T @ A @ Rm).toarray(), dtype=np.float64)


def apply_ref(A, Rm, D, v, Ac=None):
    """(gc, zc, x): gc = R^T v, zc = (R^T A R)^-1 gc (numpy.linalg.solve on the float64 Galerkin matrix), x = D R zc.
    Ac: galerkin(A, Rm) when the caller has it already."""
    gc = rt_dot(Rm, v)
    zc = np.linalg.solve(galerkin(A, Rm) if Ac is None else Ac, gc.astype(np.float64))
    x = np.asarray(D, dtype=LD) * r_dot(Rm, zc)
    return gc, zc, x
