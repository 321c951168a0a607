"""Specification of the restriction and of the multilevel preconditioner on refined simplex meshes (TEST
INFRASTRUCTURE, numpy / scipy in float64): what phifem_amd/csrc/phx_restrict.inc.hip has to equal bit for bit and
phifem_amd/csrc/phx_multilevel.inc.hip to round-off.  DESIGN.md 7f and include/phifem_hip.h state the same rules.

A HIERARCHY is a list of levels 0 .. L, each a dict(ctype, x, cells, pairs): `pairs` [nm, 2] are the coarse end
vertices (p, q) of the bisected edges of the level below, in the order of the new vertices: vertex v < nv_coarse of a
level IS vertex v of the level below, vertex nv_coarse + r the midpoint of pairs[r] (both refinements number that way;
level 0 has pairs = None).

  pairs_uniform / pairs_marked   the pairs behind refine_ref / refine_marked_ref
  prolongation_matrix            P_l (sparse): identity on the coarse vertices, 0.5 / 0.5 at the new ones
  restrict_ref                   P^T applied with the STATED ORDER OF ADDITIONS:
                                 out[p] = ((in[p] + 0.5 in[m_1]) + 0.5 in[m_2]) + ..., m ascending
  boundary_vertices              vertices of the facets that belong to one cell
  constrained_sets               level L: boundary vertex that is no active u DoF, or vertex of no cell at all (its
                                 row of K is empty); below: the vertex is constrained when its image on level L is
  stiffness                      K_l = P1 stiffness of ALL cells, constrained rows and columns -> identity
  Multilevel                     the V-cycle: damped Jacobi (omega = 2/3, nu = 2 before and after, zero initial guess),
                                 masked transfer, coarse kinds 0 (2 nu + 8 sweeps), 1 (dense inverse), 2 (the same
                                 exact solve, by whatever lattice method the library uses)
  minv                           M^-1 = R V R^T on the active u DoFs (+) Jacobi on the p DoFs
  bicgstab                       plain right-preconditioned BiCGStab, counts iterations
"""
import numpy as np
import scipy.sparse as sp

import refine_ref as RR

OMEGA = 2.0 / 3.0
NU = 2
COARSE_SWEEPS = 8
DENSE_CAP = 2048


# ---- transfer ---------------------------------------------------------------------------------------------------------
def pairs_uniform(ctype, x, cells, edges=None):
    """End vertices of the edges of the coarse mesh, in the order of the new vertices of refine_ref."""
    return np.asarray(RR.cell_nodes(ctype, x, cells, edges)[1], dtype=np.int64)


def pairs_marked(ref):
    """The same for ref = refine_marked_ref(...)."""
    return np.asarray(ref["edges"], dtype=np.int64)[ref["mid_edges"]]


def prolongation_matrix(nv, pairs):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    nm = pairs.shape[0]
    rows = np.concatenate([np.arange(nv), nv + np.repeat(np.arange(nm), 2)])
    cols = np.concatenate([np.arange(nv), pairs.reshape(-1)])
    vals = np.concatenate([np.ones(nv), np.full(2 * nm, 0.5)])
    return sp.csr_matrix((vals, (rows, cols)), shape=(nv + nm, nv))


def restriction_csr(nv, pairs):
    """(ptr [nv + 1], idx): row p lists the new fine vertices on the bisected edges that end in p, ascending.  The
    entries (p_r, nv + r), (q_r, nv + r), r ascending, sorted by their coarse vertex with a STABLE sort."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    key = pairs.reshape(-1)
    val = nv + np.repeat(np.arange(pairs.shape[0]), 2)
    order = np.argsort(key, kind="stable")
    ptr = np.searchsorted(key[order], np.arange(nv + 1), side="left")
    return ptr, val[order]


def restrict_ref(nv, pairs, values):
    """values (nvf,) or (ncomp, nvf) on the fine mesh -> (.., nv) on the coarse one, additions left to right."""
    v = np.asarray(values, dtype=np.float64)
    ptr, idx = restriction_csr(nv, pairs)
    assert v.shape[-1] == nv + np.asarray(pairs).reshape(-1, 2).shape[0]
    out = v[..., :nv].copy()
    count = np.diff(ptr)
    for j in range(int(count.max()) if count.size else 0):
        rows = np.flatnonzero(count > j)                       # every row once per pass: a plain vector addition
        out[..., rows] = out[..., rows] + 0.5 * v[..., idx[ptr[rows] + j]]
    return out


# ---- level operators --------------------------------------------------------------------------------------------------
def boundary_vertices(cells):
    """bool [max vertex + 1]: vertices of the facets that belong to exactly one cell."""
    cells = np.asarray(cells, dtype=np.int64)
    nvpc = cells.shape[1]
    fv = np.stack([np.sort(np.delete(cells, k, axis=1), axis=1) for k in range(nvpc)], axis=1).reshape(-1, nvpc - 1)
    uniq, count = np.unique(fv, axis=0, return_counts=True)
    out = np.zeros(int(cells.max()) + 1, dtype=bool)
    out[uniq[count == 1].reshape(-1)] = True
    return out


def boundary_vertices_padded(level):
    out = np.zeros(np.asarray(level["x"]).shape[0], dtype=bool)
    b = boundary_vertices(level["cells"])
    out[:b.size] = b
    return out


def constrained_sets(levels, active_u):
    """active_u: bool [nv_L], the active u DoFs of the system on the finest level -> one bool array per level."""
    top = levels[-1]
    nvL = np.asarray(top["x"]).shape[0]
    bnd = boundary_vertices_padded(top)
    used = np.zeros(nvL, dtype=bool)
    used[np.asarray(top["cells"]).reshape(-1)] = True
    cons = (bnd & ~np.asarray(active_u, dtype=bool)) | ~used
    return [cons[:np.asarray(lv["x"]).shape[0]].copy() for lv in levels]


def stiffness_full(x, cells):
    """int grad lambda_i . grad lambda_j over all cells (sparse, nv x nv)."""
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    d = x.shape[1]
    J = x[cells[:, 1:]] - x[cells[:, :1]]                       # rows: edge vectors v_k - v_0
    vol = np.abs(np.linalg.det(J)) / (2.0 if d == 2 else 6.0)
    Ji = np.linalg.inv(J)                                       # columns: gradients of lambda_1 .. lambda_d
    g = np.concatenate([-Ji.sum(axis=2, keepdims=True), Ji], axis=2).transpose(0, 2, 1)   # (nc, nvpc, d)
    Ke = vol[:, None, None] * np.einsum("cid,cjd->cij", g, g)
    n = d + 1
    rows = np.repeat(cells, n, axis=1).reshape(-1)
    cols = np.tile(cells, (1, n)).reshape(-1)
    K = sp.coo_matrix((Ke.reshape(-1), (rows, cols)), shape=(x.shape[0], x.shape[0])).tocsr()
    K.sum_duplicates()
    return K


def stiffness(x, cells, cons):
    free = sp.diags((~cons).astype(np.float64))
    return (free @ stiffness_full(x, cells) @ free + sp.diags(cons.astype(np.float64))).tocsr()


class Multilevel:
    """The V-cycle operator V ~ K_L^-1 of a hierarchy.  coarse: 0 sweeps, 1 / 2 exact; None: 1 when n_0 <= DENSE_CAP,
    else 0 (what the library picks when no lattice solve is built)."""

    def __init__(self, levels, active_u, coarse=None):
        self.levels = levels
        self.cons = constrained_sets(levels, active_u)
        if not (self.cons[-1] & boundary_vertices_padded(levels[-1])).any():
            raise ValueError("no constrained vertex: the level matrices are singular")
        self.K = [stiffness(lv["x"], lv["cells"], c) for lv, c in zip(levels, self.cons)]
        self.dinv = [1.0 / K.diagonal() for K in self.K]
        self.nv = [K.shape[0] for K in self.K]
        self.P = [None] + [prolongation_matrix(self.nv[l - 1], levels[l]["pairs"]) for l in range(1, len(levels))]
        self.coarse = coarse if coarse is not None else (1 if self.nv[0] <= DENSE_CAP else 0)
        self.K0inv = np.linalg.inv(self.K[0].toarray()) if self.coarse else None

    def smooth(self, l, b, x, sweeps):
        """Damped Jacobi; x = None: zero initial guess, whose first sweep is omega D^-1 b."""
        for _ in range(sweeps):
            x = OMEGA * self.dinv[l] * b if x is None else x + OMEGA * self.dinv[l] * (b - self.K[l] @ x)
        return x

    def cycle(self, l, b):
        if l == 0:
            return self.K0inv @ b if self.coarse else self.smooth(0, b, None, 2 * NU + COARSE_SWEEPS)
        x = self.smooth(l, b, None, NU)
        r = b - self.K[l] @ x
        rc = restrict_ref(self.nv[l - 1], self.levels[l]["pairs"], r)
        rc[self.cons[l - 1]] = 0.0
        e = self.P[l] @ self.cycle(l - 1, rc)
        e[self.cons[l]] = 0.0
        return self.smooth(l, b, x + e, NU)

    def apply(self, b):
        return self.cycle(len(self.levels) - 1, np.asarray(b, dtype=np.float64))

    def dense(self):
        n = self.nv[-1]
        return np.stack([self.apply(e) for e in np.eye(n)], axis=1)


def minv(ml, u_vertex, diag_p):
    """M^-1 on the active DoFs ordered (u DoFs, p DoFs): u_vertex[i] = vertex of u DoF i, diag_p = A_pp diagonal."""
    nu = len(u_vertex)
    nvL = ml.nv[-1]

    def apply(r):
        g = np.zeros(nvL)
        g[u_vertex] = r[:nu]
        return np.concatenate([ml.apply(g)[u_vertex], r[nu:] / diag_p])
    return apply


# ---- Krylov -----------------------------------------------------------------------------------------------------------
def bicgstab(A, b, prec, rtol=1e-8, max_iter=20000):
    """Right-preconditioned BiCGStab from x0 = 0 -> (x, iterations, converged): |r| <= rtol |b| of the recursive
    residual, checked after every iteration."""
    x = np.zeros_like(b)
    r = b.copy()
    rhat = r.copy()
    p = r.copy()
    rho = rhat @ r
    bb = np.sqrt(b @ b)
    if bb == 0.0:
        return x, 0, True
    for it in range(1, max_iter + 1):
        ph = prec(p)
        v = A @ ph
        alpha = rho / (rhat @ v)
        s = r - alpha * v
        sh = prec(s)
        t = A @ sh
        tt = t @ t
        omega = (t @ s) / tt if tt > 0.0 else 0.0
        x += alpha * ph + omega * sh
        r = s - omega * t
        if np.sqrt(r @ r) <= rtol * bb:
            return x, it, True
        rho_new = rhat @ r
        beta = (rho_new / rho) * (alpha / omega)
        rho = rho_new
        p = r + beta * (p - omega * v)
    return x, max_iter, False
