"""Specification of point location and of the evaluation of Lagrange functions at points (TEST INFRASTRUCTURE): numpy
restatements that the device code of phifem_amd/csrc/phx_locate.inc.hip has to agree with.  Nothing here is taken from
the kernels: containment is a brute-force test of ALL cells against all points, the bases are written from their
definitions.

  coords(ctype, x, cells, pts)     the coordinates that decide containment, (npts, nc, k): the d + 1 barycentric
                                   coordinates of a simplex; (xi, 1 - xi, eta, 1 - eta) of an axis-parallel rectangle
  locate_ref(...)                  cell = the SMALLEST index among the cells whose coordinates are all >= -tol (-1: none),
                                   xref = lambda_1 .. lambda_d of the stored vertex order / (xi, eta)
  input_condition(...)             True when no (point, cell) pair sits at the tolerance
  basis(ctype, degree, xref)       P1 / P2 / Q1 basis functions and their reference gradients at xref
  evaluate_ref(...)                values and physical gradients

The P2 basis: vertices lambda_v (2 lambda_v - 1), then the edges (a, b) of LOCAL_PAIRS (basix order) 4 lambda_a lambda_b.
Q1 on the rectangle with vertices in tensor-product order v0 (0,0), v1 (1,0), v2 (0,1), v3 (1,1): vertex i carries
(xi or 1 - xi by bit 0) * (eta or 1 - eta by bit 1).
"""
import numpy as np

LOCAL_PAIRS = {
    "triangle": [(1, 2), (0, 2), (0, 1)],
    "tetrahedron": [(2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1)],
}
CHUNK = 256


def jacobians(ctype, x, cells):
    """J[c][a][i] = d x_a / d xref_i of every cell (rectangles: diag(hx, hy))."""
    xc = x[cells]
    if ctype == "quadrilateral":
        J = np.zeros((cells.shape[0], 2, 2))
        J[:, 0, 0] = xc[:, 1, 0] - xc[:, 0, 0]
        J[:, 1, 1] = xc[:, 2, 1] - xc[:, 0, 1]
        return J
    return np.transpose(xc[:, 1:] - xc[:, :1], (0, 2, 1))


def ref_gradients(ctype, x, cells):
    """G[c][i][a] = d xref_i / d x_a by Cramer's rule, in extended precision (np.longdouble): the containment test
    compares EVERY cell with every point, and for a cell 30 cell widths away from a point on the line through one of
    its edges a float64 coordinate that is 0 in exact arithmetic comes out as +-1e-14; the input condition of
    tests/test_hip_evaluate.py is about the coordinates themselves, not about that round-off."""
    xc = np.asarray(x, dtype=np.longdouble)[cells]
    if ctype == "quadrilateral":
        G = np.zeros((cells.shape[0], 2, 2), dtype=np.longdouble)
        G[:, 0, 0] = 1 / (xc[:, 1, 0] - xc[:, 0, 0])
        G[:, 1, 1] = 1 / (xc[:, 2, 1] - xc[:, 0, 1])
        return G
    E = xc[:, 1:] - xc[:, :1]                        # E[c][i] = x_{i+1} - x_0
    if E.shape[1] == 2:
        det = E[:, 0, 0] * E[:, 1, 1] - E[:, 1, 0] * E[:, 0, 1]
        G = np.stack([np.stack([E[:, 1, 1], -E[:, 1, 0]], 1), np.stack([-E[:, 0, 1], E[:, 0, 0]], 1)], axis=1)
    else:
        G = np.stack([np.cross(E[:, 1], E[:, 2]), np.cross(E[:, 2], E[:, 0]), np.cross(E[:, 0], E[:, 1])], axis=1)
        det = (E[:, 0] * G[:, 0]).sum(axis=1)
    return G / det[:, None, None]


def xref_all(ctype, x, cells, pts, G=None):
    """(npts, nc, d): reference coordinates of every point in EVERY cell (np.longdouble)."""
    if G is None:
        G = ref_gradients(ctype, x, cells)
    r = np.asarray(pts, dtype=np.longdouble)[:, None, :] - np.asarray(x, dtype=np.longdouble)[cells[:, 0]][None, :, :]
    return (G[None, :, :, :] * r[:, :, None, :]).sum(axis=-1)


def coords(ctype, x, cells, pts, G=None):
    xr = xref_all(ctype, x, cells, pts, G)
    if ctype == "quadrilateral":
        return np.stack([xr[..., 0], 1 - xr[..., 0], xr[..., 1], 1 - xr[..., 1]], axis=-1)
    return np.concatenate([1 - xr.sum(axis=-1, keepdims=True), xr], axis=-1)


def locate_ref(ctype, x, cells, pts, tol=1e-12):
    """-> (cell [npts] int32, xref [npts, d] float64, holds [npts, nc] bool)."""
    npts, d = pts.shape
    G = ref_gradients(ctype, x, cells)
    cell = np.full(npts, -1, dtype=np.int32)
    xref = np.zeros((npts, d))
    holds = np.zeros((npts, cells.shape[0]), dtype=bool)
    for s in range(0, npts, CHUNK):
        p = pts[s:s + CHUNK]
        lam = coords(ctype, x, cells, p, G)
        h = np.all(lam >= -tol, axis=-1)
        holds[s:s + CHUNK] = h
        first = np.argmax(h, axis=1)                   # the smallest index that holds the point
        found = h.any(axis=1)
        cell[s:s + CHUNK] = np.where(found, first, -1)
        xr = lam[np.arange(p.shape[0]), first]
        xr = xr[:, [0, 2]] if ctype == "quadrilateral" else xr[:, 1:]
        xref[s:s + CHUNK] = np.where(found[:, None], xr.astype(np.float64), 0.0)
    return cell, xref, holds


def input_condition(ctype, x, cells, pts, inside=-1e-14, outside=-1e-9):
    """No (point, cell) pair sits where round-off decides: the SMALLEST coordinate of every pair -- the one containment
    hangs on -- is >= inside or <= outside.  (Coordinate by coordinate the condition cannot hold on a lattice mesh: a
    cell 30 widths away from a point on the line through one of its edges has one coordinate of -1e-13 there, the
    vertex coordinates being rounded, next to another one of -2 that decides.)"""
    return unsettled_points(ctype, x, cells, pts, inside, outside).size == 0


def unsettled_points(ctype, x, cells, pts, inside=-1e-14, outside=-1e-9):
    """Indices of the points that miss the input condition with some cell."""
    G = ref_gradients(ctype, x, cells)
    bad = []
    for s in range(0, pts.shape[0], CHUNK):
        lo = coords(ctype, x, cells, pts[s:s + CHUNK], G).min(axis=-1)
        bad.append(s + np.flatnonzero(np.any((lo < inside) & (lo > outside), axis=1)))
    return np.concatenate(bad) if bad else np.zeros(0, dtype=np.int64)


def basis(ctype, degree, xref):
    """-> N [npts, ndof], dN [npts, ndof, d] (gradients in the reference coordinates)."""
    xref = np.atleast_2d(xref)
    npts, d = xref.shape
    if ctype == "quadrilateral":
        if degree != 1:
            raise NotImplementedError
        xi, eta = xref[:, 0], xref[:, 1]
        one = np.ones(npts)
        N = np.stack([(1 - xi) * (1 - eta), xi * (1 - eta), (1 - xi) * eta, xi * eta], axis=1)
        dN = np.stack([np.stack([-(1 - eta), -(1 - xi)], 1), np.stack([(1 - eta), -xi], 1),
                       np.stack([-eta, (1 - xi)], 1), np.stack([eta, xi], 1)], axis=1) * one[:, None, None]
        return N, dN
    lam = np.concatenate([1.0 - xref.sum(axis=1, keepdims=True), xref], axis=1)        # [npts, d + 1]
    dlam = np.concatenate([-np.ones((1, d)), np.eye(d)], axis=0)                       # [d + 1, d]
    if degree == 1:
        return lam, np.broadcast_to(dlam, (npts, d + 1, d)).copy()
    if degree != 2:
        raise NotImplementedError
    N = [lam[:, v] * (2.0 * lam[:, v] - 1.0) for v in range(d + 1)]
    dN = [(4.0 * lam[:, v] - 1.0)[:, None] * dlam[v][None, :] for v in range(d + 1)]
    for a, b in LOCAL_PAIRS[ctype]:
        N.append(4.0 * lam[:, a] * lam[:, b])
        dN.append(4.0 * (lam[:, a, None] * dlam[b][None, :] + lam[:, b, None] * dlam[a][None, :]))
    return np.stack(N, axis=1), np.stack(dN, axis=1)


def cell_dofs(ctype, cells, degree, nv, c2e=None):
    if degree == 1:
        return np.asarray(cells, dtype=np.int64)
    return np.concatenate([np.asarray(cells, dtype=np.int64), nv + np.asarray(c2e, dtype=np.int64)], axis=1)


def evaluate_ref(ctype, x, cells, values, cell, xref, degree=1, c2e=None, fill=np.nan):
    """values (ndofs,) or (ncomp, ndofs) -> (out, grad) of shapes (..., npts) and (..., npts, d); `fill` where cell < 0."""
    v = np.atleast_2d(values)
    npts, d = xref.shape
    ok = cell >= 0
    c = np.where(ok, cell, 0)
    N, dN = basis(ctype, degree, xref)
    Ji = np.linalg.inv(jacobians(ctype, x, cells))[c]                # d xref_i / d x_a
    G = np.einsum("pki,pia->pka", dN, Ji)                             # physical gradients of the basis
    u = v[:, cell_dofs(ctype, cells, degree, x.shape[0], c2e)[c]]     # [ncomp, npts, ndof]
    out = np.einsum("pk,qpk->qp", N, u)
    grad = np.einsum("pka,qpk->qpa", G, u)
    out[:, ~ok] = fill
    grad[:, ~ok] = fill
    if np.ndim(values) == 1:
        return out[0], grad[0]
    return out, grad
