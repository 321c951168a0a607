"""Specification of marked refinement (TEST INFRASTRUCTURE): numpy restatement of the rule that
phifem_amd/csrc/phx_refine_marked.inc.hip has to equal bit for bit (meshes, degree-1 transfer) or to round-off
(degree-2 transfer).  DESIGN.md 7e and include/phifem_hip.h state the same rule in words.

  edge_positions          the strict total order of the edges: position 0 is the greatest edge
  close_marks             seed + closure (least fixed point) -> marked edges
  leaves                  recursive bisection of one cell by its greatest marked edge -> leaf tuples of local nodes
  refine_marked_ref       (x, cells, masks) -> fine x, cells, parent_cells, child_nodes, marked edges
  prolongate_marked_ref   nodal values on the coarse mesh -> nodal values on the fine mesh

Edges are numbered as refine_ref.edge_numbering does (ascending sorted pair, or the `edges` array of a generated box).
Local degree-2 node d of a cell: d < nvpc its vertex d, nvpc + k the midpoint of its local edge k (basix order).
"""
import functools

import numpy as np

import refine_ref as RR

NVPC = {"triangle": 3, "tetrahedron": 4}
MAXCHILD = {"triangle": 4, "tetrahedron": 8}
# local edges of the faces of a tetrahedron (face f is opposite vertex f)
TET_FACE_EDGES = np.array([[0, 1, 2], [0, 3, 4], [1, 3, 5], [2, 4, 5]])


def edge_positions(x, edges):
    """pos[e] = number of edges greater than e.  Edge (p, q), p < q, has the key len2 = ((dx dx + dy dy) + dz dz),
    d = x[q] - x[p]; the greater len2 wins, on equal len2 the lexicographically smaller (p, q)."""
    x = np.asarray(x, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.int64)
    d = x[edges[:, 1]] - x[edges[:, 0]]
    len2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    if x.shape[1] == 3:
        len2 = len2 + d[:, 2] * d[:, 2]
    order = np.lexsort((edges[:, 1], edges[:, 0], -len2))
    pos = np.empty(edges.shape[0], dtype=np.int64)
    pos[order] = np.arange(edges.shape[0])
    return pos


def close_marks(ctype, c2e, pos, cell_marks=None, edge_marks=None):
    """-> (marked [ne] bool, sweeps).  Seed: a marked cell marks all its edges, the edge mask is OR-ed in.  Closure:
    every cell (3-D: and every face) with a marked edge gets its greatest edge marked, until nothing changes; `sweeps`
    counts Jacobi sweeps including the last, idle one (the device's sweeps see marks earlier and may need fewer)."""
    ne = pos.shape[0]
    marked = np.zeros(ne, dtype=bool)
    if edge_marks is not None:
        marked |= np.asarray(edge_marks).astype(bool)
    if cell_marks is not None:
        marked[c2e[np.asarray(cell_marks).astype(bool)].reshape(-1)] = True
    pc = pos[c2e]                                                       # (nc, nepc)
    top_cell = c2e[np.arange(c2e.shape[0]), np.argmin(pc, axis=1)]
    if ctype == "tetrahedron":
        fe = c2e[:, TET_FACE_EDGES]                                     # (nc, 4, 3)
        k = np.argmin(pos[fe], axis=2)
        top_face = np.take_along_axis(fe, k[:, :, None], axis=2)[:, :, 0]
    sweeps = 0
    while True:
        sweeps += 1
        new = marked.copy()
        new[top_cell[marked[c2e].any(axis=1)]] = True
        if ctype == "tetrahedron":
            new[top_face[marked[fe].any(axis=2)]] = True
        if np.array_equal(new, marked):
            return marked, sweeps
        marked = new


@functools.lru_cache(maxsize=None)
def leaves(ctype, mask, ranks):
    """Leaf tuples of ONE cell: `mask` bit k = local edge k is marked, ranks[k] = number of local edges greater than
    edge k.  Recursive bisection by the greatest marked edge both of whose end nodes the tuple still holds, sitting at
    positions i < j: child 0 replaces position j by the midpoint node, child 1 position i; depth first, child 0
    first."""
    nvpc, pairs = NVPC[ctype], RR.LOCAL_PAIRS[ctype]
    out = []

    def rec(t):
        best = None
        for k, (a, b) in enumerate(pairs):
            if (mask >> k) & 1 and a in t and b in t and (best is None or ranks[k] < ranks[best]):
                best = k
        if best is None:
            out.append(t)
            return
        a, b = pairs[best]
        i, j = sorted((t.index(a), t.index(b)))
        m = nvpc + best
        rec(t[:j] + (m,) + t[j + 1:])
        rec(t[:i] + (m,) + t[i + 1:])
    rec(tuple(range(nvpc)))
    return np.array(out, dtype=np.int8)


def refine_marked_ref(ctype, x, cells, cell_marks=None, edge_marks=None, edges=None):
    """-> dict: x, cells (int64), parent_cells (int32), child_nodes (int8 [ncf, nvpc]), marked (bool [ne], after the
    closure), mid_edges (the marked edges ascending: fine vertex nv + r is the midpoint of mid_edges[r]), sweeps, c2e,
    edges."""
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    nc, nvpc = cells.shape
    nv = x.shape[0]
    c2e, edges = RR.edge_numbering(ctype, cells, edges)
    if cell_marks is not None:
        assert np.asarray(cell_marks).shape == (nc,)
    if edge_marks is not None:
        assert np.asarray(edge_marks).shape == (edges.shape[0],)
    pos = edge_positions(x, edges)
    marked, sweeps = close_marks(ctype, c2e, pos, cell_marks, edge_marks)
    mid_edges = np.flatnonzero(marked)
    erank = np.cumsum(marked) - 1
    xf = np.concatenate([x, 0.5 * x[edges[mid_edges, 0]] + 0.5 * x[edges[mid_edges, 1]]], axis=0)
    nepc = c2e.shape[1]
    lrank = np.argsort(np.argsort(pos[c2e], axis=1), axis=1)           # local ranks: 0 = the cell's greatest edge
    mbits = (marked[c2e] * (1 << np.arange(nepc))).sum(axis=1)
    key = mbits + 64 * (lrank * 6 ** np.arange(nepc)).sum(axis=1)
    uniq, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    pats = []
    for u in uniq:
        c = int(np.flatnonzero(key == u)[0])
        pats.append(leaves(ctype, int(mbits[c]), tuple(int(r) for r in lrank[c])))
    count = np.array([p.shape[0] for p in pats], dtype=np.int64)[inv]
    off = np.concatenate([[0], np.cumsum(count)])
    ncf = int(off[-1])
    nodes = np.concatenate([cells, nv + erank[c2e]], axis=1)            # (nc, nvpc + nepc); unmarked edges never used
    fcells = np.empty((ncf, nvpc), dtype=np.int64)
    child_nodes = np.empty((ncf, nvpc), dtype=np.int8)
    parent = np.empty(ncf, dtype=np.int32)
    for g, p in enumerate(pats):
        cs = np.flatnonzero(inv == g)
        rows = (off[cs][:, None] + np.arange(p.shape[0])[None, :])      # (ncs, k)
        fcells[rows] = nodes[cs][:, p.astype(np.int64)]                # (ncs, k, nvpc)
        child_nodes[rows] = p[None, :, :]
        parent[rows] = cs[:, None]
    return {"x": np.ascontiguousarray(xf), "cells": fcells, "parent_cells": parent, "child_nodes": child_nodes,
            "marked": marked, "mid_edges": mid_edges, "sweeps": sweeps, "c2e": c2e, "edges": edges}


def prolongate_marked_ref(ctype, x, cells, ref, values, degree=1):
    """values (ndofs,) or (ncomp, ndofs) on the coarse mesh -> the same on ref = refine_marked_ref(...)'s fine mesh
    (whose edges are numbered by ascending sorted pair)."""
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    v = np.asarray(values, dtype=np.float64)
    nv, nvpc = x.shape[0], cells.shape[1]
    edges, mid, c2e = ref["edges"], ref["mid_edges"], ref["c2e"]
    if degree == 1:
        assert v.shape[-1] == nv
        return np.concatenate([v, 0.5 * v[..., edges[mid, 0]] + 0.5 * v[..., edges[mid, 1]]], axis=-1)
    assert degree == 2 and v.shape[-1] == nv + edges.shape[0]
    pairs = np.array(RR.LOCAL_PAIRS[ctype])
    nepc = len(pairs)
    ndof2 = nvpc + nepc
    fcells, cn, parent = ref["cells"], ref["child_nodes"].astype(np.int64), ref["parent_cells"].astype(np.int64)
    nvf = ref["x"].shape[0]
    fc2e, fedges = RR.edge_numbering(ctype, fcells)
    bary = np.zeros((ndof2, nvpc))
    bary[np.arange(nvpc), np.arange(nvpc)] = 1.0
    for k, (a, b) in enumerate(pairs):
        bary[nvpc + k, a] = bary[nvpc + k, b] = 0.5
    pdofs = np.concatenate([cells, nv + c2e], axis=1)[parent]          # (ncf, ndof2) coarse DoFs of the parent
    val = np.zeros(v.shape[:-1] + (fcells.shape[0], nepc))
    for j, (a, b) in enumerate(pairs):
        lam = 0.5 * bary[cn[:, a]] + 0.5 * bary[cn[:, b]]              # (ncf, nvpc), multiples of 1/4
        w = np.concatenate([lam * (2.0 * lam - 1.0), 4.0 * lam[:, pairs[:, 0]] * lam[:, pairs[:, 1]]], axis=1)
        acc = np.zeros(v.shape[:-1] + (fcells.shape[0],))
        first = np.ones(fcells.shape[0], dtype=bool)
        for d in range(ndof2):                                          # ascending local DoF, zero weights skipped
            nz = w[:, d] != 0.0
            t = w[:, d] * v[..., pdofs[:, d]]
            acc = np.where(nz & first, t, np.where(nz, acc + t, acc))
            first &= ~nz
        val[..., j] = acc
    flat = fc2e.reshape(-1)                                             # fine cells ascend with their parent
    uniq, firsti = np.unique(flat, return_index=True)
    out = np.empty(v.shape[:-1] + (nvf + fedges.shape[0],))
    out[..., :nv] = v[..., :nv]
    out[..., nv:nvf] = v[..., nv + mid]
    out[..., nvf + uniq] = val.reshape(v.shape[:-1] + (-1,))[..., firsti]
    return out


# ---- meshes, masks and measures of the tests -------------------------------------------------------------------------
def kuhn_box(n):
    """n^3 cubes of side 1 split into 6 tetrahedra each (Kuhn): exact coordinates, so every length ties with many."""
    import itertools
    g = np.arange(n + 1, dtype=np.float64)
    Z, Y, X = np.meshgrid(g, g, g, indexing="ij")
    x = np.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], axis=1)
    s = np.array([1, n + 1, (n + 1) ** 2])
    cells = []
    for k in range(n):
        for j in range(n):
            for i in range(n):
                o = i + (n + 1) * (j + (n + 1) * k)
                for p in itertools.permutations(range(3)):
                    cells.append([o, o + s[p[0]], o + s[p[0]] + s[p[1]], o + s.sum()])
    return np.ascontiguousarray(x), np.array(cells, dtype=np.int64)


def nearest_mask(x, cells, point, fraction=0.1):
    """uint8 [nc]: the ceil(fraction nc) cells whose centroid is nearest `point` (stable argsort of the distance)."""
    cen = np.asarray(x)[np.asarray(cells)].mean(axis=1)
    d = ((cen - np.asarray(point, dtype=np.float64)) ** 2).sum(axis=1)
    k = int(np.ceil(fraction * len(d)))
    mask = np.zeros(len(d), dtype=np.uint8)
    mask[np.argsort(d, kind="stable")[:k]] = 1
    return mask


def seeded_mask(n, fraction=0.1, seed=0):
    mask = np.zeros(n, dtype=np.uint8)
    mask[np.random.default_rng(seed).permutation(n)[:int(np.ceil(fraction * n))]] = 1
    return mask


def signed_volumes(x, cells):
    x = np.asarray(x, dtype=np.float64)
    J = x[np.asarray(cells)[:, 1:]] - x[np.asarray(cells)[:, :1]]
    return np.linalg.det(J) / (2.0 if x.shape[1] == 2 else 6.0)


def facet_cell_counts(ctype, cells):
    """Number of cells at every facet of the mesh."""
    cells = np.asarray(cells, dtype=np.int64)
    nvpc = cells.shape[1]
    fv = np.stack([np.sort(np.delete(cells, k, axis=1), axis=1) for k in range(nvpc)], axis=1).reshape(-1, nvpc - 1)
    return np.unique(fv, axis=0, return_counts=True)[1]


def min_angle_deg(x, cells):
    x = np.asarray(x)
    p = x[np.asarray(cells)]
    best = np.inf
    for k in range(3):
        a, b = p[:, (k + 1) % 3] - p[:, k], p[:, (k + 2) % 3] - p[:, k]
        cos = (a * b).sum(axis=1) / np.sqrt((a * a).sum(axis=1) * (b * b).sum(axis=1))
        best = min(best, np.degrees(np.arccos(np.clip(cos, -1.0, 1.0))).min())
    return best


def tet_quality(x, cells):
    """min over the cells of |vol| / h^3 (h the longest edge), 1 for the regular tetrahedron."""
    x = np.asarray(x)
    p = x[np.asarray(cells)]
    h2 = np.zeros(len(p))
    for a, b in RR.LOCAL_PAIRS["tetrahedron"]:
        h2 = np.maximum(h2, ((p[:, a] - p[:, b]) ** 2).sum(axis=1))
    return (np.abs(signed_volumes(x, cells)) / h2 ** 1.5).min() / (np.sqrt(2.0) / 12.0)
