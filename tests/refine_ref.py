"""Specification of uniform refinement and the nested coarse -> fine transfer (TEST INFRASTRUCTURE): numpy restatements
that the device code of phifem_amd/csrc/phx_refine.inc.hip has to equal -- bit for bit for the meshes and the degree-1
transfer, to round-off for degree 2.

  child_table / p2_weight_table   the tables of phx_refine_tables, derived from the rule written with vertex pairs and
                                  from barycentric coordinates (exact rationals)
  refine_ref                      (x, cells) -> (fine x, fine cells)
  prolongate_ref                  nodal values on the coarse mesh -> nodal values on the fine mesh

The rules:
  * local degree-2 node d of a cell: d < nvpc its vertex d; nvpc + k its local edge k (simplices, basix order) or
    local facet k (quadrilaterals); last the quadrilateral's centre;
  * edges of a simplicial mesh are numbered by ascending sorted vertex pair (what PHX_ARR_EDGES documents for
    caller-supplied meshes; a generated box numbers them in closed form -- pass its `edges` array), the facets of a
    quadrilateral mesh as oracle.topology.Topology numbers them;
  * fine vertices: coarse vertices, then 0.5 x_p + 0.5 x_q per edge / facet (p, q), then ((x0/4 + x1/4) + x2/4) + x3/4
    per quadrilateral;
  * child k of cell c is fine cell nchild c + k, its vertices the rule below;
  * degree-2 transfer: a fine edge DoF is the parent's P2 function at the fine edge's midpoint, summed over the parent's
    local DoFs in ascending local order without the zero weights; the lowest-numbered parent cell of the edge decides.
"""
from fractions import Fraction

import numpy as np

from oracle.topology import Topology

# local vertex pairs of the local edges (basix) / of a quadrilateral's local facets
LOCAL_PAIRS = {
    "triangle": [(1, 2), (0, 2), (0, 1)],
    "tetrahedron": [(2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1)],
    "quadrilateral": [(0, 1), (0, 2), (1, 3), (2, 3)],
}
# children as the issue writes them: "i" = vertex v_i, "ij" = midpoint m_ij, "c" = the quadrilateral's centre
RULE = {
    "triangle": ["0 01 02", "01 1 12", "02 12 2", "12 02 01"],
    "tetrahedron": ["0 01 02 03", "01 1 12 13", "02 12 2 23", "03 13 23 3",
                    "01 02 03 13", "01 02 12 13", "02 03 13 23", "02 12 13 23"],
    # b = m01, l = m02, r = m13, t = m23
    "quadrilateral": ["0 01 02 c", "01 1 c 13", "02 c 2 23", "c 13 23 3"],
}
NVPC = {"triangle": 3, "tetrahedron": 4, "quadrilateral": 4}


def child_table(ctype):
    """(nchild, nvpc) local degree-2 node of every child vertex."""
    nvpc, pairs = NVPC[ctype], LOCAL_PAIRS[ctype]

    def node(tok):
        if tok == "c":
            return nvpc + len(pairs)
        if len(tok) == 1:
            return int(tok)
        return nvpc + pairs.index((int(tok[0]), int(tok[1])))
    return np.array([[node(t) for t in row.split()] for row in RULE[ctype]], dtype=np.int32)


def _node_barycentric(ctype, d):
    nvpc = NVPC[ctype]
    lam = [Fraction(0)] * nvpc
    if d < nvpc:
        lam[d] = Fraction(1)
    else:
        a, b = LOCAL_PAIRS[ctype][d - nvpc]
        lam[a] = lam[b] = Fraction(1, 2)
    return lam


def p2_basis(ctype, lam):
    """The P2 basis (vertices, then edges in basix order) at the barycentric point lam."""
    nvpc = NVPC[ctype]
    return [l * (2 * l - 1) for l in lam] + [4 * lam[a] * lam[b] for a, b in LOCAL_PAIRS[ctype]]


def p2_weight_table(ctype):
    """(nchild, nepc, ndof2) Fractions: weight of parent DoF d at the midpoint of child k's local edge j."""
    assert ctype != "quadrilateral"
    ch = child_table(ctype)
    out = []
    for k in range(ch.shape[0]):
        rows = []
        for a, b in LOCAL_PAIRS[ctype]:
            la, lb = _node_barycentric(ctype, ch[k, a]), _node_barycentric(ctype, ch[k, b])
            rows.append(p2_basis(ctype, [(p + q) / 2 for p, q in zip(la, lb)]))
        out.append(rows)
    return np.array(out, dtype=object)


def edge_numbering(ctype, cells, edges=None):
    """-> (c2e [nc, nepc], edges [ne, 2] ascending pairs).  edges=None: numbered by ascending sorted pair."""
    cells = np.asarray(cells, dtype=np.int64)
    lp = np.array(LOCAL_PAIRS[ctype])
    pr = np.sort(cells[:, lp], axis=2).reshape(-1, 2)            # (nc * nepc, 2)
    if edges is None:
        edges, inv = np.unique(pr, axis=0, return_inverse=True)
        return inv.reshape(cells.shape[0], len(lp)), edges
    edges = np.asarray(edges, dtype=np.int64)
    big = int(max(cells.max(), edges.max())) + 1
    key = edges[:, 0] * big + edges[:, 1]
    order = np.argsort(key)
    pos = np.searchsorted(key[order], pr[:, 0] * big + pr[:, 1])
    assert np.array_equal(key[order][pos], pr[:, 0] * big + pr[:, 1])
    return order[pos].reshape(cells.shape[0], len(lp)), edges


def _mid_entities(ctype, x, cells, edges=None):
    """-> (c2m [nc, nmid], pairs [nmid_global, 2])."""
    if ctype != "quadrilateral":
        return edge_numbering(ctype, cells, edges)
    cells = np.asarray(cells, dtype=np.int64)
    topo = Topology(ctype, cells, np.asarray(x).shape[0])
    pairs = np.empty((topo.nf, 2), dtype=np.int64)
    for lf, (a, b) in enumerate(LOCAL_PAIRS[ctype]):
        pairs[topo.c2f[:, lf]] = cells[:, [a, b]]
    return np.asarray(topo.c2f, dtype=np.int64), pairs


def cell_nodes(ctype, x, cells, edges=None):
    """(nc, ndof2) fine-vertex id (= global degree-2 DoF) of every local node, and the pairs of the mid entities."""
    cells = np.asarray(cells, dtype=np.int64)
    nv = np.asarray(x).shape[0]
    c2m, pairs = _mid_entities(ctype, x, cells, edges)
    cols = [cells, nv + c2m]
    if ctype == "quadrilateral":
        cols.append((nv + pairs.shape[0] + np.arange(cells.shape[0]))[:, None])
    return np.concatenate(cols, axis=1), pairs


def refine_ref(ctype, x, cells, edges=None):
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    nodes, pairs = cell_nodes(ctype, x, cells, edges)
    parts = [x, 0.5 * x[pairs[:, 0]] + 0.5 * x[pairs[:, 1]]]
    if ctype == "quadrilateral":
        xc = x[cells]
        parts.append(((0.25 * xc[:, 0] + 0.25 * xc[:, 1]) + 0.25 * xc[:, 2]) + 0.25 * xc[:, 3])
    ch = child_table(ctype)
    fine = nodes[:, ch].reshape(cells.shape[0] * ch.shape[0], ch.shape[1])
    return np.ascontiguousarray(np.concatenate(parts, axis=0)), np.ascontiguousarray(fine)


def prolongate_ref(ctype, x, cells, values, degree=1, edges=None):
    """values (ndofs,) or (ncomp, ndofs) on the coarse mesh -> the same on refine_ref's fine mesh (whose edges are
    numbered by ascending sorted pair)."""
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    v = np.asarray(values, dtype=np.float64)
    nodes, pairs = cell_nodes(ctype, x, cells, edges)
    nv = x.shape[0]
    if degree == 1:
        assert v.shape[-1] == nv
        parts = [v, 0.5 * v[..., pairs[:, 0]] + 0.5 * v[..., pairs[:, 1]]]
        if ctype == "quadrilateral":
            vc = v[..., cells]
            parts.append(((0.25 * vc[..., 0] + 0.25 * vc[..., 1]) + 0.25 * vc[..., 2]) + 0.25 * vc[..., 3])
        return np.concatenate(parts, axis=-1)
    if degree != 2 or ctype == "quadrilateral":
        raise NotImplementedError
    assert v.shape[-1] == nv + pairs.shape[0]
    xf, fine = refine_ref(ctype, x, cells, edges)
    fc2e, fedges = edge_numbering(ctype, fine)
    W = p2_weight_table(ctype)
    nchild, nepc, ndof2 = W.shape
    nc = cells.shape[0]
    val = np.zeros(v.shape[:-1] + (nc, nchild, nepc))
    for k in range(nchild):
        for j in range(nepc):
            acc = None
            for d in range(ndof2):
                if W[k, j, d] == 0:
                    continue
                t = float(W[k, j, d]) * v[..., nodes[:, d]]
                acc = t if acc is None else acc + t
            val[..., :, k, j] = acc
    flat = fc2e.reshape(-1)                                    # fine cells ascend with their parent
    uniq, first = np.unique(flat, return_index=True)
    out = np.empty(v.shape[:-1] + (xf.shape[0] + fedges.shape[0],))
    out[..., :xf.shape[0]] = v
    out[..., xf.shape[0] + uniq] = val.reshape(v.shape[:-1] + (-1,))[..., first]
    return out


# ---- measures used by the property tests ---------------------------------------------------------------------------
def cell_volumes(ctype, x, cells):
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells)
    if ctype == "quadrilateral":      # two triangles (v0, v1, v3), (v0, v3, v2)
        return cell_volumes("triangle", x, cells[:, [0, 1, 3]]) + cell_volumes("triangle", x, cells[:, [0, 3, 2]])
    d = x.shape[1]
    J = x[cells[:, 1:]] - x[cells[:, :1]]
    return np.abs(np.linalg.det(J)) / (2.0 if d == 2 else 6.0)


def single_cell(ctype):
    if ctype == "triangle":
        return np.array([[0.1, 0.0], [1.3, 0.2], [0.4, 0.9]]), np.array([[0, 1, 2]])
    if ctype == "quadrilateral":
        return np.array([[0.0, 0.0], [1.5, 0.0], [0.0, 0.7], [1.5, 0.7]]), np.array([[0, 1, 2, 3]])
    return (np.array([[0.0, 0.1, 0.0], [1.1, 0.0, 0.2], [0.3, 0.9, 0.1], [0.2, 0.3, 1.2]]), np.array([[0, 1, 2, 3]]))
