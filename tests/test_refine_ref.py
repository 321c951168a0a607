"""Properties of the numpy specification of uniform refinement (tests/refine_ref.py).  No GPU is touched."""
import numpy as np
import pytest

import partition_ref as PR
import refine_ref as RR
from datasets import load_mesh
from oracle import meshgen
from oracle.topology import Topology


def _mesh(name):
    if name == "graded_tet_box":
        x, cells = PR.graded_tet_box()
        return "tetrahedron", x, cells
    if name.startswith("single_"):
        ctype = name[len("single_"):]
        return (ctype,) + RR.single_cell(ctype)
    return load_mesh(name)


MESHES = ["disk", "square_tri", "coarse_square", "square_quad", "graded_tet_box", "single_triangle",
          "single_tetrahedron", "single_quadrilateral"]


@pytest.mark.parametrize("name", MESHES)
def test_refinement_is_conforming_and_counts(name):
    ctype, x, cells = _mesh(name)
    xf, cf = RR.refine_ref(ctype, x, cells)
    nv, nc = x.shape[0], cells.shape[0]
    topo = Topology(ctype, cells, nv)
    tf = Topology(ctype, cf, xf.shape[0])          # raises on a facet shared by more than two cells
    # every interior facet is shared by exactly two cells: the boundary facets are exactly the children of boundary
    # facets (x 2 in 2-D, x 4 in 3-D); a hanging node would leave more one-sided facets
    nb, nbf = int((topo.f2c[:, 1] < 0).sum()), int((tf.f2c[:, 1] < 0).sum())
    assert nbf == nb * (4 if ctype == "tetrahedron" else 2)
    assert np.all(np.bincount(tf.c2f.reshape(-1), minlength=tf.nf) == np.where(tf.f2c[:, 1] < 0, 1, 2))
    if ctype == "quadrilateral":
        assert xf.shape[0] == nv + topo.nf + nc
        assert tf.nf == 2 * topo.nf + 4 * nc
    else:
        ne = RR.edge_numbering(ctype, cells)[1].shape[0]
        assert xf.shape[0] == nv + ne
        assert tf.nf == (2 * topo.nf + 3 * nc if ctype == "triangle" else 4 * topo.nf + 8 * nc)
    assert cf.shape[0] == RR.child_table(ctype).shape[0] * nc
    v0, v1 = RR.cell_volumes(ctype, x, cells), RR.cell_volumes(ctype, xf, cf)
    assert np.all(v1 > 0)
    assert abs(v1.sum() - v0.sum()) <= 1e-13 * v0.sum()
    nchild = cf.shape[0] // nc
    assert np.allclose(v1.reshape(nc, nchild).sum(axis=1), v0, rtol=1e-12, atol=0)   # children tile their parent


def _cell_set(x, cells):
    return {tuple(sorted(map(tuple, x[c]))) for c in cells}


def test_bey_on_a_kuhn_box_is_the_kuhn_box_of_twice_the_resolution():
    lo, hi = [0.0, 0.0, 0.0], [1.0, 1.5, 0.5]          # dyadic spacings: the midpoints are the fine lattice exactly
    x, cells = meshgen.create_box(lo, hi, [2, 3, 2])
    xf, cf = RR.refine_ref("tetrahedron", x, cells)
    x2, c2 = meshgen.create_box(lo, hi, [4, 6, 4])
    assert _cell_set(xf, cf) == _cell_set(x2, c2)


def test_two_levels_compose():
    ctype, x, cells = load_mesh("coarse_square")
    x1, c1 = RR.refine_ref(ctype, x, cells)
    x2, c2 = RR.refine_ref(ctype, x1, c1)
    assert c2.shape[0] == 16 * cells.shape[0]
    # grandchildren of cell c are fine cells 16 c .. 16 c + 15 and tile it
    v0, v2 = RR.cell_volumes(ctype, x, cells), RR.cell_volumes(ctype, x2, c2)
    assert np.allclose(v2.reshape(-1, 16).sum(axis=1), v0, rtol=1e-12, atol=0)
    # the level-1 vertices keep their numbers and coordinates
    assert np.array_equal(x2[:x1.shape[0]], x1) and np.array_equal(x1[:x.shape[0]], x)
    Topology(ctype, c2, x2.shape[0])


@pytest.mark.parametrize("ctype", ["triangle", "tetrahedron"])
def test_weight_table_values_and_patterns(ctype):
    W = RR.p2_weight_table(ctype)
    from fractions import Fraction as F
    assert set(W.reshape(-1)) <= {F(0), F(-1, 8), F(1, 4), F(3, 8), F(1, 2), F(3, 4)}
    assert all(sum(row) == 1 for row in W.reshape(-1, W.shape[2]))
    pats = {tuple(sorted(row)) for row in W.reshape(-1, W.shape[2])}
    n0 = W.shape[2]
    half = tuple(sorted([F(3, 8), F(3, 4), F(-1, 8)] + [F(0)] * (n0 - 3)))
    seg = tuple(sorted([F(1, 2), F(1, 2), F(1, 4), F(-1, 8), F(-1, 8)] + [F(0)] * (n0 - 5)))
    diag = tuple(sorted([F(1, 4)] * 6 + [F(-1, 8)] * 4))
    assert pats == ({half, seg} if ctype == "triangle" else {half, seg, diag})


@pytest.mark.parametrize("name", ["disk", "graded_tet_box", "square_quad"])
def test_prolongation_reproduces_polynomials(name):
    ctype, x, cells = _mesh(name)
    xf, cf = RR.refine_ref(ctype, x, cells)
    d = x.shape[1]
    lin = lambda p: 0.3 + p @ np.arange(1.0, d + 1.0)                              # noqa: E731
    got = RR.prolongate_ref(ctype, x, cells, lin(x), 1)
    assert np.abs(got - lin(xf)).max() <= 16 * np.finfo(float).eps * np.abs(lin(xf)).max()
    assert np.array_equal(RR.prolongate_ref(ctype, x, cells, x.T, 1), xf.T)
    if ctype == "quadrilateral":
        return
    quad = lambda p: 0.2 + p[:, 0] * p[:, -1] - 0.7 * p[:, 0] ** 2 + p.sum(axis=1)  # noqa: E731
    _, e = RR.edge_numbering(ctype, cells)
    _, ef = RR.edge_numbering(ctype, cf)
    p2 = np.concatenate([x, 0.5 * x[e[:, 0]] + 0.5 * x[e[:, 1]]])
    p2f = np.concatenate([xf, 0.5 * xf[ef[:, 0]] + 0.5 * xf[ef[:, 1]]])
    got = RR.prolongate_ref(ctype, x, cells, quad(p2), 2)
    assert np.abs(got - quad(p2f)).max() <= 64 * np.finfo(float).eps * np.abs(quad(p2)).max()
