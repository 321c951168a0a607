"""The numpy specification of point location and evaluation (tests/locate_ref.py) against analytic cases.  No GPU."""
import numpy as np
import pytest

import locate_cases as LC
import locate_ref as LR
import refine_ref as RR

SINGLE = {
    "triangle": (np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 1.0]]), np.array([[0, 1, 2]])),
    "tetrahedron": (np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 4.0]]), np.array([[0, 1, 2, 3]])),
    "quadrilateral": (np.array([[1.0, -1.0], [3.0, -1.0], [1.0, 0.0], [3.0, 0.0]]), np.array([[0, 1, 2, 3]])),
}


def test_single_triangle():
    x, cells = SINGLE["triangle"]
    pts = np.array([[0.5, 0.25], [2.0, 0.0], [1.0, 0.5], [1.0, 0.5 + 1e-6], [-1e-6, 0.2], [0.0, 0.2]])
    cell, xref, holds = LR.locate_ref("triangle", x, cells, pts)
    assert cell.tolist() == [0, 0, 0, -1, -1, 0]
    assert np.allclose(xref[:3], [[0.25, 0.25], [1.0, 0.0], [0.5, 0.5]], atol=1e-15)      # lambda_1 = x / 2, lambda_2 = y
    assert LR.input_condition("triangle", x, cells, pts)
    assert not LR.input_condition("triangle", x, cells, np.array([[0.5, -1e-11]]))        # sits at the tolerance


def test_single_tetrahedron():
    x, cells = SINGLE["tetrahedron"]
    pts = np.array([[0.5, 0.25, 1.0], [0.0, 0.0, 4.0], [1.0, 0.5, 0.1], [0.1, 0.1, -1e-5]])
    cell, xref, _ = LR.locate_ref("tetrahedron", x, cells, pts)
    assert cell.tolist() == [0, 0, -1, -1]
    assert np.allclose(xref[:2], [[0.25, 0.25, 0.25], [0.0, 0.0, 1.0]], atol=1e-15)


def test_single_rectangle():
    x, cells = SINGLE["quadrilateral"]
    pts = np.array([[1.5, -0.75], [3.0, 0.0], [3.0 + 1e-6, -0.5], [2.0, 1e-6], [1.0, -1.0]])
    cell, xref, _ = LR.locate_ref("quadrilateral", x, cells, pts)
    assert cell.tolist() == [0, 0, -1, -1, 0]
    assert np.allclose(xref[[0, 1, 4]], [[0.25, 0.25], [1.0, 1.0], [0.0, 0.0]], atol=1e-15)


def test_smallest_index_wins():
    x = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    cells = np.array([[1, 3, 2], [0, 1, 2]])
    cell, _, holds = LR.locate_ref("triangle", x, cells, np.array([[0.5, 0.5], [0.2, 0.2], [0.8, 0.8], [1.0, 0.0]]))
    assert cell.tolist() == [0, 1, 0, 0] and holds[0].all() and holds[3].all()


def _rand_points(ctype, n=40, seed=3):
    rng = np.random.default_rng(seed)
    d = 3 if ctype == "tetrahedron" else 2
    if ctype == "quadrilateral":
        return rng.random((n, d))
    lam = rng.dirichlet(np.ones(d + 1), size=n)
    return lam[:, 1:]


@pytest.mark.parametrize("ctype,degree", [("triangle", 1), ("triangle", 2), ("tetrahedron", 1), ("tetrahedron", 2),
                                          ("quadrilateral", 1)])
def test_partition_of_unity_and_nodal_property(ctype, degree):
    xref = _rand_points(ctype)
    N, dN = LR.basis(ctype, degree, xref)
    assert np.abs(N.sum(axis=1) - 1.0).max() < 1e-14 and np.abs(dN.sum(axis=1)).max() < 1e-13
    # N_i = 1 at node i, 0 at the others
    d = xref.shape[1]
    if ctype == "quadrilateral":
        nodes = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    else:
        verts = np.concatenate([np.zeros((1, d)), np.eye(d)], axis=0)
        nodes = verts if degree == 1 else np.concatenate(
            [verts, [0.5 * (verts[a] + verts[b]) for a, b in LR.LOCAL_PAIRS[ctype]]], axis=0)
    assert np.array_equal(LR.basis(ctype, degree, nodes)[0], np.eye(nodes.shape[0]))
    # reference gradients against central differences
    e = 1e-6
    for i in range(d):
        step = np.zeros(d)
        step[i] = e
        fd = (LR.basis(ctype, degree, xref + step)[0] - LR.basis(ctype, degree, xref - step)[0]) / (2 * e)
        assert np.abs(fd - dN[:, :, i]).max() < 1e-8


def _poly(p, degree):
    lin = 0.3 + p @ np.arange(1, p.shape[1] + 1) * 0.7
    return lin if degree == 1 else lin + p[:, 0] * p[:, -1] - 0.4 * p[:, 0] ** 2 + 0.9 * p[:, -1] ** 2


def _poly_grad(p, degree):
    g = np.tile(np.arange(1, p.shape[1] + 1) * 0.7, (p.shape[0], 1))
    if degree == 2:
        g[:, 0] += p[:, -1] - 0.8 * p[:, 0]
        g[:, -1] += p[:, 0] + 1.8 * p[:, -1]
    return g


@pytest.mark.parametrize("ctype,degree", [("triangle", 1), ("triangle", 2), ("tetrahedron", 1), ("tetrahedron", 2),
                                          ("quadrilateral", 1)])
def test_polynomial_reproduction(ctype, degree):
    """P1 reproduces linear functions, P2 quadratics, Q1 bilinear ones -- values and gradients -- on a refined cell."""
    x, cells = RR.refine_ref(ctype, *SINGLE[ctype])
    c2e = None
    if degree == 2:
        c2e, edges = RR.edge_numbering(ctype, cells)
        nodes = np.concatenate([x, 0.5 * (x[edges[:, 0]] + x[edges[:, 1]])], axis=0)
    else:
        nodes = x
    f = (lambda p: _poly(p, degree)) if ctype != "quadrilateral" else (lambda p: 0.3 + p[:, 0] - 2.0 * p[:, 1] + 0.6 * p[:, 0] * p[:, 1])
    rng = np.random.default_rng(5)
    lo, hi = x.min(axis=0), x.max(axis=0)
    pts = lo + (hi - lo) * (rng.random((200, x.shape[1])) * 1.2 - 0.1)
    cell, xref, _ = LR.locate_ref(ctype, x, cells, pts)
    assert (cell >= 0).sum() > 10 and (cell < 0).sum() > 5
    vals = np.stack([f(nodes), 2.0 * f(nodes)])
    out, grad = LR.evaluate_ref(ctype, x, cells, vals, cell, xref, degree, c2e, fill=-7.0)
    ok = cell >= 0
    assert np.abs(out[0, ok] - f(pts[ok])).max() < 1e-13 and np.array_equal(out[1, ok], 2.0 * out[0, ok])
    assert np.all(out[:, ~ok] == -7.0) and np.all(grad[:, ~ok] == -7.0)
    if ctype == "quadrilateral":
        gex = np.stack([1.0 + 0.6 * pts[:, 1], -2.0 + 0.6 * pts[:, 0]], axis=1)
    else:
        gex = _poly_grad(pts, degree)
    assert np.abs(grad[0, ok] - gex[ok]).max() < 1e-12
    # the reconstruction of the point from the P1 / Q1 basis at xref
    N, _ = LR.basis(ctype, 1, xref[ok])
    assert np.abs(np.einsum("pk,pka->pa", N, x[cells[cell[ok]]]) - pts[ok]).max() < 1e-14
    one, _ = LR.evaluate_ref(ctype, x, cells, vals[0], cell, xref, degree, c2e)
    assert one.shape == (200,) and np.abs(one[ok] - out[0, ok]).max() < 1e-14 and np.all(np.isnan(one[~ok]))


@pytest.mark.parametrize("name", LC.CALLER + ["box_3d", "box_2d"])
def test_input_condition(name):
    """The input condition of tests/test_hip_evaluate.py, from the reference alone: for the centroids, vertices, edge
    midpoints and the random cloud of every test mesh the smallest coordinate of every (point, cell) pair is >= -1e-14
    or <= -1e-9, and the cloud has points inside and outside.

    On hub_3d two edge midpoints as 0.5 (x_a + x_b) rounds them miss it with three sliver cells (smallest height 3.4e-3:
    smallest coordinates -1.14e-14, -1.14e-14 and -1.86e-14); `locate_cases.settle_points` takes the neighbouring
    float64 point one ulp away that meets it, and only those two points move."""
    if name in LC.CALLER:
        pts, ncen, cell, _, _, cond = LC.reference_caller(name)
    else:
        ctype, x, cells = LC.generated_box_arrays(3 if name == "box_3d" else 2)
        pts, ncen = LC.case_points(ctype, x, cells, lattice=True)
        cell = LR.locate_ref(ctype, x, cells, pts)[0]
        cond = LR.input_condition(ctype, x, cells, pts)
    assert np.array_equal(cell[:ncen], np.arange(ncen))
    assert (cell < 0).sum() > 10 and (cell[ncen:] >= 0).sum() > 10
    assert cond
    if name in LC.CALLER:
        ctype, x, cells = LC.arrays(name)
        raw = LC.case_points(ctype, x, cells)[0]
        moved = np.flatnonzero(np.any(raw != pts, axis=1))
        assert moved.size == (2 if name == "hub_3d" else 0)
        assert np.all(np.abs(raw[moved] - pts[moved]) <= np.spacing(np.abs(raw[moved])))
