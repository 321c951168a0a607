"""CPU-only checks of the Lagrange reference elements of degree 1-3 behind `NodalFunction` / `interpolate`
(phx_lagrange_nodes, phx_lagrange_tabulate): basix's GLL-warped P3 / Q3 nodes, the Kronecker property, partition of
unity, reproduction of every cubic (bicubic) monomial, and the degree-1/2 tables bit for bit equal to those the
tagging path already uses.  No GPU is touched."""
import ctypes as C
import itertools

import numpy as np
import pytest

CELLS = ["triangle", "quadrilateral", "tetrahedron"]
TDIM = {"triangle": 2, "quadrilateral": 2, "tetrahedron": 3}
NDOF = {("triangle", 1): 3, ("triangle", 2): 6, ("triangle", 3): 10,
        ("quadrilateral", 1): 4, ("quadrilateral", 2): 9, ("quadrilateral", 3): 16,
        ("tetrahedron", 1): 4, ("tetrahedron", 2): 10, ("tetrahedron", 3): 20}
A = (1.0 - 1.0 / np.sqrt(5.0)) / 2.0        # interior 4-point Gauss-Lobatto-Legendre nodes on [0, 1]
B = (1.0 + 1.0 / np.sqrt(5.0)) / 2.0


def nodes(ctype, deg):
    from phifem_amd import _lib as L
    n = C.c_int64(0)
    L.check(L.lib.phx_lagrange_nodes(L.CELL_TYPES[ctype], deg, None, C.byref(n)))
    out = np.empty((n.value, TDIM[ctype]))
    L.check(L.lib.phx_lagrange_nodes(L.CELL_TYPES[ctype], deg, out.ctypes.data_as(C.c_void_p), C.byref(n)))
    return out


def tabulate(ctype, deg, pts):
    from phifem_amd import _lib as L
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    out = np.empty((pts.shape[0], NDOF[(ctype, deg)]))
    L.check(L.lib.phx_lagrange_tabulate(L.CELL_TYPES[ctype], deg, pts.shape[0], pts.ctypes.data_as(C.c_void_p),
                                        out.ctypes.data_as(C.c_void_p)))
    return out


def expected_nodes(ctype, deg):
    """basix's gll_warped Lagrange nodes in basix's local order, written out."""
    if ctype == "quadrilateral":
        t = {1: [0.0, 1.0], 2: [0.0, 0.5, 1.0], 3: [0.0, A, B, 1.0]}[deg]
        k = deg
        idx = [(0, 0), (k, 0), (0, k), (k, k)]
        for a, b in [(0, 1), (0, 2), (1, 3), (2, 3)]:              # local facets, first -> second vertex
            for j in range(1, k):
                pa, pb = idx[a], idx[b]
                idx.append(tuple(pa[c] if pa[c] == pb[c] else (j if pb[c] > pa[c] else k - j) for c in range(2)))
        idx += [(i, j) for j in range(1, k) for i in range(1, k)]   # interior, x fastest
        return np.array([[t[i], t[j]] for i, j in idx])
    d = TDIM[ctype]
    v = np.vstack([np.zeros(d), np.eye(d)])
    edges = [(1, 2), (0, 2), (0, 1)] if d == 2 else [(2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1)]
    s = {1: [], 2: [0.5], 3: [A, B]}[deg]
    pts = list(v)
    for a, b in edges:
        for sj in s:
            pts.append(np.where(v[b] > v[a], sj, np.where(v[a] > v[b], 1.0 - sj, 0.0)))
    if deg == 3:
        if d == 2:
            pts.append(np.array([1.0 / 3.0, 1.0 / 3.0]))
        else:
            for f in range(4):
                pts.append(v[[c for c in range(4) if c != f]].sum(axis=0) / 3.0)
    return np.array(pts)


def random_points(ctype, n, seed=0):
    rng = np.random.default_rng(seed)
    p = rng.random((4 * n, TDIM[ctype]))
    if ctype != "quadrilateral":
        p = p[p.sum(axis=1) <= 1.0]
    return p[:n]


def monomials(ctype, deg):
    d = TDIM[ctype]
    exps = itertools.product(range(deg + 1), repeat=d)
    if ctype == "quadrilateral":
        return list(exps)
    return [e for e in exps if sum(e) <= deg]


@pytest.mark.parametrize("ctype", CELLS)
@pytest.mark.parametrize("deg", [1, 2, 3])
def test_nodes_are_the_gll_warped_lattice(ctype, deg):
    got, want = nodes(ctype, deg), expected_nodes(ctype, deg)
    assert got.shape == (NDOF[(ctype, deg)], TDIM[ctype])
    assert np.all(np.abs(got - want) <= np.spacing(np.maximum(np.abs(want), 1e-300)))   # within 1 ulp


def test_p3_edge_nodes_are_not_equispaced():
    x = nodes("triangle", 3)
    assert np.isclose(x[7, 0], A) and not np.isclose(x[7, 0], 1.0 / 3.0)   # edge (0,1), node nearer vertex 0


@pytest.mark.parametrize("ctype", CELLS)
@pytest.mark.parametrize("deg", [1, 2, 3])
def test_tabulation_is_a_lagrange_basis(ctype, deg):
    x = nodes(ctype, deg)
    T = tabulate(ctype, deg, x)
    assert np.abs(T - np.eye(x.shape[0])).max() <= 1e-14
    p = random_points(ctype, 200, seed=deg)
    Tp = tabulate(ctype, deg, p)
    assert np.abs(Tp.sum(axis=1) - 1.0).max() <= 1e-13
    for e in monomials(ctype, deg):
        at_nodes = np.prod(x ** np.array(e), axis=1)
        at_pts = np.prod(p ** np.array(e), axis=1)
        assert np.abs(Tp @ at_nodes - at_pts).max() <= 1e-13, e


@pytest.mark.parametrize("ctype", CELLS)
def test_cubic_tables_do_not_reproduce_quartics(ctype):
    """A guard on the monomial check: the space is exactly (bi)cubic."""
    p = random_points(ctype, 100)
    x = nodes(ctype, 3)
    e = (4, 0) if TDIM[ctype] == 2 else (4, 0, 0)
    err = tabulate(ctype, 3, p) @ np.prod(x ** np.array(e), axis=1) - np.prod(p ** np.array(e), axis=1)
    assert np.abs(err).max() > 1e-4


@pytest.mark.parametrize("ctype", CELLS)
def test_degree_one_and_two_tables_are_the_tagging_tables(ctype):
    from phifem_amd.mesh_scripts import _p2_tab, _q2_tab, _ref_points, _shape
    for det in (0, 1, 2, 3, 4):
        p = np.ascontiguousarray(_ref_points(ctype, det, 0))
        assert np.array_equal(tabulate(ctype, 1, p), _shape(ctype, p))
        want2 = _q2_tab(p) if ctype == "quadrilateral" else _p2_tab(ctype, _shape(ctype, p))
        assert np.array_equal(tabulate(ctype, 2, p), want2)


def test_bad_cell_type_and_degree_are_rejected():
    from phifem_amd import _lib as L
    n = C.c_int64(0)
    with pytest.raises(NotImplementedError):
        L.check(L.lib.phx_lagrange_nodes(7, 3, None, C.byref(n)))
    for deg in (0, 4):
        with pytest.raises(NotImplementedError):
            L.check(L.lib.phx_lagrange_nodes(L.TRIANGLE, deg, None, C.byref(n)))
    pts = np.zeros((1, 2))
    out = np.empty(32)
    with pytest.raises(NotImplementedError):
        L.check(L.lib.phx_lagrange_tabulate(L.QUADRILATERAL, 4, 1, pts.ctypes.data_as(C.c_void_p),
                                            out.ctypes.data_as(C.c_void_p)))


def test_nodal_function_degrees():
    from phifem_amd import NodalFunction, interpolate
    assert NodalFunction(np.zeros(3), degree=3).degree == 3
    with pytest.raises(NotImplementedError):
        NodalFunction(np.zeros(3), degree=4)
    with pytest.raises(NotImplementedError):
        interpolate(None, lambda x: x[0], 4)
