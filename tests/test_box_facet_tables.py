"""Facet-class tables of a Kuhn box (phx_box_facet_tables, the tables behind PHX_OPT_BOX_FACET_ROWS) against a numpy
restatement.  No GPU is touched.

The restatement starts from the generator's rule alone -- simplex t of a cube walks o, o + e_p0, o + e_p0 + e_p1, ... for
the t-th lexicographic axis permutation p, local facet m lies opposite path vertex m, and its type and anchor are what
k_box_cells writes into c2f -- finds the two cells of every facet type among the cubes around the anchor (the cell with
the lower id first, as k_box_f2c lists them), and evaluates facet_macro's formulas on them: gradients of the
barycentric coordinates, J_j = -(g_j . g_lf) / |g_lf| per side, a shared vertex carrying both, w = sigma avg(h) |F| with
|F| = D |K| |g_lf| and h the longest edge.  Offsets and cells must be equal, J and w equal to 1e-14 relative, and an entry
that vanishes in exact arithmetic (decided with rationals) must be exactly 0.0."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

SIGMA = 20.0
SPACINGS = {
    3: [(0.25, 0.25, 0.25), (0.3, 0.2, 0.4)],
    2: [(0.25, 0.25), (0.3, 0.2)],
}
CASES = [(d, h) for d in (3, 2) for h in SPACINGS[d]]


def perms(d):
    return list(itertools.permutations(range(d)))      # lexicographic: the generator's table


def path(d, p, cube):
    v = [np.array(cube, dtype=int)]
    for a in p:
        w = v[-1].copy()
        w[a] += 1
        v.append(w)
    return v


def facet_of(d, p, m):
    """(type, anchor shift from the cell's cube) of local facet m of the simplex of permutation p (k_box_cells)."""
    shift = np.zeros(d, dtype=int)
    if d == 3:
        if m == 0:
            shift[p[0]] = 1
            return p[0] * 2 + (1 if p[1] > p[2] else 0), shift
        if m == 3:
            return p[2] * 2 + (1 if p[0] > p[1] else 0), shift
        return (6 + p[2], shift) if m == 1 else (9 + p[0], shift)
    if m == 0:
        shift[p[0]] = 1
        return p[0], shift
    return (p[1], shift) if m == 2 else (2, shift)


def macro_elements(d):
    """per type: [(cube offset from the anchor, permutation index, local facet)] of its two cells, lower cell id first"""
    nt = 12 if d == 3 else 3
    inc = [[] for _ in range(nt)]
    for cube in itertools.product((-1, 0), repeat=d):
        for t, p in enumerate(perms(d)):
            for m in range(d + 1):
                ftype, shift = facet_of(d, p, m)
                if np.array_equal(np.array(cube) + shift, np.zeros(d, dtype=int)):      # anchored at the origin
                    inc[ftype].append((cube, t, m))
    for lst in inc:
        assert len(lst) == 2                                                            # an interior facet
        lst.sort(key=lambda e: (tuple(reversed(e[0])), e[1]))                           # cube index (x fastest), then t
    return inc


def geometry(X):
    """gradients of the barycentric coordinates, volume and diameter of the simplex with vertex rows X"""
    n = X.shape[0]
    T = np.hstack([np.ones((n, 1), dtype=X.dtype), X])
    if X.dtype == object:
        g = inverse_exact(T)[1:, :].T
        return g, None, None
    g = np.linalg.inv(T)[1:, :].T
    vol = abs(np.linalg.det(X[1:] - X[0])) / (6.0 if n == 4 else 2.0)
    h = max(np.linalg.norm(X[i] - X[j]) for i in range(n) for j in range(i + 1, n))
    return g, vol, h


def inverse_exact(T):
    n = T.shape[0]
    A = [[Fraction(T[i][j]) for j in range(n)] + [Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for c in range(n):
        piv = next(r for r in range(c, n) if A[r][c] != 0)
        A[c], A[piv] = A[piv], A[c]
        A[c] = [x / A[c][c] for x in A[c]]
        for r in range(n):
            if r != c and A[r][c] != 0:
                A[r] = [x - A[r][c] * y for x, y in zip(A[r], A[c])]
    return np.array([row[n:] for row in A], dtype=object)


def reference(d, h):
    nt = 12 if d == 3 else 3
    pm = perms(d)
    cells = np.zeros((nt, 2), dtype=np.int32)
    offs = np.zeros((nt, d + 2, d), dtype=np.int32)
    J = np.zeros((nt, d + 2))
    w = np.zeros(nt)
    zero = np.zeros((nt, d + 2), dtype=bool)
    hx = [Fraction(v) for v in h]                     # the doubles the library is given, exactly
    for t, pair in enumerate(macro_elements(d)):
        side = []
        for cube, p, lf in pair:
            V = path(d, pm[p], cube)
            X = np.array([[v[a] * h[a] for a in range(d)] for v in V])
            g, vol, diam = geometry(X)
            gn = np.linalg.norm(g[lf])
            Xq = np.array([[int(v[a]) * hx[a] for a in range(d)] for v in V], dtype=object)
            gq, _, _ = geometry(Xq)
            side.append(dict(V=V, lf=lf, J=-(g @ g[lf]) / gn, area=d * vol * gn, h=diam,
                             sq=[-sum(gq[j][a] * gq[lf][a] for a in range(d)) for j in range(d + 1)],
                             gn2=sum(gq[lf][a] ** 2 for a in range(d))))
        A, B = side
        assert A["gn2"] == B["gn2"]      # the two cells are equally high over the facet: the one-sided terms share |g_lf|
        cells[t] = [pair[0][1], pair[1][1]]
        exact = list(A["sq"]) + [B["sq"][B["lf"]]]
        for l in range(d + 1):
            offs[t, l] = A["V"][l]
            J[t, l] = A["J"][l]
        offs[t, d + 1] = B["V"][B["lf"]]
        J[t, d + 1] = B["J"][B["lf"]]
        for j in range(d + 1):
            if j == B["lf"]:
                continue
            q = next(q for q in range(d + 1) if np.array_equal(A["V"][q], B["V"][j]))
            J[t, q] += B["J"][j]
            exact[q] += B["sq"][j]
        zero[t] = [e == 0 for e in exact]
        w[t] = SIGMA * 0.5 * (A["h"] + B["h"]) * A["area"]
    return cells, offs, J, w, zero


def tables(d, h):
    from phifem_amd import _lib as L
    nt = C.c_int(0)
    cells = np.full((12, 2), -7, dtype=np.int32)
    offs = np.full((12, d + 2, d), -7, dtype=np.int32)
    J = np.full((12, d + 2), np.nan)
    w = np.full(12, np.nan)
    hh = np.array(list(h) + [0.0] * (3 - d))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    L.check(L.lib.phx_box_facet_tables(d, vp(hh), SIGMA, C.byref(nt), vp(cells), vp(offs), vp(J), vp(w)))
    n = nt.value
    assert n == (12 if d == 3 else 3)
    assert np.all(cells[n:] == -7) and np.all(offs[n:] == -7) and np.all(np.isnan(J[n:])) and np.all(np.isnan(w[n:]))
    return cells[:n], offs[:n], J[:n], w[:n]


@pytest.mark.parametrize("d,h", CASES)
def test_tables_equal_the_restated_macro_elements(d, h):
    cells, offs, J, w = tables(d, h)
    rc, ro, rJ, rw, zero = reference(d, h)
    assert np.array_equal(cells, rc)
    assert np.array_equal(offs, ro)
    assert np.all(J[zero] == 0.0) and not np.any(np.signbit(J[zero]))       # exact zeros, and no negative zero
    assert np.all(J[~zero] != 0.0)
    assert np.all(np.abs(J - rJ)[~zero] <= 1e-14 * np.abs(rJ[~zero]))
    assert np.all(np.abs(rJ[zero]) <= 1e-13 * np.abs(rJ).max())             # the float restatement agrees they vanish
    assert np.all(np.abs(w - rw) <= 1e-14 * np.abs(rw)) and np.all(w > 0)
    # each macro-element has one vertex whose jump vanishes: D + 1 of its D + 2 coefficients act
    assert np.all(zero.sum(axis=1) == (1 if d == 3 else 0))


@pytest.mark.parametrize("d,h", CASES)
def test_jumps_annihilate_affine_functions(d, h):
    """the jump of the normal derivative of an affine function vanishes: sum_l J_l = 0 and sum_l J_l x_l = 0"""
    _, offs, J, _ = tables(d, h)
    x = offs * np.asarray(h)[None, None, :]
    scale = np.abs(J).max(axis=1)
    assert np.all(np.abs(J.sum(axis=1)) <= 1e-14 * scale)
    assert np.all(np.abs(np.einsum("tl,tla->ta", J, x)) <= 1e-14 * scale[:, None] * np.abs(x).max())


def test_bad_arguments_are_refused():
    from phifem_amd import _lib as L
    h = np.array([0.1, 0.1, 0.1])
    n = C.c_int(0)
    L.check(L.lib.phx_box_facet_tables(3, h.ctypes.data_as(C.c_void_p), 1.0, C.byref(n), None, None, None, None))
    assert n.value == 12
    with pytest.raises(ValueError):
        L.check(L.lib.phx_box_facet_tables(4, h.ctypes.data_as(C.c_void_p), 1.0, C.byref(n), None, None, None, None))
    h[1] = 0.0
    with pytest.raises(ValueError):
        L.check(L.lib.phx_box_facet_tables(3, h.ctypes.data_as(C.c_void_p), 1.0, C.byref(n), None, None, None, None))
