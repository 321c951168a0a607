"""Residual error indicators and Doerfler marking on the GPU (`phifem_amd.estimate`, `mark_dorfler`,
`PhiFEMSolver.estimate`) against the numpy specification tests/estimate_ref.py (closed-form / Gauss-Legendre
quadrature, independent of the library's rules).

TOLERANCE: each part agrees with the specification to 1e-12 x (largest SCALE of that part over the cells); the scale is
the part with every product of a nodal value and a basis quantity replaced by its absolute value, so the bound keeps
its meaning where a residual is small by cancellation.  The input conditions (tags 1, 2, 3 present, margins of the
marking thresholds) are asserted on the CPU in tests/test_estimate_ref.py and, where they depend on device results,
from the specification's numbers here.

Meshes: tests/estimate_cases.py.  Two of its choices differ from the wording of the issue that asked for these tests,
because that wording contradicts itself: the generated 2-D box has 7 x 9 squares (the 3 x 4 squares of locate_cases.BOX
are 24 triangles, fewer than the 64 cells every mesh must exceed), and on the 3 x 4 x 5 boxes the sphere has 0.8 instead
of 0.62 times the half extent (at 0.62 it holds no whole tetrahedron, so no cell is tagged 1); there the cut cells
reach the mesh boundary.  `mark_dorfler` takes one indicator per cell, so the exact marking cases run on strips of
exactly n rectangles."""
import ctypes as C
import warnings

import numpy as np
import pytest

import estimate_cases as EC
import estimate_ref as ER

pytestmark = pytest.mark.gpu
TOL = 1e-12          # the project's oracle tolerance


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def live_bytes():
    from phifem_amd import _lib as L
    a, b = C.c_int64(0), C.c_int64(0)
    L.check(L.lib.phx_pool_stats(C.byref(a), C.byref(b)))
    return a.value


def make_mesh(P, name):
    if name == "box_3d":
        from locate_cases import BOX
        return P.create_box(*BOX)
    if name == "box_2d":
        return P.create_box(*EC.BOX_2D)
    ctype, x, cells = EC.arrays(name)
    return P.Mesh.from_arrays(ctype, x, cells)


def tag(P, mesh, name, box_mode=True):
    from phifem_amd.mesh_scripts import NodalFunction
    x = mesh.x
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = P.compute_tags_measures(mesh, NodalFunction(EC.levelset(x, x, EC.RADIUS_FACTOR.get(name, 0.62))), 1,
                                      box_mode=box_mode, single_layer_cut=True)
    return out[2]        # the sub-mesh (None in box mode)


_CASES = {}


def case(P, name, degree, submesh=False):
    """One tagged device mesh per (name, mode), and per degree its nodal fields and the specification's numbers, computed
    once and shared by the tests."""
    mkey = (name, submesh)
    if mkey not in _CASES:
        mesh = make_mesh(P, name)
        sub = tag(P, mesh, name, box_mode=not submesh)
        work = sub if submesh else mesh
        _CASES[mkey] = {"mesh": work, "keep": mesh, "x": work.x, "cells": work.cells.astype(np.int64),
                        "tags": work.cell_tag_values()}
    c = _CASES[mkey]
    if degree not in c:
        work = c["mesh"]
        pts = work.lagrange_dof_points(degree)
        F = EC.nodal_fields(c["x"], pts, factor=EC.RADIUS_FACTOR.get(name, 0.62))
        c2e = work.c2e.astype(np.int64) if degree == 2 else None
        parts, scales = ER.estimate_ref(work.cell_type, c["x"], c["cells"], c["tags"], degree, F["u"], F["p"], F["phi"],
                                        F["f"], F["ud"], c2e)
        c[degree] = (F, parts, scales)
    return (c["mesh"], c["tags"]) + c[degree]


def run(P, mesh, F, degree, parts=True):
    return P.estimate(mesh, F["u"], F["p"], F["phi"], F["f"], F["ud"], degree=degree, parts=parts)


def check_parts(got, sums, parts, scales, tags, what):
    omega = (tags == 1) | (tags == 2)
    nc = tags.size
    assert got.shape == (3, nc) and got.dtype == np.float64
    assert np.all(got[:, ~omega] == 0.0), "cells outside Omega_h are not exactly 0"
    assert np.all(got[2, tags == 1] == 0.0)
    for k, part in enumerate("RJB"):
        smax = scales[k].max()
        err = np.abs(got[k] - parts[k]).max()
        serr = abs(sums[k] - parts[k].sum())
        print(f"{what} {part}: max |device - ref| = {err:.3e} = {err / smax:.2e} of the largest scale {smax:.3e}; "
              f"sum {sums[k]:.6e}, |sum - ref| / scale = {serr / smax:.2e} (bound {TOL * nc:.1e})")
        assert smax > 0.0 and parts[k].max() > 0.0
        assert err <= TOL * smax
        assert serr <= TOL * smax * nc


PARITY = [(n, k, False) for n in EC.MESHES for k in EC.degrees(EC.arrays(n)[0])] + \
         [(n, k, True) for n in EC.SUBMESH for k in (1, 2)]


# ---- 1. parity with the specification -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,degree,submesh", PARITY)
def test_parity(P, name, degree, submesh):
    mesh, tags, F, parts, scales = case(P, name, degree, submesh)
    assert mesh.nc > 64 and mesh.nc % 64 != 0
    if submesh:
        assert mesh.parent is not None and set(np.unique(tags)) == {1, 2}
    else:
        assert all((tags == t).any() for t in (1, 2, 3))
    got = run(P, mesh, F, degree)
    assert isinstance(got, np.ndarray)
    check_parts(got, P.estimate.last_sums, parts, scales, tags, f"{name} k={degree}{' sub-mesh' if submesh else ''}")
    eta2 = run(P, mesh, F, degree, parts=False)
    assert eta2.shape == (mesh.nc,) and np.array_equal(eta2, got[0] + got[1] + got[2])


def test_nodal_functions_are_accepted(P):
    from phifem_amd.mesh_scripts import NodalFunction
    mesh, tags, F, parts, scales = case(P, "disk", 2)
    G = {k: NodalFunction(v, 2) for k, v in F.items()}
    assert np.array_equal(run(P, mesh, G, 2), run(P, mesh, F, 2))
    with pytest.raises(ValueError):
        run(P, mesh, dict(F, u=NodalFunction(F["u"][:mesh.nv], 1)), 2)


# ---- 2. one solved case ---------------------------------------------------------------------------------------------------
_SOLVED = {}


def solved(P, degree):
    """PhiFEMSolver on `disk` with the manufactured solution of demo/weak-dirichlet/estimate.py."""
    if degree not in _SOLVED:
        mesh = make_mesh(P, "disk")
        tag(P, mesh, "disk")
        x = mesh.x
        pts = mesh.lagrange_dof_points(degree)
        phi = EC.levelset(x, pts)
        uex = np.sin(pts[:, 0]) * np.cos(pts[:, 1])
        solver = P.PhiFEMSolver(mesh, degree=degree, levelset_degree=degree)
        solver.assemble(phi, 2.0 * uex, uex)
        w = solver.solve(rtol=1e-11, max_iter=200000)
        u, p = solver.split(w)
        tags = mesh.cell_tag_values()
        c2e = mesh.c2e.astype(np.int64) if degree == 2 else None
        parts, scales = ER.estimate_ref(mesh.cell_type, x, mesh.cells.astype(np.int64), tags, degree, u, p, phi,
                                        2.0 * uex, uex, c2e)
        _SOLVED[degree] = (mesh, solver, w, tags, parts, scales)
    return _SOLVED[degree]


@pytest.mark.parametrize("degree", [1, 2])
def test_solved_case(P, degree):
    mesh, solver, w, tags, parts, scales = solved(P, degree)
    got = solver.estimate(w, parts=True)
    cut = tags == 2
    print(f"disk k={degree}: eta = {np.sqrt(got.sum()):.4e}; B / its scale on the cut cells: "
          f"{parts[2, cut].max() / scales[2, cut].max():.2e} (small by cancellation)")
    check_parts(got, P.estimate.last_sums, parts, scales, tags, f"solved disk k={degree}")
    assert np.array_equal(solver.estimate(w), got[0] + got[1] + got[2])


# ---- 3. reproducibility -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,degree", [("disk", 1), ("disk", 2), ("square_quad", 1), ("box_3d", 1), ("box_3d", 2)])
def test_bit_reproducible(P, name, degree):
    import torch
    mesh, tags, F, parts, scales = case(P, name, degree)
    a = run(P, mesh, F, degree)
    sa = P.estimate.last_sums
    b = run(P, mesh, F, degree)
    sb = P.estimate.last_sums
    assert a.tobytes() == b.tobytes() and np.array(sa).tobytes() == np.array(sb).tobytes()
    dev = torch.device("cuda", mesh.device)
    T = {k: torch.from_numpy(v).to(dev) for k, v in F.items()}
    t = run(P, mesh, T, degree)
    st = P.estimate.last_sums
    assert isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == (3, mesh.nc)
    assert t.cpu().numpy().tobytes() == a.tobytes() and np.array(st).tobytes() == np.array(sa).tobytes()


# ---- 4. marking, exact ------------------------------------------------------------------------------------------------------
_STRIPS = {}


def strip(P, n):
    """A mesh of exactly n cells (a row of n rectangles): `mark_dorfler` takes one indicator per cell."""
    if n not in _STRIPS:
        _STRIPS[n] = P.create_rectangle([[0.0, 0.0], [float(n), 1.0]], [n, 1], cell_type="quadrilateral")
    return _STRIPS[n]


@pytest.mark.parametrize("n", EC.MARK_LENGTHS)
def test_marking_exact(P, n):
    """Small non-negative integers stored as float64: their sums are exact in any order, the mask is defined bit for bit."""
    import torch
    mesh = strip(P, n)
    assert mesh.nc == n
    for kind in ("ties", "zeros"):
        eta2 = EC.integer_indicators(n, kind)
        for theta in EC.MARK_THETAS:
            want = ER.mark_dorfler_ref(eta2, theta)
            got = P.mark_dorfler(mesh, eta2, theta)
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (n,)
            assert np.array_equal(got, want), f"n={n} {kind} theta={theta}"
            assert P.mark_dorfler.last_count == int(want.sum())
            if theta == 1.0:
                assert np.array_equal(got.astype(bool), eta2 > 0.0)
        t = P.mark_dorfler(mesh, torch.from_numpy(eta2).to(torch.device("cuda", mesh.device)), 0.5)
        assert t.is_cuda and t.dtype == torch.uint8
        assert np.array_equal(t.cpu().numpy(), ER.mark_dorfler_ref(eta2, 0.5))


# ---- 5. marking, real -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 2])
def test_marking_real(P, degree):
    mesh, solver, w, tags, parts, scales = solved(P, degree)
    eta2 = solver.estimate(w)
    ref_eta2 = parts.sum(axis=0)
    for theta in (0.3, 0.5, 0.8):
        margin = ER.dorfler_margin(ref_eta2, theta)
        print(f"disk k={degree} theta={theta}: margin {margin:.2e}")
        assert margin > 1e-9, "input condition: a partial sum sits at the threshold"
        got = P.mark_dorfler(mesh, eta2, theta)
        assert np.array_equal(got, ER.mark_dorfler_ref(ref_eta2, theta))
        assert P.mark_dorfler.last_count == int(got.sum()) and not got[tags == 3].any()


# ---- 6. refusals and leaks --------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind(P):
    mesh, tags, F, parts, scales = case(P, "disk", 1)
    quad, _, Fq, _, _ = case(P, "square_quad", 1)
    base = live_bytes()
    run(P, mesh, F, 1)
    assert live_bytes() == base, "a successful estimate leaks"
    eta2 = parts.sum(axis=0)
    P.mark_dorfler(mesh, eta2, 0.5)
    assert live_bytes() == base, "a successful mark_dorfler leaks"

    untagged = make_mesh(P, "disk")
    base = live_bytes()
    with pytest.raises(ValueError, match="compute_tags_measures"):
        run(P, untagged, F, 1)
    assert live_bytes() == base
    with pytest.raises(ValueError):
        run(P, mesh, dict(F, f=F["f"][:-1]), 1)
    with pytest.raises(ValueError):
        P.mark_dorfler(mesh, eta2[:-1], 0.5)
    with pytest.raises(NotImplementedError):
        P.estimate(quad, *(np.zeros(quad.nv + quad.nf + quad.nc),) * 5, degree=2)
    with pytest.raises(NotImplementedError):
        run(P, mesh, F, 3)
    for theta in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            P.mark_dorfler(mesh, eta2, theta)
    for bad in (float("nan"), -1.0):
        e = eta2.copy()
        e[7] = bad
        with pytest.raises(ValueError):
            P.mark_dorfler(mesh, e, 0.5)
        assert live_bytes() == base
    assert live_bytes() == base

    solver = P.PhiFEMSolver(mesh)
    with pytest.raises(RuntimeError):
        solver.estimate(np.zeros(2 * mesh.nv))
    for cls in (P.StrongDirichletSolver, P.NeumannRobinSolver, P.InterfaceElasticitySolver):
        with pytest.raises(NotImplementedError):
            cls(mesh).estimate(np.zeros(2 * mesh.nv))
    assert live_bytes() == base
