"""Gradient recovery and the recovery-based indicator on the GPU (`phifem_amd.recover_gradient`, `estimate_zz`) against
the numpy specification tests/recover_ref.py.

TOLERANCE: G and eta2 agree with the specification to 1e-12 x (largest SCALE of that output over the mesh); the scale is
the same formula with every product of a nodal value and a basis gradient replaced by its absolute value, so the bound
keeps its meaning where a difference is small by cancellation.  The total agrees within 1e-12 x scale x nc.  The input
conditions (cell counts, tags 1, 2, 3, partly selected and long stars, margins of the marking thresholds) are asserted
on the CPU in tests/test_recover_ref.py, the margins again here from the specification's numbers.

Meshes: tests/recover_cases.py (the seven of tests/estimate_cases.py and two hub meshes).

The solved case: the strong-Dirichlet scheme imposes u = 0 on the circle, which u = sin x cos y of
demo/weak-dirichlet/estimate.py does not satisfy; demo/strong-dirichlet/adapt.py therefore multiplies it by the
level-set (u = phi sin x cos y, f = -Laplace u), and the test runs that demo's loop.  Recorded by that loop on `disk`
(eta and eta / H10 per level, printed, not asserted): DESIGN.md 7g."""
import ctypes as C
import importlib.util
import os
import warnings

import numpy as np
import pytest

import estimate_cases as EC
import estimate_ref as ER
import recover_cases as RC
import recover_ref as RR

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
    ctype, x, cells = RC.arrays(name)
    return P.Mesh.from_arrays(ctype, x, cells)


def tag(P, mesh, name, box_mode=True):
    from phifem_amd.mesh_scripts import NodalFunction
    x = mesh.x
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = P.compute_tags_measures(mesh, NodalFunction(EC.levelset(x, x, RC.radius_factor(name))), 1,
                                      box_mode=box_mode, single_layer_cut=True)
    return out[2]        # the sub-mesh (None in box mode)


_CASES = {}


def case(P, name, degree, submesh=False, vector=False):
    """One tagged device mesh per (name, mode), and per (degree, vector) its nodal values and the specification's
    numbers for S = Omega_h, computed once and shared by the tests."""
    mkey = (name, submesh)
    if mkey not in _CASES:
        mesh = make_mesh(P, name)
        sub = tag(P, mesh, name, box_mode=not submesh)
        work = sub if submesh else mesh
        _CASES[mkey] = {"mesh": work, "keep": mesh, "x": work.x, "cells": work.cells.astype(np.int64),
                        "tags": work.cell_tag_values()}
    c = _CASES[mkey]
    key = (degree, vector)
    if key not in c:
        work = c["mesh"]
        u = RC.field(c["x"], work.lagrange_dof_points(degree), work.gdim if vector else None)
        c2e = work.c2e.astype(np.int64) if degree == 2 else None
        c[key] = (u, RR.recover_ref(work.cell_type, c["x"], c["cells"], degree, u, RR.omega_mask(c["tags"]), c2e))
    return (c["mesh"], c["tags"]) + c[key]


def check(P, mesh, got_eta2, got_G, last_sum, ref, mask, what, lone=False):
    """lone: no two selected cells share a vertex, so G is every cell's own gradient up to the rounding of
    (|T| g) / |T| and eta2 is zero up to that: only the tolerance is asserted, not that the indicator is positive."""
    sel = np.asarray(mask).astype(bool)
    star = RR.star_lengths(mesh.nv, mesh.cells.astype(np.int64), sel)[0] > 0
    assert got_G.shape == ref.G.shape and got_G.dtype == np.float64
    assert got_eta2.shape == (mesh.nc,) and got_eta2.dtype == np.float64
    gs, es = ref.G_scale.max(), ref.eta2_scale.max()
    gerr = np.abs(got_G - ref.G).max()
    eerr = np.abs(got_eta2 - ref.eta2).max()
    serr = abs(last_sum - ref.eta2.sum())
    print(f"{what}: max |G - ref| = {gerr:.3e} = {gerr / gs:.2e} of the largest scale {gs:.3e}; max |eta2 - ref| = "
          f"{eerr:.3e} = {eerr / es:.2e} of the largest scale {es:.3e}; sum {last_sum:.6e}, |sum - ref| / scale = "
          f"{serr / es:.2e} (bound {TOL * mesh.nc:.1e})")
    assert np.all(got_eta2[~sel] == 0.0), "cells outside S are not exactly 0"
    assert np.all(np.moveaxis(got_G, -2, 0)[~star] == 0.0), "vertices with no selected star are not exactly 0"
    assert gs > 0.0 and es > 0.0 and np.abs(ref.G).max() > 0.0
    assert lone or ref.eta2.max() > 0.0
    assert gerr <= TOL * gs
    assert eerr <= TOL * es
    assert serr <= TOL * es * mesh.nc


PARITY = [(n, k, False, False) for n in RC.MESHES for k in EC.degrees(RC.arrays(n)[0])] + \
         [(n, k, True, False) for n in EC.SUBMESH for k in (1, 2)] + \
         [(n, k, False, True) for n in RC.VECTOR for k in (1, 2)]


# ---- 1. parity with the specification -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,degree,submesh,vector", PARITY)
def test_parity(P, name, degree, submesh, vector):
    mesh, tags, u, ref = case(P, name, degree, submesh, vector)
    assert mesh.nc > 64 and mesh.nc % 64 != 0
    if submesh:
        assert mesh.parent is not None and set(np.unique(tags)) == {1, 2}
    else:
        assert all((tags == t).any() for t in (1, 2, 3))
    eta2, G = P.estimate_zz(mesh, u, degree=degree, gradient=True)
    assert isinstance(eta2, np.ndarray) and isinstance(G, np.ndarray)
    assert G.shape == ((mesh.gdim,) if vector else ()) + (mesh.nv, mesh.gdim)
    check(P, mesh, eta2, G, P.estimate_zz.last_sum, ref, RR.omega_mask(tags),
          f"{name} k={degree}{' sub-mesh' if submesh else ''}{' vector' if vector else ''}")
    assert np.array_equal(P.recover_gradient(mesh, u, degree=degree), G)
    assert np.array_equal(P.estimate_zz(mesh, u, degree=degree), eta2)


def test_nodal_functions_are_accepted(P):
    from phifem_amd.mesh_scripts import NodalFunction
    mesh, tags, u, ref = case(P, "disk", 2)
    assert np.array_equal(P.recover_gradient(mesh, NodalFunction(u, 2), degree=2), P.recover_gradient(mesh, u, degree=2))
    with pytest.raises(ValueError):
        P.estimate_zz(mesh, NodalFunction(u[:mesh.nv], 1), degree=2)


# ---- 2. masks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,degree", [("disk", 2), ("flux_2d", 1), ("square_quad", 1), ("box_3d", 1)])
def test_masks(P, name, degree):
    mesh, tags, u, ref = case(P, name, degree)
    omega = RR.omega_mask(tags)
    a, Ga = P.estimate_zz(mesh, u, degree=degree, gradient=True)
    sa = P.estimate_zz.last_sum
    b, Gb = P.estimate_zz(mesh, u, degree=degree, cells=omega, gradient=True)
    assert a.tobytes() == b.tobytes() and Ga.tobytes() == Gb.tobytes() and sa == P.estimate_zz.last_sum
    assert np.array_equal(P.estimate_zz(mesh, u, degree=degree, cells=omega.astype(bool)), a)
    # every cell, on a mesh that carries no tags
    untagged = make_mesh(P, name)
    c2e = untagged.c2e.astype(np.int64) if degree == 2 else None
    x, cells = untagged.x, untagged.cells.astype(np.int64)
    for what, mask in (("all cells", np.ones(untagged.nc, dtype=np.uint8)),
                       ("one cell", (np.arange(untagged.nc) == untagged.nc // 3).astype(np.uint8)),
                       ("every third cell, not from 0", (np.arange(untagged.nc) % 3 == 1).astype(np.uint8))):
        want = RR.recover_ref(untagged.cell_type, x, cells, degree, u, mask, c2e)
        eta2, G = P.estimate_zz(untagged, u, degree=degree, cells=mask, gradient=True)
        check(P, untagged, eta2, G, P.estimate_zz.last_sum, want, mask, f"{name} k={degree} {what}",
              lone=what == "one cell")
    base = live_bytes()
    eta2, G = P.estimate_zz(untagged, u, degree=degree, cells=np.zeros(untagged.nc, dtype=np.uint8), gradient=True)
    assert not eta2.any() and not G.any() and P.estimate_zz.last_sum == 0.0
    assert live_bytes() == base


def test_unaligned_device_mask(P):
    """A mask that is a view into a larger tensor starts at any byte."""
    import torch
    mesh, tags, u, ref = case(P, "disk", 1)
    dev = torch.device("cuda", mesh.device)
    buf = torch.zeros(mesh.nc + 8, dtype=torch.uint8, device=dev)
    want = P.estimate_zz(mesh, u)
    for off in (1, 2, 3, 4):
        view = buf[off:off + mesh.nc]
        view.copy_(torch.from_numpy(RR.omega_mask(tags)).to(dev))
        got = P.estimate_zz(mesh, torch.from_numpy(u).to(dev), cells=view)
        assert got.cpu().numpy().tobytes() == want.tobytes()
        buf.zero_()


# ---- 3. reproducibility -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,degree", [("flux_2d", 1), ("p2_3d", 2), ("box_3d", 1), ("box_3d", 2)])
def test_bit_reproducible(P, name, degree):
    import torch
    mesh, tags, u, ref = case(P, name, degree)
    a, Ga = P.estimate_zz(mesh, u, degree=degree, gradient=True)
    sa = P.estimate_zz.last_sum
    b, Gb = P.estimate_zz(mesh, u, degree=degree, gradient=True)
    assert a.tobytes() == b.tobytes() and Ga.tobytes() == Gb.tobytes() and sa == P.estimate_zz.last_sum
    dev = torch.device("cuda", mesh.device)
    t, Gt = P.estimate_zz(mesh, torch.from_numpy(u).to(dev), degree=degree, gradient=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == (mesh.nc,)
    assert isinstance(Gt, torch.Tensor) and Gt.is_cuda and tuple(Gt.shape) == (mesh.nv, mesh.gdim)
    assert t.cpu().numpy().tobytes() == a.tobytes() and Gt.cpu().numpy().tobytes() == Ga.tobytes()
    assert sa == P.estimate_zz.last_sum
    # a second mesh object made from the same arrays: an adjacency filled by atomics would order its stars otherwise
    other = make_mesh(P, name)
    tag(P, other, name)
    assert np.array_equal(other.cell_tag_values(), tags)
    c, Gc = P.estimate_zz(other, u, degree=degree, gradient=True)
    assert c.tobytes() == a.tobytes() and Gc.tobytes() == Ga.tobytes() and sa == P.estimate_zz.last_sum


# ---- 4. marking ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,degree", RC.MARK_MESHES)
def test_marking(P, name, degree):
    mesh, tags, u, ref = case(P, name, degree)
    eta2 = P.estimate_zz(mesh, u, degree=degree)
    for theta in RC.MARK_THETAS:
        margin = ER.dorfler_margin(ref.eta2, theta)
        print(f"{name} k={degree} theta={theta}: margin {margin:.2e}")
        assert margin > 1e-9, "input condition: a partial sum sits at the threshold"
        got = P.mark_dorfler(mesh, eta2, theta)
        assert np.array_equal(got, ER.mark_dorfler_ref(ref.eta2, theta))
        assert not got[RR.omega_mask(tags) == 0].any()


# ---- 5. one solved case ---------------------------------------------------------------------------------------------------
def load_demo():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "demo", "strong-dirichlet", "adapt.py")
    spec = importlib.util.spec_from_file_location("strong_dirichlet_adapt", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_solved_case(P):
    demo = load_demo()
    ctype, x, cells = RC.arrays("disk")
    levelset, exact, source = demo.problem(x)
    mesh = make_mesh(P, "disk")
    row = demo.solve_level(mesh, levelset, exact, source)
    want = RR.recover_ref(ctype, mesh.x, mesh.cells.astype(np.int64), 1, row["u"], RR.omega_mask(row["tags"]))
    G = P.recover_gradient(mesh, row["u"])
    check(P, mesh, row["eta2"], G, P.estimate_zz.last_sum, want, RR.omega_mask(row["tags"]), "solved disk k=1")

    lines = []
    rows = demo.run_loop(ctype, x, cells, 3, theta=0.5, report=lines.append)
    print("\n".join(lines))
    assert len(rows) == 3
    for lv, r in enumerate(rows):
        assert np.isfinite(r["eta"]) and r["eta"] > 0.0
        print(f"level {lv}: eta = {r['eta']:.4e}, H10 = {r['h10']:.4e}, effectivity index {r['eta'] / r['h10']:.3f}")
        if lv + 1 < len(rows):
            assert r["marked"].any() and not r["marked"][RR.omega_mask(r["tags"]) == 0].any(), "marked outside Omega_h"
            assert rows[lv + 1]["nc"] > r["nc"]
        else:
            assert r["marked"] is None


# ---- 6. refusals and leaks --------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind(P):
    import torch
    mesh, tags, u, ref = case(P, "disk", 1)
    quad, _, uq, _ = case(P, "square_quad", 1)
    base = live_bytes()
    P.estimate_zz(mesh, u)
    assert live_bytes() == base, "a successful estimate_zz leaks"
    P.recover_gradient(quad, uq)
    assert live_bytes() == base, "a successful recover_gradient leaks"

    untagged = make_mesh(P, "disk")
    sheared = P.Mesh.from_arrays(*RC.sheared_quads())
    base = live_bytes()
    dev = torch.device("cuda", mesh.device)
    ut = torch.from_numpy(u).to(dev)

    def refused(exc, match, fn, *args, **kw):
        with pytest.raises(exc, match=match):
            fn(*args, **kw)
        assert live_bytes() == base, f"a refusal ({exc.__name__}) leaks"

    for fn in (P.recover_gradient, P.estimate_zz):
        refused(ValueError, "compute_tags_measures", fn, untagged, u)
        refused(NotImplementedError, None, fn, mesh, u, degree=3)
        refused(NotImplementedError, None, fn, quad, np.zeros(quad.nv + quad.nf + quad.nc), degree=2)
        refused(NotImplementedError, "rectangles", fn, sheared, uq, cells=np.ones(sheared.nc, dtype=np.uint8))
        refused(ValueError, None, fn, mesh, u[:-1])                                   # a wrong length
        refused(ValueError, None, fn, mesh, np.zeros((2, 3, mesh.nv)))
        refused(ValueError, None, fn, mesh, u, cells=np.ones(mesh.nc - 1, dtype=np.uint8))
        refused(ValueError, None, fn, mesh, ut, cells=np.ones(mesh.nc, dtype=np.uint8))   # mixed kinds
        refused(ValueError, None, fn, mesh, u, cells=torch.ones(mesh.nc, dtype=torch.uint8, device=dev))
        fn(mesh, u)
        assert live_bytes() == base, "a success after the refusals leaks"
    # the refusals of the solver classes stay as they are
    for cls in (P.StrongDirichletSolver, P.NeumannRobinSolver, P.InterfaceElasticitySolver):
        with pytest.raises(NotImplementedError):
            cls(mesh).estimate(np.zeros(2 * mesh.nv))
    assert live_bytes() == base
