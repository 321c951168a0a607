"""Marked refinement and the nested transfer onto its meshes on the GPU (`phifem_amd.refine(mesh, marked=, edges=)`,
`phifem_amd.prolongate`) against the numpy specification tests/refine_marked_ref.py: meshes, parents, leaf tuples and
the degree-1 transfer bit for bit, degree 2 to round-off."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import hub_meshes as HM
import partition_ref as PR
import refine_marked_ref as RM
import refine_ref as RR
from datasets import load_mesh
from oracle.topology import Topology

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
MESHES = ["disk", "coarse_square", "graded_tet_box", "hub_3d", "box_3x4x5"]
HUB_3D = min((k for k, c in HM.CASES.items() if c["d"] == 3), key=lambda k: (HM.CASES[k]["nbg"] + sum(h[1] for h in HM.CASES[k]["hubs"]), k))


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


@functools.lru_cache(maxsize=None)
def arrays(name):
    if name == "graded_tet_box":
        return ("tetrahedron",) + PR.graded_tet_box()
    if name == "hub_3d":
        x, cells, _ = HM.case_mesh(HUB_3D)
        return "tetrahedron", np.ascontiguousarray(x, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    if name.startswith("single_"):
        return (name[7:],) + RR.single_cell(name[7:])
    return load_mesh(name)


def coarse_mesh(P, name):
    """-> (mesh, cell type, x, cells, edges): `edges` is the library's numbering where it is not the ascending sorted
    pair (generated boxes), else None."""
    if name == "box_3x4x5":
        mesh = P.create_box([-1.0, 0.0, 0.5], [1.0, 1.5, 2.0], [3, 4, 5])
        return mesh, "tetrahedron", mesh.x, mesh.cells.astype(np.int64), mesh.edges
    ctype, x, cells = arrays(name)
    return P.Mesh.from_arrays(ctype, x, cells), ctype, np.asarray(x, dtype=np.float64), np.asarray(cells, dtype=np.int64), None


def live_bytes():
    from phifem_amd import _lib as L
    a, b = C.c_int64(0), C.c_int64(0)
    L.check(L.lib.phx_pool_stats(C.byref(a), C.byref(b)))
    return a.value


def assert_equals_spec(fine, ref, what):
    assert fine.nv == ref["x"].shape[0] and fine.nc == ref["cells"].shape[0], what
    assert np.array_equal(fine.x, ref["x"]), f"{what}: fine coordinates differ from the specification"
    assert np.array_equal(fine.cells, ref["cells"]), f"{what}: fine cells differ from the specification"
    assert np.array_equal(fine.parent_cells, ref["parent_cells"]), f"{what}: parent_cells differ"
    assert np.array_equal(fine.child_nodes, ref["child_nodes"]), f"{what}: child_nodes differ"
    assert fine.refine_info[0] == int(ref["marked"].sum()), f"{what}: marked edges after the closure differ"
    assert fine.refine_info[2] == fine.nc and fine.refine_info[1] >= 1
    assert fine.nchild is None and fine.parent is None


# ---- 1. every edge mask of one cell, 200 of the six tetrahedra around one diagonal ------------------------------------
@pytest.mark.parametrize("name", ["single_triangle", "single_tetrahedron"])
def test_single_cell_every_edge_mask(P, name):
    mesh, ctype, x, cells, _ = coarse_mesh(P, name)
    ne = mesh.ne
    assert np.array_equal(mesh.edges, RR.edge_numbering(ctype, cells)[1])
    for bits in range(1 << ne):
        em = np.array([(bits >> k) & 1 for k in range(ne)], dtype=np.uint8)
        fine = P.refine(mesh, edges=em)
        assert fine.coarse is mesh
        assert_equals_spec(fine, RM.refine_marked_ref(ctype, x, cells, edge_marks=em), f"{name} mask {bits}")


def test_one_cube_random_edge_masks(P):
    mesh = P.create_box([0.0] * 3, [1.0, 2.0, 3.0], [1, 1, 1])
    x, cells, edges = mesh.x, mesh.cells.astype(np.int64), mesh.edges
    assert mesh.nc == 6 and mesh.ne == 19
    rng = np.random.default_rng(0)
    for k in range(200):
        em = (rng.random(mesh.ne) < rng.random()).astype(np.uint8)
        fine = mesh.refine(edges=em)
        assert_equals_spec(fine, RM.refine_marked_ref("tetrahedron", x, cells, edge_marks=em, edges=edges), f"mask {k}")


# ---- 2. cell masks on real meshes -------------------------------------------------------------------------------------
def _point(x):
    lo, hi = x.min(axis=0), x.max(axis=0)
    return lo + (hi - lo) * np.array([0.37, 0.58, 0.44][:x.shape[1]])


def _check_topology(fine, ctype, ref):
    topo = Topology(ctype, ref["cells"], ref["x"].shape[0])
    assert np.array_equal(fine.c2f, topo.c2f) and np.array_equal(fine.f2c, topo.f2c)


@pytest.mark.parametrize("name", MESHES)
def test_cell_masks_equal_reference(P, name):
    import torch
    mesh, ctype, x, cells, edges = coarse_mesh(P, name)
    nc = mesh.nc
    for what, mask in (("none", np.zeros(nc, dtype=np.uint8)), ("all", np.ones(nc, dtype=np.uint8)),
                       ("seeded", RM.seeded_mask(nc))):
        fine = P.refine(mesh, marked=mask)
        ref = RM.refine_marked_ref(ctype, x, cells, cell_marks=mask, edges=edges)
        assert_equals_spec(fine, ref, f"{name}/{what}")
        _check_topology(fine, ctype, ref)
        if what == "none":
            assert fine.nc == nc and np.array_equal(fine.cells, cells) and np.array_equal(fine.x, x)
        if what == "all":
            assert fine.nc == RM.MAXCHILD[ctype] * nc and fine.nv == mesh.nv + mesh.ne
        if what == "seeded":             # a mask on the device, as mark_dorfler returns it, gives the same mesh
            dev = P.refine(mesh, marked=torch.from_numpy(mask).cuda())
            assert np.array_equal(dev.x, fine.x) and np.array_equal(dev.cells, fine.cells)
            assert np.array_equal(dev.parent_cells, fine.parent_cells) and dev.refine_info[0] == fine.refine_info[0]
    # a refined mesh is refined again: three rounds near a point
    point = _point(x)
    for rnd in range(3):
        mask = RM.nearest_mask(x, cells, point)
        fine = P.refine(mesh, marked=mask)
        ref = RM.refine_marked_ref(ctype, x, cells, cell_marks=mask, edges=edges)
        assert_equals_spec(fine, ref, f"{name}/nearest round {rnd}")
        _check_topology(fine, ctype, ref)
        mesh, x, cells, edges = fine, ref["x"], ref["cells"], None
        assert np.array_equal(mesh.edges, RR.edge_numbering(ctype, cells)[1])


def test_cell_and_edge_masks_together(P):
    mesh, ctype, x, cells, _ = coarse_mesh(P, "disk")
    cm = RM.seeded_mask(mesh.nc, 0.05, 1)
    em = RM.seeded_mask(mesh.ne, 0.05, 2)
    assert_equals_spec(P.refine(mesh, marked=cm, edges=em), RM.refine_marked_ref(ctype, x, cells, cm, em), "both masks")


# ---- 3. transfer ------------------------------------------------------------------------------------------------------
def _quadratic(p):
    return 0.2 + p[:, 0] * p[:, -1] - 0.7 * p[:, 0] ** 2 + 0.4 * p[:, -1] ** 2 + p.sum(axis=1)


@pytest.mark.parametrize("name", ["disk", "graded_tet_box", "box_3x4x5"])
def test_prolongate(P, name):
    import torch
    mesh, ctype, x, cells, edges = coarse_mesh(P, name)
    mask = RM.nearest_mask(x, cells, _point(x), 0.2)
    fine = P.refine(mesh, marked=mask)
    ref = RM.refine_marked_ref(ctype, x, cells, cell_marks=mask, edges=edges)
    # degree 1: the coordinate arithmetic
    assert np.array_equal(P.prolongate(fine, np.ascontiguousarray(mesh.x.T)), fine.x.T)
    rng = np.random.default_rng(11)
    v1 = rng.standard_normal((2, mesh.nv))
    assert np.array_equal(P.prolongate(fine, v1), RM.prolongate_marked_ref(ctype, x, cells, ref, v1, 1))
    # degree 2.  |got - ref| <= 64 eps max|u|: at most 10 terms with sum |w| <= 2 give 22 eps max|u| per side
    n2 = mesh.lagrange_ndofs(2)
    v = rng.standard_normal((3, n2))
    want = RM.prolongate_marked_ref(ctype, x, cells, ref, v, 2)
    got = P.prolongate(fine, v, degree=2)
    assert got.shape == want.shape == (3, fine.lagrange_ndofs(2))
    err = np.abs(got - want).max()
    print(f"{name}: P2 prolongation |got - ref| = {err:.3e} ({err / (EPS * np.abs(v).max()):.2f} eps max|u|)")
    assert err <= 64 * EPS * np.abs(v).max()
    assert np.array_equal(got[:, :mesh.nv], v[:, :mesh.nv])
    assert np.array_equal(got[:, mesh.nv:fine.nv], v[:, mesh.nv + ref["mid_edges"]])
    assert np.array_equal(P.prolongate(fine, v, degree=2), got)                       # the same bits on every run
    gd = P.prolongate(fine, torch.from_numpy(v[1]).cuda(), degree=2)
    assert gd.is_cuda and np.array_equal(gd.cpu().numpy(), got[1])
    q, qf = _quadratic(mesh.lagrange_dof_points(2)), _quadratic(fine.lagrange_dof_points(2))
    errq = np.abs(P.prolongate(fine, q, degree=2) - qf).max()
    print(f"{name}: quadratic |got - interpolant| = {errq:.3e} ({errq / (EPS * np.abs(q).max()):.2f} eps max|u|)")
    assert errq <= 64 * EPS * np.abs(q).max()


# ---- 4. the adaptive loop ---------------------------------------------------------------------------------------------
def _adaptive_loop(P, rounds=3):
    from phifem_amd.mesh_scripts import NodalFunction
    ctype, x0, cells0 = load_mesh("disk")
    cen = x0.mean(axis=0) + np.array([0.013, -0.007])
    r = 0.62 * 0.5 * (x0.max(axis=0) - x0.min(axis=0)).min()
    mesh = P.Mesh.from_arrays(ctype, x0, cells0)
    etas, eta2s, cells, conv = [], [], [], []
    for _ in range(rounds):
        x = mesh.x
        phi = ((x - cen) ** 2).sum(axis=1) - r ** 2
        uD = np.sin(x[:, 0]) * np.cos(x[:, 1])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=True, single_layer_cut=True)
            s = P.PhiFEMSolver(mesh, deterministic=True)
            s.assemble(phi, 2.0 * uD, uD)
            w = s.solve(rtol=1e-10)
        conv.append(s.stats["converged"])
        eta2 = s.estimate(w)
        eta2s.append(eta2)
        etas.append(float(np.sqrt(eta2.sum())))
        mesh = P.refine(mesh, marked=P.mark_dorfler(mesh, eta2, theta=0.5))
        cells.append(mesh.cells)
    return etas, eta2s, cells, conv


def test_adaptive_loop_on_disk(P):
    etas, eta2s, cells, conv = _adaptive_loop(P)
    print("eta per level:", etas, "cells:", [c.shape[0] for c in cells])
    assert all(conv)
    assert etas[-1] < etas[0]
    _, eta2s_b, cells_b, _ = _adaptive_loop(P)
    for a, b in zip(eta2s + cells, eta2s_b + cells_b):
        assert np.array_equal(a, b)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind(P):
    from phifem_amd import _lib as L
    ctype, x, cells = arrays("disk")
    coarse = P.Mesh.from_arrays(ctype, x, cells)
    quad = P.create_rectangle([[0.0, 0.0], [1.0, 1.0]], [3, 2], cell_type="quadrilateral")
    slab = P.create_box([0.0] * 3, [1.0] * 3, [2, 2, 2], offset=[0, 0, 2], n_global=[2, 2, 6])
    L.check(L.lib.phx_mesh_set_slab_faces(slab._h, 1, 1))
    assert coarse.ne + slab.ne > 0                           # (edge arrays are built on first use and stay)
    P.refine(coarse, marked=np.ones(coarse.nc, dtype=np.uint8))   # (first use of every staging buffer)
    before = live_bytes()
    with pytest.raises(NotImplementedError):
        P.refine(quad, marked=np.ones(quad.nc, dtype=np.uint8))
    assert live_bytes() == before
    with pytest.raises(NotImplementedError):                  # the C entry refuses as well
        h = C.c_void_p()
        L.check(L.lib.phx_mesh_refine_marked(quad._h, None, None, L.HOST, C.byref(h), None))
    assert live_bytes() == before
    for kw in ({"marked": np.ones(coarse.nc + 1, dtype=np.uint8)}, {"edges": np.ones(coarse.ne - 1, dtype=np.uint8)},
               {"marked": np.ones((coarse.nc, 1), dtype=np.uint8)}):
        with pytest.raises(ValueError):
            P.refine(coarse, **kw)
        assert live_bytes() == before
    with pytest.raises(ValueError):
        P.refine(slab, marked=np.ones(slab.nc, dtype=np.uint8))
    assert live_bytes() == before
    fine = P.refine(coarse, marked=RM.seeded_mask(coarse.nc))
    other = P.Mesh.from_arrays(ctype, x, cells)
    held = live_bytes()
    fine.coarse = other                                      # refined, but from another mesh
    with pytest.raises(ValueError):
        P.prolongate(fine, np.zeros(coarse.nv))
    fine.coarse = coarse
    with pytest.raises(ValueError):
        P.prolongate(fine, np.zeros(coarse.nv + 1))          # wrong length
    with pytest.raises(NotImplementedError):
        P.prolongate(fine, np.zeros(coarse.lagrange_ndofs(3)), degree=3)
    with pytest.raises(ValueError):
        coarse.parent_cells                                  # not made by marked refinement
    assert live_bytes() == held
    del fine, other
    assert live_bytes() == before
