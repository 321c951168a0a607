"""Point location and evaluation of P1 / P2 / Q1 functions on the GPU (`phifem_amd.locate`, `evaluate`,
`interpolate_nonmatching`) against the numpy specification tests/locate_ref.py: a brute-force containment test of all
cells against all points with the smallest-index rule, and bases written from their definitions.

INPUT CONDITION, asserted from the reference alone (tests/test_locate_ref.py::test_input_condition for the
caller-supplied meshes, here for the generated ones): the smallest reference coordinate of every (point, cell) pair is
>= -1e-14 or <= -1e-9, so no pair sits at the tolerance 1e-12 where round-off could decide."""
import ctypes as C
import warnings

import numpy as np
import pytest

import flower_data as FD
import locate_ref as LR
from locate_cases import BOX, CALLER, GENERATED, MESHES, arrays, case_points, reference_caller

pytestmark = pytest.mark.gpu
TOL = 1e-12          # the project's oracle tolerance (relative to max|u|)


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


_MESH_CACHE = {}


def get_mesh(P, name):
    """-> (mesh, cell type, x, cells); one device mesh per name for the whole module (its locator is built once)."""
    if name not in _MESH_CACHE:
        if name == "box_3d":
            mesh = P.create_box(*BOX)
        elif name == "box_2d":
            mesh = P.create_box(BOX[0][:2], BOX[1][:2], BOX[2][:2])
        elif name == "box_slab":     # cubes 2 .. 3 of the last axis of the same box
            mesh = P.create_box(BOX[0], BOX[1], [3, 4, 2], offset=[0, 0, 2], n_global=BOX[2])
        else:
            ctype, x, cells = arrays(name)
            mesh = P.Mesh.from_arrays(ctype, x, cells)
        if name in GENERATED:
            _MESH_CACHE[name] = (mesh, mesh.cell_type, mesh.x, mesh.cells.astype(np.int64))
        else:
            _MESH_CACHE[name] = (mesh,) + arrays(name)
    return _MESH_CACHE[name]


_REF_GENERATED = {}


def reference(P, name):
    """(points, number of centroids, cell, xref, holds, input condition) of the specification, once per mesh."""
    if name in CALLER:
        return reference_caller(name)
    if name not in _REF_GENERATED:
        _, ctype, x, cells = get_mesh(P, name)
        pts, ncen = case_points(ctype, x, cells, lattice=True)
        _REF_GENERATED[name] = (pts, ncen) + LR.locate_ref(ctype, x, cells, pts) + (LR.input_condition(ctype, x, cells, pts),)
    return _REF_GENERATED[name]


_LOCATED = {}


def located(P, name):
    """The device's (cells, xref) of the test points, once per mesh."""
    if name not in _LOCATED:
        _LOCATED[name] = P.locate(get_mesh(P, name)[0], reference(P, name)[0])
    return _LOCATED[name]


def live_bytes():
    from phifem_amd import _lib as L
    a, b = C.c_int64(0), C.c_int64(0)
    L.check(L.lib.phx_pool_stats(C.byref(a), C.byref(b)))
    return a.value


def min_height(ctype, x, cells):
    """The smallest height of a cell (rectangles: side): 1 / max |grad lambda_i|, the scale of the basis gradients."""
    Ji = np.linalg.inv(LR.jacobians(ctype, x, cells))                 # rows: gradients of the reference coordinates
    g = np.linalg.norm(Ji, axis=2)
    if ctype != "quadrilateral":
        g = np.concatenate([g, np.linalg.norm(Ji.sum(axis=1), axis=1)[:, None]], axis=1)
    return 1.0 / g.max()


# ---- 1. location ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_location(P, name):
    mesh, ctype, x, cells = get_mesh(P, name)
    pts, ncen, rcell, rxref, holds, cond = reference(P, name)
    if name in GENERATED:      # (the caller-supplied meshes: tests/test_locate_ref.py::test_input_condition, on the CPU)
        assert cond, "input condition: a (point, cell) pair sits at the tolerance"
    info = P.locator_info(mesh)
    gcell, gxref = located(P, name)
    assert isinstance(gcell, np.ndarray) and gcell.dtype == np.int32 and gcell.shape == (pts.shape[0],)
    assert gxref.shape == pts.shape
    assert np.array_equal(gcell[:ncen], np.arange(ncen)), "a centroid is not in its own cell"
    assert np.array_equal(gcell < 0, rcell < 0), "-1 exactly where the reference finds no cell"
    assert (rcell < 0).sum() > 0 and (rcell[ncen:] >= 0).sum() > 0
    ok = gcell >= 0
    if name in GENERATED:
        assert info["path"] == "closed-form" and info["pairs"] == 0 and info["bytes"] == 0 and not info["built"]
        assert holds[np.flatnonzero(ok), gcell[ok]].all(), "a returned cell does not hold its point"
    else:
        assert np.array_equal(gcell, rcell), "not the smallest-index cell of the reference"
        after = P.locator_info(mesh)
        assert after["path"] == "bins" and after["built"] and after["pairs"] >= mesh.nc and after["bytes"] > 0
        assert after["pairs"] <= 16 * mesh.nc or all(b == 1 for b in after["bins"])
    # basis reconstruction: the P1 / Q1 basis at xref applied to the cell's vertices gives the point back
    N, _ = LR.basis(ctype, 1, gxref[ok])
    back = np.einsum("pk,pka->pa", N, x[cells[gcell[ok]]])
    err = np.abs(back - pts[ok]).max()
    extent = (x.max(axis=0) - x.min(axis=0)).max()
    print(f"{name}: {pts.shape[0]} points, {int((~ok).sum())} outside, reconstruction {err / extent:.2e} of the extent, {info}")
    assert err <= 1e-12 * extent


# ---- 2. values --------------------------------------------------------------------------------------------------------
def _poly(p, degree, ctype):
    lin = 0.3 + p @ (0.7 * np.arange(1, p.shape[1] + 1))
    if ctype == "quadrilateral":
        return lin + 0.6 * p[:, 0] * p[:, 1]                     # bilinear
    return lin if degree == 1 else lin + p[:, 0] * p[:, -1] - 0.4 * p[:, 0] ** 2 + 0.9 * p[:, -1] ** 2


def _degrees(ctype):
    return (1,) if ctype == "quadrilateral" else (1, 2)


@pytest.mark.parametrize("name", MESHES)
def test_polynomial_reproduction(P, name):
    """P1 reproduces a linear function, P2 a quadratic, Q1 a bilinear one."""
    mesh, ctype, x, cells = get_mesh(P, name)
    pts = reference(P, name)[0]
    gcell, gxref = located(P, name)
    ok = gcell >= 0
    for degree in _degrees(ctype):
        nodes = mesh.lagrange_dof_points(degree)
        u = _poly(nodes, degree, ctype)
        got = P.evaluate(mesh, u, pts, degree=degree, located=(gcell, gxref))
        err = np.abs(got[ok] - _poly(pts[ok], degree, ctype)).max()
        print(f"{name} degree {degree}: reproduction error {err / np.abs(u).max():.2e} max|u|")
        assert err <= TOL * np.abs(u).max()
        assert np.all(np.isnan(got[~ok]))


@pytest.mark.parametrize("name", MESHES)
def test_random_functions_against_reference(P, name):
    mesh, ctype, x, cells = get_mesh(P, name)
    pts = reference(P, name)[0]
    gcell, gxref = located(P, name)
    ok = gcell >= 0
    hmin = min_height(ctype, x, cells)
    rng = np.random.default_rng(31)
    for degree in _degrees(ctype):
        c2e = mesh.c2e.astype(np.int64) if degree == 2 else None
        ndofs = mesh.lagrange_ndofs(degree)
        for shape in [(ndofs,), (3, ndofs)]:
            u = rng.standard_normal(shape)
            rval, rgrad = LR.evaluate_ref(ctype, x, cells, u, gcell, gxref, degree, c2e, fill=-3.5)
            val, grad = P.evaluate(mesh, u, pts, degree=degree, gradient=True, fill=-3.5, located=(gcell, gxref))
            assert val.shape == rval.shape == shape[:-1] + (pts.shape[0],) and grad.shape == rgrad.shape
            ev = np.abs(val - rval).max()
            eg = np.abs(grad - rgrad).max()
            umax = np.abs(u).max()
            print(f"{name} degree {degree} ncomp {len(shape) * 2 - 1}: values {ev / umax:.2e} max|u|, "
                  f"gradients {eg * hmin / umax:.2e} max|u| / h_min")
            assert ev <= TOL * umax
            assert eg <= TOL * umax / hmin
            assert np.all(val[..., ~ok] == -3.5) and np.all(grad[..., ~ok, :] == -3.5)      # fill exactly at the -1 points
            assert not np.any(val[..., ok] == -3.5)
            only = P.evaluate(mesh, u, pts, degree=degree, fill=-3.5, located=(gcell, gxref))
            assert np.array_equal(only, val)


# ---- 3. the nested special case ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["single_triangle", "single_tetrahedron", "single_quadrilateral", "disk", "square_quad",
                                  "graded_tet_box", "box_3d"])
def test_nested_equals_prolongate(P, name):
    mesh, ctype, x, cells = get_mesh(P, name)
    fine = P.refine(mesh)
    rng = np.random.default_rng(41)
    for degree in _degrees(ctype):
        u = rng.standard_normal((2, mesh.lagrange_ndofs(degree)))
        want = P.prolongate(fine, u, degree=degree)
        got = P.evaluate(mesh, u, fine.lagrange_dof_points(degree), degree=degree)
        # a vertex that belongs to no cell (vertex 0 of `disk`, the centre its mesher left behind) carries no part of the
        # function: prolongate copies its value, evaluate reads the cell that covers its coordinates
        used = np.zeros(mesh.lagrange_ndofs(degree), dtype=bool)
        used[cells.reshape(-1)] = True
        used[mesh.nv:] = True
        keep = np.ones(want.shape[-1], dtype=bool)
        keep[:used.size] = used
        err = np.abs(got - want)[:, keep].max()
        print(f"{name} degree {degree}: |evaluate - prolongate| = {err / np.abs(u).max():.2e} max|u|, "
              f"{int((~keep).sum())} vertices in no cell")
        assert not np.any(np.isnan(got)) and err <= TOL * np.abs(u).max() and (~keep).sum() <= 1


# ---- 4. generated box against the same arrays through from_arrays ------------------------------------------------------
def test_generated_box_equals_caller_arrays(P):
    """The same box, generated (closed form) and handed over with shuffled vertices and cells (bins): the same function
    -- the interpolant of one smooth expression at each mesh's own DoF points -- has the same values; cell ids differ."""
    box = get_mesh(P, "box_3d")[0]
    twin = get_mesh(P, "box_shuffled")[0]
    pts = reference(P, "box_3d")[0]

    def f(p):
        return np.sin(1.3 * p[:, 0] + 0.4) * np.cos(0.7 * p[:, 1]) + 0.3 * p[:, 2] ** 3

    for degree in (1, 2):
        ua, ub = f(box.lagrange_dof_points(degree)), f(twin.lagrange_dof_points(degree))
        a, b = P.evaluate(box, ua, pts, degree=degree), P.evaluate(twin, ub, pts, degree=degree)
        assert np.array_equal(np.isnan(a), np.isnan(b))
        ok = ~np.isnan(a)
        err = np.abs(a[ok] - b[ok]).max()
        print(f"degree {degree}: generated box against shuffled arrays {err / np.abs(ua).max():.2e} max|u|")
        assert ok.sum() > 1000 and err <= TOL * np.abs(ua).max()
    assert P.locator_info(box)["path"] == "closed-form" and P.locator_info(twin)["path"] == "bins"


# ---- 5. sub-meshes and non-matching meshes ----------------------------------------------------------------------------
def test_submesh_points_outside_get_minus_one(P):
    from phifem_amd.mesh_scripts import NodalFunction
    bg = P.create_rectangle([[-4.5, -4.5], [4.5, 4.5]], [24, 24])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, sub, _, maps = P.compute_tags_measures(bg, NodalFunction(FD.detection_levelset(bg.x.T)), 1, box_mode=False,
                                                     single_layer_cut=True)
    c_map = maps[0]
    xb, cb = bg.x, bg.cells
    pts = xb[cb].mean(axis=1)                                   # one point strictly inside every background cell
    got, _ = P.locate(sub, pts)
    want = np.full(bg.nc, -1, dtype=np.int32)
    want[c_map] = np.arange(sub.nc, dtype=np.int32)
    assert 0 < sub.nc < bg.nc and np.array_equal(got, want)
    assert P.locator_info(sub)["path"] == "bins"
    u = np.random.default_rng(5).standard_normal(sub.nv)
    val = P.evaluate(sub, u, pts)
    assert np.array_equal(np.isnan(val), want < 0)
    rv, _ = LR.evaluate_ref("triangle", sub.x, sub.cells.astype(np.int64), u, got, P.locate(sub, pts)[1])
    assert np.abs(val[want >= 0] - rv[want >= 0]).max() <= TOL * np.abs(u).max()


@pytest.mark.parametrize("kind", ["triangle", "quadrilateral"])
def test_interpolate_nonmatching(P, kind):
    import torch
    src = P.create_rectangle([[-4.5, -4.5], [4.5, 4.5]], [24, 24], cell_type=kind)
    dst = P.create_rectangle([[-4.5, -4.5], [4.5, 4.5]], [17, 17], cell_type=kind)
    xs, cs, xd = src.x, src.cells.astype(np.int64), dst.x
    u = np.random.default_rng(7).standard_normal((2, src.nv))
    rcell, rxref, _ = LR.locate_ref(kind, xs, cs, xd)
    assert LR.input_condition(kind, xs, cs, xd) and np.all(rcell >= 0)
    want, _ = LR.evaluate_ref(kind, xs, cs, u, rcell, rxref)
    got = P.interpolate_nonmatching(dst, src, u)
    assert isinstance(got, np.ndarray) and got.shape == (2, dst.nv)
    assert np.abs(got - want).max() <= TOL * np.abs(u).max()
    gd = P.interpolate_nonmatching(dst, src, torch.from_numpy(u[1]).cuda())
    assert gd.is_cuda and np.array_equal(gd.cpu().numpy(), got[1])
    from phifem_amd.mesh_scripts import NodalFunction
    nf = P.interpolate_nonmatching(dst, src, NodalFunction(u[0], 1))
    assert isinstance(nf, NodalFunction) and nf.degree == 1 and np.array_equal(nf.values, got[0])


# ---- 6. kinds and errors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["disk", "box_3d", "square_quad"])
def test_kinds_and_bits(P, name):
    import torch
    mesh, ctype, x, cells = get_mesh(P, name)
    pts = reference(P, name)[0]
    u = np.random.default_rng(3).standard_normal((2, mesh.nv))
    c1, r1 = P.locate(mesh, pts)
    pt = torch.from_numpy(pts).cuda()
    c2, r2 = P.locate(mesh, pt)
    assert c2.is_cuda and c2.dtype == torch.int32 and r2.is_cuda and r2.dtype == torch.float64
    assert np.array_equal(c2.cpu().numpy(), c1) and np.array_equal(r2.cpu().numpy(), r1)        # two runs, the same bits
    v1, g1 = P.evaluate(mesh, u, pts, gradient=True)
    v2, g2 = P.evaluate(mesh, torch.from_numpy(u).cuda(), pt, gradient=True, located=(c2, r2))
    assert isinstance(v1, np.ndarray) and v2.is_cuda and g2.is_cuda
    assert np.array_equal(v2.cpu().numpy(), v1, equal_nan=True) and np.array_equal(g2.cpu().numpy(), g1, equal_nan=True)
    v3 = P.evaluate(mesh, u, pts, located=(c1, r1))
    assert np.array_equal(v3, v1, equal_nan=True)
    perm = np.random.default_rng(4).permutation(pts.shape[0])                                   # the order of the points
    cp, rp = P.locate(mesh, np.ascontiguousarray(pts[perm]))
    assert np.array_equal(cp, c1[perm]) and np.array_equal(rp, r1[perm])
    from phifem_amd.mesh_scripts import NodalFunction
    assert np.array_equal(P.evaluate(mesh, NodalFunction(u[0], 1), pts, degree=2), v1[0], equal_nan=True)
    t = mesh.timings()
    assert t["locate"] > 0.0 and t["evaluate"] > 0.0 and {"tag_cells", "solve", "refine_kernels", "locate_build"} <= set(t)


def test_refusals_leave_nothing_behind(P):
    P.create_box([0.0] * 3, [1.0] * 3, [2, 2, 2]).ne          # (first use of the pool and of the read-back staging)
    start = live_bytes()
    ctype, x, cells = arrays("square_quad")
    quad = P.Mesh.from_arrays(ctype, x, cells)
    tri = P.Mesh.from_arrays(*arrays("disk"))
    pq, pt = x[:5].copy(), arrays("disk")[1][:5].copy()
    P.locate(quad, pq), P.locate(tri, pt), tri.ne               # locators and edges are built: they stay with the meshes
    before = live_bytes()
    failing = [
        (NotImplementedError, lambda: P.evaluate(quad, np.zeros(quad.lagrange_ndofs(2)), pq, degree=2)),
        (NotImplementedError, lambda: P.evaluate(tri, np.zeros(tri.lagrange_ndofs(3)), pt, degree=3)),
        (ValueError, lambda: P.locate(tri, pt, tol=-1e-3)),
        (ValueError, lambda: P.evaluate(tri, np.zeros(tri.nv), pt, tol=-1.0)),
        (ValueError, lambda: P.locate(tri, np.zeros((4, 3)))),
        (ValueError, lambda: P.locate(tri, np.zeros(6))),
        (ValueError, lambda: P.evaluate(tri, np.zeros(tri.nv + 1), pt)),
        (ValueError, lambda: P.evaluate(tri, np.zeros((2, 2, tri.nv)), pt)),
        (ValueError, lambda: P.evaluate(tri, np.zeros(tri.nv), pt, located=(np.zeros(4, dtype=np.int32), np.zeros((5, 2))))),
    ]
    for exc, call in failing:
        with pytest.raises(exc):
            call()
        assert live_bytes() == before
    from phifem_amd import _lib as L
    buf = np.zeros(64)
    ibuf = np.zeros(8, dtype=np.int32)
    for handle, deg in ((quad._h, 2), (tri._h, 3)):             # the C entry refuses as well
        rc = L.lib.phx_eval_points(handle, deg, 1, buf.ctypes.data_as(C.c_void_p), L.HOST, 2,
                                   ibuf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), L.HOST, 0, 0.0,
                                   buf.ctypes.data_as(C.c_void_p), None, L.HOST)
        with pytest.raises(NotImplementedError):
            L.check(rc)
    rc = L.lib.phx_locate_points(tri._h, 2, buf.ctypes.data_as(C.c_void_p), L.HOST, -1.0,
                                 ibuf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), L.HOST)
    with pytest.raises(ValueError):
        L.check(rc)
    assert live_bytes() == before
    # a quadrilateral mesh with one vertex moved is no mesh of rectangles: refused before anything is kept
    xm = x.copy()
    xm[cells[len(cells) // 2, 3]] += [0.01, 0.003]
    bent = P.Mesh.from_arrays(ctype, xm, cells)
    held = live_bytes()
    with pytest.raises(NotImplementedError):
        P.locate(bent, pq)
    assert live_bytes() == held
    with pytest.raises(NotImplementedError):
        P.evaluate(bent, np.zeros(bent.nv), pq, located=(np.zeros(5, dtype=np.int32), np.zeros((5, 2))))
    assert live_bytes() == held and not P.locator_info(bent)["built"]
    del bent
    assert live_bytes() == before
    del failing, call, handle, quad, tri
    assert live_bytes() == start


def test_tensor_on_the_host_is_refused(P):
    import torch
    mesh = get_mesh(P, "disk")[0]
    with pytest.raises(ValueError):
        P.locate(mesh, torch.zeros((3, 2), dtype=torch.float64))            # a tensor that is not on the mesh's GPU
    with pytest.raises(ValueError):
        P.evaluate(mesh, torch.zeros(mesh.nv, dtype=torch.float64), np.zeros((3, 2)))


# ---- 7. sizes where indexing can go wrong -----------------------------------------------------------------------------
def _linear(p):
    return 0.25 + p[:, 0] - 2.0 * p[:, 1] + 0.5 * p[:, 2]


def test_large_generated_box(P):
    import torch
    mesh = P.create_box([-1.0, 0.0, 0.5], [1.0, 1.5, 2.0], [64, 64, 64])
    dev = torch.device("cuda", mesh.device)
    gen = torch.Generator(device=dev).manual_seed(1)
    lo = torch.tensor([-1.0, 0.0, 0.5], dtype=torch.float64, device=dev)
    ext = torch.tensor([2.0, 1.5, 1.5], dtype=torch.float64, device=dev)
    pts = lo - 0.05 * ext + 1.1 * ext * torch.rand((1000000, 3), dtype=torch.float64, device=dev, generator=gen)
    cell, xref = P.locate(mesh, pts)
    inside = torch.all((pts >= lo) & (pts <= lo + ext), dim=1)
    assert torch.equal(cell >= 0, inside) and 0 < int(inside.sum()) < pts.shape[0]
    # containment on the device: the point is the barycentric combination of the returned cell's vertices
    x = mesh.lagrange_dof_points(1, device=True)
    cells = torch.from_numpy(mesh.cells.astype(np.int64)).to(dev)
    ok = cell >= 0
    lam = torch.cat([1.0 - xref.sum(dim=1, keepdim=True), xref], dim=1)[ok]
    assert float(lam.min()) >= -1e-12 and float(lam.max()) <= 1.0 + 1e-12
    back = torch.einsum("pk,pka->pa", lam, x[cells[cell[ok].long()]])
    assert float((back - pts[ok]).abs().max()) <= 1e-12 * 2.0
    u = _linear(x)
    val = P.evaluate(mesh, u, pts, located=(cell, xref))
    assert float((val[ok] - _linear(pts[ok])).abs().max()) <= TOL * float(u.abs().max())
    assert bool(torch.isnan(val[~ok]).all())
    assert P.locator_info(mesh)["bytes"] == 0


def test_large_refined_graded_mesh(P):
    import torch
    mesh = P.refine(P.refine(get_mesh(P, "graded_tet_box")[0]))
    dev = torch.device("cuda", mesh.device)
    gen = torch.Generator(device=dev).manual_seed(2)
    pts = -1.6 + 3.2 * torch.rand((100000, 3), dtype=torch.float64, device=dev, generator=gen)
    cell, xref = P.locate(mesh, pts)
    info = P.locator_info(mesh)
    print(f"refined graded box: {mesh.nc} cells, {info}, timings {mesh.timings()}")
    assert info["path"] == "bins" and mesh.nc <= info["pairs"] <= 16 * mesh.nc
    inside = torch.all(pts.abs() <= 1.5, dim=1)
    assert torch.equal(cell >= 0, inside) and 0 < int(inside.sum()) < pts.shape[0]
    x = mesh.lagrange_dof_points(1, device=True)
    u = _linear(x)
    ok = cell >= 0
    val = P.evaluate(mesh, u, pts, located=(cell, xref))
    assert float((val[ok] - _linear(pts[ok])).abs().max()) <= TOL * float(u.abs().max())
    assert float(xref[ok].min()) >= -1e-12 and float(xref[ok].sum(dim=1).max()) <= 1.0 + 1e-12
