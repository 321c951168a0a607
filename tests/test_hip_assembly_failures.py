"""A failed assembly gives back what it took: the bytes the library's device allocator has handed out
(`phx_pool_stats`) are the same after a second failing `assemble` as after the first one, for the four secondary
entry points (`phx_assemble_poisson_flux` on triangles and quadrilaterals, `phx_assemble_poisson_sd`,
`phx_assemble_elasticity_if` on quadrilaterals), every path of `phx_assemble_poisson_wd` (Q1; P1 on a generated box
and on the box behind a caller-supplied Kuhn mesh) and `phx_assemble_poisson_wd_p2` (2-D; 3-D, whose valid follow-up
is a structured system), and a valid assembly of the same kind succeeds afterwards.  The comparison is exact: these are byte counters.  The first failing call may
build tables the MESH owns (integration entities, edges); they stay, so the first reading is taken after it.

Failures the library already raises:
 (a) "sheared": a 4 x 4 quadrilateral mesh whose cells are parallelograms -> NotImplementedError from the kernels'
     rectangle test, after numbering, work lists and slots were allocated;
 (b) "empty": no active DoF -> ValueError after the numbering.  The level-set r^2 + 1 is positive everywhere, so every
     cell of the 4 x 4 mesh is tagged 3 (outside).  Interface elasticity keeps u_out on the cells tagged 3 (every cell
     tagged 1, 2 or 3 carries DoFs there), so its cells get the user tag 4 through `overwrite_tags`, and no vertex is
     a Dirichlet vertex.

And a SUCCESSFUL assembly gives back everything but the system: assemble, drop solver and system, read the counter --
three rounds on one tagged mesh; the first may build mesh-owned tables (v2c, edges, entities, box codes), so rounds
two and three are compared (`test_dropped_system_releases_everything`).
"""
import ctypes as C
import gc
import warnings

import numpy as np
import pytest

from test_oracle_flux_quad import quad_mesh

pytestmark = pytest.mark.gpu
BBOX = [[-1.5, -1.5], [1.5, 1.5]]
N = 4


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def live_bytes(P):
    live, cached = C.c_int64(-1), C.c_int64(-1)
    P._lib.check(P._lib.lib.phx_pool_stats(C.byref(live), C.byref(cached)))
    assert live.value >= 0 and cached.value >= 0
    return live.value


def make_mesh(P, kind, n, sheared=False):
    if kind == "triangle":
        return P.create_box(BBOX[0], BBOX[1], [n, n])
    if kind == "tetrahedron":
        return P.create_box([-1.5] * 3, [1.5] * 3, [n] * 3)
    if kind == "triangle_arrays":       # the Kuhn triangles as a caller's arrays: served by the generated box behind them
        box = P.create_box(BBOX[0], BBOX[1], [n, n])
        return P.Mesh.from_arrays("triangle", box.x, box.cells)
    x, cells = quad_mesh(n)
    if sheared:
        x = x.copy()
        x[:, 0] += 0.2 * x[:, 1]
    return P.Mesh.from_arrays("quadrilateral", x, cells.astype(np.int32))


def tag(P, mesh, phi, **kw):
    from phifem_amd.mesh_scripts import NodalFunction
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=True, **kw)


def prepare(P, solver, mode, n):
    """-> (tagged mesh, Solver instance, arguments of its assemble) for mode "valid" | "sheared" | "empty"."""
    from phifem_amd.mesh import MeshTags
    quad = solver != "flux_tri" and solver != "sd_tri" and solver not in WD_SIMPLEX
    kind = WD_SIMPLEX.get(solver, "quadrilateral" if quad else "triangle")
    mesh = make_mesh(P, kind, n, sheared=mode == "sheared")
    r2 = (mesh.x ** 2).sum(axis=1)
    phi = r2 + 1.0 if mode == "empty" else r2 - 1.0
    nv = mesh.nv
    if solver == "el_quad":
        extra = {}
        if mode != "empty":
            phi = -phi                                                 # data.py:39-40: positive inside
        else:
            extra["overwrite_tags"] = {"cells": MeshTags(2, np.arange(mesh.nc), np.full(mesh.nc, 4))}
        tag(P, mesh, phi, **extra)
        bcv = np.zeros(0, dtype=np.int32) if mode == "empty" else np.unique(mesh.cells[:2].reshape(-1))
        return mesh, P.InterfaceElasticitySolver(mesh), (phi, np.zeros((nv, 2)), np.zeros((nv, 2)), bcv)
    if solver == "wd_quad":
        tag(P, mesh, phi, single_layer_cut=True)
        return mesh, P.PhiFEMSolver(mesh), (phi, np.ones(nv), np.ones(nv))
    if solver in WD_SIMPLEX:
        tag(P, mesh, phi, single_layer_cut=True)
        if "p2" not in solver:
            return mesh, P.PhiFEMSolver(mesh), (phi, np.ones(nv), np.ones(nv))
        nd = nv + mesh.ne
        return mesh, P.PhiFEMSolver(mesh, degree=2), (phi, np.ones(nd), np.ones(nd))
    tag(P, mesh, phi)
    if solver == "sd_tri":
        return mesh, P.StrongDirichletSolver(mesh), (phi, np.ones(nv))
    # Neumann / Robin: a degree-2 level-set (P2: vertices + edges; Q2: vertices + facets + cells)
    pts = mesh.q2_dof_points() if quad else mesh.p2_dof_points()
    phi2 = (pts ** 2).sum(axis=1) + (1.0 if mode == "empty" else -1.0)
    return mesh, P.NeumannRobinSolver(mesh, facet_tag=3), (phi2, np.ones(nv), np.ones(nv))


# PhiFEMSolver on simplices -> the mesh it runs on; cells per direction where that is not N
WD_SIMPLEX = {"wd_p1_tri": "triangle", "wd_p1_inner": "triangle_arrays", "wd_p2_tri": "triangle",
              "wd_p2_tet": "tetrahedron"}
SIZES = {"wd_p2_tet": 3}
CASES = [("flux_tri", "empty"), ("flux_quad", "empty"), ("flux_quad", "sheared"), ("sd_tri", "empty"),
         ("el_quad", "empty"), ("el_quad", "sheared"), ("wd_quad", "empty"), ("wd_quad", "sheared"),
         ("wd_p1_tri", "empty"), ("wd_p1_inner", "empty"), ("wd_p2_tri", "empty"), ("wd_p2_tet", "empty")]


@pytest.mark.parametrize("solver,mode", CASES)
def test_failed_assembly_releases_everything(P, solver, mode):
    error = NotImplementedError if mode == "sheared" else ValueError
    n = SIZES.get(solver, N)
    mesh, s, args = prepare(P, solver, mode, n)
    if mode == "empty":
        assert not np.isin(mesh.cell_tag_values(), (1, 2)).any()
    gc.collect()                       # systems of earlier tests are released now, not between the two readings
    with pytest.raises(error):
        s.assemble(*args)
    first = live_bytes(P)
    with pytest.raises(error):
        s.assemble(*args)
    second = live_bytes(P)
    print(f"{solver} / {mode}: live bytes after the first failure {first}, after the second {second}")
    assert second == first
    # a failed assembly does not poison the next one
    _, ok, ok_args = prepare(P, solver, "valid", 2 * n)
    info = ok.assemble(*ok_args)
    assert info["n_active"] > 0
    # the route: nothing a mesh exposes names it for the FAILED calls; the valid system shows it
    if solver in ("wd_p1_inner", "wd_p2_tet"):
        # structured systems never form the CSR copy: P1 only on a generated box (here the one behind the arrays), P2
        # only on a 3-D one
        assert info["has_csr"] == 0


def alternating_triangles(P, n):
    """n x n squares over BBOX, the diagonal alternating with the parity of the square -- not the Kuhn split, so no
    generated box stands behind the mesh -- in a random vertex, cell and local order."""
    g = np.linspace(BBOX[0][0], BBOX[1][0], n + 1)
    x = np.stack([np.tile(g, n + 1), np.repeat(g, n + 1)], axis=1)
    i, j = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    a = i + (n + 1) * j
    b, c, d = a + 1, a + n + 1, a + n + 2
    even = ((i + j) % 2 == 0)[:, None]
    cells = np.concatenate([np.where(even, np.stack([a, b, d], 1), np.stack([a, b, c], 1)),
                            np.where(even, np.stack([a, d, c], 1), np.stack([b, d, c], 1))])
    rng = np.random.default_rng(3)
    perm = rng.permutation(x.shape[0])
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    cs = inv[cells][rng.permutation(cells.shape[0])]
    cs = np.take_along_axis(cs, rng.permuted(np.tile(np.arange(3), (cs.shape[0], 1)), axis=1), axis=1)
    return P.Mesh.from_arrays("triangle", x[perm], cs.astype(np.int32))


# case -> (mesh: d, n | "alternating" | "submesh", degree, deterministic, PHX_OPT_EXPORT_CSR)
DROPPED = {"p1_box_2d": ((2, 8), 1, False, False), "p1_box_3d": ((3, 4), 1, False, False),
           "p1_box_2d_export_csr": ((2, 8), 1, False, True), "p1_submesh_2d": ("submesh", 1, False, False),
           "p1_alternating_det": ("alternating", 1, True, False), "p2_2d": ((2, 4), 2, False, False),
           "p2_3d_structured": ((3, 4), 2, False, False), "p2_2d_det": ((2, 4), 2, True, False)}


@pytest.mark.parametrize("case", list(DROPPED))
def test_dropped_system_releases_everything(P, case):
    from phifem_amd import _lib as L
    from phifem_amd.mesh_scripts import NodalFunction
    what, degree, det, export = DROPPED[case]
    if what == "alternating":
        mesh = alternating_triangles(P, 8)
    else:
        d, n = (2, 8) if what == "submesh" else what
        mesh = P.create_box([-1.5] * d, [1.5] * d, [n] * d)
    phi = (mesh.x ** 2).sum(axis=1) - 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # (the single-layer pass leaves the 4^3 box without a cell tagged 1 or 2: plain tags in 3-D)
        sub = P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=what != "submesh",
                                      single_layer_cut=mesh.gdim == 2)[2]
    work = sub if what == "submesh" else mesh
    phi = (work.x ** 2).sum(axis=1) - 1.0
    nd = work.nv + (work.ne if degree == 2 else 0)
    L.check(L.lib.phx_set_option(work._h, L.OPT_EXPORT_CSR, int(export)))
    live = []
    for _ in range(3):
        s = P.PhiFEMSolver(work, degree=degree, deterministic=det)
        info = s.assemble(phi, np.ones(nd), np.ones(nd))
        assert info["n_active"] > 0
        # the path: structured (stencil rows, no CSR copy) only for a box without PHX_OPT_EXPORT_CSR; P2 only in 3-D
        structured = isinstance(what, tuple) and not export and (degree == 1 or what[0] == 3)
        assert (info["has_csr"] == 0) == structured, info
        del s, info
        gc.collect()
        live.append(live_bytes(P))
    L.check(L.lib.phx_set_option(work._h, L.OPT_EXPORT_CSR, 0))
    print(f"{case}: live bytes after each round {live}")
    assert live[2] == live[1]
