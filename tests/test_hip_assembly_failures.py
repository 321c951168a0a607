"""A failed assembly gives back what it took: the bytes the library's device allocator has handed out
(`phx_pool_stats`) are the same after a second failing `assemble` as after the first one, for the four secondary
entry points (`phx_assemble_poisson_flux` on triangles and quadrilaterals, `phx_assemble_poisson_sd`,
`phx_assemble_elasticity_if` on quadrilaterals) and the Q1 path of `phx_assemble_poisson_wd`, and a valid assembly
of the same kind succeeds afterwards.  The comparison is exact: these are byte counters.  The first failing call may
build tables the MESH owns (integration entities, edges); they stay, so the first reading is taken after it.

Failures the library already raises:
 (a) "sheared": a 4 x 4 quadrilateral mesh whose cells are parallelograms -> NotImplementedError from the kernels'
     rectangle test, after numbering, work lists and slots were allocated;
 (b) "empty": no active DoF -> ValueError after the numbering.  The level-set r^2 + 1 is positive everywhere, so every
     cell of the 4 x 4 mesh is tagged 3 (outside).  Interface elasticity keeps u_out on the cells tagged 3 (every cell
     tagged 1, 2 or 3 carries DoFs there), so its cells get the user tag 4 through `overwrite_tags`, and no vertex is
     a Dirichlet vertex.
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
    quad = solver != "flux_tri" and solver != "sd_tri"
    mesh = make_mesh(P, "quadrilateral" if quad else "triangle", n, sheared=mode == "sheared")
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
    tag(P, mesh, phi)
    if solver == "sd_tri":
        return mesh, P.StrongDirichletSolver(mesh), (phi, np.ones(nv))
    # Neumann / Robin: a degree-2 level-set (P2: vertices + edges; Q2: vertices + facets + cells)
    pts = mesh.q2_dof_points() if quad else mesh.p2_dof_points()
    phi2 = (pts ** 2).sum(axis=1) + (1.0 if mode == "empty" else -1.0)
    return mesh, P.NeumannRobinSolver(mesh, facet_tag=3), (phi2, np.ones(nv), np.ones(nv))


CASES = [("flux_tri", "empty"), ("flux_quad", "empty"), ("flux_quad", "sheared"), ("sd_tri", "empty"),
         ("el_quad", "empty"), ("el_quad", "sheared"), ("wd_quad", "empty"), ("wd_quad", "sheared")]


@pytest.mark.parametrize("solver,mode", CASES)
def test_failed_assembly_releases_everything(P, solver, mode):
    error = NotImplementedError if mode == "sheared" else ValueError
    mesh, s, args = prepare(P, solver, mode, N)
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
    _, ok, ok_args = prepare(P, solver, "valid", 2 * N)
    info = ok.assemble(*ok_args)
    assert info["n_active"] > 0
