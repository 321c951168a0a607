"""GPU parity of weak-Dirichlet elasticity (`phifem_amd.ElasticitySolver`, `phx_assemble_elasticity_wd`) against its
numpy specification tests/elasticity_wd_ref.py.  Tolerances are those of the other slot-scattered assemblies
(tests/test_hip_elasticity.py): 1e-11 relative to the largest matrix / vector entry (atomic accumulation order, FMA)."""
import ctypes as C
import functools
import gc
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import elasticity_wd_ref as R
import hub_meshes as H
from datasets import load_mesh
from oracle.topology import Topology

pytestmark = pytest.mark.gpu
CENTRE = (0.04, -0.03, 0.02)
TOL = 1e-11
HUB_INSIDE, HUB_ABOVE = "p1_3d_d_retry", "p1_3d_e_refusal"    # widest rows 233 (-> capacity 256) and 783 (> 512)
CAPACITIES = {2: (64, 128, 256), 3: (128, 256, 512)}           # the retry ladder of phx_assemble_elasticity_wd


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def live_bytes(P):
    live, cached = C.c_int64(-1), C.c_int64(-1)
    P._lib.check(P._lib.lib.phx_pool_stats(C.byref(live), C.byref(cached)))
    assert live.value >= 0
    return live.value


def tag(P, mesh, phi, box_mode=True):
    from phifem_amd.mesh_scripts import NodalFunction
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=box_mode, single_layer_cut=True)


def smooth_data(x, seed=5):
    d = x.shape[1]
    rng = np.random.default_rng(seed)
    return np.sin(x @ rng.standard_normal((d, d))) + 0.3, np.cos(x @ rng.standard_normal((d, d)))


def spec(work, ds, phi, f, uD, **par):
    """The specification's system on the library's own numbering -> (active CSR, active rhs, active indices, A, b, act)."""
    ctype = "triangle" if work.gdim == 2 else "tetrahedron"
    topo = Topology(ctype, work.cells.astype(np.int64), work.nv)
    topo.c2f, topo.f2c, topo.nf = work.c2f.astype(np.int64), work.f2c.astype(np.int64), work.nf
    A, b, act = R.assemble_elasticity_wd(topo, work.x, work.cell_tag_values(), work.facet_tag_values(), ds, phi, f, uD, **par)
    idx = np.flatnonzero(act)
    return A[idx][:, idx].tocsr(), b[idx], idx, A, b, act


@functools.lru_cache(maxsize=None)
def box_case(d, n, box_mode=True):
    """Generated box, tagged by the library -> (mesh the solver works on, its ds entities, phi on its vertices)."""
    import phifem_amd as P
    mesh = P.create_box([-1.5] * d, [1.5] * d, [n] * d)
    phi = ((mesh.x - np.asarray(CENTRE)[:d]) ** 2).sum(axis=1) - 1.0
    _, _, sub, meas, maps = tag(P, mesh, phi, box_mode)
    if box_mode:
        return mesh, meas(100), phi
    return sub, sub.boundary_facets.reshape(-1), phi[maps[1]]      # vertex map of phx_submesh_maps


def compare(s, info, Ao, bo, idx, label):
    rowptr, col, val, rhs, dof = s.export_csr()
    assert info["n_active"] == idx.size and np.array_equal(dof, idx), "active DoF numbering differs"
    Hm = sp.csr_matrix((val, col, rowptr), shape=(idx.size, idx.size))
    scale = np.abs(Ao.data).max()
    xv = np.random.default_rng(0).standard_normal(idx.size)
    y, yo = s.spmv(xv), Ao @ xv
    errs = (abs(Hm - Ao).max() / scale, np.abs(rhs - bo).max() / max(np.abs(bo).max(), 1e-300),
            np.abs(y - yo).max() / np.abs(yo).max())
    print(f"{label}: n_active={idx.size} nnz={Hm.nnz} widest row {int(np.diff(Ao.indptr).max())} slot_capacity="
          f"{info['slot_capacity']} | relative errors: matrix {errs[0]:.2e} rhs {errs[1]:.2e} spmv {errs[2]:.2e}")
    assert errs[0] <= TOL and errs[1] <= TOL and errs[2] <= TOL
    return Hm, rhs


@pytest.mark.parametrize("d,n,nu", [(2, 12, 0.3), (2, 16, 0.3), (2, 16, 0.45), (3, 5, 0.3), (3, 6, 0.3), (3, 6, 0.45)])
def test_matrix_rhs_active_set_and_spmv_vs_specification(P, d, n, nu):
    mesh, ds, phi = box_case(d, n)
    f, uD = smooth_data(mesh.x)
    par = dict(E=1.3, nu=nu, pen_coef=1.2, stab_coef=0.8)
    Ao, bo, idx, *_ = spec(mesh, ds, phi, f, uD, **par)
    s = P.ElasticitySolver(mesh, **par)
    info = s.assemble(phi, f, uD)
    assert info["n_full"] == 2 * d * mesh.nv and info["slot_capacity"] == CAPACITIES[d][0]
    compare(s, info, Ao, bo, idx, f"box d={d} n={n} nu={nu}")
    u, p = s.split(np.arange(2.0 * d * mesh.nv))
    assert u.shape == (mesh.nv, d) and p.shape == (mesh.nv, d) and u[3, d - 1] == (d - 1) * mesh.nv + 3
    with pytest.raises(NotImplementedError):
        s.estimate(np.zeros(2 * d * mesh.nv))


@pytest.mark.parametrize("d,n", [(2, 12), (3, 5)])
def test_submesh_mode_vs_specification(P, d, n):
    """box_mode=False: the solver works on the sub-mesh, ds is every exterior facet of it."""
    sub, ds, phi = box_case(d, n, False)
    assert sub.nv < (n + 1) ** d
    f, uD = smooth_data(sub.x)
    Ao, bo, idx, *_ = spec(sub, ds, phi, f, uD)
    s = P.ElasticitySolver(sub)
    compare(s, s.assemble(phi, f, uD), Ao, bo, idx, f"sub-mesh d={d} n={n}")


def test_disk_fixture_vs_specification(P):
    """212 unstructured triangles (`Mesh.from_arrays`), cut by the circle of radius sqrt(0.125) about the origin."""
    ctype, x, cells = load_mesh("disk")
    x = np.ascontiguousarray(x[:, :2])
    mesh = P.Mesh.from_arrays(ctype, x, cells)
    phi = (mesh.x ** 2).sum(axis=1) - 0.125
    _, _, _, meas, _ = tag(P, mesh, phi)
    assert set(np.unique(mesh.cell_tag_values())) == {1, 2, 3}
    f, uD = smooth_data(mesh.x)
    Ao, bo, idx, *_ = spec(mesh, meas(100), phi, f, uD)
    s = P.ElasticitySolver(mesh)
    compare(s, s.assemble(phi, f, uD), Ao, bo, idx, "disk")


def hub_problem(P, name):
    x, cells, _ = H.case_mesh(name)
    mesh = P.Mesh.from_arrays("tetrahedron", x, cells)
    phi = H.levelset(mesh.x)
    _, _, _, meas, _ = tag(P, mesh, phi)
    f, uD = smooth_data(mesh.x)
    return mesh, phi, f, uD, spec(mesh, meas(100), phi, f, uD)


def test_hub_mesh_inside_the_capacity_ladder(P):
    """A Delaunay mesh with a vertex of 70 neighbours on Gamma: rows of more than 128 entries, assembled at the second
    capacity of the ladder."""
    mesh, phi, f, uD, (Ao, bo, idx, *_) = hub_problem(P, HUB_INSIDE)
    widest = int(np.diff(Ao.indptr).max())
    assert CAPACITIES[3][0] < widest <= CAPACITIES[3][1], widest
    s = P.ElasticitySolver(mesh)
    info = s.assemble(phi, f, uD)
    assert info["slot_capacity"] == CAPACITIES[3][1]
    compare(s, info, Ao, bo, idx, HUB_INSIDE)


def test_hub_mesh_above_the_ladder_is_refused(P):
    """A vertex of 260 neighbours: rows wider than the last capacity.  MemoryError naming the capacity, nothing left
    behind, and the next assembly on another mesh is not poisoned."""
    mesh, phi, f, uD, (Ao, *_) = hub_problem(P, HUB_ABOVE)
    last = CAPACITIES[3][-1]
    assert int(np.diff(Ao.indptr).max()) > last
    s = P.ElasticitySolver(mesh)
    gc.collect()
    with pytest.raises(MemoryError, match=f"capacity {last} exceeded"):
        s.assemble(phi, f, uD)
    first = live_bytes(P)
    with pytest.raises(MemoryError, match=f"capacity {last} exceeded"):
        s.assemble(phi, f, uD)
    assert live_bytes(P) == first
    box, ds, phib = box_case(2, 12)
    fb, ub = smooth_data(box.x)
    Ao2, bo2, idx2, *_ = spec(box, ds, phib, fb, ub)
    s2 = P.ElasticitySolver(box)
    compare(s2, s2.assemble(phib, fb, ub), Ao2, bo2, idx2, "box after the refusal")


@pytest.mark.parametrize("d,n", [(2, 16), (3, 6)])
def test_patch_test_through_the_device(P, d, n):
    """Linear displacement, f = 0, u_D = u_lin: (u_lin, 0) satisfies the assembled system."""
    mesh, ds, phi = box_case(d, n)
    G = np.array([[0.3, -0.2, 0.1], [0.15, 0.25, -0.05], [0.05, 0.1, -0.3]])[:d, :d]
    ulin = mesh.x @ G.T + 0.1
    s = P.ElasticitySolver(mesh)
    s.assemble(phi, np.zeros((mesh.nv, d)), ulin)
    rowptr, col, val, rhs, dof = s.export_csr()
    w = np.concatenate([ulin.T.reshape(-1), np.zeros(d * mesh.nv)])
    r = s.spmv(w[dof]) - rhs
    print(f"patch test d={d} n={n}: residual {np.abs(r).max():.3e}, max|val| {np.abs(val).max():.3e}")
    assert np.abs(r).max() <= 1e-10 * np.abs(val).max()


@pytest.mark.parametrize("d,n", [(2, 16), (3, 8)])
def test_solve_vs_direct_solve_of_the_specification(P, d, n):
    mesh, ds, phi = box_case(d, n)
    x = mesh.x
    f = np.stack([np.sin(x[:, 0]) + 0.2, np.cos(x[:, 1]), 0.5 * x[:, -1]][:d], axis=1)
    uD = 0.1 * np.stack([x[:, 0] * x[:, 1], np.sin(x[:, -1]), x[:, 0] - x[:, 1]][:d], axis=1)
    *_, A, b, act = spec(mesh, ds, phi, f, uD)
    wo = R.solve_direct(A, b, act)
    s = P.ElasticitySolver(mesh)
    s.assemble(phi, f, uD)
    w = s.solve(rtol=1e-11, max_iter=200000)
    print(f"weak-Dirichlet elasticity d={d} n={n}: {s.stats['iterations']} iterations, relres {s.stats['relres']:.2e}, "
          f"precond {s.stats['precond']}, n_active {int(act.sum())}")
    assert s.stats["converged"] and s.stats["relres"] <= 1e-11
    assert np.abs(w - wo).max() <= 1e-6 * np.abs(wo).max()
    assert np.all(w[~act] == 0.0)
    assert s.stats["precond"] == "vertex-block-jacobi"


def test_device_inputs_and_deterministic_assembly(P):
    """Device tensors (component-major) give the bytes of the host inputs under deterministic=True, and two
    deterministic assemblies of one problem are bit-identical."""
    import torch
    d, n = 3, 5
    mesh, ds, phi = box_case(d, n)
    f, uD = smooth_data(mesh.x)
    out = []
    for k in range(3):
        s = P.ElasticitySolver(mesh, deterministic=True)
        if k == 2:
            dev = torch.device("cuda", mesh.device)
            s.assemble(torch.as_tensor(phi, device=dev), torch.as_tensor(np.ascontiguousarray(f.T), device=dev),
                       torch.as_tensor(np.ascontiguousarray(uD.T), device=dev))
        else:
            s.assemble(phi, f, uD)
        out.append(s.export_csr())
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert a.tobytes() == b.tobytes()
    Ao, bo, idx, *_ = spec(mesh, ds, phi, f, uD)
    assert np.array_equal(out[0][4], idx)


def test_refusals_leave_nothing_behind(P):
    import torch
    d = 2
    mesh, ds, phi = box_case(d, 12)
    f, uD = smooth_data(mesh.x)
    quad = P.create_rectangle([[-1.5, -1.5], [1.5, 1.5]], [8, 8], cell_type="quadrilateral")
    phiq = (quad.x ** 2).sum(axis=1) - 1.0
    tag(P, quad, phiq)
    untagged = P.create_box([-1.5] * d, [1.5] * d, [6] * d)
    s = P.ElasticitySolver(mesh)
    gc.collect()
    before = live_bytes(P)
    with pytest.raises(NotImplementedError):
        P.ElasticitySolver(quad)
    with pytest.raises(NotImplementedError):      # and the C ABI itself
        fq = np.zeros(2 * quad.nv)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        P._lib.check(P._lib.lib.phx_assemble_elasticity_wd(quad._h, vp(s.params), vp(phiq), vp(fq), vp(fq), P._lib.HOST,
                                                           C.byref(h)))
    for kw in (dict(degree=2), dict(coarse_space="auto"), dict(multilevel=True)):
        with pytest.raises(NotImplementedError):
            P.ElasticitySolver(mesh, **kw)
    with pytest.raises(ValueError, match="all live on the host or all on the device"):
        s.assemble(torch.as_tensor(phi, device=torch.device("cuda", mesh.device)), f, uD)
    with pytest.raises(ValueError):
        s.assemble(phi, f.T, uD)                   # component-major on the host
    with pytest.raises(ValueError):
        s.assemble(phi[:-1], f, uD)
    with pytest.raises(ValueError):
        s.assemble(phi, f, uD[:, :1])
    with pytest.raises(ValueError, match="tags must be computed"):
        P.ElasticitySolver(untagged).assemble(np.zeros(untagged.nv), np.zeros((untagged.nv, d)), np.zeros((untagged.nv, d)))
    gc.collect()
    assert live_bytes(P) == before
    # the solver still assembles after the refusals
    Ao, bo, idx, *_ = spec(mesh, ds, phi, f, uD)
    compare(s, s.assemble(phi, f, uD), Ao, bo, idx, "after the refusals")
