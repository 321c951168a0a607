"""GPU parity of the reaction / heat scheme (`phifem_amd.ReactionSolver`, `phifem_amd.HeatSolver`,
`phx_assemble_reaction_wd`, `phx_system_update_rhs`, `phx_solve_from`) against its numpy specification
tests/heat_ref.py.  Matrix / vector tolerances are those of the P1 parity test (tests/test_hip_assembly.py): 1e-12
relative to the largest entry; solutions 1e-6 max|w| at rtol 1e-11 (tests/test_hip_elasticity_wd.py)."""
import ctypes as C
import functools
import gc
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import heat_ref as R
from datasets import load_mesh
from oracle import assembly as OA
from oracle.topology import Topology

pytestmark = pytest.mark.gpu
CENTRE = (0.04, -0.03, 0.02)
MAT_TOL = 1e-12
SOL_TOL = 1e-6
PAR = dict(pen_coef=1.2, stab_coef=0.8)


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
    """f, u_D, g and a second set of the three."""
    d = x.shape[1]
    rng = np.random.default_rng(seed)
    return [np.sin(x @ rng.standard_normal(d) + k) + 0.3 for k in range(6)]


def topo_of(work):
    ctype = "triangle" if work.gdim == 2 else "tetrahedron"
    topo = Topology(ctype, work.cells.astype(np.int64), work.nv)
    topo.c2f, topo.f2c, topo.nf = work.c2f.astype(np.int64), work.f2c.astype(np.int64), work.nf
    return topo


def spec(work, ds, phi, f, uD, c, g, **par):
    """The specification's system on the library's own numbering -> (active CSR, active rhs, active indices, A, b, act)."""
    A, b, act = R.assemble_reaction_wd(topo_of(work), work.x, work.cell_tag_values(), work.facet_tag_values(), ds, phi,
                                       f, uD, c, g, **par)
    idx = np.flatnonzero(act)
    Ao = A[idx][:, idx].tocsr()
    Ao.sort_indices()
    return Ao, b[idx], idx, A, b, act


@functools.lru_cache(maxsize=None)
def box_case(d, n, box_mode=True):
    """Generated box, tagged by the library -> (mesh the solver works on, its ds entities, phi on its vertices, h)."""
    import phifem_amd as P
    mesh = P.create_box([-1.5] * d, [1.5] * d, [n] * d)
    phi = ((mesh.x - np.asarray(CENTRE)[:d]) ** 2).sum(axis=1) - 1.0
    _, _, sub, meas, maps = tag(P, mesh, phi, box_mode)
    if box_mode:
        return mesh, meas(100), phi, 3.0 / n
    return sub, sub.boundary_facets.reshape(-1), phi[maps[1]], 3.0 / n


@functools.lru_cache(maxsize=None)
def disk_case():
    import phifem_amd as P
    ctype, x, cells = load_mesh("disk")
    mesh = P.Mesh.from_arrays(ctype, np.ascontiguousarray(x[:, :2]), cells)
    phi = (mesh.x ** 2).sum(axis=1) - 0.125
    _, _, _, meas, _ = tag(P, mesh, phi)
    h = float(np.median(R.cell_volume_diameter(mesh.x, mesh.cells.astype(np.int64))[1]))
    return mesh, meas(100), phi, h


def case(kind, d=2, n=0):
    return disk_case() if kind == "disk" else box_case(d, n, kind == "box")


def hip_matrix(s):
    rowptr, col, val, rhs, dof = s.export_csr()
    n = rowptr.size - 1
    return sp.csr_matrix((val, col, rowptr), shape=(n, n)), rhs, dof


def compare(s, info, Ao, bo, idx, label):
    Hm, rhs, dof = hip_matrix(s)
    assert info["n_active"] == idx.size and np.array_equal(dof, idx), "active DoF numbering differs"
    assert np.array_equal(Hm.indptr, Ao.indptr) and np.array_equal(Hm.indices, Ao.indices), "structural pattern differs"
    xv = np.random.default_rng(0).standard_normal(idx.size)
    y, yo = s.spmv(xv), Ao @ xv
    errs = (np.abs(Hm.data - Ao.data).max() / np.abs(Ao.data).max(), np.abs(rhs - bo).max() / max(np.abs(bo).max(), 1e-300),
            np.abs(y - yo).max() / np.abs(yo).max())
    print(f"{label}: n_active={idx.size} nnz={Hm.nnz} | relative errors: matrix {errs[0]:.2e} rhs {errs[1]:.2e} "
          f"spmv {errs[2]:.2e}")
    assert errs[0] <= MAT_TOL and errs[1] <= MAT_TOL and errs[2] <= MAT_TOL
    return Hm, rhs


MESHES = [("box", 2, 12), ("box", 2, 16), ("box", 3, 5), ("box", 3, 6), ("sub", 2, 12), ("sub", 3, 5), ("disk", 2, 0)]


@pytest.mark.parametrize("kind,d,n", MESHES)
def test_matrix_rhs_active_set_and_spmv_vs_specification(P, kind, d, n):
    work, ds, phi, h = case(kind, d, n)
    f, uD, g, *_ = smooth_data(work.x)
    for c in (0.0, 1.0 / h, 1.0 / h ** 2):
        Ao, bo, idx, *_ = spec(work, ds, phi, f, uD, c, g, **PAR)
        s = P.ReactionSolver(work, c, **PAR)
        info = s.assemble(phi, f, uD, g)
        assert info["n_full"] == 2 * work.nv and info["stencil_rows"] == 0 and info["has_csr"] == 1
        Hm, rhs = compare(s, info, Ao, bo, idx, f"{kind} d={d} n={n} c={c:g}")
        if c == 0.0:       # the Poisson system, also as PhiFEMSolver assembles it
            ps = P.PhiFEMSolver(work, **PAR)
            ps.assemble(phi, f, uD)
            Pm, prhs, pdof = hip_matrix(ps)
            assert np.array_equal(pdof, idx) and np.array_equal(Pm.indptr, Hm.indptr) and np.array_equal(Pm.indices, Hm.indices)
            assert np.abs(Pm.data - Hm.data).max() <= MAT_TOL * np.abs(Hm.data).max()
            assert np.abs(prhs - rhs).max() <= MAT_TOL * np.abs(rhs).max()
    u, p = s.split(np.arange(2.0 * work.nv))
    assert u.shape == (work.nv,) and p[3] == work.nv + 3
    with pytest.raises(NotImplementedError):
        s.estimate(np.zeros(2 * work.nv))


@pytest.mark.parametrize("kind,d,n", [("box", 2, 16), ("box", 3, 6), ("sub", 3, 5), ("disk", 2, 0)])
def test_refresh_of_the_right_hand_side(P, kind, d, n):
    work, ds, phi, h = case(kind, d, n)
    f, uD, g, f2, uD2, g2 = smooth_data(work.x)
    c = 1.0 / h
    s = P.ReactionSolver(work, c, **PAR)
    s.assemble(phi, f, uD, g)
    rhs0, dof = s.export_rhs_dof()
    xv = np.random.default_rng(1).standard_normal(dof.size)
    y0 = s.spmv(xv)
    s.update_rhs(f, uD, g)
    assert s.export_rhs_dof()[0].tobytes() == rhs0.tobytes(), "refresh with the assembly's data changed the bytes"
    s.update_rhs(f2, uD2, g2)
    rhs2 = s.export_rhs_dof()[0]
    s.update_rhs(f2, uD2, g2)
    assert s.export_rhs_dof()[0].tobytes() == rhs2.tobytes(), "two refreshes differ"
    _, bo, idx, *_ = spec(work, ds, phi, f2, uD2, c, g2, **PAR)
    err = np.abs(rhs2 - bo).max() / np.abs(bo).max()
    print(f"refresh {kind} d={d} n={n}: rhs error {err:.2e}")
    assert np.array_equal(dof, idx) and err <= MAT_TOL
    assert s.spmv(xv).tobytes() == y0.tobytes(), "the refresh touched the matrix"
    s.update_rhs(f2, uD2)                         # g_h = None counts as 0
    _, bo, *_ = spec(work, ds, phi, f2, uD2, c, None, **PAR)
    assert np.abs(s.export_rhs_dof()[0] - bo).max() <= MAT_TOL * np.abs(bo).max()


@pytest.mark.parametrize("kind,d,n", [("box", 2, 16), ("box", 3, 8), ("disk", 2, 0)])
def test_solve_vs_direct_solve_of_the_specification(P, kind, d, n):
    work, ds, phi, h = case(kind, d, n)
    x = work.x
    f, uD, g = np.sin(x[:, 0]) + 0.2, 0.1 * x[:, 0] * x[:, 1], np.cos(x[:, -1])
    *_, A, b, act = spec(work, ds, phi, f, uD, 1.0 / h, g)
    wo = OA.solve_direct(A, b, act)
    s = P.ReactionSolver(work, 1.0 / h)
    s.assemble(phi, f, uD, g)
    w = s.solve(rtol=1e-11, max_iter=200000)
    print(f"reaction {kind} d={d} n={n}: {s.stats['iterations']} iterations, relres {s.stats['relres']:.2e}, "
          f"precond {s.stats['precond']}, n_active {int(act.sum())}")
    assert s.stats["converged"] and s.stats["relres"] <= 1e-11
    assert np.abs(w - wo).max() <= SOL_TOL * np.abs(wo).max()
    assert np.all(w[~act] == 0.0)
    assert s.stats["precond"] == ("jacobi" if kind == "disk" else "box-dst")
    assert s.precond_info()["precond"] == s.stats["precond"]


def residual(s, w):
    """||b - A w|| / ||b|| from the library's operator and the exported right-hand side."""
    rhs, dof = s.export_rhs_dof()
    return np.linalg.norm(rhs - s.spmv(np.ascontiguousarray(w[dof]))) / np.linalg.norm(rhs)


@pytest.mark.parametrize("d,n", [(2, 16), (3, 6)])
def test_warm_start(P, d, n):
    work, ds, phi, h = case("box", d, n)
    f, uD, g, *_ = smooth_data(work.x)
    s = P.ReactionSolver(work, 1.0 / h)
    s.assemble(phi, f, uD, g)
    x0 = s.solve(rtol=1e-11)
    cold_iterations = s.stats["iterations"]
    assert s.stats["converged"] and cold_iterations > 0
    w = s.solve(rtol=1e-8, x0=x0)
    assert s.stats["iterations"] == 0 and s.stats["converged"] and s.stats["relres"] <= 1e-8
    assert w is not x0 and w.tobytes() == x0.tobytes()
    rhs_before = s.export_rhs_dof()[0]
    rng = np.random.default_rng(3)
    rtol = 1e-8
    pert = x0 * (1.0 + 1e-3 * rng.standard_normal(x0.size))
    w = s.solve(rtol=rtol, x0=pert)
    res = residual(s, w)
    print(f"warm start d={d} n={n} rtol={rtol:g}: {s.stats['iterations']} iterations (cold to 1e-11: {cold_iterations}), "
          f"reported {s.stats['relres']:.2e}, recomputed {res:.2e}")
    assert s.stats["converged"] and 0 < s.stats["iterations"]
    assert res <= rtol * (1.0 + 1e-6)
    assert s.export_rhs_dof()[0].tobytes() == rhs_before.tobytes(), "the right-hand side was not put back"
    # in place: x0 and out are one buffer
    buf = pert.copy()
    assert s.solve(rtol=1e-8, x0=buf, out=buf) is buf and residual(s, buf) <= 1e-8 * (1.0 + 1e-6)


@pytest.mark.parametrize("n", [8, 16])
def test_warm_start_on_a_stencil_coded_poisson_system(P, n):
    """n = 8: the structured formats with every row stored (no vertex has its whole neighbourhood inside); n = 16: rows
    applied from the stencil, and the identity loop."""
    work, ds, phi, h = case("box", 3, n)
    f, uD, *_ = smooth_data(work.x)
    s = P.PhiFEMSolver(work)
    info = s.assemble(phi, f, uD)
    assert info["has_csr"] == 0 and (info["stencil_rows"] > 0) == (n == 16)
    w = s.solve(rtol=1e-11).copy()
    ident = s.stats["identity_loop"]
    pert = w * (1.0 + 1e-3 * np.random.default_rng(4).standard_normal(w.size))
    w2 = s.solve(rtol=1e-11, x0=pert)
    print(f"stencil-coded box: identity loop {ident}, warm start {s.stats['iterations']} iterations, "
          f"relres {s.stats['relres']:.2e}")
    assert s.stats["converged"] and s.stats["identity_loop"] == ident
    assert np.abs(w2 - w).max() <= SOL_TOL * np.abs(w).max()


@pytest.mark.parametrize("scheme", ["bdf1", "bdf2"])
@pytest.mark.parametrize("d,n", [(2, 16), (3, 6)])
def test_heat_solver_vs_the_specifications_stepper(P, d, n, scheme):
    """The exactness case of tests/test_heat_ref.py: data P1 in space, u_D the scheme's own scalar recurrence."""
    work, ds, phi, dt = case("box", d, n)
    ell = 1.0 + work.x @ np.arange(1.0, d + 1.0)
    dgamma = lambda t: 3.0 * t * t
    nsteps = 4
    gam = R.scalar_recurrence(1.0, dgamma, dt, scheme, nsteps)
    ws = R.heat_steps(topo_of(work), work.x, work.cell_tag_values(), work.facet_tag_values(), ds, phi, dt, scheme, ell,
                      lambda t: ell * dgamma(t), lambda t: ell * gam[int(round(t / dt)) - 1], nsteps)
    wmax = max(np.abs(w).max() for w in ws)
    for warm in (True, False):
        heat = P.HeatSolver(work, dt, scheme=scheme)
        heat.assemble(phi)
        heat.set_state(ell, t=0.0)
        err, iters = 0.0, []
        for k in range(nsteps):
            t = (k + 1) * dt
            u_before = heat.u
            w = heat.step(ell * dgamma(t), ell * gam[k], rtol=1e-11, warm_start=warm)
            assert heat.t == pytest.approx(t) and heat.u is not u_before and np.array_equal(heat.u, w[:work.nv])
            assert heat.stats["converged"] and heat.stats["rhs_seconds"] > 0.0
            err = max(err, np.abs(w - ws[k]).max())
            iters.append(heat.stats["iterations"])
        print(f"heat d={d} n={n} {scheme} warm_start={warm}: iterations {iters}, error {err:.2e} on max|w| {wmax:.2f}")
        assert err <= 4 * SOL_TOL * wmax


def test_device_inputs_and_deterministic_assembly(P):
    """Tensors in give a tensor out; under deterministic=True the system's bytes equal those from host inputs, and two
    assemblies are bit-identical."""
    import torch
    work, ds, phi, h = case("box", 3, 5)
    f, uD, g, *_ = smooth_data(work.x)
    dev = torch.device("cuda", work.device)
    out = []
    for k in range(3):
        s = P.ReactionSolver(work, 1.0 / h, deterministic=True)
        if k == 2:
            s.assemble(*(torch.as_tensor(a, device=dev) for a in (phi, f, uD, g)))
        else:
            s.assemble(phi, f, uD, g)
        out.append(s.export_csr())
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert a.tobytes() == b.tobytes()
    # the last solver holds device data: refresh and solve stay on the device
    s.update_rhs(*(torch.as_tensor(a, device=dev) for a in (f, uD, g)))
    assert s.export_rhs_dof()[0].tobytes() == out[0][3].tobytes()
    wd = torch.empty(2 * work.nv, dtype=torch.float64, device=dev)
    assert s.solve(rtol=1e-11, out=wd) is wd
    w2 = s.solve(rtol=1e-8, x0=wd)
    assert isinstance(w2, torch.Tensor) and w2.is_cuda and s.stats["iterations"] == 0 and torch.equal(w2, wd)
    with pytest.raises(ValueError, match="both live on the host or both on the device"):
        s.solve(x0=wd.cpu().numpy(), out=wd)
    heat = P.HeatSolver(work, h)
    heat.assemble(torch.as_tensor(phi, device=dev))
    heat.set_state(torch.as_tensor(g, device=dev))
    w = heat.step(torch.as_tensor(f, device=dev), torch.as_tensor(uD, device=dev), rtol=1e-11)
    assert isinstance(w, torch.Tensor) and w.is_cuda and heat.u.is_cuda
    host = P.HeatSolver(work, h)
    host.assemble(phi)
    host.set_state(g)
    wh = host.step(f, uD, rtol=1e-11)
    assert np.abs(w.cpu().numpy() - wh).max() <= SOL_TOL * np.abs(wh).max()


def test_refusals_leave_nothing_behind(P):
    import torch
    work, ds, phi, h = case("box", 2, 12)
    f, uD, g, *_ = smooth_data(work.x)
    quad = P.create_rectangle([[-1.5, -1.5], [1.5, 1.5]], [8, 8], cell_type="quadrilateral")
    phiq = (quad.x ** 2).sum(axis=1) - 1.0
    tag(P, quad, phiq)
    s = P.ReactionSolver(work, 2.0)
    poisson = P.PhiFEMSolver(work)
    poisson.assemble(phi, f, uD)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    gc.collect()
    before = live_bytes(P)
    for make in (lambda: P.ReactionSolver(quad, 1.0), lambda: P.HeatSolver(quad, 0.1), lambda: P.ReactionSolver(work, 1.0, degree=2)):
        with pytest.raises(NotImplementedError):
            make()
    with pytest.raises(NotImplementedError):      # and the C ABI itself
        fq = np.zeros(quad.nv)
        hq = C.c_void_p()
        P._lib.check(P._lib.lib.phx_assemble_reaction_wd(quad._h, 1.0, 1.0, 1.0, vp(phiq), vp(fq), None, vp(fq),
                                                         P._lib.HOST, C.byref(hq)))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.ReactionSolver(work, bad)
        with pytest.raises(ValueError):
            hb = C.c_void_p()
            P._lib.check(P._lib.lib.phx_assemble_reaction_wd(work._h, 1.0, 1.0, bad, vp(phi), vp(f), None, vp(uD),
                                                             P._lib.HOST, C.byref(hb)))
    for bad in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            P.HeatSolver(work, bad)
    with pytest.raises(ValueError):
        P.HeatSolver(work, 0.1, scheme="cn")
    with pytest.raises(ValueError):
        s.assemble(phi[:-1], f, uD)
    with pytest.raises(ValueError):
        s.assemble(phi, f, uD, g[:-1])
    with pytest.raises(ValueError, match="all live on the host or all on the device"):
        s.assemble(torch.as_tensor(phi, device=torch.device("cuda", work.device)), f, uD)
    with pytest.raises(RuntimeError):
        s.update_rhs(f, uD)                        # nothing assembled
    with pytest.raises(ValueError, match="phx_assemble_reaction_wd"):     # update_rhs on a Poisson system
        P._lib.check(P._lib.lib.phx_system_update_rhs(poisson._sys, vp(phi), vp(f), None, vp(uD), P._lib.HOST))
    heat = P.HeatSolver(work, 0.1)
    with pytest.raises(RuntimeError):
        heat.step(f, uD)                           # before assemble
    with pytest.raises(ValueError):
        heat.assemble(phi[:-1])
    with pytest.raises(ValueError):
        heat.set_state(g[:-1])
    del heat
    gc.collect()
    assert live_bytes(P) == before
    heat = P.HeatSolver(work, 0.1)
    heat.assemble(phi)
    with pytest.raises(RuntimeError, match="set_state"):
        heat.step(f, uD)                           # before set_state
    # the solver still assembles after the refusals
    Ao, bo, idx, *_ = spec(work, ds, phi, f, uD, 2.0, g)
    compare(s, s.assemble(phi, f, uD, g), Ao, bo, idx, "after the refusals")
