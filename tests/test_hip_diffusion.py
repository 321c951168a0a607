"""GPU parity of the variable-coefficient diffusion scheme (`phifem_amd.DiffusionSolver`, `phifem_amd.HeatSolver(kappa=)`,
`phx_assemble_diffusion_wd`, `phx_system_update_rhs`) against its numpy specification tests/diffusion_ref.py, and at
kappa = 1 against `phifem_amd.ReactionSolver`.  Fixtures and tolerances are those of tests/test_hip_heat.py: matrices
and vectors 1e-12 relative to the largest entry, solutions 1e-6 max|w| at rtol 1e-11."""
import ctypes as C
import gc

import numpy as np
import pytest

import diffusion_ref as D
import heat_ref as R
from oracle import assembly as OA
from test_hip_heat import MAT_TOL, MESHES, PAR, SOL_TOL, case, compare, hip_matrix, live_bytes, smooth_data, tag, topo_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def kappa_of(x):
    """Smooth, contrast 10 over R^2 (a little less on the meshes here)."""
    return D.smooth_kappa(x, 10.0)


def spec(work, ds, kap, phi, f, uD, c, g, **par):
    """The specification's system on the library's own numbering -> (active CSR, active rhs, active indices, A, b, act)."""
    A, b, act = D.assemble_diffusion_wd(topo_of(work), work.x, work.cell_tag_values(), work.facet_tag_values(), ds, kap,
                                        phi, f, uD, c, g, **par)
    idx = np.flatnonzero(act)
    Ao = A[idx][:, idx].tocsr()
    Ao.sort_indices()
    return Ao, b[idx], idx, A, b, act


@pytest.mark.parametrize("kind,d,n", MESHES)
def test_matrix_rhs_active_set_and_spmv_vs_specification(P, kind, d, n):
    work, ds, phi, h = case(kind, d, n)
    f, uD, g, *_ = smooth_data(work.x)
    kap = kappa_of(work.x)
    for c in (0.0, 1.0 / h, 1.0 / h ** 2):
        Ao, bo, idx, *_ = spec(work, ds, kap, phi, f, uD, c, g, **PAR)
        s = P.DiffusionSolver(work, c, **PAR)
        info = s.assemble(kap, phi, f, uD, g)
        assert info["n_full"] == 2 * work.nv and info["stencil_rows"] == 0 and info["has_csr"] == 1
        compare(s, info, Ao, bo, idx, f"{kind} d={d} n={n} c={c:g} contrast {kap.max() / kap.min():.1f}")
    u, p = s.split(np.arange(2.0 * work.nv))
    assert u.shape == (work.nv,) and p[3] == work.nv + 3
    with pytest.raises(NotImplementedError):
        s.estimate(np.zeros(2 * work.nv))


@pytest.mark.parametrize("kind,d,n", MESHES)
def test_unit_conductivity_is_the_reaction_solver(P, kind, d, n):
    work, ds, phi, h = case(kind, d, n)
    f, uD, g, *_ = smooth_data(work.x)
    one = np.ones(work.nv)
    for c in (0.0, 1.0 / h, 1.0 / h ** 2):
        r = P.ReactionSolver(work, c, **PAR)
        rinfo = r.assemble(phi, f, uD, g)
        Rm, rrhs, rdof = hip_matrix(r)
        s = P.DiffusionSolver(work, c, **PAR)
        info = s.assemble(one, phi, f, uD, g)
        Hm, rhs, dof = hip_matrix(s)
        assert info["n_active"] == rinfo["n_active"] and info["n_active_u"] == rinfo["n_active_u"]
        assert np.array_equal(dof, rdof) and np.array_equal(Hm.indptr, Rm.indptr) and np.array_equal(Hm.indices, Rm.indices)
        em = np.abs(Hm.data - Rm.data).max() / np.abs(Rm.data).max()
        ev = np.abs(rhs - rrhs).max() / np.abs(rrhs).max()
        xv = np.random.default_rng(0).standard_normal(dof.size)
        y, yr = s.spmv(xv), r.spmv(xv)
        ey = np.abs(y - yr).max() / np.abs(yr).max()
        print(f"kappa = 1 {kind} d={d} n={n} c={c:g}: matrix {em:.2e} rhs {ev:.2e} spmv {ey:.2e} vs ReactionSolver")
        assert em <= MAT_TOL and ev <= MAT_TOL and ey <= MAT_TOL


@pytest.mark.parametrize("kind,d,n", [("box", 2, 16), ("box", 3, 6), ("sub", 3, 5), ("disk", 2, 0)])
def test_refresh_of_the_right_hand_side(P, kind, d, n):
    work, ds, phi, h = case(kind, d, n)
    f, uD, g, f2, uD2, g2 = smooth_data(work.x)
    kap = kappa_of(work.x)
    c = 1.0 / h
    s = P.DiffusionSolver(work, c, **PAR)
    s.assemble(kap, phi, f, uD, g)
    rhs0, dof = s.export_rhs_dof()
    xv = np.random.default_rng(1).standard_normal(dof.size)
    y0 = s.spmv(xv)
    s.update_rhs(f, uD, g)
    assert s.export_rhs_dof()[0].tobytes() == rhs0.tobytes(), "refresh with the assembly's data changed the bytes"
    s.update_rhs(f2, uD2, g2)
    rhs2 = s.export_rhs_dof()[0]
    s.update_rhs(f2, uD2, g2)
    assert s.export_rhs_dof()[0].tobytes() == rhs2.tobytes(), "two refreshes differ"
    _, bo, idx, *_ = spec(work, ds, kap, phi, f2, uD2, c, g2, **PAR)
    err = np.abs(rhs2 - bo).max() / np.abs(bo).max()
    print(f"refresh {kind} d={d} n={n}: rhs error {err:.2e}")
    assert np.array_equal(dof, idx) and err <= MAT_TOL
    assert s.spmv(xv).tobytes() == y0.tobytes(), "the refresh touched the matrix"
    s.update_rhs(f2, uD2)                         # g_h = None counts as 0
    _, bo, *_ = spec(work, ds, kap, phi, f2, uD2, c, None, **PAR)
    assert np.abs(s.export_rhs_dof()[0] - bo).max() <= MAT_TOL * np.abs(bo).max()


@pytest.mark.parametrize("kind,d,n", [("box", 2, 16), ("box", 3, 8), ("disk", 2, 0)])
def test_solve_vs_direct_solve_of_the_specification(P, kind, d, n):
    work, ds, phi, h = case(kind, d, n)
    x = work.x
    f, uD, g = np.sin(x[:, 0]) + 0.2, 0.1 * x[:, 0] * x[:, 1], np.cos(x[:, -1])
    kap = kappa_of(x)
    *_, A, b, act = spec(work, ds, kap, phi, f, uD, 1.0 / h, g)
    wo = OA.solve_direct(A, b, act)
    s = P.DiffusionSolver(work, 1.0 / h)
    s.assemble(kap, phi, f, uD, g)
    w = s.solve(rtol=1e-11, max_iter=200000)
    print(f"diffusion {kind} d={d} n={n}: {s.stats['iterations']} iterations, relres {s.stats['relres']:.2e}, "
          f"precond {s.stats['precond']}, n_active {int(act.sum())}")
    assert s.stats["converged"] and s.stats["relres"] <= 1e-11
    assert np.abs(w - wo).max() <= SOL_TOL * np.abs(wo).max()
    assert np.all(w[~act] == 0.0)
    assert s.stats["precond"] == ("jacobi" if kind == "disk" else "box-dst")


@pytest.mark.parametrize("d,n", [(2, 16), (3, 8)])
def test_high_contrast_is_solved_with_jacobi(P, d, n):
    """Above contrast 50 the plain lattice Laplacian loses to Jacobi: the library picks Jacobi on a box
    too, and the solution is the direct solve's."""
    work, ds, phi, h = case("box", d, n)
    x = work.x
    f, uD = np.sin(x[:, 0]) + 0.2, 0.1 * x[:, 0] * x[:, 1]
    for contrast, name in ((40.0, "box-dst"), (400.0, "jacobi")):
        kap = D.smooth_kappa(x, contrast)
        on_mesh = kap.max() / kap.min()
        assert (on_mesh > 50.0) == (name == "jacobi")
        *_, A, b, act = spec(work, ds, kap, phi, f, uD, 0.0, None)
        wo = OA.solve_direct(A, b, act)
        s = P.DiffusionSolver(work)
        s.assemble(kap, phi, f, uD)
        w = s.solve(rtol=1e-11, max_iter=200000)
        print(f"contrast {on_mesh:.1f} d={d} n={n}: {s.stats['iterations']} iterations, precond {s.stats['precond']}")
        assert s.stats["converged"] and s.stats["precond"] == name and s.precond_info()["precond"] == name
        assert np.abs(w - wo).max() <= SOL_TOL * np.abs(wo).max()


@pytest.mark.parametrize("d,n", [(2, 16), (3, 6)])
def test_patch_test_through_the_public_api(P, d, n):
    """kappa and u linear, f = c u - grad kappa . grad u, u_D = u: the solver returns u with p = 0, to the solve's
    accuracy (SOL_TOL max|u| at rtol 1e-11)."""
    work, ds, phi, h = case("box", d, n)
    x = work.x
    wts = np.arange(1.0, d + 1.0)
    kap, u = 4.0 + 0.3 * (x @ wts), 1.0 + x @ wts
    gkgu = 0.3 * (wts ** 2).sum()
    for c in (0.0, 1.0 / h):
        s = P.DiffusionSolver(work, c)
        s.assemble(kap, phi, c * u - gkgu, u)
        w = s.solve(rtol=1e-11, max_iter=200000)
        uh, ph = s.split(w)
        au = s.export_rhs_dof()[1]
        au = au[au < work.nv]
        err, perr, umax = np.abs(uh[au] - u[au]).max(), np.abs(ph).max(), np.abs(u[au]).max()
        print(f"patch test d={d} n={n} c={c:g}: |u_h - u| {err:.2e}, |p| {perr:.2e}, max|u| {umax:.2f}, "
              f"{s.stats['iterations']} iterations")
        assert s.stats["converged"] and err <= SOL_TOL * umax and perr <= SOL_TOL * umax


@pytest.mark.parametrize("scheme", ["bdf1", "bdf2"])
@pytest.mark.parametrize("d,n", [(2, 16), (3, 6)])
def test_heat_solver_with_a_conductivity_vs_the_specifications_stepper(P, d, n, scheme):
    """The exactness case of tests/test_diffusion_ref.py: kappa linear, data P1 in space."""
    work, ds, phi, dt = case("box", d, n)
    wts = np.arange(1.0, d + 1.0)
    ell, kap = 1.0 + work.x @ wts, 4.0 + 0.3 * (work.x @ wts)
    gkgl = 0.3 * (wts ** 2).sum()
    dgamma = lambda t: 3.0 * t * t
    nsteps = 4
    gam = R.scalar_recurrence(1.0, dgamma, dt, scheme, nsteps)
    f_of = lambda k: ell * dgamma((k + 1) * dt) - gam[k] * gkgl
    k_of = lambda t: int(round(t / dt)) - 1
    ws = D.diffusion_steps(topo_of(work), work.x, work.cell_tag_values(), work.facet_tag_values(), ds, kap, phi, dt,
                           scheme, ell, lambda t: f_of(k_of(t)), lambda t: ell * gam[k_of(t)], nsteps)
    wmax = max(np.abs(w).max() for w in ws)
    heat = P.HeatSolver(work, dt, scheme=scheme, kappa=kap)
    heat.assemble(phi)
    heat.set_state(ell, t=0.0)
    err, iters = 0.0, []
    for k in range(nsteps):
        w = heat.step(f_of(k), ell * gam[k], rtol=1e-11)
        assert heat.t == pytest.approx((k + 1) * dt) and np.array_equal(heat.u, w[:work.nv])
        assert heat.stats["converged"] and heat.stats["rhs_seconds"] > 0.0
        err = max(err, np.abs(w - ws[k]).max())
        iters.append(heat.stats["iterations"])
    print(f"heat with kappa d={d} n={n} {scheme}: iterations {iters}, error {err:.2e} on max|w| {wmax:.2f}")
    assert isinstance(heat._solver, P.DiffusionSolver)
    assert err <= 4 * SOL_TOL * wmax


def test_heat_solver_without_a_conductivity_is_unchanged(P):
    work, ds, phi, dt = case("box", 2, 16)
    ell = 1.0 + work.x @ np.arange(1.0, 3.0)
    dgamma = lambda t: 3.0 * t * t
    nsteps = 4
    gam = R.scalar_recurrence(1.0, dgamma, dt, "bdf2", nsteps)
    ws = R.heat_steps(topo_of(work), work.x, work.cell_tag_values(), work.facet_tag_values(), ds, phi, dt, "bdf2", ell,
                      lambda t: ell * dgamma(t), lambda t: ell * gam[int(round(t / dt)) - 1], nsteps)
    wmax = max(np.abs(w).max() for w in ws)
    heat = P.HeatSolver(work, dt, scheme="bdf2")
    heat.assemble(phi)
    heat.set_state(ell, t=0.0)
    assert heat.kappa is None
    for k in range(nsteps):
        w = heat.step(ell * dgamma((k + 1) * dt), ell * gam[k], rtol=1e-11)
        assert type(heat._solver) is P.ReactionSolver
        assert np.abs(w - ws[k]).max() <= 4 * SOL_TOL * wmax


def test_device_inputs_and_deterministic_assembly(P):
    """Tensors in give a tensor out; under deterministic=True the system's bytes equal those from host inputs, and two
    assemblies are bit-identical, iteration counts included."""
    import torch
    work, ds, phi, h = case("box", 3, 5)
    f, uD, g, *_ = smooth_data(work.x)
    kap = kappa_of(work.x)
    dev = torch.device("cuda", work.device)
    out, iters, sols = [], [], []
    for k in range(3):
        s = P.DiffusionSolver(work, 1.0 / h, deterministic=True)
        if k == 2:
            s.assemble(*(torch.as_tensor(a, device=dev) for a in (kap, phi, f, uD, g)))
        else:
            s.assemble(kap, phi, f, uD, g)
        out.append(s.export_csr())
        if k < 2:
            sols.append(s.solve(rtol=1e-10))
            iters.append(s.stats["iterations"])
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert a.tobytes() == b.tobytes()
    assert iters[0] == iters[1] and sols[0].tobytes() == sols[1].tobytes()
    # the last solver holds device data: refresh and solve stay on the device
    s.update_rhs(*(torch.as_tensor(a, device=dev) for a in (f, uD, g)))
    assert s.export_rhs_dof()[0].tobytes() == out[0][3].tobytes()
    wd = torch.empty(2 * work.nv, dtype=torch.float64, device=dev)
    assert s.solve(rtol=1e-11, out=wd) is wd
    assert np.abs(wd.cpu().numpy() - sols[0]).max() <= SOL_TOL * np.abs(sols[0]).max()
    heat = P.HeatSolver(work, h, kappa=torch.as_tensor(kap, device=dev))
    heat.assemble(torch.as_tensor(phi, device=dev))
    heat.set_state(torch.as_tensor(g, device=dev))
    w = heat.step(torch.as_tensor(f, device=dev), torch.as_tensor(uD, device=dev), rtol=1e-11)
    assert isinstance(w, torch.Tensor) and w.is_cuda and heat.u.is_cuda
    host = P.HeatSolver(work, h, kappa=kap)
    host.assemble(phi)
    host.set_state(g)
    wh = host.step(f, uD, rtol=1e-11)
    assert np.abs(w.cpu().numpy() - wh).max() <= SOL_TOL * np.abs(wh).max()


def test_refusals_leave_nothing_behind(P):
    import torch
    work, ds, phi, h = case("box", 2, 12)
    f, uD, g, *_ = smooth_data(work.x)
    kap = kappa_of(work.x)
    quad = P.create_rectangle([[-1.5, -1.5], [1.5, 1.5]], [8, 8], cell_type="quadrilateral")
    phiq = (quad.x ** 2).sum(axis=1) - 1.0
    tag(P, quad, phiq)
    s = P.DiffusionSolver(work, 2.0)
    poisson = P.PhiFEMSolver(work)
    poisson.assemble(phi, f, uD)
    dev = torch.device("cuda", work.device)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    gc.collect()
    before = live_bytes(P)
    for where, value in ((0, 0.0), (work.nv // 2, -1.0), (work.nv - 1, float("nan")), (3, float("inf"))):
        bad = kap.copy()
        bad[where] = value
        with pytest.raises(ValueError, match="kappa_h"):
            s.assemble(bad, phi, f, uD)
        with pytest.raises(ValueError, match="kappa_h"):      # device inputs go through the same check
            s.assemble(*(torch.as_tensor(a, device=dev) for a in (bad, phi, f, uD)))
        assert s._sys is None and live_bytes(P) == before
    with pytest.raises(ValueError):
        s.assemble(kap[:-1], phi, f, uD)
    with pytest.raises(ValueError):
        s.assemble(kap, phi, f, uD, g[:-1])
    with pytest.raises(ValueError, match="all live on the host or all on the device"):
        s.assemble(torch.as_tensor(kap, device=dev), phi, f, uD)
    assert live_bytes(P) == before
    with pytest.raises(NotImplementedError):
        P.DiffusionSolver(quad, 1.0)
    with pytest.raises(NotImplementedError):
        P.HeatSolver(quad, 0.1, kappa=np.ones(quad.nv))
    with pytest.raises(NotImplementedError):      # and the C ABI itself
        fq = np.ones(quad.nv)
        hq = C.c_void_p()
        P._lib.check(P._lib.lib.phx_assemble_diffusion_wd(quad._h, 1.0, 1.0, 1.0, vp(fq), vp(phiq), vp(fq), None, vp(fq),
                                                          P._lib.HOST, C.byref(hq)))
    for badc in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.DiffusionSolver(work, badc)
        with pytest.raises(ValueError):
            hb = C.c_void_p()
            P._lib.check(P._lib.lib.phx_assemble_diffusion_wd(work._h, 1.0, 1.0, badc, vp(kap), vp(phi), vp(f), None,
                                                              vp(uD), P._lib.HOST, C.byref(hb)))
    with pytest.raises(ValueError):
        P.HeatSolver(work, 0.1, kappa=kap[:-1])
    with pytest.raises(RuntimeError):
        s.update_rhs(f, uD)                        # nothing assembled
    with pytest.raises(ValueError, match="phx_assemble_reaction_wd"):     # update_rhs on a Poisson system
        P._lib.check(P._lib.lib.phx_system_update_rhs(poisson._sys, vp(phi), vp(f), None, vp(uD), P._lib.HOST))
    assert live_bytes(P) == before
    # the system's own copy of kappa_h is visible in the pool statistics and released with the system
    s.assemble(kap, phi, f, uD, g)
    assert live_bytes(P) >= before + 8 * work.nv
    s._free()
    assert live_bytes(P) == before
    # the solver still assembles after the refusals
    Ao, bo, idx, *_ = spec(work, ds, kap, phi, f, uD, 2.0, g)
    compare(s, s.assemble(kap, phi, f, uD, g), Ao, bo, idx, "after the refusals")
