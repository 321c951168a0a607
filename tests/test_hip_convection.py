"""GPU parity of the convection-diffusion scheme (`phifem_amd.ConvectionDiffusionSolver`, `phifem_amd.HeatSolver(velocity=)`,
`phx_assemble_convection_wd`, `phx_system_update_rhs`) against its numpy specification tests/convection_ref.py, and at
beta = 0 against `phifem_amd.DiffusionSolver`.  Fixtures and tolerances are those of tests/test_hip_heat.py: matrices
and vectors 1e-12 relative to the largest entry, solutions 1e-6 max|w| at rtol 1e-11."""
import ctypes as C
import gc

import numpy as np
import pytest

import convection_ref as V
import diffusion_ref as D
import heat_ref as R
from oracle import assembly as OA
from test_hip_heat import MAT_TOL, MESHES, PAR, SOL_TOL, case, compare, hip_matrix, live_bytes, smooth_data, tag, topo_of

pytestmark = pytest.mark.gpu
SUPG = 0.3
# the library's rule (phx_precond.inc.hip: PHX_DIFF_LATTICE_MAX_CONTRAST, PHX_CD_LATTICE_MAX_PECLET)
MAX_CONTRAST, MAX_PECLET = 50.0, 1.0


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def kappa_of(x):
    return D.smooth_kappa(x, 10.0)


def beta_of(x, scale=3.0):
    """A smooth rotating field of magnitude about `scale` on the meshes here."""
    b = np.zeros_like(x)
    b[:, 0] = -x[:, 1] + 0.4
    b[:, 1] = x[:, 0] + 0.2 * np.sin(2.0 * x[:, -1])
    if x.shape[1] == 3:
        b[:, 2] = 0.5 * np.cos(x[:, 0])
    return scale * b


def spec(work, ds, kap, beta, phi, f, uD, c, g, **par):
    """The specification's system on the library's own numbering -> (active CSR, active rhs, active indices, A, b, act)."""
    A, b, act = V.assemble_convection_wd(topo_of(work), work.x, work.cell_tag_values(), work.facet_tag_values(), ds, kap,
                                         beta, phi, f, uD, c, g, **par)
    idx = np.flatnonzero(act)
    Ao = A[idx][:, idx].tocsr()
    Ao.sort_indices()
    return Ao, b[idx], idx, A, b, act


def spec_peclet(work, kap, beta):
    return V.peclet_max(topo_of(work), work.x, work.cell_tag_values(), kap, beta)


@pytest.mark.parametrize("kind,d,n", MESHES)
def test_matrix_rhs_active_set_and_spmv_vs_specification(P, kind, d, n):
    work, ds, phi, h = case(kind, d, n)
    f, uD, g, *_ = smooth_data(work.x)
    kap, beta = kappa_of(work.x), beta_of(work.x)
    for c in (0.0, 1.0 / h, 1.0 / h ** 2):
        Ao, bo, idx, *_ = spec(work, ds, kap, beta, phi, f, uD, c, g, supg_coef=SUPG, **PAR)
        s = P.ConvectionDiffusionSolver(work, c, supg_coef=SUPG, **PAR)
        info = s.assemble(beta, phi, f, uD, g, kappa_h=kap)
        assert info["n_full"] == 2 * work.nv and info["stencil_rows"] == 0 and info["has_csr"] == 1
        compare(s, info, Ao, bo, idx, f"{kind} d={d} n={n} c={c:g} |beta| <= {np.abs(beta).max():.1f}")
        pe = spec_peclet(work, kap, beta)
        assert abs(info["peclet_max"] - pe) <= 1e-12 * pe
        assert abs(info["beta_max"] - np.sqrt((beta ** 2).sum(axis=1)).max()) <= 1e-12 * info["beta_max"]
    u, p = s.split(np.arange(2.0 * work.nv))
    assert u.shape == (work.nv,) and p[3] == work.nv + 3
    with pytest.raises(NotImplementedError):
        s.estimate(np.zeros(2 * work.nv))
    # kappa_h = None counts as ones
    Ao, bo, idx, *_ = spec(work, ds, np.ones(work.nv), beta, phi, f, uD, c, g, supg_coef=SUPG, **PAR)
    compare(s, s.assemble(beta, phi, f, uD, g), Ao, bo, idx, f"{kind} d={d} n={n} kappa = None")


@pytest.mark.parametrize("kind,d,n", MESHES)
def test_zero_velocity_is_the_diffusion_solver(P, kind, d, n):
    work, ds, phi, h = case(kind, d, n)
    f, uD, g, *_ = smooth_data(work.x)
    kap = kappa_of(work.x)
    zero = np.zeros((work.nv, work.gdim))
    for c in (0.0, 1.0 / h, 1.0 / h ** 2):
        r = P.DiffusionSolver(work, c, **PAR)
        rinfo = r.assemble(kap, phi, f, uD, g)
        Rm, rrhs, rdof = hip_matrix(r)
        s = P.ConvectionDiffusionSolver(work, c, supg_coef=SUPG, **PAR)
        info = s.assemble(zero, phi, f, uD, g, kappa_h=kap)
        Hm, rhs, dof = hip_matrix(s)
        assert info["n_active"] == rinfo["n_active"] and info["n_active_u"] == rinfo["n_active_u"]
        assert info["peclet_max"] == 0.0
        assert np.array_equal(dof, rdof) and np.array_equal(Hm.indptr, Rm.indptr) and np.array_equal(Hm.indices, Rm.indices)
        em = np.abs(Hm.data - Rm.data).max() / np.abs(Rm.data).max()
        ev = np.abs(rhs - rrhs).max() / np.abs(rrhs).max()
        print(f"beta = 0 {kind} d={d} n={n} c={c:g}: matrix {em:.2e} rhs {ev:.2e} vs DiffusionSolver")
        assert em <= MAT_TOL and ev <= MAT_TOL


@pytest.mark.parametrize("kind,d,n", [("box", 2, 16), ("box", 3, 6), ("sub", 3, 5), ("disk", 2, 0)])
def test_refresh_of_the_right_hand_side(P, kind, d, n):
    work, ds, phi, h = case(kind, d, n)
    f, uD, g, f2, uD2, g2 = smooth_data(work.x)
    kap, beta = kappa_of(work.x), beta_of(work.x)
    c = 1.0 / h
    s = P.ConvectionDiffusionSolver(work, c, supg_coef=SUPG, **PAR)
    s.assemble(beta, phi, f, uD, g, kappa_h=kap)
    rhs0, dof = s.export_rhs_dof()
    xv = np.random.default_rng(1).standard_normal(dof.size)
    y0 = s.spmv(xv)
    s.update_rhs(f, uD, g)
    assert s.export_rhs_dof()[0].tobytes() == rhs0.tobytes(), "refresh with the assembly's data changed the bytes"
    s.update_rhs(f2, uD2, g2)
    rhs2 = s.export_rhs_dof()[0]
    s.update_rhs(f2, uD2, g2)
    assert s.export_rhs_dof()[0].tobytes() == rhs2.tobytes(), "two refreshes differ"
    _, bo, idx, *_ = spec(work, ds, kap, beta, phi, f2, uD2, c, g2, supg_coef=SUPG, **PAR)
    err = np.abs(rhs2 - bo).max() / np.abs(bo).max()
    print(f"refresh {kind} d={d} n={n}: rhs error {err:.2e}")
    assert np.array_equal(dof, idx) and err <= MAT_TOL
    assert s.spmv(xv).tobytes() == y0.tobytes(), "the refresh touched the matrix"
    s.update_rhs(f2, uD2)                         # g_h = None counts as 0
    _, bo, *_ = spec(work, ds, kap, beta, phi, f2, uD2, c, None, supg_coef=SUPG, **PAR)
    assert np.abs(s.export_rhs_dof()[0] - bo).max() <= MAT_TOL * np.abs(bo).max()


@pytest.mark.parametrize("regime", ["diffusive", "convective"])
@pytest.mark.parametrize("kind,d,n", [("box", 2, 16), ("box", 3, 8), ("disk", 2, 0)])
def test_solve_vs_direct_solve_of_the_specification(P, kind, d, n, regime):
    """Once at pe_max < 1 and once at pe_max about 10 (kappa scaled to get there), with supg 0.3."""
    work, ds, phi, h = case(kind, d, n)
    x = work.x
    f, uD, g = np.sin(x[:, 0]) + 0.2, 0.1 * x[:, 0] * x[:, 1], np.cos(x[:, -1])
    beta = beta_of(x)
    kap = kappa_of(x)
    target = 0.5 if regime == "diffusive" else 10.0
    kap = kap * (spec_peclet(work, kap, beta) / target)
    pe = spec_peclet(work, kap, beta)
    assert abs(pe - target) <= 1e-9 * target
    *_, A, b, act = spec(work, ds, kap, beta, phi, f, uD, 1.0 / h, g, supg_coef=SUPG)
    wo = OA.solve_direct(A, b, act)
    s = P.ConvectionDiffusionSolver(work, 1.0 / h, supg_coef=SUPG)
    s.assemble(beta, phi, f, uD, g, kappa_h=kap)
    w = s.solve(rtol=1e-11, max_iter=200000)
    print(f"convection {kind} d={d} n={n} pe_max {pe:.2f}: {s.stats['iterations']} iterations, relres "
          f"{s.stats['relres']:.2e}, precond {s.stats['precond']}, n_active {int(act.sum())}")
    assert s.stats["converged"] and s.stats["relres"] <= 1e-11
    assert abs(s.stats["peclet_max"] - pe) <= 1e-12 * pe
    assert np.abs(w - wo).max() <= SOL_TOL * np.abs(wo).max()
    assert np.all(w[~act] == 0.0)
    lattice = kind != "disk" and pe <= MAX_PECLET
    assert s.stats["precond"] == ("box-dst" if lattice else "jacobi")


@pytest.mark.parametrize("d,n", [(2, 16), (3, 8)])
def test_preconditioner_follows_the_rule(P, d, n):
    """Lattice box: the lattice solve below the Peclet threshold at contrast <= 50, Jacobi above either bound."""
    work, ds, phi, h = case("box", d, n)
    x = work.x
    f, uD = np.sin(x[:, 0]) + 0.2, 0.1 * x[:, 0] * x[:, 1]
    beta = beta_of(x)
    for contrast, target, name in ((10.0, 0.5 * MAX_PECLET, "box-dst"), (10.0, 2.0 * MAX_PECLET, "jacobi"),
                                   (400.0, 0.01 * MAX_PECLET, "jacobi")):
        kap = D.smooth_kappa(x, contrast)
        kap = kap * (spec_peclet(work, kap, beta) / target)
        assert (kap.max() / kap.min() > MAX_CONTRAST) == (contrast > MAX_CONTRAST)
        s = P.ConvectionDiffusionSolver(work, supg_coef=SUPG)
        s.assemble(beta, phi, f, uD, kappa_h=kap)
        s.solve(rtol=1e-8, max_iter=200000)
        print(f"contrast {kap.max() / kap.min():.1f} pe_max {s.stats['peclet_max']:.2f} d={d} n={n}: "
              f"{s.stats['iterations']} iterations, precond {s.stats['precond']}")
        assert s.stats["converged"] and s.stats["precond"] == name and s.precond_info()["precond"] == name


@pytest.mark.parametrize("d,n", [(2, 16), (3, 6)])
def test_patch_test_through_the_public_api(P, d, n):
    """kappa, beta and u linear, f = c u + beta . grad u - grad kappa . grad u, u_D = u: the solver returns u with
    p = 0, to the solve's accuracy (SOL_TOL max|u| at rtol 1e-11)."""
    work, ds, phi, h = case("box", d, n)
    x = work.x
    wts = np.arange(1.0, d + 1.0)
    kap, u = 4.0 + 0.3 * (x @ wts), 1.0 + x @ wts
    beta = 5.0 * np.stack([0.5 + x[:, 0] - 0.4 * x[:, d - 1], -1.0 + 0.7 * x[:, 1], 0.2 + x[:, 0]], axis=1)[:, :d]
    beta = np.ascontiguousarray(beta)
    gkgu = 0.3 * (wts ** 2).sum()
    for c in (0.0, 1.0 / h):
        s = P.ConvectionDiffusionSolver(work, c, supg_coef=SUPG)
        s.assemble(beta, phi, c * u + beta @ wts - gkgu, u, kappa_h=kap)
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
def test_heat_solver_with_a_velocity_vs_the_specifications_stepper(P, d, n, scheme):
    """The exactness case of tests/test_convection_ref.py: kappa and beta linear, data P1 in space."""
    work, ds, phi, dt = case("box", d, n)
    x = work.x
    wts = np.arange(1.0, d + 1.0)
    ell, kap = 1.0 + x @ wts, 4.0 + 0.3 * (x @ wts)
    beta = np.ascontiguousarray(
        5.0 * np.stack([0.5 + x[:, 0] - 0.4 * x[:, d - 1], -1.0 + 0.7 * x[:, 1], 0.2 + x[:, 0]], axis=1)[:, :d])
    space = beta @ wts - 0.3 * (wts ** 2).sum()
    dgamma = lambda t: 3.0 * t * t
    nsteps = 4
    gam = R.scalar_recurrence(1.0, dgamma, dt, scheme, nsteps)
    f_of = lambda k: ell * dgamma((k + 1) * dt) + gam[k] * space
    k_of = lambda t: int(round(t / dt)) - 1
    ws = V.convection_steps(topo_of(work), x, work.cell_tag_values(), work.facet_tag_values(), ds, kap, beta, phi, dt,
                            scheme, ell, lambda t: f_of(k_of(t)), lambda t: ell * gam[k_of(t)], nsteps, supg_coef=SUPG)
    wmax = max(np.abs(w).max() for w in ws)
    heat = P.HeatSolver(work, dt, scheme=scheme, kappa=kap, velocity=beta, supg_coef=SUPG)
    heat.assemble(phi)
    heat.set_state(ell, t=0.0)
    err, iters = 0.0, []
    for k in range(nsteps):
        w = heat.step(f_of(k), ell * gam[k], rtol=1e-11)
        assert heat.t == pytest.approx((k + 1) * dt) and np.array_equal(heat.u, w[:work.nv])
        assert heat.stats["converged"] and heat.stats["rhs_seconds"] > 0.0
        err = max(err, np.abs(w - ws[k]).max())
        iters.append(heat.stats["iterations"])
    print(f"heat with velocity d={d} n={n} {scheme}: iterations {iters}, error {err:.2e} on max|w| {wmax:.2f}")
    assert isinstance(heat._solver, P.ConvectionDiffusionSolver)
    assert err <= 4 * SOL_TOL * wmax


def test_heat_solver_without_a_velocity_is_unchanged(P):
    """The stepper's systems without `velocity` are the ReactionSolver's / DiffusionSolver's own, byte for byte."""
    work, ds, phi, dt = case("box", 2, 16)
    f, uD, g, *_ = smooth_data(work.x)
    kap = kappa_of(work.x)
    for kappa, cls, args in ((None, P.ReactionSolver, ()), (kap, P.DiffusionSolver, (kap,))):
        heat = P.HeatSolver(work, dt, scheme="bdf1", kappa=kappa, deterministic=True)
        heat.assemble(phi)
        heat.set_state(g)
        assert heat.velocity is None and type(heat._solver) is cls
        w = heat.step(f, uD, rtol=1e-11)
        ref = cls(work, 1.0 / dt, deterministic=True)
        ref.assemble(*args, phi, f, uD, g)
        for a, b in zip(heat._solver.export_csr(), ref.export_csr()):
            assert a.tobytes() == b.tobytes()
        assert w.tobytes() == ref.solve(rtol=1e-11).tobytes()


def test_device_inputs_and_deterministic_assembly(P):
    """Tensors in give a tensor out; under deterministic=True the system's bytes equal those from host inputs, and two
    assemblies are bit-identical, iteration counts included."""
    import torch
    work, ds, phi, h = case("box", 3, 5)
    f, uD, g, *_ = smooth_data(work.x)
    kap, beta = kappa_of(work.x), beta_of(work.x)
    dev = torch.device("cuda", work.device)
    out, iters, sols = [], [], []
    for k in range(3):
        s = P.ConvectionDiffusionSolver(work, 1.0 / h, supg_coef=SUPG, deterministic=True)
        if k == 2:
            tb, tphi, tf, tu, tg, tk = (torch.as_tensor(a, device=dev) for a in (beta, phi, f, uD, g, kap))
            s.assemble(tb, tphi, tf, tu, tg, kappa_h=tk)
        else:
            s.assemble(beta, phi, f, uD, g, kappa_h=kap)
        out.append(s.export_csr())
        if k < 2:
            sols.append(s.solve(rtol=1e-10))
            iters.append(s.stats["iterations"])
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert a.tobytes() == b.tobytes()
    assert iters[0] == iters[1] and sols[0].tobytes() == sols[1].tobytes()
    # the last solver holds device data: refresh and solve stay on the device
    s.update_rhs(tf, tu, tg)
    assert s.export_rhs_dof()[0].tobytes() == out[0][3].tobytes()
    wd = torch.empty(2 * work.nv, dtype=torch.float64, device=dev)
    assert s.solve(rtol=1e-11, out=wd) is wd
    assert np.abs(wd.cpu().numpy() - sols[0]).max() <= SOL_TOL * np.abs(sols[0]).max()
    heat = P.HeatSolver(work, h, velocity=tb, supg_coef=SUPG)       # kappa = None: ones
    heat.assemble(tphi)
    heat.set_state(tg)
    w = heat.step(tf, tu, rtol=1e-11)
    assert isinstance(w, torch.Tensor) and w.is_cuda and heat.u.is_cuda
    host = P.HeatSolver(work, h, velocity=beta, supg_coef=SUPG)
    host.assemble(phi)
    host.set_state(g)
    wh = host.step(f, uD, rtol=1e-11)
    assert np.abs(w.cpu().numpy() - wh).max() <= SOL_TOL * np.abs(wh).max()


def test_refusals_leave_nothing_behind(P):
    import torch
    work, ds, phi, h = case("box", 2, 12)
    f, uD, g, *_ = smooth_data(work.x)
    kap, beta = kappa_of(work.x), beta_of(work.x)
    quad = P.create_rectangle([[-1.5, -1.5], [1.5, 1.5]], [8, 8], cell_type="quadrilateral")
    phiq = (quad.x ** 2).sum(axis=1) - 1.0
    tag(P, quad, phiq)
    s = P.ConvectionDiffusionSolver(work, 2.0, supg_coef=SUPG)
    dev = torch.device("cuda", work.device)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    gc.collect()
    before = live_bytes(P)
    for where, value in (((0, 0), float("nan")), ((work.nv // 2, 1), float("inf")), ((work.nv - 1, 1), -float("inf"))):
        bad = beta.copy()
        bad[where] = value
        with pytest.raises(ValueError, match="beta_h"):
            s.assemble(bad, phi, f, uD, kappa_h=kap)
        with pytest.raises(ValueError, match="beta_h"):      # device inputs go through the same check
            s.assemble(*(torch.as_tensor(a, device=dev) for a in (bad, phi, f, uD)))
        assert s._sys is None and live_bytes(P) == before
    badk = kap.copy()
    badk[3] = 0.0
    with pytest.raises(ValueError, match="kappa_h"):
        s.assemble(beta, phi, f, uD, kappa_h=badk)
    for shape_bad in (beta[:-1], beta[:, :1], beta.T.copy(), beta.reshape(-1)):
        with pytest.raises(ValueError, match="shape"):
            s.assemble(shape_bad, phi, f, uD)
    with pytest.raises(ValueError):
        s.assemble(beta, phi, f, uD, g[:-1])
    with pytest.raises(ValueError, match="all live on the host or all on the device"):
        s.assemble(torch.as_tensor(beta, device=dev), phi, f, uD)
    with pytest.raises(ValueError, match="all live on the host or all on the device"):
        s.assemble(beta, phi, f, uD, kappa_h=torch.as_tensor(kap, device=dev))
    assert s._sys is None and live_bytes(P) == before
    for bads in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="supg_coef"):
            P.ConvectionDiffusionSolver(work, 1.0, supg_coef=bads)
        with pytest.raises(ValueError, match="supg_coef"):
            P.HeatSolver(work, 0.1, velocity=beta, supg_coef=bads)
        with pytest.raises(ValueError, match="supg_coef"):      # and the C ABI itself
            hb = C.c_void_p()
            P._lib.check(P._lib.lib.phx_assemble_convection_wd(work._h, 1.0, 1.0, bads, 1.0, vp(kap), vp(beta), vp(phi),
                                                               vp(f), None, vp(uD), P._lib.HOST, C.byref(hb)))
    with pytest.raises(NotImplementedError):
        P.ConvectionDiffusionSolver(quad, 1.0)
    with pytest.raises(NotImplementedError):
        P.HeatSolver(quad, 0.1, velocity=np.ones((quad.nv, 2)))
    with pytest.raises(NotImplementedError):      # and the C ABI itself
        fq, bq = np.ones(quad.nv), np.ones((quad.nv, 2))
        hq = C.c_void_p()
        P._lib.check(P._lib.lib.phx_assemble_convection_wd(quad._h, 1.0, 1.0, 0.0, 1.0, vp(fq), vp(bq), vp(phiq), vp(fq),
                                                           None, vp(fq), P._lib.HOST, C.byref(hq)))
    with pytest.raises(ValueError, match="shape"):
        P.HeatSolver(work, 0.1, velocity=beta[:-1])
    with pytest.raises(RuntimeError):
        s.update_rhs(f, uD)                        # nothing assembled
    assert live_bytes(P) == before
    # the system's own copies of kappa_h and beta_h are visible in the pool statistics and released with the system
    s.assemble(beta, phi, f, uD, g, kappa_h=kap)
    assert live_bytes(P) >= before + 8 * 3 * work.nv
    s._free()
    assert live_bytes(P) == before
    # the solver still assembles after the refusals
    Ao, bo, idx, *_ = spec(work, ds, kap, beta, phi, f, uD, 2.0, g, supg_coef=SUPG)
    compare(s, s.assemble(beta, phi, f, uD, g, kappa_h=kap), Ao, bo, idx, "after the refusals")
