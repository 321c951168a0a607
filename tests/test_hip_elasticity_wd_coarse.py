"""Two-level preconditioner of the weak-Dirichlet elasticity solve (`ElasticitySolver(coarse=...)`,
PHX_OPT_ELWD_COARSE): the vertex blocks plus the additive Galerkin correction R Ac^-1 R^T on multilinear hats of spacing
H = ratio h, one set per displacement component u_a, Ac = R^T A R probed through the solver's own operator.  Checked
against the numpy specification tests/elasticity_wd_ref.py on the sphere of radius 1 about CENTRE in [-1.5, 1.5]^d: the
option handling, the default (nothing changes), Ac against R^T A R built here from the exported node map, the solution
against a direct solve, the iteration count against the vertex blocks alone, the refusals, reproducibility and the
device memory given back."""
import ctypes as C
import functools
import gc
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import elasticity_wd_ref as R
from test_hip_elasticity_wd import CENTRE, box_case, live_bytes, smooth_data, spec, tag

pytestmark = pytest.mark.gpu
PLAIN, COARSE = "vertex-block-jacobi", "vertex-block-jacobi+coarse"


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


@functools.lru_cache(maxsize=None)
def problem(d, n, nu=0.3, direct=False):
    """(mesh, phi, f, u_D, active mask, direct solution of the specification's system or None), computed once."""
    mesh, ds, phi = box_case(d, n)
    f, uD = smooth_data(mesh.x)
    if not direct:
        return mesh, phi, f, uD, None, None
    *_, A, b, act = spec(mesh, ds, phi, f, uD, nu=nu)
    return mesh, phi, f, uD, act, R.solve_direct(A, b, act)


def solved(P, d, n, coarse=None, nu=0.3, rtol=1e-8, deterministic=True, direct=False):
    """A solver of problem(d, n) after one solve -> (solver, solution).  coarse=None: the keyword is not passed."""
    mesh, phi, f, uD, _, _ = problem(d, n, nu, direct)
    kw = {} if coarse is None else {"coarse": coarse}
    s = P.ElasticitySolver(mesh, nu=nu, deterministic=deterministic, **kw)
    s.assemble(phi, f, uD)
    w = s.solve(rtol=rtol, max_iter=200000)
    return s, w


def restriction(x, dof, nv, node_of, ncubes, ratio, d):
    """R (active rows x compact coarse DoFs): multilinear hats of spacing H_a = ratio h_a on [-1.5, 1.5]^d at the lattice
    points c * H_a, c = 0 .. ceil(n_a / ratio), one set per displacement component (block a < d of the DoF layout);
    the rows of p carry nothing."""
    h = [3.0 / ncubes[a] for a in range(d)]
    m = [-(-ncubes[a] // ratio) + 1 if a < d else 1 for a in range(3)]
    M = m[0] * m[1] * m[2]
    blk, node = node_of // M, node_of % M
    ijk = np.stack([node % m[0], (node // m[0]) % m[1], node // (m[0] * m[1])], axis=1)[:, :d]
    xv = x[dof % nv]
    w = np.ones((dof.size, node_of.size))
    for a in range(d):
        w *= np.clip(1.0 - np.abs(xv[:, a:a + 1] - (-1.5 + ijk[None, :, a] * ratio * h[a])) / (ratio * h[a]), 0.0, None)
    w *= (dof // nv)[:, None] == blk[None, :]
    return sp.csr_matrix(w)


def test_option_handling(P):
    L = P._lib
    mesh = P.create_box([-1.5] * 3, [1.5] * 3, [4] * 3)
    for bad in (1, 3, 4, -2):
        with pytest.raises(ValueError):
            L.check(L.lib.phx_set_option(mesh._h, L.OPT_ELWD_COARSE, bad))
    for ok in (0, -1, 5, 12):
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_ELWD_COARSE, ok))
    L.check(L.lib.phx_set_option(mesh._h, L.OPT_ELWD_COARSE, 0))
    for bad in (3, 1, 4, -2, 5.5, "auto", True):
        with pytest.raises(ValueError):
            P.ElasticitySolver(mesh, coarse=bad)
    for kw in (dict(coarse_space=5), dict(multilevel=True)):       # the spellings of other systems' options
        with pytest.raises(NotImplementedError):
            P.ElasticitySolver(mesh, coarse=5, **kw)
    sub, _, _ = box_case(2, 12, False)
    with pytest.raises(NotImplementedError):
        P.ElasticitySolver(sub, coarse=5)


def test_submesh_automatic_stays_on_the_blocks(P):
    """coarse=-1 on a sub-mesh: no refusal, no warning, the vertex blocks, and the reason is there to be read."""
    sub, ds, phi = box_case(2, 12, False)
    f, uD = smooth_data(sub.x)
    s = P.ElasticitySolver(sub, coarse=-1)
    s.assemble(phi, f, uD)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s.solve(rtol=1e-8, max_iter=200000)
    assert s.stats["converged"] and s.stats["precond"] == PLAIN and s.stats["coarse_dofs"] == 0
    assert "not a box" in s.stats["coarse_reason"]


@pytest.mark.parametrize("d,n", [(2, 40), (3, 12)])
def test_default_is_plain(P, d, n):
    """No keyword: vertex blocks alone, and bit for bit the solve of coarse=0."""
    s0, w0 = solved(P, d, n)
    s1, w1 = solved(P, d, n, coarse=0)
    for s in (s0, s1):
        assert s.stats["precond"] == PLAIN
        ci = s.coarse_info()
        assert ci["coarse_dofs"] == 0 and ci["coarse_reason"] is None
    assert s0.stats["iterations"] == s1.stats["iterations"]
    assert w0.tobytes() == w1.tobytes()


def galerkin_case(P, case):
    if case == "box3":
        ncubes, d, n = [12, 10, 15], 3, None
        mesh = P.create_box([-1.5] * 3, [1.5] * 3, ncubes)
        phi = ((mesh.x - np.asarray(CENTRE)) ** 2).sum(axis=1) - 1.0
        tag(P, mesh, phi)
    else:
        d, n = case
        ncubes = [n] * d
        mesh, _, phi = box_case(d, n)
    return mesh, phi, ncubes, d


@pytest.mark.parametrize("case", [(2, 24), (3, 10), "box3"], ids=["2-24", "3-10", "3-12x10x15"])
def test_galerkin_matrix(P, case):
    """Ac^-1 (R^T A R) = I with R built here from the vertex coordinates and the exported node map.

    Which operator: the loop iterates on the column-scaled A D^-1 (x = D^-1 y, D = diag A) and the probes are D R e, so
    the images are (A D^-1)(D R e) = A R e and the exported inverse is that of R^T A R with the UNSCALED matrix of
    `export_csr()` and the plain hats R -- neither is scaled here; the prolongation the solver applies is D R.
    The box of 12 x 10 x 15 cubes has another h, another number of coarse nodes and a cut-short last cell along every
    axis: an axis mix-up in the lattice sizes cannot pass it."""
    mesh, phi, ncubes, d = galerkin_case(P, case)
    f, uD = smooth_data(mesh.x)
    s = P.ElasticitySolver(mesh, coarse=5)
    s.assemble(phi, f, uD)
    s.solve(rtol=1e-8, max_iter=200000)
    assert s.stats["converged"] and s.stats["precond"] == COARSE and s.stats["coarse_ratio"] == 5
    rowptr, col, val, rhs, dof = s.export_csr()
    Aa = sp.csr_matrix((val, col, rowptr), shape=(dof.size,) * 2)
    node_of, ainv = s.coarse_export()
    Rm = restriction(mesh.x, dof, mesh.nv, node_of, ncubes, 5, d)
    assert Rm.shape[1] == s.stats["coarse_dofs"] == s.coarse_info()["coarse_dofs"] > 0
    assert np.all(np.asarray(Rm.sum(axis=0)).ravel() > 0)      # every compact coarse DoF touches an active row
    assert Rm[dof // mesh.nv >= d].nnz == 0
    # ... and no hat that touches an active u row was left out: R is a partition of unity on the active u rows
    assert np.abs(np.asarray(Rm[dof // mesh.nv < d].sum(axis=1)).ravel() - 1.0).max() <= 1e-12
    Ac = (Rm.T @ Aa @ Rm).toarray()
    rel = np.linalg.norm(ainv @ Ac - np.eye(Ac.shape[0])) / np.sqrt(Ac.shape[0])
    print(f"{case}: {Ac.shape[0]} coarse DoFs, cond(Ac) {np.linalg.cond(Ac):.1e}, |Ac^-1 R^T A R - I|_F / sqrt(nc) = {rel:.2e}")
    assert rel <= 1e-8


@pytest.mark.parametrize("d,n,ratio,nu", [(2, 40, 8, 0.3), (2, 40, 8, 0.45), (3, 12, 6, 0.3), (3, 11, 5, 0.3)])
def test_against_direct_solve(P, d, n, ratio, nu):
    """(3, 11, 5): the last coarse cell is cut short by the box."""
    *_, act, wo = problem(d, n, nu, True)
    its = {}
    for coarse in (0, ratio):
        s, w = solved(P, d, n, coarse=coarse, nu=nu, rtol=1e-11, direct=True)
        err = np.abs(w - wo).max() / np.abs(wo).max()
        print(f"d={d} n={n} nu={nu} coarse={coarse}: {s.stats['iterations']} iterations, relres {s.stats['relres']:.2e}, "
              f"max error against the direct solve {err:.2e}, {s.stats['precond']}")
        assert s.stats["relres"] <= 1e-11 and s.stats["converged"]
        assert err <= 1e-6
        assert np.all(w[~act] == 0.0)
        assert s.stats["precond"] == (COARSE if coarse else PLAIN)
        its[coarse] = s.stats["iterations"]
    assert s.stats["coarse_ratio"] == ratio and s.stats["coarse_dofs"] > 0


@pytest.mark.parametrize("d,n,ratio", [(2, 64, 8), (3, 16, 5)])
def test_fewer_iterations(P, d, n, ratio):
    """CPU prototype (tools/experiments/elasticity_wd_coarse.py, rtol 1e-8): 162 -> 78 (0.48) at 64^2 with H = 8h,
    326 -> 122 (0.37) at 16^3 with H = 5h.  0.7 leaves room for the run-to-run spread of BiCGStab counts."""
    its, sol = {}, {}
    for coarse in (0, ratio):
        s, sol[coarse] = solved(P, d, n, coarse=coarse)
        assert s.stats["converged"] and s.stats["precond"] == (COARSE if coarse else PLAIN)
        its[coarse] = s.stats["iterations"]
    diff = np.linalg.norm(sol[ratio] - sol[0]) / np.linalg.norm(sol[0])
    print(f"d={d} n={n}: {its[0]} iterations with the vertex blocks, {its[ratio]} with H = {ratio} h "
          f"({its[ratio] / its[0]:.2f}), {s.stats['coarse_dofs']} coarse DoFs, build {s.stats['coarse_build_s']:.3f} s, "
          f"solutions differ by {diff:.2e}")
    assert its[ratio] <= 0.7 * its[0]
    assert diff <= 1e-6


def test_small_box(P):
    """A ratio that cannot be served is said, never dropped silently; the automatic mode decides quietly."""
    *_, act, wo = problem(2, 12, 0.3, True)
    mesh, phi, f, uD, _, _ = problem(2, 12, 0.3, True)
    s = P.ElasticitySolver(mesh, coarse=8)
    s.assemble(phi, f, uD)
    with pytest.warns(RuntimeWarning, match="smaller than 2 H"):
        w = s.solve(rtol=1e-11, max_iter=200000)
    assert s.stats["precond"] == PLAIN and s.stats["coarse_dofs"] == 0 and s.stats["converged"]
    assert np.abs(w - wo).max() <= 1e-6 * np.abs(wo).max()
    s = P.ElasticitySolver(mesh, coarse=-1)
    s.assemble(phi, f, uD)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        w = s.solve(rtol=1e-11, max_iter=200000)
    assert s.stats["precond"] == PLAIN and "automatic" in s.stats["coarse_reason"]
    assert np.abs(w - wo).max() <= 1e-6 * np.abs(wo).max()


def test_reproducible_and_clean(P):
    """Deterministic mode: probe, inverse, gemv and line passes run in a fixed order; everything the build and the
    correction hold goes back to the pool with the system."""
    sa, wa = solved(P, 3, 12, coarse=6)
    sa._free()
    gc.collect()
    before = live_bytes(P)
    sb, wb = solved(P, 3, 12, coarse=6)
    assert sb.stats["precond"] == COARSE
    assert sa.stats["iterations"] == sb.stats["iterations"]
    assert wa.tobytes() == wb.tobytes()
    assert live_bytes(P) > before
    sb._free()
    gc.collect()
    assert live_bytes(P) == before


def test_the_two_elasticity_solvers_share_a_mesh(P):
    """PHX_OPT_EL_COARSE and PHX_OPT_ELWD_COARSE are two options of one mesh: neither solver moves the other's."""
    from phifem_amd.mesh_scripts import NodalFunction
    d, n = 3, 12
    mesh = P.create_box([-1.5] * d, [1.5] * d, [n] * d)
    x = mesh.x
    f, uD = smooth_data(x)
    phi = ((x - np.asarray(CENTRE)) ** 2).sum(axis=1) - 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(mesh, NodalFunction(-phi), 1, box_mode=True)
    bcv = np.flatnonzero(np.abs(x).max(axis=1) == 1.5)
    si = P.InterfaceElasticitySolver(mesh, coarse=6)
    si.assemble(-phi, f, uD, bcv)
    tag(P, mesh, phi)
    se = P.ElasticitySolver(mesh, coarse=0)
    se.assemble(phi, f, uD)
    for _ in range(2):
        si.solve(rtol=1e-8, max_iter=200000)
        assert si.stats["converged"] and si.stats["precond"] == COARSE
        se.solve(rtol=1e-8, max_iter=200000)
        assert se.stats["converged"] and se.stats["precond"] == PLAIN
    # and the other way round: the weak-Dirichlet system with its correction next to an interface system without
    si0 = P.InterfaceElasticitySolver(mesh, coarse=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(mesh, NodalFunction(-phi), 1, box_mode=True)
    si0.assemble(-phi, f, uD, bcv)
    tag(P, mesh, phi)
    se6 = P.ElasticitySolver(mesh, coarse=6)
    se6.assemble(phi, f, uD)
    for _ in range(2):
        si0.solve(rtol=1e-8, max_iter=200000)
        assert si0.stats["precond"] == PLAIN
        se6.solve(rtol=1e-8, max_iter=200000)
        assert se6.stats["converged"] and se6.stats["precond"] == COARSE
