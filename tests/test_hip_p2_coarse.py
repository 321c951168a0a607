"""Two-level preconditioner of the P2 weak-Dirichlet solve (PhiFEMSolver(coarse_space=...), PHX_OPT_P2_COARSE):
the h/2-lattice sine transform on u and Jacobi on p plus the additive Galerkin correction R Ac^-1 R^T, Ac = R^T A R
probed through the solver's own operator.  Checked: the option handling, Ac against R^T A R built in numpy from the
exported coarse node map, the solution against a direct solve, the iteration count against the plain run, and bit
reproducibility in deterministic mode."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import assembly as OA
from test_hip_p2 import setup as p2_setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def restriction(pts, dof, nd, node_of, n, ratio, d):
    """R (active rows x compact coarse DoFs): multilinear hats of spacing H = ratio h on [-1.5, 1.5]^d, one set per field."""
    h = 3.0 / n
    H = ratio * h
    m = [-(-n // ratio) + 1 if a < d else 1 for a in range(3)]
    M = m[0] * m[1] * m[2]
    fld, node = node_of // M, node_of % M
    ijk = np.stack([node % m[0], (node // m[0]) % m[1], node // (m[0] * m[1])], axis=1)[:, :d]
    X = -1.5 + ijk * H                                          # (nc, d)
    x = pts[dof % nd]                                           # (n_active, d)
    w = np.ones((x.shape[0], X.shape[0]))
    for a in range(d):
        w *= np.clip(1.0 - np.abs(x[:, a:a + 1] - X[None, :, a]) / H, 0.0, None)
    w *= (dof // nd)[:, None] == fld[None, :]
    return sp.csr_matrix(w)


def test_option_handling(P):
    from phifem_amd import _lib as L
    mesh = P.create_box([-1.5] * 3, [1.5] * 3, [4] * 3)
    with pytest.raises(NotImplementedError):
        P.PhiFEMSolver(mesh, degree=1, coarse_space=5)
    with pytest.raises(NotImplementedError):
        P.PhiFEMSolver(mesh, degree=1, coarse_space="auto")
    for bad in (3, 4, 0, -1, "yes", 5.5):
        with pytest.raises(ValueError):
            P.PhiFEMSolver(mesh, degree=2, coarse_space=bad)
    for bad in (1, 3, 4, -2):
        with pytest.raises(ValueError):
            L.check(L.lib.phx_set_option(mesh._h, L.OPT_P2_COARSE, bad))
    for ok in (0, -1, 5, 12):
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_P2_COARSE, ok))
    L.check(L.lib.phx_set_option(mesh._h, L.OPT_P2_COARSE, 0))


def test_submesh_raises(P):
    work = p2_setup(P, 2, 6, 1, box=False)[0]
    with pytest.raises(NotImplementedError):
        P.PhiFEMSolver(work, degree=2, coarse_space=5)


def test_default_is_plain(P):
    work, V, phi, f, uex, A, b, act = p2_setup(P, 2, 12, 1)
    s = P.PhiFEMSolver(work, degree=2)
    s.assemble(phi, f, uex)
    s.solve(rtol=1e-8, max_iter=50000)
    assert s.stats["precond"] == "box-dst"
    ci = s.coarse_info()
    assert ci["coarse_dofs"] == 0 and ci["coarse_reason"] is None


def test_small_box_warns(P):
    """A correction that cannot be built is said, never dropped silently: box smaller than 2 H."""
    work, V, phi, f, uex, A, b, act = p2_setup(P, 2, 12, 1)
    s = P.PhiFEMSolver(work, degree=2, coarse_space=8)
    s.assemble(phi, f, uex)
    with pytest.warns(RuntimeWarning, match="smaller than 2 H"):
        s.solve(rtol=1e-8, max_iter=50000)
    assert s.stats["precond"] == "box-dst" and s.stats["coarse_dofs"] == 0


@pytest.mark.parametrize("d,n", [(2, 24), (3, 10)])
def test_galerkin_matrix(P, d, n):
    """Ac^-1 (R^T A R) = I with R built here from the P2 points and the exported node map, A the exported matrix: pins
    the probing colours (images of one colour disjoint) and the column scaling of the probes."""
    work, V, phi, f, uex, A, b, act = p2_setup(P, d, n, 1)
    s = P.PhiFEMSolver(work, degree=2, coarse_space=5)
    s.assemble(phi, f, uex)
    s.solve(rtol=1e-8, max_iter=100000)
    assert s.stats["precond"] == "box-dst+coarse" and s.stats["coarse_ratio"] == 5
    rowptr, col, val, rhs, dof = s.export_csr()
    Aa = sp.csr_matrix((val, col, rowptr), shape=(rowptr.size - 1,) * 2)
    node_of, ainv = s.coarse_export()
    R = restriction(work.p2_dof_points(), dof, V.ndofs, node_of, n, 5, d)
    assert R.shape[1] == s.stats["coarse_dofs"] == s.stats["coarse_dofs_u"] + s.stats["coarse_dofs_p"]
    assert s.stats["coarse_dofs_u"] > 0 and s.stats["coarse_dofs_p"] > 0
    assert np.all(np.asarray(R.sum(axis=0)).ravel() > 0)      # every compact coarse DoF touches an active row
    Ac = (R.T @ Aa @ R).toarray()
    E = ainv @ Ac - np.eye(Ac.shape[0])
    rel = np.linalg.norm(E) / np.sqrt(Ac.shape[0])
    print(f"d={d} n={n}: {Ac.shape[0]} coarse DoFs, |Ac^-1 R^T A R - I| = {rel:.2e}")
    assert rel <= 1e-8


@pytest.mark.parametrize("d,n", [(2, 16), (3, 10)])
def test_against_direct_solve(P, d, n):
    work, V, phi, f, uex, A, b, act = p2_setup(P, d, n, 2)
    wo = OA.solve_direct(A, b, act)
    res = {}
    for cs in (None, 5):
        s = P.PhiFEMSolver(work, degree=2, levelset_degree=2, coarse_space=cs)
        s.assemble(phi, f, uex)
        w = s.solve(rtol=1e-11, max_iter=100000)
        assert s.stats["relres"] <= 1e-11
        assert np.abs(w - wo).max() <= 1e-6 * np.abs(wo).max()
        assert np.all(w[~act] == 0.0)
        res[cs] = (s.stats["precond"], s.stats["iterations"])
    assert res[None][0] == "box-dst" and res[5][0] == "box-dst+coarse"
    print(f"d={d} n={n}: iterations plain {res[None][1]}, H = 5h {res[5][1]}")


def _p2problem_solve(n, coarse_space, rtol=1e-8):
    import torch
    from phifem_amd.distributed import P2Problem
    prob = P2Problem(n, rtol=rtol, coarse_space=coarse_space)
    prob.setup()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = prob.step()
    w = prob.out.cpu().numpy().copy()
    st = dict(prob.solver.stats)
    del prob
    torch.cuda.empty_cache()
    return res, st, w


def test_fewer_iterations_n24():
    """3-D n = 24 on the data P2Problem generates, deterministic, with and without H = 5 h.  CPU prototype
    (tools/experiments/p2_band_precond.py, rtol 1e-8): 956 -> 534 iterations (0.56).  The counts are taken at rtol 1e-8
    as the prototype's; the solutions are compared at rtol 1e-11 (at 1e-8 two iterates differ by ~4e-6 relative)."""
    r0, s0, w0 = _p2problem_solve(24, None)
    r1, s1, w1 = _p2problem_solve(24, 5)
    assert r0["converged"] and r1["converged"]
    assert s0["precond"] == "box-dst" and s1["precond"] == "box-dst+coarse"
    x0 = _p2problem_solve(24, None, rtol=1e-11)[2]
    x1 = _p2problem_solve(24, 5, rtol=1e-11)[2]
    assert np.linalg.norm(x1 - x0) <= 1e-6 * np.linalg.norm(x0)
    ratio = r1["iterations"] / r0["iterations"]
    print(f"n=24: plain {r0['iterations']} iterations, H = 5h {r1['iterations']} ({ratio:.2f}; prototype 956 -> 534, 0.56), "
          f"{s1['coarse_dofs']} coarse DoFs, build {s1['coarse_build_s']:.3f} s")
    assert r1["iterations"] <= 0.7 * r0["iterations"]


def test_reproducible():
    """Deterministic mode: the probe, the inverse, the gemv and the line passes run in a fixed order."""
    ra, sa, wa = _p2problem_solve(16, 5)
    rb, sb, wb = _p2problem_solve(16, 5)
    assert sa["precond"] == "box-dst+coarse"
    assert ra["iterations"] == rb["iterations"]
    assert np.array_equal(wa, wb)


def test_p2_256():
    """P2Problem(256): "auto" leaves the correction off at this size, where it does not pay, and says so;
    an explicit H = 9 h (the largest compact space the dense inverse takes here) converges to rtol 1e-8, true residual
    verified inside phx_solve, in fewer iterations than the plain run."""
    r0, s0, w0 = _p2problem_solve(256, None)
    with pytest.warns(RuntimeWarning, match="does not pay"):
        ra, sa, wa = _p2problem_solve_warned(256, "auto")
    assert sa["precond"] == "box-dst" and ra["iterations"] == r0["iterations"] and np.array_equal(wa, w0)
    r1, s1, w1 = _p2problem_solve(256, 9)
    assert r0["converged"] and r1["converged"] and r1["relres"] <= 1e-8
    assert s1["precond"] == "box-dst+coarse" and s1["coarse_ratio"] == 9
    print(f"256^3: plain {r0['iterations']} iterations {r0['stage_s']['solve']:.2f} s; H = 9h, {s1['coarse_dofs']} coarse "
          f"DoFs: {r1['iterations']} iterations {r1['stage_s']['solve']:.2f} s (build {s1['coarse_build_s']:.2f} s)")
    assert r1["iterations"] < r0["iterations"]


def _p2problem_solve_warned(n, coarse_space):
    """As _p2problem_solve, but the solver's own warnings reach the caller."""
    import torch
    from phifem_amd.distributed import P2Problem
    prob = P2Problem(n, rtol=1e-8, coarse_space=coarse_space)
    prob.setup()
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="The detection function")
        res = prob.step()
    w = prob.out.cpu().numpy().copy()
    st = dict(prob.solver.stats)
    del prob
    torch.cuda.empty_cache()
    return res, st, w
