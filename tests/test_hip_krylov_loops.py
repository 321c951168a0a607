"""The three native BiCGStab loops of `phx_solve` (mode 0: standard, identity, reduced) through TRUNCATED solves.

`phx_solve` with max_iter = k returns x_k and the recursive relres_k (a ConvergenceWarning, not an error: `kr_drive`
leaves the loop at it == max_iter before the true-residual branch).  k = 1 .. 5 covers both parities, two rolls and two
clears of each slot set.  The loop switches are read once per process, so each setting runs in a child process of its
own (as test_hip_kr_reduced.py): default (reduced loop), PHX_KR_REDUCED=0 (identity loop), PHX_KR_IDENTITY=0 (standard
loop with the lattice preconditioner).  Every system keeps its own CSR copy (PHX_OPT_EXPORT_CSR), so A, b are the bits
the device iterated on (P2: the deterministic re-assembly).

(a) Consistency of x and r, no trajectory needed.  In float64 on the host, A the exported CSR, m its longest row:

        | |b - A x_k|_2 - relres_k |b|_2 |  <=  4 B_k,
        B_k = eps sum_{j <= k} [ (m + 3) | |A| |x_j| |_2 + 3 relres_j |b|_2 ]

    the accumulated rounding of k SpMV pairs and vector updates, every x_j from the truncated solves themselves.  The
    identity and reduced loops add 1e-12 | |A| |x_k| |_2, the project's f64 lattice tolerance (TOL[8] of
    test_hip_precond_operator.py): they take A M^-1 = I on the C rows, which the transforms satisfy to that level.  A
    wrong x, r or s update or a wrong SpMV operand misses this by ten orders of magnitude.

(b) Trajectory: x_k against `krylov_ref.bicgstab` on the exported A, b with a float64 M^-1 per case
    (`precond_ref.apply_minv`, `apply_block_jacobi`; the reduced loop starts from `krylov_ref.reduced_start`, C the
    complement of the stored-row list of `phx_system_export_sell`).  The tolerance is measured, not chosen: sigma_k is
    the largest relative change of x_k^ref over three seeded runs in which every entry of A and b is perturbed by a
    relative 2^-50 U(-1, 1) (the rounding differences the device is entitled to) and every M^-1 output by a relative
    1e-12 U(-1, 1) (the lattice tolerance again);

        |x_k - x_k^ref|_inf <= 100 sigma_k |x_k^ref|_inf,

    100 the margin over a spread measured from three draws.  Condition on the cases (not a measurement): sigma_k <= 1e-8
    for every k <= 5.  `stats["restarts"]` equals the reference's count (0).  A wrong beta, parity or C-row share is an
    O(1e-2) change at k = 2.

(c) PHX_OPT_DETERMINISTIC: the truncated solves k = 1 .. 5 twice on one system give the same bits in x_k and relres_k
    (P1 box under all three loops, P2); for P2 a second, identically built system gives them too (P1 boxes assemble
    with plain atomics, so only repeats on one system are asked of them)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import krylov_ref as K
import precond_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
KMAX = 5
LATTICE_TOL = 1e-12          # TOL[8] of test_hip_precond_operator.py
SIGMA_MAX = 1e-8
MARGIN = 100.0

# child process: per case the truncated solves k = 1 .. KMAX (twice with "repeat", once more on a second system with
# "twin"), the exported system and what the float64 preconditioner needs to know about it
CHILD = r"""
import ctypes as C, json, sys, warnings
import numpy as np
import phifem_amd as P
from phifem_amd import _lib as L
import test_hip_precond_operator as T
cases, kmax, out = json.loads(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
BUILD = {
    "box": lambda c: T.weak_system(P, *T.BOX, [c["n"]] * 3, T.SETS["sphere"], precond=c.get("precond", 1),
                                   deterministic=c.get("det", False)),
    "submesh": lambda c: T.weak_system(P, *T.BOX, [c["n"]] * 3, T.SETS["offset_ellipsoid"], submesh=True),
    "p2": lambda c: T.weak_system(P, *T.BOX, [c["n"]] * 3, T.ball([0.03, -0.02, 0.01]), degree=2, kphi=2, deterministic=True),
    "elasticity": lambda c: T.elasticity_system(P, 2, c["n"], 1.0, False),
}
def solves(s):
    xs, rel, st = [], [], []
    for k in range(1, kmax + 1):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            xs.append(s.solve(rtol=1e-300, max_iter=k).copy())
        rel.append(s.stats["relres"])
        st.append([s.stats["iterations"], s.stats["restarts"], int(s.stats["identity_loop"]), int(s.stats["reduced_loop"]),
                   int(s.stats["converged"])])
    return np.array(xs), np.array(rel), np.array(st), s.stats["precond"]
arrs = {}
for i, c in enumerate(cases):
    sysm = BUILD[c["kind"]](c)
    s = sysm.solver
    xs, rel, st, pname = solves(s)
    info = s.info()
    rowptr, col, val, rhs, dof = s.export_csr()
    rhs_own, dof_own = s.export_rhs_dof()
    assert np.array_equal(dof, dof_own)
    perm = np.zeros(info["n_active"], np.int32)
    L.check(L.lib.phx_system_get_perm(s._sys, L.ptr(perm)[0], None, None, 0))
    rec = dict(x=xs, relres=rel, stats=st, rowptr=rowptr, col=col, val=val, rhs=rhs_own, dof=dof, perm=perm, ijk=sysm.ijk,
               nmesh=np.asarray(sysm.n), nv=np.int64(sysm.mesh.nv),
               info=np.array([info[k] for k in ("n_active", "n_active_u", "n_full", "stencil_rows", "n_slices", "has_csr")]))
    if getattr(sysm, "hl", None) is not None:
        rec["hl"] = np.asarray(sysm.hl, dtype=np.float64)
    if st[0][3]:      # reduced loop: the stored rows in solver order
        rows = np.zeros(max(16 * info["n_slices"], 1), np.int32)
        L.check(L.lib.phx_system_export_sell(s._sys, None, None, None, L.ptr(rows)[0]))
        rec["sell_rows"] = rows[:16 * info["n_slices"]]
    if c.get("repeat"):
        rec["x2"], rec["relres2"], _, _ = solves(s)
    if c.get("twin"):
        rec["x3"], rec["relres3"], _, _ = solves(BUILD[c["kind"]](c).solver)
    for k, v in rec.items():
        arrs[f"c{i}_{k}"] = v
    print("CASE " + json.dumps(dict(name=c["name"], precond=pname, n=info["n_active"], stencil_rows=info["stencil_rows"])), flush=True)
np.savez(out, **arrs)
"""

BOXES = [dict(name="box16", kind="box", n=16), dict(name="box24", kind="box", n=24),
         dict(name="box16_det", kind="box", n=16, det=True, repeat=True)]
SETTINGS = {
    "reduced": ({}, BOXES + [
        dict(name="jacobi_box16", kind="box", n=16, precond=0),       # the structured k_jacobi_u path
        dict(name="submesh16", kind="submesh", n=16),
        dict(name="p2_8", kind="p2", n=8, repeat=True, twin=True),
        dict(name="elasticity16", kind="elasticity", n=16)]),
    "identity": ({"PHX_KR_REDUCED": "0"}, BOXES),
    "standard": ({"PHX_KR_IDENTITY": "0"}, BOXES),
}
# (identity loop, reduced loop) each case must report
FLAGS = {"reduced": (1, 1), "identity": (1, 0), "standard": (0, 0)}
PRECOND = {"box": "box-dst", "submesh": "box-dst", "p2": "box-dst", "elasticity": "vertex-block-jacobi"}


class Case:
    def __init__(self, spec, setting, arrs, i, line):
        self.spec, self.setting, self.line = spec, setting, line
        for k in list(arrs):
            if k.startswith(f"c{i}_"):
                setattr(self, k[len(f"c{i}_"):], arrs[k])
        n = int(self.info[0])
        self.n = n
        self.A = sp.csr_matrix((self.val, self.col, self.rowptr), shape=(n, n))
        self.b = self.rhs
        self.xk = [w[self.dof] for w in self.x]            # x_k in active numbering
        box = spec["kind"] == "box" and spec.get("precond", 1) == 1
        self.ident, self.red = FLAGS[setting] if box else (0, 0)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("krylov_loops")
    out = {}
    for setting, (env_set, cases) in SETTINGS.items():
        env = dict(os.environ)
        env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
        env.pop("PHX_KR_IDENTITY", None)
        env.pop("PHX_KR_REDUCED", None)
        env.update(env_set)
        path = str(tmp / f"{setting}.npz")
        r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(cases), str(KMAX), path], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines = [json.loads(l[5:]) for l in r.stdout.splitlines() if l.startswith("CASE ")]
        assert len(lines) == len(cases)
        arrs = np.load(path)
        arrs = {k: arrs[k] for k in arrs.files}
        for i, (c, line) in enumerate(zip(cases, lines)):
            out[(setting, c["name"])] = Case(c, setting, arrs, i, line)
    return out


ALL = [(s, c["name"]) for s, (_, cases) in SETTINGS.items() for c in cases]


@pytest.mark.parametrize("setting,name", ALL)
def test_each_case_takes_its_loop(runs, setting, name):
    c = runs[(setting, name)]
    assert np.array_equal(c.stats[:, 0], np.arange(1, KMAX + 1)), c.stats          # k iterations were run
    assert np.all(c.stats[:, 2] == c.ident) and np.all(c.stats[:, 3] == c.red), (setting, name, c.stats)
    assert np.all(c.stats[:, 4] == 0)
    want = "jacobi" if c.spec.get("precond", 1) == 0 else PRECOND[c.spec["kind"]]
    assert c.line["precond"] == want, c.line
    if c.spec["kind"] == "box":
        assert c.info[3] > 0, "no stencil rows"                                       # n >= 12 has them
        assert c.info[5] == 1
    print(f"[{setting}/{name}] n={c.n} stencil rows={int(c.info[3])} precond={c.line['precond']} identity={c.ident} "
          f"reduced={c.red}")


@pytest.mark.parametrize("setting,name", ALL)
def test_iterate_and_recursive_residual_agree(runs, setting, name):
    """(a) of the module docstring."""
    c = runs[(setting, name)]
    absA = abs(c.A)
    m = int(np.diff(c.A.indptr).max())
    nb = float(np.linalg.norm(c.b))
    B, worst = 0.0, 0.0
    for k in range(KMAX):
        x = c.xk[k]
        ax = float(np.linalg.norm(absA @ np.abs(x)))
        B += EPS * ((m + 3) * ax + 3 * c.relres[k] * nb)
        tol = 4 * B + (LATTICE_TOL * ax if c.ident else 0.0)
        true = float(np.linalg.norm(c.b - c.A @ x))
        gap = abs(true - c.relres[k] * nb)
        assert gap <= tol, (f"{setting}/{name} k={k + 1}: |b - A x_k| = {true:.17g}, relres_k |b| = {c.relres[k] * nb:.17g}, "
                            f"gap {gap:.3e} > {tol:.3e}")
        worst = max(worst, gap / tol)
    print(f"[{setting}/{name}] (a) n={c.n} m={m} relres_1..{KMAX}={np.array2string(c.relres, precision=3)}: worst "
          f"{worst:.2e} of the bound")


def minv_of(c):
    """float64 M^-1 in active numbering (x-space) of the case's preconditioner."""
    kind = c.spec["kind"]
    diag = c.A.diagonal()
    if kind == "elasticity":
        nv = int(c.nv)
        return lambda A: (lambda p: R.apply_block_jacobi(p, A, c.dof, nv)[0])
    nent = int(c.info[2]) // 2
    is_u = c.dof < nent
    assert is_u.sum() == c.info[1]
    if c.spec.get("precond", 1) == 0:
        return lambda A: (lambda p: R.apply_minv(p, A.diagonal(), is_u))
    act = c.ijk[c.dof[is_u]]
    L, lo = R.lattice_box(act, c.nmesh, 3, p2=kind == "p2")
    assert c.line["precond"] == "box-dst"
    h = list(c.hl)
    return lambda A: (lambda p: R.apply_minv(p, A.diagonal(), is_u, act, L, lo, h))


def c_rows(c):
    """Active indices of the C rows: the complement of the stored-row list (solver order) of the SELL export."""
    rows = c.sell_rows
    rows = np.unique(rows[(rows >= 0) & (rows < c.n)])
    assert rows.size == c.n - int(c.info[3]), (rows.size, c.n, int(c.info[3]))
    stored = np.zeros(c.n, dtype=bool)
    stored[rows] = True
    C = np.sort(c.perm[~stored].astype(np.int64))
    nent = int(c.info[2]) // 2
    assert np.all(c.dof[C] < nent)                      # C rows are u rows
    return C


def reference(A, b, minv, C, seed=None):
    """x_1 .. x_KMAX of krylov_ref.bicgstab; seed: the perturbed run of the sensitivity measurement."""
    if seed is not None:
        rng = np.random.default_rng(seed)
        A = sp.csr_matrix((A.data * (1.0 + 2.0 ** -50 * rng.uniform(-1, 1, A.nnz)), A.indices, A.indptr), shape=A.shape)
        b = b * (1.0 + 2.0 ** -50 * rng.uniform(-1, 1, b.size))
        exact = minv(A)
        m = lambda p: exact(p) * (1.0 + LATTICE_TOL * rng.uniform(-1, 1, p.size))
    else:
        m = minv(A)
    x0 = K.reduced_start(A, b, m, C) if C is not None else None
    return K.bicgstab(A, b, m, x0=x0, k=KMAX)


def sensitivity(A, b, minv, C):
    ref = reference(A, b, minv, C)
    sigma = np.zeros(KMAX)
    for seed in (1, 2, 3):
        pert = reference(A, b, minv, C, seed=seed)
        for k in range(KMAX):
            sigma[k] = max(sigma[k], np.abs(pert.x[k] - ref.x[k]).max() / np.abs(ref.x[k]).max())
    return ref, sigma


@pytest.mark.parametrize("setting,name", ALL)
def test_trajectory_matches_the_float64_iteration(runs, setting, name):
    """(b) of the module docstring."""
    c = runs[(setting, name)]
    C = c_rows(c) if c.red else None
    ref, sigma = sensitivity(c.A, c.b, minv_of(c), C)
    assert np.all(sigma <= SIGMA_MAX), f"{setting}/{name}: the case is too sensitive for this check: sigma = {sigma}"
    nb = float(np.linalg.norm(c.b))
    ratios = np.zeros(KMAX)
    for k in range(KMAX):
        scale = np.abs(ref.x[k]).max()
        err = np.abs(c.xk[k] - ref.x[k]).max()
        ratios[k] = err / (MARGIN * sigma[k] * scale)
    print(f"[{setting}/{name}] (b) sigma_k={np.array2string(sigma, precision=2)} achieved/(100 sigma_k)="
          f"{np.array2string(ratios, precision=2)} relres ref={np.array2string(np.array(ref.rnorm) / nb, precision=3)}")
    assert np.all(ratios <= 1.0), f"{setting}/{name}: x_k leaves the reference: ratios {ratios}, sigma {sigma}"
    # restarts: the identity and reduced loops decide inside the x / r / p pass of iteration k, the standard loop in
    # KR_UPDATE_P, whose k-th run comes after the host has read the scalars it reports
    for k in range(KMAX):
        want = sum(ref.restart[:k + 1]) if c.ident else sum(ref.restart[:k])
        assert c.stats[k, 1] == want, (k, c.stats[:, 1], ref.restart)
    assert not any(ref.restart)


DET = [(s, "box16_det") for s in SETTINGS] + [("reduced", "p2_8")]


@pytest.mark.parametrize("setting,name", DET)
def test_deterministic_truncated_solves_repeat_bit_for_bit(runs, setting, name):
    """(c) of the module docstring."""
    c = runs[(setting, name)]
    for k in range(KMAX):
        assert np.array_equal(c.x[k], c.x2[k]), f"{setting}/{name}: x_{k + 1} differs between two solves of one system " \
            f"(max {np.abs(c.x[k] - c.x2[k]).max():.3e})"
        assert c.relres[k] == c.relres2[k], f"{setting}/{name}: relres_{k + 1} {c.relres[k]!r} vs {c.relres2[k]!r}"
    twin = ""
    if c.spec.get("twin"):
        for k in range(KMAX):
            assert np.array_equal(c.x[k], c.x3[k]) and c.relres[k] == c.relres3[k], \
                f"{setting}/{name}: iteration {k + 1} differs on a second, identically built system"
        twin = ", and on a second system"
    print(f"[{setting}/{name}] (c) x_k and relres_k of k = 1 .. {KMAX} repeat bit for bit on one system{twin}")
