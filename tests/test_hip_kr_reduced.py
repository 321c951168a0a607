"""Reduced identity loop of the native BiCGStab (phx_solve.hip, kr_reduced).

B = A M^-1 is the identity on the rows the stencil kernel applies (C rows).  Started from x0 = M^-1 E_C b_C the
residual vanishes on C and so does every later Krylov vector: the loop runs on compact vectors over the stored rows
and forms x = M^-1 u only where a solution is handed out.  Checked here against the full-length identity loop
(PHX_KR_REDUCED=0) and the standard loop (PHX_KR_IDENTITY=0), each setting in a child process (the switches are read
once per process): convergence with the true residual computed on the host from the exported CSR, the C-row residual at
rounding level, repeated solves of one system, and the systems that must not take the reduced loop."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEVELSETS = {
    "sphere": "(x ** 2).sum(axis=1) - 1.0",
    "torus": "(np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2) - 0.8) ** 2 + x[:, 2] ** 2 - 0.16",
    "two_balls": "np.minimum(((x - [0.65, 0.1, 0.0]) ** 2).sum(axis=1) - 0.36, ((x + [0.65, 0.0, 0.2]) ** 2).sum(axis=1) - 0.30)",
}

# child process: per case one JSON line with the stats, the host residuals of the solution (all rows; rows of vertices
# deep inside the domain, phi < phi_min / 2, which are stencil rows) and, with "repeat", of a second solve
CHILD = r"""
import json, sys, warnings
import numpy as np
import scipy.sparse as sp
import phifem_amd as P
from phifem_amd import _lib as L_
from phifem_amd.mesh_scripts import NodalFunction
cases, out = json.loads(sys.argv[1]), sys.argv[2]
sols = {}
for k, c in enumerate(cases):
    d = 3
    mesh = P.create_box([-1.5] * d, [1.5] * d, [c["n"]] * d)
    x = mesh.x
    phi = eval(c["phi"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, sub, _, _ = P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=c["mode"] == "box",
                                                  single_layer_cut=True)
    m = mesh if c["mode"] == "box" else sub
    L_.check(L_.lib.phx_set_option(m._h, L_.OPT_PRECOND, c.get("precond", 1)))
    if c.get("det"):
        L_.check(L_.lib.phx_set_option(m._h, L_.OPT_DETERMINISTIC, 1))
    x = m.x
    phi = eval(c["phi"])
    deg = c.get("degree", 1)
    if deg == 2:
        x = m.p2_dof_points()
    uex = np.prod(np.sin(x), axis=1)
    s = P.PhiFEMSolver(m, degree=deg) if deg == 2 else P.PhiFEMSolver(m, deterministic=bool(c.get("det")))
    s.assemble(phi, float(d) * uex, uex)
    w = s.solve(rtol=c["rtol"], max_iter=20000)
    st = dict(s.stats)
    rec = {"it": st["iterations"], "relres": st["relres"], "conv": st["converged"], "ident": st["identity_loop"],
           "red": st["reduced_loop"], "precond": st["precond"], "restarts": st["restarts"]}
    if c.get("repeat"):
        w2 = s.solve(rtol=c["rtol"], max_iter=20000)
        rec.update(it2=s.stats["iterations"], red2=s.stats["reduced_loop"], conv2=s.stats["converged"])
        sols[f"r{k}"] = w2
    if deg == 1:
        rowptr, col, val, rhs, dof = s.export_csr()
        A = sp.csr_matrix((val, col, rowptr), shape=(rowptr.size - 1,) * 2)
        nb = float(np.linalg.norm(rhs))
        res = rhs - A @ w[dof]
        isu = dof < m.x.shape[0]
        deep = isu.copy()
        deep[isu] = phi[dof[isu]] < 0.5 * phi.min()
        rec.update(host_relres=float(np.linalg.norm(res)) / nb, deep=int(deep.sum()),
                   deep_res=float(np.abs(res[deep]).max()) / float(np.abs(rhs).max()))
        if c.get("repeat"):
            rec["host_relres2"] = float(np.linalg.norm(rhs - A @ w2[dof])) / nb
    sols[f"w{k}"] = w
    print("CASE " + json.dumps(rec), flush=True)
np.savez(out, **sols)
"""


def _run(cases, tmp_path, tag, env_set):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.pop("PHX_KR_IDENTITY", None)
    env.pop("PHX_KR_REDUCED", None)
    env.update(env_set)
    out = str(tmp_path / f"{tag}.npz")
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(cases), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    stats = [json.loads(l[5:]) for l in r.stdout.splitlines() if l.startswith("CASE ")]
    assert len(stats) == len(cases)
    sols = np.load(out)
    return stats, {k: sols[k] for k in sols.files}


RTOL = 1e-9
CASES = [
    {"n": 64, "phi": LEVELSETS["sphere"], "mode": "box", "rtol": RTOL, "repeat": True},
    {"n": 64, "phi": LEVELSETS["torus"], "mode": "box", "rtol": RTOL, "repeat": True},
    {"n": 48, "phi": LEVELSETS["two_balls"], "mode": "box", "rtol": RTOL, "repeat": True},
    {"n": 48, "phi": LEVELSETS["sphere"], "mode": "box", "rtol": RTOL, "repeat": True, "det": True},
]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kr_reduced")
    return {tag: _run(CASES, tmp, tag, e) for tag, e in
            (("red", {}), ("full", {"PHX_KR_REDUCED": "0"}), ("std", {"PHX_KR_IDENTITY": "0"}))}


def test_reduced_loop_converges(runs):
    """The reduced loop is in force by default on the stencil-coded box systems, the switches turn it off, and every
    solve meets rtol in the host-computed true residual."""
    for tag in ("red", "full", "std"):
        for c, a in zip(CASES, runs[tag][0]):
            assert a["red"] == (tag == "red") and a["ident"] == (tag != "std"), (tag, c, a)
            assert a["precond"] == "box-dst" and a["conv"] and a["relres"] <= RTOL, (tag, c, a)
            assert a["host_relres"] <= RTOL * (1 + 1e-4), (tag, c, a)


def test_reduced_loop_matches_the_other_loops(runs):
    """Iteration counts within 20 % of the full-length identity loop and of the standard loop; solutions within 100 rtol."""
    red, wred = runs["red"]
    for tag in ("full", "std"):
        other, wo = runs[tag]
        for k, (c, a, b) in enumerate(zip(CASES, red, other)):
            assert abs(a["it"] - b["it"]) <= max(3, 0.2 * b["it"]), (tag, c, a, b)
            wa, wb = wred[f"w{k}"], wo[f"w{k}"]
            assert np.abs(wa - wb).max() <= 100 * RTOL * np.abs(wb).max(), (tag, c, np.abs(wa - wb).max())


def test_stencil_rows_residual_at_rounding_level(runs):
    """The iteration never touches the C rows: their residual b_C - (A M^-1 u)_C with u_C = b_C is the rounding of the
    transforms (measured 1e-14 .. 7e-13 of max |b| on these systems), two orders below rtol and more."""
    for c, a in zip(CASES, runs["red"][0]):
        assert a["deep"] > 100, (c, a)
        assert a["deep_res"] <= 1e-2 * RTOL, (c, a)


def test_repeated_solve_gives_the_same_answer(runs):
    """A second solve of the same system (workspace and maps kept) takes the reduced loop again and returns the same
    solution within 100 rtol.  (Without PHX_OPT_DETERMINISTIC repeated solves need not be bit-identical: the dot
    products are summed by atomics in arrival order, and the iteration counts of the full-length and the standard loop
    may move between solves of one system as well.  With it they ARE bit-identical, iterate by iterate, under all three
    loops: tests/test_hip_krylov_loops.py.  The option has to be the solver's own, `PhiFEMSolver(deterministic=True)`:
    `solve()` sets PHX_OPT_DETERMINISTIC from that flag, whatever was set on the mesh before.)"""
    stats, sols = runs["red"]
    for k, (c, a) in enumerate(zip(CASES, stats)):
        assert a["red2"] and a["conv2"] and a["host_relres2"] <= RTOL * (1 + 1e-4), (c, a)
        w, w2 = sols[f"w{k}"], sols[f"r{k}"]
        assert np.abs(w - w2).max() <= 100 * RTOL * np.abs(w).max(), (c, np.abs(w - w2).max())


def test_gated_systems_keep_their_loop(tmp_path):
    """Sub-mesh, Jacobi, the f32 lattice and P2 do not take the reduced loop; they still converge."""
    cases = [
        {"n": 40, "phi": LEVELSETS["sphere"], "mode": "sub", "rtol": 1e-8},
        {"n": 24, "phi": LEVELSETS["sphere"], "mode": "box", "rtol": 1e-8, "precond": 0},
        {"n": 24, "phi": LEVELSETS["sphere"], "mode": "box", "rtol": 1e-8, "precond": 2},
        {"n": 12, "phi": LEVELSETS["sphere"], "mode": "box", "rtol": 1e-8, "degree": 2},
    ]
    st, _ = _run(cases, tmp_path, "gate", {})
    for c, s in zip(cases, st):
        assert not s["red"] and not s["ident"] and s["conv"], (c, s)
