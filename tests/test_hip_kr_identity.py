"""Identity loop of the native BiCGStab (phx_solve.hip, kr_identity).

On a structured P1 system with the f64 lattice preconditioner M = R K_box^-1 R^T, a row the stencil kernel applies is
the 7-point lattice row of K_box, so (A M p)_i = p_i there: the loop skips those rows in both SpMVs and fuses the
x / r / p passes.  Checked here: the identity on the exported matrix, the same solutions and iteration counts with the
loop on and forced off (PHX_KR_IDENTITY=0, read once per process: each setting runs in a child process), the systems
that must keep the standard loop."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import scipy.fft as sf
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


LEVELSETS = {
    "sphere": "(x ** 2).sum(axis=1) - 1.0",
    "torus": "(np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2) - 0.8) ** 2 + x[:, 2] ** 2 - 0.16",
    "two_balls": "np.minimum(((x - [0.65, 0.1, 0.0]) ** 2).sum(axis=1) - 0.36, ((x + [0.65, 0.0, 0.2]) ** 2).sum(axis=1) - 0.30)",
}

# child process: solve a list of cases, print one JSON line per case, save the solutions
CHILD = r"""
import json, sys, warnings
import numpy as np
import phifem_amd as P
from phifem_amd import _lib as L_
from phifem_amd.mesh_scripts import NodalFunction
cases, out = json.loads(sys.argv[1]), sys.argv[2]
sols = {}
for k, c in enumerate(cases):
    d = c.get("d", 3)
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
    s = P.PhiFEMSolver(m, degree=deg) if deg == 2 else P.PhiFEMSolver(m)
    s.assemble(phi, float(d) * uex, uex)
    w = s.solve(rtol=c["rtol"], max_iter=20000)
    sols[f"w{k}"] = w
    if c.get("repeat"):   # the same system solved again
        sols[f"r{k}"] = s.solve(rtol=c["rtol"], max_iter=20000)
    print("CASE " + json.dumps({"it": s.stats["iterations"], "relres": s.stats["relres"],
                                "conv": s.stats["converged"], "ident": s.stats["identity_loop"],
                                "precond": s.stats["precond"], "restarts": s.stats["restarts"]}), flush=True)
np.savez(out, **sols)
"""


def _run(cases, tmp_path, tag, identity_env):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.pop("PHX_KR_IDENTITY", None)
    if identity_env is not None:
        env["PHX_KR_IDENTITY"] = identity_env
    out = str(tmp_path / f"{tag}.npz")
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(cases), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    stats = [json.loads(l[5:]) for l in r.stdout.splitlines() if l.startswith("CASE ")]
    assert len(stats) == len(cases)
    sols = np.load(out)
    return stats, [sols[f"w{k}"] for k in range(len(cases))], {k: sols[k] for k in sols.files if k[0] == "r"}


SWITCH_CASES = [
    {"n": 32, "phi": LEVELSETS["sphere"], "mode": "box", "rtol": 1e-9},
    {"n": 64, "phi": LEVELSETS["sphere"], "mode": "box", "rtol": 1e-9},
    {"n": 128, "phi": LEVELSETS["sphere"], "mode": "box", "rtol": 1e-9},
    {"n": 64, "phi": LEVELSETS["torus"], "mode": "box", "rtol": 1e-9},
    {"n": 48, "phi": LEVELSETS["two_balls"], "mode": "box", "rtol": 1e-9},
    {"n": 64, "phi": LEVELSETS["sphere"], "mode": "sub", "rtol": 1e-9},
    {"n": 40, "phi": LEVELSETS["torus"], "mode": "sub", "rtol": 1e-9},
]


def test_identity_loop_matches_the_standard_loop(tmp_path):
    """Both switch settings: same convergence (iteration counts within 20 %: on these small systems the count moves
    by 10 of 66 from run to run with the order of the atomic dot products, 56 = 56 on the 256^3 benchmark), true residual <= rtol, solutions within 100 rtol of
    each other (two iterates that both meet rtol: measured 4 and 22 rtol); the loop is in force (box mode) only with the switch
    unset."""
    st_on, w_on, _ = _run(SWITCH_CASES, tmp_path, "on", None)
    st_off, w_off, _ = _run(SWITCH_CASES, tmp_path, "off", "0")
    for c, a, b, wa, wb in zip(SWITCH_CASES, st_on, st_off, w_on, w_off):
        # sub-mesh systems are not stencil-coded: they keep the standard loop either way
        assert a["ident"] == (c["mode"] == "box") and not b["ident"], (c, a, b)
        assert a["precond"] == b["precond"] == "box-dst"
        assert a["conv"] and b["conv"] and a["relres"] <= c["rtol"] and b["relres"] <= c["rtol"], (c, a, b)
        assert abs(a["it"] - b["it"]) <= max(3, 0.2 * b["it"]), (c, a, b)
        assert np.abs(wa - wb).max() <= 100 * c["rtol"] * np.abs(wb).max(), (c, np.abs(wa - wb).max())


def test_other_systems_keep_the_standard_loop(tmp_path):
    """Jacobi, the f32 lattice and P2: the standard loop with the switch unset; the solves still converge."""
    cases = [
        {"n": 24, "phi": LEVELSETS["sphere"], "mode": "box", "rtol": 1e-8, "precond": 0},
        {"n": 24, "phi": LEVELSETS["sphere"], "mode": "box", "rtol": 1e-8, "precond": 2},
        {"n": 12, "phi": LEVELSETS["sphere"], "mode": "box", "rtol": 1e-8, "degree": 2},
    ]
    st, _, _ = _run(cases, tmp_path, "gate", None)
    assert [s["precond"] for s in st] == ["jacobi", "box-dst", st[2]["precond"]]
    for s in st:
        assert not s["ident"] and s["conv"], st


def test_stencil_rows_satisfy_the_identity(P):
    """(A M p)_i = p_i on every row of the exported system that is the 7-point lattice row over active u columns,
    M = R K_box^-1 R^T with K_box the lattice Laplacian of a box around the mesh (scipy DST-I)."""
    from phifem_amd.mesh_scripts import NodalFunction
    n = 24
    mesh = P.create_box([-1.5] * 3, [1.5] * 3, [n] * 3)
    x = mesh.x
    phi = (x ** 2).sum(axis=1) - 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=True, single_layer_cut=True)
    uex = np.prod(np.sin(x), axis=1)
    s = P.PhiFEMSolver(mesh)
    s.assemble(phi, 3.0 * uex, uex)
    rowptr, col, val, rhs, dof = s.export_csr()
    nv = x.shape[0]
    A = sp.csr_matrix((val, col, rowptr), shape=(rowptr.size - 1,) * 2)
    h = 3.0 / n
    c = np.array([h, h, h])           # h_b h_c / h_a on a cube lattice
    # lattice index of every vertex, from the coordinates
    ijk = np.rint((x + 1.5) / h).astype(np.int64)
    N = n + 1
    isu = dof < nv
    lat = np.full((N + 2,) * 3, -1, dtype=np.int64)   # one Dirichlet plane around the mesh on every side
    lat[ijk[dof[isu], 2] + 1, ijk[dof[isu], 1] + 1, ijk[dof[isu], 0] + 1] = np.nonzero(isu)[0]
    # rows that are the lattice row: 7 stored entries, all u columns, the right values at the 6 neighbours
    Acoo = A.tocsr()
    rows, n7, nlat = [], 0, 0
    offs = [(0, 0, 0, 2 * c.sum())] + [(dz, dy, dx, -c[a]) for a, (dz, dy, dx) in
                                        ((0, (0, 0, 1)), (0, (0, 0, -1)), (1, (0, 1, 0)), (1, (0, -1, 0)),
                                         (2, (1, 0, 0)), (2, (-1, 0, 0)))]
    for i in np.nonzero(isu)[0]:
        lo, hi = Acoo.indptr[i], Acoo.indptr[i + 1]
        cols, vals = Acoo.indices[lo:hi], Acoo.data[lo:hi]
        nzm = vals != 0.0
        cols, vals = cols[nzm], vals[nzm]
        if cols.size != 7:
            continue
        n7 += 1
        v = dof[i]
        k0, j0, i0 = ijk[v, 2] + 1, ijk[v, 1] + 1, ijk[v, 0] + 1
        want = {}
        for dz, dy, dx, cv in offs:
            q = lat[k0 + dz, j0 + dy, i0 + dx]
            if q < 0:
                break
            want[int(q)] = cv
        if len(want) != 7:
            continue
        nlat += 1
        got = dict(zip(cols.tolist(), vals.tolist()))
        if set(got) == set(want) and all(abs(got[q] - want[q]) <= 1e-12 * 2 * c.sum() for q in want):
            rows.append(i)
    rows = np.array(rows)
    assert rows.size > 0.2 * isu.sum(), (rows.size, n7, nlat, int(isu.sum()), A.shape)
    # M p: extend by zero to the lattice, solve K_box z = R^T p (DST-I), restrict
    rng = np.random.default_rng(5)
    p = rng.standard_normal(A.shape[0])
    f = np.zeros((N, N, N))
    f[ijk[dof[isu], 2], ijk[dof[isu], 1], ijk[dof[isu], 0]] = p[isu]
    L = N + 1
    lam = c[0] * (2.0 - 2.0 * np.cos(np.pi * np.arange(1, L) / L))
    lam3 = lam[:, None, None] + lam[None, :, None] + lam[None, None, :]
    z = sf.idstn(sf.dstn(f, type=1) / lam3, type=1)
    Mp = p.copy()                      # p rows: identity
    Mp[isu] = z[ijk[dof[isu], 2], ijk[dof[isu], 1], ijk[dof[isu], 0]]
    AMp = A @ Mp
    assert np.abs(AMp[rows] - p[rows]).max() <= 1e-11 * np.abs(p).max()
