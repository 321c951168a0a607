"""CPU experiment (numpy / scipy on the specification tests/heat_ref.py): BiCGStab iterations on the reaction system
c u - Lap u (weak-Dirichlet P1 x P1, unit sphere in [-1.5, 1.5]^d, c = 1 / h) with three preconditioners of the u block
  J    Jacobi
  K    the plain lattice Laplacian of the box around the active vertices (what the library applies by sine transforms)
  K+c  the same with the lumped reaction term folded in: K + c h^d I
(the p block keeps Jacobi in all three), and on the Poisson system (c = 0) with J and K for comparison.  Decides
whether the shifted lattice is worth a device implementation: it is not.  Not part of the product.
usage: heat_precond.py [d:n ...]      default 2:32 2:64 3:12 3:20"""
import os
import sys
import warnings

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import heat_ref as R  # noqa: E402
from elasticity_wd_ref import box_problem  # noqa: E402


def lattice(d, n, uidx, shift, margin=4):
    """(LU of K + shift I on the lattice box around the active vertices, positions of the active vertices in it)."""
    n1 = n + 1
    ijk = np.stack([(uidx // n1 ** a) % n1 for a in range(d)], axis=1)
    lo, hi = ijk.min(0) - margin, ijk.max(0) + margin
    m = hi - lo + 1
    h = 3.0 / n
    T = lambda k: sp.diags([-np.ones(k - 1), 2 * np.ones(k), -np.ones(k - 1)], [-1, 0, 1])
    K = sp.csr_matrix((int(np.prod(m)),) * 2)
    for a in range(d):
        term = sp.identity(1)
        for b in reversed(range(d)):          # x fastest
            term = sp.kron(term, T(m[b]) if b == a else sp.identity(m[b]))
        K = K + term
    K = h ** (d - 2) * K + shift * sp.identity(K.shape[0])
    pos = np.zeros(uidx.size, dtype=np.int64)
    for a in reversed(range(d)):
        pos = pos * m[a] + (ijk[:, a] - lo[a])
    return spla.splu(K.tocsc()), pos


def iterations(A, b, M, rtol=1e-8):
    count = [0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, info = spla.bicgstab(A, b, rtol=rtol, atol=0.0, maxiter=5000, M=spla.LinearOperator(A.shape, M),
                                callback=lambda xk: count.__setitem__(0, count[0] + 1))
    assert info == 0 and np.linalg.norm(A @ x - b) <= 10 * rtol * np.linalg.norm(b)
    return count[0]


def main(d, n):
    topo, x, ct, ft, ds, phi = box_problem(d, n, (0.0, 0.0, 0.0))
    h = 3.0 / n
    f, uD, g = np.sin(x[:, 0]) + 0.2, 0.1 * x[:, 0] * x[:, 1], np.cos(x[:, -1])
    row = []
    for c in (1.0 / h, 0.0):
        A, b, act = R.assemble_reaction_wd(topo, x, ct, ft, ds, phi, f, uD, c, g)
        idx = np.flatnonzero(act)
        Aa, ba = A[idx][:, idx].tocsr(), b[idx]
        nu = int((idx < topo.nv).sum())
        dg = Aa.diagonal()

        def with_lattice(shift):
            lu, pos = lattice(d, n, idx[:nu], shift)

            def M(r):
                grid = np.zeros(lu.shape[0])
                grid[pos] = r[:nu]
                return np.concatenate([lu.solve(grid)[pos], r[nu:] / dg[nu:]])
            return M
        row.append(iterations(Aa, ba, lambda r: r / dg))
        row.append(iterations(Aa, ba, with_lattice(0.0)))
        if c > 0.0:
            row.append(iterations(Aa, ba, with_lattice(c * h ** d)))
    print(f"{d}-D, n = {n}: c = 1/h: Jacobi {row[0]}, lattice K {row[1]}, lattice K + c h^d I {row[2]} | "
          f"Poisson: Jacobi {row[3]}, lattice K {row[4]}", flush=True)


if __name__ == "__main__":
    for arg in sys.argv[1:] or ["2:32", "2:64", "3:12", "3:20"]:
        main(*(int(v) for v in arg.split(":")))
