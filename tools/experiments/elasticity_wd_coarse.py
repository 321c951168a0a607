"""CPU experiment: two-level preconditioner for the weak-Dirichlet elasticity system (u, p) in P1^d x P1^d
(tests/elasticity_wd_ref.py): vertex-block Jacobi  +  the exact Galerkin correction R Ac^-1 R^T, Ac = R^T A R, on
multilinear hats of spacing H = ratio * h, one set per displacement component u_a on its active DoFs; the p blocks
have no coarse part.  Additive, right-preconditioned BiCGStab to rtol 1e-8; box_problem's default centre, E = 1,
f and u_D as tests/test_hip_elasticity_wd.py::smooth_data with seed 5.
usage: elasticity_wd_coarse.py [d n ratio nu ...]      (no arguments: the table of DESIGN.md 7h)"""
import os, sys, time
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", ".."), os.path.join(HERE, "..", "..", "tests")]
import elasticity_wd_ref as W


def bicgstab(A, b, M, rtol=1e-8, maxit=5000):
    """Right-preconditioned BiCGStab as tools/experiments/precond_variants.py -> (x, iterations)."""
    x = np.zeros_like(b); r = b.copy(); rh = r.copy(); rho = alpha = om = 1.0
    v = np.zeros_like(b); p = np.zeros_like(b); bn = np.linalg.norm(b)
    for it in range(1, maxit + 1):
        rho1 = rh @ r
        beta = (rho1 / rho) * (alpha / om); rho = rho1
        p = r + beta * (p - om * v)
        ph = M(p); v = A @ ph
        alpha = rho / (rh @ v)
        s = r - alpha * v
        sh = M(s); t = A @ sh
        om = (t @ s) / (t @ t)
        x += alpha * ph + om * sh
        r = s - om * t
        if np.linalg.norm(r) <= rtol * bn:
            return x, it
    return x, maxit

TABLE = [(2, 32, 8, 0.3), (2, 40, 8, 0.3), (2, 64, 8, 0.3), (2, 64, 5, 0.3), (2, 128, 8, 0.3), (2, 128, 16, 0.3),
         (2, 64, 8, 0.45), (3, 11, 5, 0.3), (3, 12, 6, 0.3), (3, 16, 5, 0.3), (3, 24, 6, 0.3), (3, 32, 8, 0.3),
         (3, 16, 5, 0.45)]


def restriction(idx, nv, d, n, ratio):
    """R (active rows x used coarse DoFs): hats at the lattice points c * ratio, c = 0 .. ceil(n / ratio), per u_a."""
    m = -(-n // ratio) + 1
    blk, vert = idx // nv, idx % nv
    ijk = np.stack([(vert // (n + 1) ** a) % (n + 1) for a in range(d)], axis=1)
    rows, cols, vals = [], [], []
    sel = np.flatnonzero(blk < d)
    for corner in np.ndindex(*(2,) * d):
        c = np.minimum(ijk[sel] // ratio, m - 2) + np.asarray(corner)
        w = np.prod(np.clip(1.0 - np.abs(ijk[sel] / ratio - c), 0.0, None), axis=1)
        node = sum(c[:, a] * m ** a for a in range(d))
        keep = w > 0.0
        rows.append(sel[keep]); cols.append(blk[sel][keep] * m ** d + node[keep]); vals.append(w[keep])
    R = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(idx.size, d * m ** d))
    used = np.flatnonzero(np.asarray(R.sum(axis=0)).ravel() > 0)
    return R[:, used].tocsr()


def main(d, n, ratio, nu):
    t0 = time.time()
    topo, x, ct, ft, ds, phi = W.box_problem(d, n)
    rng = np.random.default_rng(5)
    f, uD = np.sin(x @ rng.standard_normal((d, d))) + 0.3, np.cos(x @ rng.standard_normal((d, d)))
    A, b, act = W.assemble_elasticity_wd(topo, x, ct, ft, ds, phi, f, uD, E=1.0, nu=nu)
    idx = np.flatnonzero(act)
    Aa, ba = A[idx][:, idx].tocsr(), b[idx]
    R = restriction(idx, topo.nv, d, n, ratio)
    Ac = (R.T @ Aa @ R).toarray()
    cond = np.linalg.cond(Ac)
    Aci = np.linalg.inv(Ac)
    vert = idx % topo.nv
    order = np.argsort(vert, kind="stable")
    groups = np.split(order, np.flatnonzero(np.diff(vert[order])) + 1)
    Binv = sp.block_diag([np.linalg.inv(Aa[g][:, g].toarray()) for g in groups], format="csr")
    perm = np.concatenate(groups)

    def MB(r):
        z = np.empty_like(r); z[perm] = Binv @ r[perm]; return z

    its = [bicgstab(Aa, ba, M, rtol=1e-8, maxit=5000)[1] for M in (MB, lambda r: MB(r) + R @ (Aci @ (R.T @ r)))]
    print(f"| {d}-D {n}^{d}, H = {ratio}h | {nu} | {its[0]} -> {its[1]} | {R.shape[1]} |   "
          f"(cond Ac {cond:.1e}, {idx.size} DoFs, {time.time() - t0:.0f} s)", flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    for q in ([(int(a[i]), int(a[i + 1]), int(a[i + 2]), float(a[i + 3])) for i in range(0, len(a), 4)] or TABLE):
        main(*q)
