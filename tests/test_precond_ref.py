"""CPU checks of the preconditioner restatement (`tests/precond_ref.py`): the sine-transform solve against an
independent float64 route (conjugate gradients on the Kronecker-assembled K_box), the placement rule of the lattice
box on hand-worked cases, symmetry of R K_box^-1 R^T, and K_box applied to the un-gathered solution.

Measured on the CPU, DST against CG (rtol 1e-15) on a ball-shaped sparse right-hand side, relative to max |u|:
(64, 64, 41): 3.1e-15, (128, 64, 73): 9.6e-15.  Asserted: 1e-13, ten times what the two references differ by."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import precond_ref as R

H3 = (0.011, 0.017, 0.013)


def ball_points(L, margin=5):
    """Lattice points of a ball inside the interior of a box of lengths L, as (m, 3) coordinates with lo = -1."""
    m = [l - 1 for l in L]
    z, y, x = np.meshgrid(*[np.arange(k) for k in m[::-1]], indexing="ij")
    act = ((x - m[0] / 2) ** 2 + (y - m[1] / 2) ** 2 + (z - m[2] / 2) ** 2) < (min(m) / 2 - margin) ** 2
    return np.stack([x[act], y[act], z[act]], axis=1)


@pytest.mark.parametrize("L", [(64, 64, 41), (128, 64, 73)])
def test_dst_route_equals_cg_on_the_kronecker_matrix(L):
    pts = ball_points(L)
    lo = [-1, -1, -1]
    rng = np.random.default_rng(3)
    p = rng.standard_normal(pts.shape[0])
    x, u = R.apply_minv_u(p, pts, L, lo, H3, full=True)
    c = R.box_coefficients(H3, 3)
    f = R.scatter_u(p, pts, L, lo)
    u2, info = spla.cg(R.box_matrix(L, c), f.ravel(), rtol=1e-15, maxiter=5000)
    assert info == 0
    err = np.abs(u.ravel() - u2).max() / np.abs(u).max()
    print(f"L={L}: DST vs CG {err:.2e} of max|u|")
    assert err <= 1e-13
    # and on the gathered entries alone
    x2 = u2.reshape(u.shape)[R.box_index(pts, L, lo)]
    assert np.abs(x - x2).max() <= 1e-13 * np.abs(x).max()


def test_k_box_of_the_ungathered_solution_is_the_scattered_input():
    L, lo = (64, 128, 30), [3, -7, 2]
    pts = ball_points(L) + np.asarray(lo) + 1
    p = np.random.default_rng(4).standard_normal(pts.shape[0])
    for gdim, h in ((3, H3), (3, (0.02, 0.02, 0.02))):
        x, u = R.apply_minv_u(p, pts, L, lo, h, full=True, gdim=gdim)
        f = R.scatter_u(p, pts, L, lo)
        assert np.abs(R.box_apply(u, R.box_coefficients(h, gdim)) - f).max() <= 1e-10 * np.abs(f).max()
        assert np.array_equal(x, u[R.box_index(pts, L, lo)])
    # 2-D: one plane, c2 = 0
    L2, lo2 = (64, 64, 2), [-1, -1, -1]
    disk = slab(0, 62, 0, 62, 0, 0)
    pts2 = disk[((disk[:, :2] - 31) ** 2).sum(axis=1) < 25 ** 2]
    assert pts2.shape[0] > 100 and np.all(pts2[:, 2] == 0)
    p2 = np.random.default_rng(5).standard_normal(pts2.shape[0])
    x, u = R.apply_minv_u(p2, pts2, L2, lo2, H3[:2] + (0.0,), full=True, gdim=2)
    c = R.box_coefficients(H3, 2)
    assert c[2] == 0.0
    assert np.abs(R.box_apply(u, c) - R.scatter_u(p2, pts2, L2, lo2)).max() <= 1e-10 * np.abs(p2).max()


@pytest.mark.parametrize("weighted", [False, True])
def test_apply_minv_u_is_symmetric(weighted):
    L, lo = (64, 64, 41), [-1, -1, -1]
    pts = ball_points(L)
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((2, pts.shape[0]))
    w = np.exp(rng.uniform(-8.0, 2.0, pts.shape[0])) if weighted else None
    Ma, Mb = (R.apply_minv_u(v, pts, L, lo, H3, weights=w) for v in (a, b))
    lhs, rhs = a @ Mb, Ma @ b
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(a) @ np.abs(Mb))
    assert a @ Ma > 0.0                                      # positive definite


def test_weighted_form_is_the_scaled_plain_form():
    L, lo = (64, 64, 20), [-1, -1, -1]
    pts = ball_points(L, margin=24)
    rng = np.random.default_rng(7)
    p = rng.standard_normal(pts.shape[0])
    D = np.exp(rng.uniform(-6.0, 1.0, pts.shape[0]))
    kd = 2.0 * R.box_coefficients(H3, 3).sum()
    sinv = np.sqrt(kd / D)
    ref = sinv * R.apply_minv_u(sinv * p, pts, L, lo, H3)
    got = R.apply_minv_u(p, pts, L, lo, H3, weights=-D)       # |diag A|
    assert np.abs(got - ref).max() <= 1e-14 * np.abs(ref).max()
    got_ld = R.apply_minv_u(p, pts, L, lo, H3, weights=D, scalings=np.longdouble)
    assert np.abs(got_ld - ref).max() <= 1e-14 * np.abs(ref).max()


def slab(x0, x1, y0, y1, z0, z1):
    """All lattice points of [x0, x1] x [y0, y1] x [z0, z1]."""
    g = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1), np.arange(z0, z1 + 1), indexing="ij")
    return np.stack([a.ravel() for a in g], axis=1)


def test_lattice_box_pick_length_boundary():
    # extent 55: 55 + 9 = 64 -> L = 64, (L - 1 - extent) = 8 -> lo = bb_lo - 1 - 4
    L, lo = R.lattice_box(slab(7, 61, 3, 12, 5, 9), (70, 20, 20), 3)
    assert L[0] == 64 and lo[0] == 7 - 1 - 4
    # extent 56: 65 -> L = 128, (127 - 56) // 2 = 35
    L, lo = R.lattice_box(slab(7, 62, 3, 12, 5, 9), (70, 20, 20), 3)
    assert L[0] == 128 and lo[0] == 7 - 1 - 35
    # the same in y; y extent 10 -> L = 64, (63 - 10) // 2 = 26 (odd remainder rounds down)
    L, lo = R.lattice_box(slab(3, 12, 7, 62, 5, 9), (20, 70, 20), 3)
    assert L[:2] == [64, 128] and lo[:2] == [3 - 1 - 26, 7 - 1 - 35]
    assert R.pick_length(1024) == 1024 and R.pick_length(1025) is None
    assert R.lattice_box(slab(0, 1020, 0, 3, 4, 8), (1020, 8, 12), 3) is None


def test_lattice_box_z_margins():
    n = (20, 20, 40)
    # touching neither face: 4 + 4
    L, lo = R.lattice_box(slab(3, 12, 3, 12, 5, 30), n, 3)
    assert L[2] == 26 + 4 + 4 + 1 and lo[2] == 5 - 1 - 4
    # touching z = 0: open below
    L, lo = R.lattice_box(slab(3, 12, 3, 12, 0, 30), n, 3)
    assert L[2] == 31 + 32 + 4 + 1 and lo[2] == 0 - 1 - 32
    # touching the top vertex plane (index n2): open above
    L, lo = R.lattice_box(slab(3, 12, 3, 12, 5, 40), n, 3)
    assert L[2] == 36 + 4 + 32 + 1 and lo[2] == 5 - 1 - 4
    # both
    L, lo = R.lattice_box(slab(3, 12, 3, 12, 0, 40), n, 3)
    assert L[2] == 41 + 64 + 1 and lo[2] == -33
    # one plane below the top is closed
    L, lo = R.lattice_box(slab(3, 12, 3, 12, 1, 39), n, 3)
    assert L[2] == 39 + 8 + 1 and lo[2] == 1 - 1 - 4
    # too long with open margins: back to 4 + 4
    L, lo = R.lattice_box(slab(3, 5, 3, 5, 0, 1000), (8, 8, 1000), 3)
    assert L[2] == 1001 + 8 + 1 and lo[2] == -5
    assert R.lattice_box(slab(3, 5, 3, 5, 0, 1020), (8, 8, 1020), 3) is None


def test_lattice_box_2d():
    pts = slab(10, 40, 20, 50, 0, 0)
    L, lo = R.lattice_box(pts, (64, 64, 0), 2)
    assert L == [64, 64, 2]
    assert lo == [10 - 1 - (63 - 31) // 2, 20 - 1 - 16, -1]
    assert np.all(R.box_index(pts, L, lo)[0] == 0)


def test_lattice_box_p2():
    # 3 x 3 x 3 vertices of a 4^3 box, cells 1 .. 2 per axis, with the edges of its x lines: the h / 2 lattice holds
    # points 2 .. 6 per axis; touching neither face (top of the fine lattice: 8)
    vijk = slab(0, 4, 0, 4, 0, 4)
    vid = {tuple(q): i for i, q in enumerate(vijk)}
    edges = np.array([[vid[(i, j, k)], vid[(i + 1, j, k)]] for i in (1, 2) for j in (1, 2, 3) for k in (1, 2, 3)])
    pts = R.p2_lattice_points(vijk, edges)
    assert pts.shape[0] == vijk.shape[0] + edges.shape[0]
    assert np.array_equal(pts[vid[(1, 2, 3)]], [2, 4, 6])
    assert np.array_equal(pts[vijk.shape[0]], [3, 2, 2])                  # midpoint of (1,1,1)-(2,1,1)
    act = np.concatenate([[vid[(i, j, k)] for i in (1, 2, 3) for j in (1, 2, 3) for k in (1, 2, 3)],
                          vijk.shape[0] + np.arange(edges.shape[0])])
    L, lo = R.lattice_box(pts[act], (4, 4, 4), 3, p2=True)
    assert L == [64, 64, 5 + 8 + 1] and lo == [2 - 1 - (63 - 5) // 2] * 2 + [2 - 1 - 4]
    # vertices up to the top plane of the mesh: fine index 8 = 2 n2 is the face, not index 4 = n2
    top = np.array([vid[(i, j, k)] for i in (1, 2) for j in (1, 2) for k in (2, 3, 4)])
    L, lo = R.lattice_box(pts[top], (4, 4, 4), 3, p2=True)
    assert L[2] == 5 + 4 + 32 + 1
    mid = np.array([vid[(i, j, k)] for i in (1, 2) for j in (1, 2) for k in (1, 2)])
    L, lo = R.lattice_box(pts[mid], (4, 4, 4), 3, p2=True)              # highest point at index 4 = n2: interior
    assert L[2] == 3 + 4 + 4 + 1


def test_block_jacobi_and_whole_vector():
    import scipy.sparse as sp
    rng = np.random.default_rng(8)
    nvert, nblk = 6, 3
    dof = np.sort(rng.choice(nvert * nblk, 13, replace=False))
    A = sp.csr_matrix(rng.standard_normal((13, 13)) + 6.0 * np.eye(13))
    p = rng.standard_normal(13)
    x, groups, conds = R.apply_block_jacobi(p, A, dof, nvert)
    assert sorted(np.concatenate(groups).tolist()) == list(range(13))
    for rows, cnd in zip(groups, conds):
        assert len(set((dof[rows] % nvert).tolist())) == 1 and np.all(np.diff(dof[rows] // nvert) > 0)
        B = A[rows][:, rows].toarray()
        assert np.abs(B @ x[rows] - p[rows]).max() <= 1e-13 * cnd * np.abs(p[rows]).max()
        assert cnd >= 1.0
    # whole vector: u rows through the lattice, the rest Jacobi
    L, lo = (64, 64, 20), [-1, -1, -1]
    pts = ball_points(L, margin=26)
    nu = pts.shape[0]
    n = nu + 17
    is_u = np.zeros(n, dtype=bool)
    is_u[rng.choice(n, nu, replace=False)] = True
    diag = rng.uniform(0.5, 2.0, n)
    pv = rng.standard_normal(n)
    xv = R.apply_minv(pv, diag, is_u, pts, L, lo, H3)
    assert np.array_equal(xv[~is_u], pv[~is_u] / diag[~is_u])
    assert np.array_equal(xv[is_u], R.apply_minv_u(pv[is_u], pts, L, lo, H3))
    assert np.array_equal(R.apply_minv(pv, diag, is_u), pv / diag)
