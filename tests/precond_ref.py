"""The preconditioner application M^-1 p of the Krylov loop (test infrastructure): a numpy / scipy restatement, in
float64, of the operator that `phx_precond.inc.hip` and `phx_blockjac.inc.hip` apply between the Krylov vector and
the lattice.

    M^-1 = R K_box^-1 R^T   on the u block,    p_i / A_ii   on every other row,

K_box = c0 T_x + c1 T_y + c2 T_z (T = tridiag(-1, 2, -1), c_a = h_b h_c / h_a) on the interior of a lattice box of
L0 x L1 x L2 intervals with homogeneous Dirichlet faces, R the restriction of that box to the active u DoFs.  The
box is placed by `lattice_box` (the rule of `box_precond_setup`, "Builds the (rank-local) preconditioner"): the
constants below restate the `#define`s of the library and appear nowhere else.  The elasticity system takes the
inverse of the diagonal block of A over the active DoFs of each vertex (`k_bj_build` / `k_bj_apply`).

Lattice coordinates are integers: vertex (i, j, k) of the mesh box for P1, the point (2 i, 2 j, 2 k) of the lattice
of spacing h / 2 for a P2 vertex and the sum of its two vertices' coordinates for an edge midpoint
(`p2_lattice_points`).  2-D sets carry k = 0.
"""
import numpy as np
import scipy.fft as sf
import scipy.sparse as sp

MARGIN = 4            # PHX_PRECOND_MARGIN: planes between the active points and a closed Dirichlet face
MARGIN_OPEN = 32      # PHX_PRECOND_MARGIN_OPEN: z margin on a side where the active set reaches the mesh box face
PICK_LENGTHS = (64, 128, 192, 256, 384, 512, 768, 1024)   # dst_pick_length: L = 2^a 3^b, b <= 1, 64 | L
MAX_COLUMN = 1025     # the longest z column (box_precond_setup: "> 1025")


def pick_length(need):
    """Smallest transform length >= need, None beyond the longest."""
    for c in PICK_LENGTHS:
        if c >= need:
            return c
    return None


def p2_lattice_points(vertex_ijk, edges):
    """Lattice points (spacing h / 2) of the P2 entities: vertices at even points, then the edge midpoints."""
    vertex_ijk = np.asarray(vertex_ijk, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.int64)
    return np.concatenate([2 * vertex_ijk, vertex_ijk[edges[:, 0]] + vertex_ijk[edges[:, 1]]], axis=0)


def lattice_box(active_ijk, mesh_n, gdim, p2=False):
    """(L[3], lo[3]) of the lattice box around the active u lattice points `active_ijk` (m, 3) of a mesh box of
    `mesh_n` cells per axis: interior point q of the box sits at lattice coordinate lo + 1 + q.  With p2 the points
    and the top face are those of the h / 2 lattice.  None where the library stays with Jacobi (box too long)."""
    q = np.asarray(active_ijk, dtype=np.int64).reshape(-1, 3)
    bb_lo, bb_hi = q.min(axis=0), q.max(axis=0)
    L, lo = [0, 0, 0], [0, 0, 0]
    for a in range(3):
        extent = int(bb_hi[a] - bb_lo[a] + 1)
        if a == 2 and gdim == 3:
            # the z planes are solved as tridiagonal systems: exactly extent + margins planes.  The top face of the
            # mesh box is its last vertex plane, on the h / 2 lattice for P2
            top = int(mesh_n[2]) * (2 if p2 else 1)
            mlo = MARGIN_OPEN if bb_lo[2] == 0 else MARGIN
            mhi = MARGIN_OPEN if bb_hi[2] == top else MARGIN
            if extent + mlo + mhi + 1 > MAX_COLUMN:
                mlo = mhi = MARGIN
            L[a] = extent + mlo + mhi + 1
            if L[a] > MAX_COLUMN:
                return None
            lo[a] = int(bb_lo[a]) - 1 - mlo
            continue
        if a == 2:
            L[a] = 2                                   # 2-D: one real plane
        else:
            L[a] = pick_length(extent + 2 * MARGIN + 1)
            if L[a] is None:
                return None
        lo[a] = int(bb_lo[a]) - 1 - (L[a] - 1 - extent) // 2
    return L, lo


def box_coefficients(h, gdim):
    """c_a of K_box for lattice spacings h (3-D: h_b h_c / h_a; 2-D: (h1 / h0, h0 / h1, 0))."""
    if gdim == 3:
        return np.array([h[1] * h[2] / h[0], h[0] * h[2] / h[1], h[0] * h[1] / h[2]])
    return np.array([h[1] / h[0], h[0] / h[1], 0.0])


def box_eigenvalues(L, c):
    lam = [c[a] * (2.0 - 2.0 * np.cos(np.pi * np.arange(1, L[a]) / L[a])) for a in range(3)]
    return lam[2][:, None, None] + lam[1][None, :, None] + lam[0][None, None, :]


def box_solve(f, L, c):
    """K_box^-1 f on the (L2 - 1, L1 - 1, L0 - 1) interior by type-I sine transforms in float64."""
    return sf.idstn(sf.dstn(f, type=1) / box_eigenvalues(L, c), type=1)


def box_apply(u, c):
    """K_box u (7-point operator, zero outside the interior)."""
    up = np.pad(u, 1)
    mid = up[1:-1, 1:-1, 1:-1]
    return (c[0] * (2 * mid - up[1:-1, 1:-1, :-2] - up[1:-1, 1:-1, 2:])
            + c[1] * (2 * mid - up[1:-1, :-2, 1:-1] - up[1:-1, 2:, 1:-1])
            + c[2] * (2 * mid - up[:-2, 1:-1, 1:-1] - up[2:, 1:-1, 1:-1]))


def box_matrix(L, c):
    """K_box as a sparse matrix (Kronecker sums), rows in [z, y, x] order: the independent route of the CPU tests."""
    def T(m):
        return sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    m = [l - 1 for l in L]
    I = [sp.identity(k) for k in m]
    return (c[0] * sp.kron(I[2], sp.kron(I[1], T(m[0]))) + c[1] * sp.kron(I[2], sp.kron(T(m[1]), I[0]))
            + c[2] * sp.kron(T(m[2]), sp.kron(I[1], I[0]))).tocsr()


def box_index(active_ijk, L, lo):
    """(z, y, x) index arrays of the active points inside the interior; every point must lie inside."""
    q = np.asarray(active_ijk, dtype=np.int64).reshape(-1, 3) - np.asarray(lo, dtype=np.int64) - 1
    m = np.asarray(L, dtype=np.int64) - 1
    if not np.all((q >= 0) & (q < m)):
        raise ValueError("an active lattice point lies outside the interior of the box")
    return q[:, 2], q[:, 1], q[:, 0]


def scatter_u(p_u, active_ijk, L, lo):
    f = np.zeros((L[2] - 1, L[1] - 1, L[0] - 1))
    f[box_index(active_ijk, L, lo)] = p_u
    return f


def apply_minv_u(p_u, active_ijk, L, lo, h, weights=None, gdim=3, scalings=np.float64, full=False):
    """R K_box^-1 R^T p_u for lattice spacings h (already halved for P2); `weights` = |diag A| of the u rows gives the
    weighted form S^-1 K_box^-1 S^-1, S^2 = |diag A| / kd, kd = 2 (c0 + c1 + c2) (strong Dirichlet, `k_dscale_weighted`;
    rows with a zero diagonal are dropped).  `scalings`: number type of the two S^-1 multiplications around the
    float64 transforms (numpy.longdouble for the second evaluation that measures the reference's own error).
    full=True also returns the un-gathered lattice solution."""
    c = box_coefficients(h, gdim)
    p_u = np.asarray(p_u, dtype=np.float64)
    if weights is None:
        rhs, sinv = p_u, None
    else:
        D = np.abs(np.asarray(weights, dtype=np.float64)).astype(scalings)
        kd = scalings(2.0) * (scalings(c[0]) + scalings(c[1]) + scalings(c[2]))
        sinv = np.where(D > 0, np.sqrt(kd / np.where(D > 0, D, 1)), scalings(0.0))
        rhs = (sinv * p_u.astype(scalings)).astype(np.float64)
    u = box_solve(scatter_u(rhs, active_ijk, L, lo), L, c)
    x = u[box_index(active_ijk, L, lo)]
    if sinv is not None:
        x = (sinv * x.astype(scalings)).astype(np.float64 if scalings is np.float64 else scalings)
    return (x, u) if full else x


def vertex_blocks(A, dof, nvert):
    """Active rows of every vertex of a block-major system (full index = block * nvert + vertex), in block order:
    list of index arrays, one per vertex that carries an active DoF."""
    dof = np.asarray(dof, dtype=np.int64)
    vert = dof % nvert
    order = np.lexsort((dof // nvert, vert))
    cuts = np.flatnonzero(np.diff(vert[order])) + 1
    return np.split(order, cuts)


def apply_block_jacobi(p, A, dof, nvert):
    """B_v^-1 p_v per vertex, B_v the diagonal block of A over the active DoFs of vertex v (numpy.linalg.inv).
    Returns (x, rows per vertex, cond_inf(B_v) per vertex)."""
    A = sp.csr_matrix(A)
    x = np.zeros_like(p)
    groups = vertex_blocks(A, dof, nvert)
    conds = np.empty(len(groups))
    for g, rows in enumerate(groups):
        B = A[rows][:, rows].toarray()
        Binv = np.linalg.inv(B)
        x[rows] = Binv @ p[rows]
        conds[g] = np.abs(B).sum(axis=1).max() * np.abs(Binv).sum(axis=1).max()
    return x, groups, conds


def apply_minv(p, diag, is_u, active_ijk=None, L=None, lo=None, h=None, weights=None, gdim=3):
    """M^-1 p for a whole vector in solver order: u rows (`is_u`) through the lattice (in the order of `active_ijk`),
    every other row p_i / A_ii.  Without a lattice (L is None) every row is Jacobi."""
    p = np.asarray(p, dtype=np.float64)
    x = p / diag
    if L is not None:
        x[is_u] = apply_minv_u(p[is_u], active_ijk, L, lo, h, weights=weights, gdim=gdim)
    return x
