"""The structured stencil SpMVs on the branches only large systems reach, against the float64 CSR of the same system.

Structured systems (Kuhn boxes) never store their interior rows: P2 applies them from eight class stencils over runs of
one x line (`k_spmv_p2s`, phx_spmv_p2s.inc.hip), P1 from the 7-point lattice row in the stencil blocks of `k_spmv_sell`
(phx_solve.hip).  The size-dependent branches of those kernels -- several 124-row trips per P2 run, the grid-stride loop
over more than 16 384 runs, the per-plane eighth map of the P1 stencil blocks -- are reached here on cheap anisotropic
boxes, and every case first ASSERTS that it reaches its branch.

Reference: `PhiFEMSolver.export_csr()`, the generic re-assembly with every row stored (pinned to the numpy oracle by
test_p2_matrix_and_rhs_vs_oracle / test_matrix_and_rhs_vs_oracle).  Products are compared ROW BY ROW:

    |y_i - (A x)_i| <= c eps (|A| |x|)_i,   c = 4 k,  k = the longest row of the CSR (125 stencil terms, ~165 cut P2 rows),

because the kernel's FMA chain and the float64 product are each recursive sums of at most k products (error at most
gamma_k ~ k eps / 2 of (|A| |x|)_i each), and the stencil tables / stored values and the re-assembled CSR differ in the
last bits of each entry (summation order of the element contributions): together below 2 k eps, doubled for margin.
A single wrong row, or a wrong coefficient in one trip of one run, exceeds this by many orders of magnitude."""
import math
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TRIP = 124                    # rows per trip of a k_spmv_p2s wavefront
P2S_WAVES = 4096 * 4          # grid cap of k_spmv_p2s (blocks of four waves): more runs than this -> grid stride
PLANE_ROWS_DEFAULT = 32768    # PHX_OPT_STENCIL_PLANE_ROWS default (phx_common.h)


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


# ---- shapes -----------------------------------------------------------------------------------------------------------
# 1: a bar long in x whose two end planes are slanted in y with different slopes: the c0i runs of neighbouring x lines
#    differ in length by about one row and start at either parity, lengths 240 .. 253 (two and three trips).
# 2: a short, wide box split in x into two slabs: every interior line carries two runs, 18 018 runs in all.
# 4: P1, an elliptic cylinder through the whole z extent of a 400 x 256 x 8 box: ~8e4 C0 rows per plane.
SHAPES = {
    "multi_trip": dict(degree=2, lo=[0.0, -0.5, -0.3], hi=[3.0, 0.5, 0.3], n=[150, 32, 10],
                       phi=lambda x: np.maximum.reduce([np.abs(x[:, 1]) - 0.42, np.abs(x[:, 2]) - 0.22,
                                                        0.213 + 0.07 * x[:, 1] - x[:, 0],
                                                        x[:, 0] - (2.787 + 0.27 * x[:, 1])])),
    "grid_stride": dict(degree=2, lo=[0.0, -1.0, -1.0], hi=[1.2, 1.0, 1.0], n=[32, 60, 56],
                        phi=lambda x: np.maximum.reduce([
                            np.abs(x[:, 1]) - 0.913, np.abs(x[:, 2]) - 0.913,
                            np.minimum(np.maximum(0.113 - x[:, 0], x[:, 0] - 0.547),
                                       np.maximum(0.653 - x[:, 0], x[:, 0] - 1.087))])),
    "plane_map": dict(degree=1, lo=[-2.0, -1.28, -0.2], hi=[2.0, 1.28, 0.2], n=[400, 256, 8],
                      phi=lambda x: (x[:, 0] / 1.83) ** 2 + (x[:, 1] / 1.17) ** 2 - 1.0),
}


def build(P, name, kphi=None, deterministic=False, export=False):
    """Tagged box of SHAPES[name] and its assembled structured system."""
    from phifem_amd import _lib as L
    from phifem_amd.mesh_scripts import NodalFunction
    sh = SHAPES[name]
    mesh = P.create_box(sh["lo"], sh["hi"], sh["n"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, _, meas, _ = P.compute_tags_measures(mesh, NodalFunction(sh["phi"](mesh.x)), 1, box_mode=True,
                                                   single_layer_cut=True)
    if sh["degree"] == 2:
        kphi = kphi or 2
        pts = mesh.p2_dof_points()
        phi = sh["phi"](pts) if kphi == 2 else sh["phi"](mesh.x)
        s = P.PhiFEMSolver(mesh, degree=2, levelset_degree=kphi, deterministic=deterministic)
    else:
        pts = mesh.x
        phi = sh["phi"](pts)
        s = P.PhiFEMSolver(mesh, deterministic=deterministic)
    uex = np.prod(np.sin(pts + 0.3), axis=1)
    L.check(L.lib.phx_set_option(mesh._h, L.OPT_EXPORT_CSR, int(export)))
    try:
        info = s.assemble(phi, 3.0 * uex, uex)
    finally:
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_EXPORT_CSR, 0))
    assert info["stencil_rows"] > 0 and info["stencil_runs"] > 0, info
    return mesh, meas, s, info


def csr(s):
    rowptr, col, val, rhs, dof = s.export_csr()
    n = rowptr.size - 1
    return sp.csr_matrix((val, col, rowptr), shape=(n, n)), dof


def check_rows(y, M, x, what):
    """Row-wise bound of the module docstring; returns the largest error in units of eps (|A| |x|)_i."""
    k = int(np.diff(M.indptr).max())
    ref = M @ x
    mag = abs(M) @ np.abs(x)
    assert np.all(mag > 0.0)
    ratio = np.abs(y - ref) / (EPS * mag)
    bad = np.flatnonzero(ratio > 4 * k)
    assert bad.size == 0, (f"{what}: {bad.size} rows off (k = {k}), first {bad[:8].tolist()}: ratio {ratio[bad[:8]]}, "
                           f"y {y[bad[:4]]} ref {ref[bad[:4]]}")
    return float(ratio.max()), k


def describe(name, info, M, extra=""):
    print(f"[{name}] n={SHAPES[name]['n']} rows={info['n_active']} nnz={M.nnz} stencil_rows={info['stencil_rows']} "
          f"runs={info['stencil_runs']} {extra}")


# ---- host copy of the structured P2 lattice classification -----------------------------------------------------------
def p2_c0i_lattice(mesh, meas, dof, name):
    """C0 / c0i flags of the fine lattice (spacing h / 2) rebuilt on the host after k_p2s_mark_bad_cells / _facets /
    _ents, k_p2s_lat_c0 and three k_p2s_erode passes: returns c0i as a [z, y, x] boolean array."""
    sh = SHAPES[name]
    lo, n = np.asarray(sh["lo"], float), np.asarray(sh["n"])
    h = (np.asarray(sh["hi"], float) - lo) / n
    F = 2 * n + 1
    nv, edges, cells, c2e = mesh.nv, mesh.edges.astype(np.int64), mesh.cells.astype(np.int64), mesh.c2e.astype(np.int64)
    nent = nv + edges.shape[0]
    bad = np.zeros(nent, dtype=bool)

    def mark(cs):
        cs = np.unique(np.asarray(cs, dtype=np.int64))
        bad[cells[cs].ravel()] = True
        bad[nv + c2e[cs].ravel()] = True

    ct = mesh.cell_tag_values() & 0x7f
    ft = mesh.facet_tag_values() & 0x7f
    f2c = mesh.f2c.astype(np.int64)
    mark(np.flatnonzero(ct != 1))                                         # every DoF of a cell not inside
    ghost = np.flatnonzero(((ft == 2) | (ft == 3)) & (f2c[:, 1] >= 0))    # SelGhostFacet
    mark(f2c[ghost].ravel())
    mark(meas(100)[0::2])                                                 # cells of the one-sided boundary term
    act = np.zeros(nent, dtype=bool)
    act[dof[dof < nent]] = True
    q = np.rint((mesh.p2_dof_points() - lo) / (0.5 * h)).astype(np.int64)
    ok = act & ~bad & np.all((q >= 1) & (q <= F - 2), axis=1)
    lat = np.zeros(F[::-1], dtype=bool)
    lat[q[ok, 2], q[ok, 1], q[ok, 0]] = True
    for ax in (2, 1, 0):                     # x, y, z: AND over p - 2 .. p + 2, zero within 2 of the lattice border
        Lx = lat.shape[ax]
        out = np.ones_like(lat)
        for k in range(-2, 3):
            out[_sl(ax, 2, Lx - 2)] &= lat[_sl(ax, 2 + k, Lx - 2 + k)]
        out[_sl(ax, 0, 2)] = False
        out[_sl(ax, Lx - 2, Lx)] = False
        lat = out
    return lat


def _sl(ax, a, b):
    s = [slice(None)] * 3
    s[ax] = slice(a, b)
    return tuple(s)


def runs_of(lat):
    """(start x index, length) of every maximal run of c0i points along the fine x lines (k_p2s_run_flags)."""
    lines = lat.reshape(-1, lat.shape[2]).astype(np.int8)
    d = np.diff(np.pad(lines, ((0, 0), (1, 1))), axis=1)
    _, start = np.nonzero(d == 1)
    _, end = np.nonzero(d == -1)
    return start, end - start


def p2_reach(mesh, meas, s, info, name):
    rhs, dof = s.export_rhs_dof()
    lat = p2_c0i_lattice(mesh, meas, dof, name)
    start, length = runs_of(lat)
    assert int(lat.sum()) == info["stencil_rows"], (int(lat.sum()), info["stencil_rows"])
    assert start.size == info["stencil_runs"], (start.size, info["stencil_runs"])
    return start, length


# ---- 1. P2: runs of several trips --------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("kphi", [1, 2])
def test_p2_runs_of_several_trips(P, kphi, deterministic):
    """k_spmv_p2s walks a run in trips of 124 rows; lanes 62 / 63 only feed entries 124 .. 127 of a trip to their
    neighbours.  The runs here are 240 .. 253 rows long: the host rebuild of the lattice must find the library's c0i
    count and run count, runs of three trips, lengths whose residue mod 124 puts the last rows of a trip on every lane
    pair around the trip boundary (0 .. 3 and 121 .. 123), and runs starting at both x parities (the class of a
    lane's first row)."""
    mesh, meas, s, info = build(P, "multi_trip", kphi, deterministic)
    start, length = p2_reach(mesh, meas, s, info, "multi_trip")
    long = length > TRIP
    residues = set((length[long] % TRIP).tolist())
    parities = set((start[long] & 1).tolist())
    assert (length > 2 * TRIP).any(), length.max()
    assert {0, 1, 2, 3, 121, 122, 123} <= residues, sorted(residues)
    assert parities == {0, 1}
    x = np.random.default_rng(11).standard_normal(info["n_active"])
    y = s.spmv(x)
    M, dof = csr(s)
    worst, k = check_rows(y, M, x, "multi_trip")
    describe("multi_trip", info, M, f"kphi={kphi} det={deterministic} run lengths {length.min()}..{length.max()} "
             f"(> {2 * TRIP}: {(length > 2 * TRIP).sum()}) residues {sorted(residues)} parities {sorted(parities)} "
             f"worst row {worst:.1f} eps (bound {4 * k})")


# ---- 2. P2: more runs than waves ---------------------------------------------------------------------------------------
def test_p2_grid_stride_over_runs(P):
    """Beyond 16 384 runs the grid of k_spmv_p2s is capped and a wavefront walks several runs, carrying its
    dot-product shares across them (checked by test_spmv_phase_dot_products)."""
    mesh, meas, s, info = build(P, "grid_stride")
    start, length = p2_reach(mesh, meas, s, info, "grid_stride")
    assert info["stencil_runs"] > P2S_WAVES, info["stencil_runs"]
    x = np.random.default_rng(12).standard_normal(info["n_active"])
    y = s.spmv(x)
    M, dof = csr(s)
    worst, k = check_rows(y, M, x, "grid_stride")
    describe("grid_stride", info, M, f"(> {P2S_WAVES} waves) run lengths {length.min()}..{length.max()} "
             f"worst row {worst:.1f} eps (bound {4 * k})")


# ---- 4. P1: the per-plane eighth map at its default threshold ----------------------------------------------------------
def test_p1_plane_map_at_the_default_threshold(P):
    """Planes of at least PHX_OPT_STENCIL_PLANE_ROWS = 32 768 C0 rows switch the P1 stencil blocks to the per-plane
    eighth map (k_plane_starts, k_stmap_build).  It is on here at the default option: the SpMV stream of the system
    carries 64 st_chunk bytes of map more than with the option at 0, st_chunk = ceil(nq / 64) / 128 + 2 nzp + 2 for
    the nq C0 rows over nzp planes, stencil_rows <= nq <= n_active_u.  The rows match the CSR, and the product is
    bit-identical with the map off on every row whose matrix row is: placement changes no arithmetic.  (The P1
    assembly sums the ghost penalty with f64 atomics in arrival order, deterministic or not, so two assemblies may
    differ in the last bits of some rows; both systems keep their own CSR copy, PHX_OPT_EXPORT_CSR, to tell those
    rows apart, and only stored rows -- never more than n_active - stencil_rows -- may be among them.)"""
    from phifem_amd import _lib as L
    mesh, meas, s, info = build(P, "plane_map", export=True)
    try:
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_STENCIL_PLANE_ROWS, 0))
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_EXPORT_CSR, 1))
        s0 = P.PhiFEMSolver(mesh)
        info0 = s0.assemble(*s._keep)
    finally:
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_STENCIL_PLANE_ROWS, PLANE_ROWS_DEFAULT))
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_EXPORT_CSR, 0))
    assert info["has_csr"] == 1 and info0["has_csr"] == 1
    assert info0["stencil_rows"] == info["stencil_rows"] and info0["n_active"] == info["n_active"]
    nzp = SHAPES["plane_map"]["n"][2] + 1
    extra = info["spmv_matrix_bytes"] - info0["spmv_matrix_bytes"]
    assert extra > 0 and extra % 64 == 0, extra
    chunk = extra // 64
    lo_nw, hi_nw = -(-info["stencil_rows"] // 64), -(-info["n_active_u"] // 64)
    assert lo_nw // 128 + 2 * nzp + 2 <= chunk <= hi_nw // 128 + 2 * nzp + 2, (chunk, lo_nw, hi_nw)
    x = np.random.default_rng(14).standard_normal(info["n_active"])
    y = s.spmv(x)
    y0 = s0.spmv(x)
    M, dof = csr(s)
    M0, dof0 = csr(s0)
    assert np.array_equal(dof, dof0) and np.array_equal(M.indptr, M0.indptr) and np.array_equal(M.indices, M0.indices)
    worst, k = check_rows(y, M, x, "plane_map")
    check_rows(y0, M0, x, "plane_map, map off")
    differs = np.add.reduceat((M.data != M0.data).astype(np.int64), M.indptr[:-1]) > 0
    mism = y != y0
    assert not (mism & ~differs).any(), np.flatnonzero(mism & ~differs)[:8]
    # ... and only stored rows may differ: never more rows than the system stores
    assert mism.sum() <= info["n_active"] - info["stencil_rows"], (mism.sum(), info)
    describe("plane_map", info, M, f"st_chunk={chunk} (map {extra} B) worst row {worst:.1f} eps (bound {4 * k}); "
             f"{differs.sum()} rows differ in their matrix bits, {mism.sum()} in y")


# ---- 3. fused dot products of the SpMV phases --------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("name", ["multi_trip", "grid_stride", "plane_map"])
def test_spmv_phase_dot_products(P, name, deterministic):
    """KR_SPMV_P (v = A C phat, (rhat, v) -> R_RV) and KR_SPMV_S (t = A C shat, (s, t) -> R_TS, (t, t) -> R_TT) of the
    phase API on one rank, mode 1 (the phases fold their dot products into R), against float64: the products row by
    row in solver order (phx_system_get_perm), C = 1 on u columns and 1 / diag on p columns (k_cscale); the dot
    products against an exact sum (math.fsum) of the reference terms, to sum_i |a_i| |b_i - b_ref_i| plus gamma_n of
    sum |a b| for any summation order of n terms.  The stencil kernels run with DOTS = 1 and 2 here (phx_spmv runs
    them with DOTS = 0)."""
    import torch
    from phifem_amd.dist_solver import (HipBackend, KR_SPMV_P, KR_SPMV_S, R_OFF, R_RV, R_TS, R_TT, SCAL_DOUBLES)
    mesh, meas, s, info = build(P, name, deterministic=deterministic)
    n, nu = info["n_active"], info["n_active_u"]
    dev = torch.device("cuda", mesh.device)
    b = HipBackend(s, dev)
    perm = b.perm.cpu().numpy()
    g = torch.Generator(device="cpu").manual_seed(21)
    work0 = torch.randn(10 * n, generator=g, dtype=torch.float64)
    work = work0.to(dev)
    scal = torch.zeros(SCAL_DOUBLES, dtype=torch.float64, device=dev)
    own = torch.ones(n, dtype=torch.uint8, device=dev)
    b.attach(work, scal, own)
    hat = b.precond_active()            # phat / shat are vectors of their own (8 n, 9 n), else p (2 n) / s (4 n)
    M, dof = csr(s)
    assert np.array_equal(dof, s.export_rhs_dof()[1])
    As = M[perm][:, perm].tocsr()
    diag = M.diagonal()[perm]
    cs = np.where(perm < nu, 1.0, 1.0 / diag)
    w0 = work0.numpy()
    vec = {k: w0[i * n:(i + 1) * n] for i, k in enumerate(("r", "rhat", "p", "v", "s", "t", "y", "b", "phat", "shat"))}
    phat, shat = (vec["phat"], vec["shat"]) if hat else (vec["p"], vec["s"])

    def run():
        torch.cuda.synchronize(dev)
        s._apply_options()
        b.phase(KR_SPMV_P)
        b.phase(KR_SPMV_S)
        mesh.synchronize()
        w = work.cpu().numpy()
        sc = scal.cpu().numpy()
        out = (w[3 * n:4 * n].copy(), w[5 * n:6 * n].copy(), sc[R_OFF + R_RV], sc[R_OFF + R_TS], sc[R_OFF + R_TT])
        work.copy_(work0.to(dev))
        scal.zero_()
        torch.cuda.synchronize(dev)
        return out

    v, t, rv, ts, tt = run()
    wv, kv = check_rows(v, As, cs * phat, f"{name} v")
    wt, kt = check_rows(t, As, cs * shat, f"{name} t")
    vref, tref = As @ (cs * phat), As @ (cs * shat)
    err_v = 4 * kv * EPS * (abs(As) @ np.abs(cs * phat))      # the row bounds just checked
    err_t = 4 * kt * EPS * (abs(As) @ np.abs(cs * shat))

    def dot_ok(got, ref_terms, tol, what):
        ref = math.fsum(ref_terms.tolist())
        assert abs(got - ref) <= tol, f"{name} {what}: {got!r} vs {ref!r} (tol {tol:.3e})"
        return abs(got - ref) / tol

    # |computed - exact| <= sum |a| |b - b_ref| (the row bounds) + n eps sum |a b| (any order of n additions)
    rhat, sv = vec["rhat"], vec["s"]
    q = [dot_ok(rv, rhat * vref, float(np.abs(rhat) @ err_v) + n * EPS * float(np.abs(rhat) @ np.abs(v)), "(rhat, v)"),
         dot_ok(ts, sv * tref, float(np.abs(sv) @ err_t) + n * EPS * float(np.abs(sv) @ np.abs(t)), "(s, t)"),
         dot_ok(tt, tref * tref, float((np.abs(t) + np.abs(tref)) @ err_t) + n * EPS * float(t @ t), "(t, t)")]
    if deterministic:
        again = run()
        assert all(np.array_equal(a1, a2) for a1, a2 in zip(again, (v, t, rv, ts, tt))), "deterministic phases differ"
    describe(name, info, M, f"det={deterministic} hat={hat} worst rows v {wv:.1f} / t {wt:.1f} eps; dot errors "
             f"{', '.join(f'{x:.2e}' for x in q)} of their bounds")


# ---- 5. placement options change no arithmetic -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["multi_trip", "grid_stride", "plane_map"])
def test_xcd_group_placement_is_bit_identical(P, name):
    """PHX_OPT_SPMV_XCD_GROUP only permutes which block takes which slice group (default 0): phx_spmv must give the
    same bits for 0, 1, 3 and 8, and back at 0 again."""
    from phifem_amd import _lib as L
    mesh, meas, s, info = build(P, name)
    x = np.random.default_rng(15).standard_normal(info["n_active"])
    ys = {}
    try:
        for gsz in (0, 1, 3, 8):
            L.check(L.lib.phx_set_option(mesh._h, L.OPT_SPMV_XCD_GROUP, gsz))
            ys[gsz] = s.spmv(x)
    finally:
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_SPMV_XCD_GROUP, 0))
    ys["0 again"] = s.spmv(x)
    for k, y in ys.items():
        assert np.array_equal(y, ys[0]), (name, k, np.flatnonzero(y != ys[0])[:8])
    print(f"[{name}] rows={info['n_active']} runs={info['stencil_runs']}: XCD groups {list(ys)} bit-identical")
