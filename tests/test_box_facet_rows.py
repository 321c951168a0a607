"""Ghost penalty as row gathers on Kuhn boxes (k_assemble_facet_rows_box, PHX_OPT_BOX_FACET_ROWS = 1, the default)
against the facet kernel that scatters with f64 atomics (PHX_OPT_BOX_FACET_ROWS = 0) on the same mesh and tags.

The gather evaluates jump coefficients and weights in closed form per facet type, the scatter evaluates two simplices
per facet, and the two add in different orders: the stored rows, read as column -> value maps through
phx_system_export_sell, must agree to 1e-12 of the largest entry (the tolerance tests/test_box_slots.py uses for a
different summation order).  The SELL fill drops exact zeros, and where the closed form has an exact zero the generic
geometry may leave a rounding residue: an entry only one path stores must itself be below that bound, so neither
sell_nnz nor the slice pointers are compared.  The structural counts, the active numbering, the
product with a random vector and the solution must agree; an assembly that met a column outside the code table would
fail (overflow flag), so two successful assemblies are also the check that the flag stayed clear."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def problem(P, lo, hi, n, centre, semi):
    from phifem_amd.mesh_scripts import NodalFunction
    mesh = P.create_box(list(lo), list(hi), list(n))
    x = mesh.x
    phi = (((x - np.asarray(centre)) / np.asarray(semi)) ** 2).sum(axis=1) - 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=True, single_layer_cut=True)
    uex = np.prod(np.sin(x), axis=1)
    return mesh, phi, len(n) * uex, uex


def assemble(P, mesh, phi, f, uex, flag):
    """solver, info, active numbering and the stored entries (active row, active column, value), sorted by (row, column)"""
    from phifem_amd import _lib as L
    L.check(L.lib.phx_set_option(mesh._h, L.OPT_BOX_FACET_ROWS, flag))
    try:
        s = P.PhiFEMSolver(mesh)
        info = s.assemble(phi, f, uex)            # raises when the overflow flag is set
    finally:
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_BOX_FACET_ROWS, 1))
    nsl, ne = info["n_slices"], info["sell_padded_nnz"]
    slice_ptr = np.zeros(nsl + 1, np.int64)
    col = np.zeros(max(ne, 1), np.int32)
    val = np.zeros(max(ne, 1), np.float64)
    rows = np.zeros(max(16 * nsl, 1), np.int32)
    L.check(L.lib.phx_system_export_sell(s._sys, L.ptr(slice_ptr)[0], L.ptr(col)[0], L.ptr(val)[0], L.ptr(rows)[0]))
    n = info["n_active"]
    perm = np.zeros(n, np.int32)
    du = np.zeros(mesh.nv, np.int32)
    dp = np.zeros(mesh.nv, np.int32)
    L.check(L.lib.phx_system_get_perm(s._sys, L.ptr(perm)[0], L.ptr(du)[0], L.ptr(dp)[0], 0))
    col, val, rows = col[:ne], val[:ne], rows[:16 * nsl]
    # entry e of slice s sits in lane (e - slice_ptr[s]) % 16
    sl = np.repeat(np.arange(nsl), np.diff(slice_ptr))
    lane = (np.arange(ne) - slice_ptr[sl]) % 16
    pos = rows[16 * sl + lane]
    keep = (pos >= 0) & (val != 0.0)
    key = perm[pos[keep]].astype(np.int64) * n + perm[col[keep]]
    order = np.argsort(key)
    key, v = key[order], val[keep][order]
    assert np.all(np.diff(key) > 0)               # one entry per (row, column)
    stored = np.sort(perm[rows[rows >= 0]])
    return s, info, (perm, du, dp), stored, key, v


CASES = [
    # lo, hi, n, centre, semi-axes
    pytest.param([-1.5] * 3, [1.5] * 3, (12, 12, 12), (0.03, -0.02, 0.01), (1.0,) * 3, id="3d-12-generic-band"),
    pytest.param([-1.5, -1.2, -1.8], [1.5, 1.2, 1.8], (10, 12, 9), (0.0, 0.0, 0.0), (1.0, 0.8, 1.2),
                 id="3d-anisotropic-0.3-0.2-0.4"),
    pytest.param([-1.5] * 3, [1.5] * 3, (16, 16, 16), (0.55, 0.0, 0.0), (1.0,) * 3, id="3d-16-band-at-face"),
    pytest.param([-1.5] * 3, [1.5] * 3, (5, 5, 5), (0.0, 0.0, 0.0), (1.2,) * 3, id="3d-5-all-rows-near-faces"),
    pytest.param([-1.5] * 3, [1.5] * 3, (20, 20, 20), (0.03, -0.02, 0.01), (1.0,) * 3, id="3d-20-inexact-spacing"),
    pytest.param([-1.5] * 3, [1.5] * 3, (27, 27, 27), (0.11, 0.07, -0.05), (0.8,) * 3, id="3d-27-inexact-spacing"),
    pytest.param([-1.5] * 2, [1.5] * 2, (40, 40), (0.03, -0.02), (1.0,) * 2, id="2d-40"),
    pytest.param([-1.5] * 2, [1.5] * 2, (64, 64), (0.0, 0.45), (1.0,) * 2, id="2d-64-band-at-face"),
]


@pytest.mark.parametrize("lo,hi,n,centre,semi", CASES)
def test_facet_rows_equal_facet_scatter(P, lo, hi, n, centre, semi):
    mesh, phi, f, uex = problem(P, lo, hi, n, centre, semi)
    sg, ig, ng, rg, kg, vg = assemble(P, mesh, phi, f, uex, 1)
    ss, is_, ns, rs, ks, vs = assemble(P, mesh, phi, f, uex, 0)
    for k in ("n_active", "n_active_u", "stencil_rows", "stencil_runs", "nnz"):
        assert ig[k] == is_[k], (k, ig[k], is_[k])
    for a, b in zip(ng, ns):
        assert np.array_equal(a, b)               # the same active numbering
    assert np.array_equal(rg, rs)                 # the same stored rows
    assert ig["n_active_u"] > 0 and rg.size > 0
    scale = np.abs(vs).max()
    bound = 1e-12 * scale
    both = np.intersect1d(kg, ks, assume_unique=True)
    dg = np.abs(vg[np.searchsorted(kg, both)] - vs[np.searchsorted(ks, both)])
    only_g = np.abs(vg[~np.isin(kg, both, assume_unique=True)])
    only_s = np.abs(vs[~np.isin(ks, both, assume_unique=True)])
    print(f"entries {kg.size} / {ks.size}, common {both.size}; max diff / scale = {dg.max() / scale:.3e}; "
          f"one-sided: {only_g.size} gather (max {only_g.max(initial=0.0) / scale:.3e}), "
          f"{only_s.size} scatter (max {only_s.max(initial=0.0) / scale:.3e})")
    assert both.size > 0.9 * ks.size
    assert dg.max() <= bound
    assert only_g.max(initial=0.0) <= bound and only_s.max(initial=0.0) <= bound
    # the same operator and the same solve
    x = np.random.default_rng(3).standard_normal(ig["n_active"])
    yg, ys = sg.spmv(x), ss.spmv(x)
    print(f"spmv: max diff / (scale |x|) = {np.abs(yg - ys).max() / (scale * np.abs(x).max()):.3e}")
    assert np.abs(yg - ys).max() <= 64 * 1e-12 * scale * np.abs(x).max()
    wg, ws = sg.solve(rtol=1e-10), ss.solve(rtol=1e-10)
    print(f"solve: max diff / max = {np.abs(wg - ws).max() / np.abs(ws).max():.3e}")
    assert np.abs(wg - ws).max() <= 1e-8 * np.abs(ws).max()
