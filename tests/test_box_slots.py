"""Box slots (structured P1 systems on Kuhn boxes): every stored row addresses its entries directly by lattice offset
code instead of a hashed column table, and the compaction walks the codes in order instead of sorting.  The solver
formats must come out as with the hashed slots (PHX_BOX_SLOTS=0): the same SELL-16 slices, row lists and columns,
the same structural counts, values equal to 1e-12 of the largest entry (f64 atomics add in a different order), and
the columns of every stored row ascending.  An assembly that emitted a column outside the code table would fail
(overflow flag), so a successful assembly is also the check that the flag stayed clear."""
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def problem(P, d, n, centre, radius):
    from phifem_amd.mesh_scripts import NodalFunction
    mesh = P.create_box([-1.5] * d, [1.5] * d, [n] * d)
    x = mesh.x
    phi = ((x - np.asarray(centre[:d])) ** 2).sum(axis=1) - radius ** 2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=True, single_layer_cut=True)
    uex = np.prod(np.sin(x), axis=1)
    return mesh, phi, d * uex, uex


def assemble(P, mesh, phi, f, uex, flag):
    from phifem_amd import _lib as L
    old = os.environ.get("PHX_BOX_SLOTS")
    os.environ["PHX_BOX_SLOTS"] = flag
    try:
        s = P.PhiFEMSolver(mesh)
        info = s.assemble(phi, f, uex)
    finally:
        if old is None:
            del os.environ["PHX_BOX_SLOTS"]
        else:
            os.environ["PHX_BOX_SLOTS"] = old
    nsl, ne = info["n_slices"], info["sell_padded_nnz"]
    slice_ptr = np.zeros(nsl + 1, np.int64)
    col = np.zeros(max(ne, 1), np.int32)
    val = np.zeros(max(ne, 1), np.float64)
    rows = np.zeros(max(16 * nsl, 1), np.int32)
    L.check(L.lib.phx_system_export_sell(s._sys, L.ptr(slice_ptr)[0], L.ptr(col)[0], L.ptr(val)[0], L.ptr(rows)[0]))
    perm = np.zeros(info["n_active"], np.int32)
    L.check(L.lib.phx_system_get_perm(s._sys, L.ptr(perm)[0], None, None, 0))
    return s, info, slice_ptr, col[:ne], val[:ne], rows[:16 * nsl], perm


CASES = [
    (3, 12, (0.03, -0.02, 0.01), 1.0),
    (3, 20, (0.03, -0.02, 0.01), 1.0),
    (3, 27, (0.11, 0.07, -0.05), 0.8),
    (3, 16, (0.55, 0.0, 0.0), 1.0),      # the band reaches the face x = 1.5: one-sided boundary term on cut cells
    (2, 40, (0.03, -0.02, 0.0), 1.0),
    (2, 64, (0.0, 0.45, 0.0), 1.0),      # the band reaches the cells at the face y = 1.5
]


@pytest.mark.parametrize("d,n,centre,radius", CASES)
def test_box_slots_equal_hashed_slots(P, d, n, centre, radius):
    mesh, phi, f, uex = problem(P, d, n, centre, radius)
    sb, ib, spb, cb, vb, rb, pb = assemble(P, mesh, phi, f, uex, "1")
    sh, ih, sph, ch, vh, rh, ph = assemble(P, mesh, phi, f, uex, "0")
    for k in ("n_active", "n_active_u", "nnz", "sell_nnz", "sell_padded_nnz", "n_slices", "stencil_rows",
              "stencil_runs"):
        assert ib[k] == ih[k], (k, ib[k], ih[k])
    assert np.array_equal(pb, ph)
    assert np.array_equal(spb, sph)
    assert np.array_equal(rb, rh)
    assert np.array_equal(cb, ch)
    scale = np.abs(vh).max()
    assert np.abs(vb - vh).max() <= 1e-12 * scale
    # ascending active columns along every stored row (padding: the row's own position with value 0)
    width = np.diff(spb) // 16
    for s in range(ib["n_slices"]):
        for li in range(16):
            if rb[16 * s + li] < 0:
                continue
            o = spb[s] + np.arange(width[s]) * 16 + li
            keep = vb[o] != 0.0
            act = pb[cb[o][keep]]
            assert np.all(np.diff(act) > 0), (s, li, act)
    # the same operator and the same solve
    x = np.random.default_rng(3).standard_normal(ib["n_active"])
    yb, yh = sb.spmv(x), sh.spmv(x)
    assert np.abs(yb - yh).max() <= 1e-12 * scale * np.abs(x).max() * 64
    wb, wh = sb.solve(rtol=1e-10), sh.solve(rtol=1e-10)
    assert np.abs(wb - wh).max() <= 1e-8 * np.abs(wh).max()
