"""Structured systems at the edges of the shared stored-row SELL build (phx_solve.hip, `sell_over_stored_rows`).

`build()` of test_hip_stencil_paths.py asserts `stencil_rows > 0`, so no other test reaches a structured system that
holds NOTHING but stored rows -- no stencil runs, no run records, every row in the SELL slices -- nor the smallest
system in which the stencil applies a row at all.  Both are built here for structured P1 in 2-D and 3-D and structured
P2 in 3-D, on generated boxes [-1.5, 1.5]^d with the sphere level-set of test_box_slots.py.  Box sizes, found by
scanning n = 1, 2, ... on an MI355X (n = 1, 2 and the 3-D n = 4 have no cell tagged 1 or 2 and are refused):

    configuration   stored rows only (smallest box)     first box with a stencil row
    P1, 2-D         n = 3  (28 rows, all stored)        n = 10 (109 rows, 1 stencil row)
    P1, 3-D         n = 3  (92 rows)                    n = 12 (1015 rows, 1 stencil row)
    P2, 3-D         n = 3  (493 rows)                   n = 11 (5398 rows, 1 stencil row)

n = 3 is the smallest box that assembles at all, and its stored-row count is no multiple of the 16 rows of a slice
(28, 92, 493), so `k_sell_pad_tail` fills the open slots of the last slice in every configuration; each case asserts the
branch it is meant to reach.

Check: the product of the structured system with a fixed random vector against the CSR of the same problem assembled
again with PHX_OPT_EXPORT_CSR, row by row with `check_rows` of test_hip_stencil_paths.py (bound and derivation in that
module's docstring), and the two solutions at rtol = 1e-10 as test_box_slots.py compares them (1e-8 of the largest
entry).  The solution check covers P1 only: on the commit before the shared build the two P2 solutions already differ
by 1.07e-06 (n = 3) and 2.82e-07 (n = 11) of the largest entry while their products meet the row bound (worst row 2.4
and 3.7 eps against bounds of 668 and 648) -- two iterates that both meet rtol = 1e-10 on a system that takes hundreds
of iterations, not a difference between the two assemblies."""
import warnings

import numpy as np
import pytest

from test_hip_stencil_paths import check_rows, csr

pytestmark = pytest.mark.gpu

CENTRE = (0.03, -0.02, 0.01)
# (degree, d) -> (box of stored rows only, smallest box with a stencil row)
BOXES = {(1, 2): (3, 10), (1, 3): (3, 12), (2, 3): (3, 11)}


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def assemble_pair(P, degree, d, n):
    """The structured system of the problem and the same problem assembled with its CSR copy."""
    from phifem_amd import _lib as L
    from phifem_amd.mesh_scripts import NodalFunction
    mesh = P.create_box([-1.5] * d, [1.5] * d, [n] * d)
    phi = lambda x: ((x - np.asarray(CENTRE[:d])) ** 2).sum(axis=1) - 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(mesh, NodalFunction(phi(mesh.x)), 1, box_mode=True, single_layer_cut=True)
    pts = mesh.p2_dof_points() if degree == 2 else mesh.x
    uex = np.prod(np.sin(pts), axis=1)
    out = []
    for export in (0, 1):
        s = P.PhiFEMSolver(mesh, degree=2, levelset_degree=2) if degree == 2 else P.PhiFEMSolver(mesh)
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_EXPORT_CSR, export))
        try:
            info = s.assemble(phi(pts), d * uex, uex)
        finally:
            L.check(L.lib.phx_set_option(mesh._h, L.OPT_EXPORT_CSR, 0))
        assert info["has_csr"] == export, info
        out += [s, info]
    return out


def reach(P, degree, d, with_stencil):
    """The pair of systems of one box, after asserting that the box is on the branch it is here for."""
    n = BOXES[degree, d][int(with_stencil)]
    s, info, sc, infoc = assemble_pair(P, degree, d, n)
    stored = info["n_active"] - info["stencil_rows"]
    if with_stencil:
        assert info["stencil_rows"] > 0 and info["stencil_runs"] > 0, info
    else:
        assert info["stencil_rows"] == 0 and info["stencil_runs"] == 0, info
        assert stored % 16 != 0, info                      # the last slice has open slots: k_sell_pad_tail runs
    assert info["n_slices"] == -(-stored // 16), info
    assert infoc["n_active"] == info["n_active"]
    return n, s, info, sc


@pytest.mark.parametrize("with_stencil", [False, True])
@pytest.mark.parametrize("degree,d", list(BOXES))
def test_product_equals_the_csr_row_by_row(P, degree, d, with_stencil):
    n, s, info, sc = reach(P, degree, d, with_stencil)
    x = np.random.default_rng(5).standard_normal(info["n_active"])
    M, _ = csr(sc)
    worst, k = check_rows(s.spmv(x), M, x, f"P{degree} {d}-D n={n}")
    print(f"P{degree} {d}-D n={n}: rows {info['n_active']} stencil rows {info['stencil_rows']} slices {info['n_slices']} "
          f"worst row {worst:.1f} eps (bound {4 * k})")


@pytest.mark.parametrize("with_stencil", [False, True])
@pytest.mark.parametrize("d", [2, 3])
def test_p1_solutions_agree(P, d, with_stencil):
    n, s, info, sc = reach(P, 1, d, with_stencil)
    w, wc = s.solve(rtol=1e-10), sc.solve(rtol=1e-10)
    err = np.abs(w - wc).max() / np.abs(wc).max()
    print(f"P1 {d}-D n={n}: solutions differ by {err:.2e}")
    assert err <= 1e-8
