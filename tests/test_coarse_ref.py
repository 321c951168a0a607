"""CPU checks of tests/coarse_ref.py, the numpy specification the device's coarse-space correction is compared with
(tests/test_hip_coarse_apply.py): on the weak-Dirichlet elasticity systems of tests/elasticity_wd_ref.py, 2-D n = 12 with
H = 5 h (12 is no multiple of 5: the last coarse cell is cut short) and 3-D n = 6 with H = 3 h (the largest H with
n >= 2 H, the library's own condition; 3 divides 6: the last fine index sits on the last node)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import coarse_ref as CR
import elasticity_wd_ref as R

CASES = [(2, 12), (3, 6)]


def ratio_of(n):
    return min(5, n // 2)


@functools.lru_cache(maxsize=None)
def system(d, n):
    """(x, active CSR, dof, nv, ratio, R, D) of the specification's system."""
    topo, x, ct, ft, ds, phi = R.box_problem(d, n)
    rng = np.random.default_rng(5)
    f, uD = np.sin(x @ rng.standard_normal((d, d))) + 0.3, np.cos(x @ rng.standard_normal((d, d)))
    A, b, act = R.assemble_elasticity_wd(topo, x, ct, ft, ds, phi, f, uD)
    dof = np.flatnonzero(act)
    Aa = A[dof][:, dof].tocsr()
    ratio = ratio_of(n)
    Rm = CR.restriction(x, dof, topo.nv, None, [n] * d, ratio, d)
    return x, Aa, dof, topo.nv, ratio, Rm, CR.scaling(Aa, dof, topo.nv, "elwd")


def same_matrix(Ra, Rb):
    assert Ra.shape == Rb.shape
    assert np.array_equal(Ra.indptr, Rb.indptr) and np.array_equal(Ra.indices, Rb.indices)
    assert np.abs(Ra.data - Rb.data).max() <= 4 * CR.EPS


@pytest.mark.parametrize("d,n", CASES)
def test_hat_formula_equals_axis_form(d, n):
    x, Aa, dof, nv, ratio, Rm, D = system(d, n)
    nodes = CR.used_nodes(x, dof, nv, [n] * d, ratio, d)
    for node_of in (None, nodes):
        same_matrix(CR.restriction(x, dof, nv, node_of, [n] * d, ratio, d, form="hat"),
                    CR.restriction(x, dof, nv, node_of, [n] * d, ratio, d, form="axis"))
    assert Rm.shape == (dof.size, nodes.size) and nodes.size > 0
    m, M = CR.coarse_dims([n] * d, ratio, d)
    assert m[:d] == [-(-n // ratio) + 1] * d and (n % ratio != 0) == (d == 2)


@pytest.mark.parametrize("layout,ncubes,ratio", [("elwd", (12, 10, 15), 5), ("interface", (11, 11, 11), 5),
                                                 ("p2", (10, 7, 6), 5), ("elwd", (12, 12, 12), 6)])
def test_hat_formula_equals_axis_form_on_full_lattices(layout, ncubes, ratio):
    """Every lattice point of an anisotropic box active, in every block: cut-short last cells of three different
    lengths, the h/2 lattice of P2, and a ratio that divides n (the clamp of cc_axis)."""
    d, steps = 3, CR.steps_per_cube(layout)
    ax = [np.linspace(CR.LO, CR.HI, ncubes[a] * steps + 1) for a in range(d)]
    pts = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, d)
    nent = pts.shape[0]
    nblk = CR.blocks_with_hats(layout, d) + 1                 # one more block that carries nothing
    dof = np.arange(nblk * nent)
    bcv = np.flatnonzero(np.abs(pts).max(axis=1) == CR.HI) if layout == "interface" else None
    Rh = CR.restriction(pts, dof, nent, None, ncubes, ratio, d, layout, bcv, form="hat")
    Ra = CR.restriction(pts, dof, nent, None, ncubes, ratio, d, layout, bcv, form="axis")
    same_matrix(Rh, Ra)
    ok = CR.eligible(dof, nent, d, layout, bcv)
    rs = np.asarray(Rh.sum(axis=1)).ravel()
    assert np.abs(rs[ok] - 1.0).max() <= 8 * CR.EPS and np.all(rs[~ok] == 0.0)
    m, M = CR.coarse_dims(ncubes, ratio, d)
    if layout != "interface":                                 # every node of every block is used
        assert Rh.shape[1] == CR.blocks_with_hats(layout, d) * M
    else:
        assert not ok[:d * nent][np.isin(dof[:d * nent] % nent, bcv)].any() and ok[d * nent:2 * d * nent].all()


@pytest.mark.parametrize("d,n", CASES)
def test_partition_of_unity(d, n):
    x, Aa, dof, nv, ratio, Rm, D = system(d, n)
    ok = CR.eligible(dof, nv, d, "elwd")
    assert ok.any() and (~ok).any() and np.array_equal(ok, dof // nv < d)
    rs = np.asarray(Rm.sum(axis=1)).ravel()
    assert np.abs(rs[ok] - 1.0).max() <= 8 * CR.EPS
    assert np.all(rs[~ok] == 0.0) and Rm[~ok].nnz == 0
    assert Rm.data.min() > 0.0 and np.all(np.asarray(Rm.sum(axis=0)).ravel() > 0.0)


@pytest.mark.parametrize("d,n", CASES)
def test_galerkin_projection_identity(d, n):
    """R^T A (R zc) = gc: ties apply_ref to A; and x = D R zc."""
    x, Aa, dof, nv, ratio, Rm, D = system(d, n)
    v = np.random.default_rng(11).standard_normal(dof.size)
    gc, zc, xr = CR.apply_ref(Aa, Rm, D, v)
    back = CR.rt_dot(Rm, Aa @ np.asarray(CR.r_dot(Rm, zc), dtype=np.float64))
    rel = float(np.abs(back - gc).max() / np.abs(gc).max())
    print(f"d={d} n={n}: {Rm.shape[1]} coarse DoFs, cond(Ac) {np.linalg.cond(CR.galerkin(Aa, Rm)):.1e}, "
          f"|R^T A R zc - gc| / |gc| = {rel:.2e}")
    assert rel <= 1e-10
    assert np.abs(np.asarray(gc, dtype=np.float64) - Rm.T @ v).max() <= 1e-13 * np.abs(gc).max()
    assert np.abs(np.asarray(xr, dtype=np.float64) - D * (Rm @ zc)).max() <= 1e-13 * float(np.abs(xr).max())
    assert np.all(xr[dof // nv >= d] == 0.0)


@pytest.mark.parametrize("d,n", CASES)
def test_symmetric_when_A_is(d, n):
    """R Ac^-1 R^T is symmetric for a symmetric A: (the boundary term of the weak-Dirichlet form is not, so the
    symmetric part of the system matrix stands in)."""
    x, Aa, dof, nv, ratio, Rm, D = system(d, n)
    As = ((Aa + Aa.T) * 0.5).tocsr()
    assert abs(As - As.T).max() == 0.0
    Rd = Rm.toarray()
    B = Rd @ np.linalg.solve(CR.galerkin(As, Rm), Rd.T)       # R Ac^-1 R^T, dense (nc = 22 and 81)
    assert np.abs(B - B.T).max() <= 1e-10 * np.abs(B).max()
    # ... and it is what apply_ref applies
    v = np.random.default_rng(3).standard_normal(dof.size)
    x = np.asarray(CR.apply_ref(As, Rm, np.ones(dof.size), v)[2], dtype=np.float64)
    assert np.abs(x - B @ v).max() <= 1e-10 * np.abs(x).max()
