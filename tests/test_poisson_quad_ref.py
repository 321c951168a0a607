"""CPU checks of the quadrilateral weak-Dirichlet restatement (`tests/poisson_quad_ref.py`, the forms of
demo/weak-dirichlet/flower/main.py:112-151 in Q1 x Q1 on rectangles): the minimal rules (3 x 3 Gauss on the cells,
2 points on the facets) are exact, the patch test, the Laplacian terms vanish identically, the u-u rows away from
the cut cells sum to zero, and a non-rectangle is refused.  Tags come from `oracle.tagging`."""
import warnings

import numpy as np
import pytest

import poisson_quad_ref as PQ
from oracle import tagging as T
from oracle.topology import Topology

from test_oracle_flux_quad import quad_mesh


def setup(n, centre=(0.0, 0.0), box_mode=True):
    """Disc of radius 1 around `centre` in [-1.5, 1.5]^2; -> dict of the arguments of PQ.assemble (work mesh)."""
    x, cells = quad_mesh(n)
    topo = Topology("quadrilateral", cells, x.shape[0])
    phi = ((x - np.asarray(centre)) ** 2).sum(axis=1) - 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ct, ft, sub, meas, _, _ = T.compute_tags_measures("quadrilateral", x, topo, T.NodalP1(phi), 1,
                                                          box_mode=box_mode, single_layer_cut=True)
    if box_mode:
        cv = np.zeros(topo.nc, dtype=np.int64)
        cv[ct.indices] = ct.values
        return dict(cells=topo.cells, x=x, c2f=topo.c2f, f2c=topo.f2c, cell_tags=cv, facet_tags=ft.values,
                    ds=meas(100), phi=phi)
    st = sub.topology
    bf = np.flatnonzero(st.f2c[:, 1] < 0)
    c0 = st.f2c[bf, 0]
    lf = np.argmax(st.c2f[c0] == bf[:, None], axis=1)
    return dict(cells=st.cells, x=sub.x, c2f=st.c2f, f2c=st.f2c, cell_tags=ct.values, facet_tags=ft.values,
                ds=np.stack([c0, lf], axis=1), phi=phi[sub.v_map])


def data(x, seed=3):
    rng = np.random.default_rng(seed)
    return np.sin(x @ rng.standard_normal(2)) + 0.3, np.cos(x @ rng.standard_normal(2))


def test_tags_cover_every_form():
    g = setup(12, (0.04, -0.03))
    assert set(np.unique(g["cell_tags"])) == {1, 2, 3}
    assert np.isin(g["facet_tags"], (2, 3)).any() and np.asarray(g["ds"]).size > 0


@pytest.mark.parametrize("box", [True, False])
def test_minimal_rules_are_exact(box):
    """3 x 3 cell / 2-point facet Gauss rules give the system of the 5 x 5 / 4-point rules to round-off."""
    g = setup(12, (0.04, -0.03), box_mode=box)
    f, uD = data(g["x"])
    A3, b3, a3 = PQ.assemble(**g, f=f, uD=uD, gamma=1.3, sigma=0.7, nq=3, nqf=2)
    A5, b5, a5 = PQ.assemble(**g, f=f, uD=uD, gamma=1.3, sigma=0.7, nq=5, nqf=4)
    assert np.array_equal(a3, a5)
    assert abs(A3 - A5).max() <= 1e-13 * abs(A5).max()
    assert np.abs(b3 - b5).max() <= 1e-13 * np.abs(b5).max()
    # and the rules one order lower are NOT exact: the claim is sharp
    A2, b2, _ = PQ.assemble(**g, f=f, uD=uD, gamma=1.3, sigma=0.7, nq=2, nqf=1)
    assert abs(A2 - A5).max() > 1e-6 * abs(A5).max()


@pytest.mark.parametrize("n", [16, 24])
def test_patch_test(n):
    """f = 0, u_D = u linear: Q1 reproduces u exactly and p = 0 (consistency of main.py:112-151)."""
    g = setup(n)
    x = g["x"]
    ulin = x @ np.array([1.0, 2.0]) + 0.5
    A, b, act = PQ.assemble(**g, f=np.zeros(x.shape[0]), uD=ulin)
    w = PQ.solve_direct(A, b, act)
    nv = x.shape[0]
    ua = act[:nv]
    assert ua.sum() > 0 and act[nv:].sum() > 0
    assert np.abs(w[:nv][ua] - ulin[ua]).max() <= 1e-10
    assert np.abs(w[nv:]).max() <= 1e-10
    assert np.all(w[~act] == 0.0)


def test_laplacian_terms_contribute_nothing():
    """main.py:123-128,150: div(grad(.)) of a Q1 function on a rectangle vanishes identically."""
    g = setup(12, (0.04, -0.03))
    f, uD = data(g["x"])
    A0, b0, _ = PQ.assemble(**g, f=f, uD=uD, sigma=2.5)
    A1, b1, _ = PQ.assemble(**g, f=f, uD=uD, sigma=2.5, with_laplacian=True)
    assert np.array_equal(A0.indptr, A1.indptr) and np.array_equal(A0.indices, A1.indices)
    assert np.array_equal(A0.data, A1.data) and np.array_equal(b0, b1)
    # the second derivatives the term is built from are those of the basis: zero at every point
    _, _, d2 = PQ.q1_basis(np.array([0.1, 0.7]), np.array([0.4, 0.9]))
    assert np.all(d2 == 0.0)


def test_uu_rows_away_from_cut_cells_sum_to_zero():
    """Stiffness, the one-sided boundary term and the ghost penalty annihilate constants; only the cut-cell
    penalisation (a mass term) does not."""
    g = setup(16, (0.04, -0.03))
    f, uD = data(g["x"])
    A, b, act = PQ.assemble(**g, f=f, uD=uD)
    nv = g["x"].shape[0]
    cutv = np.unique(g["cells"][g["cell_tags"] == 2])
    interior = np.setdiff1d(np.flatnonzero(act[:nv]), cutv)
    assert interior.size > 20
    Auu = A[:nv, :nv]
    assert np.abs(np.asarray(Auu[interior].sum(axis=1))).max() <= 1e-13 * abs(Auu).max()
    assert np.abs(np.asarray(Auu[cutv].sum(axis=1))).max() > 1e-3
    # p is coupled on the cut cells only
    assert A[:nv, nv:][interior].nnz == 0


def test_rejects_non_rectangles():
    g = setup(8)
    x = g["x"].copy()
    x[:, 0] += 0.2 * x[:, 1]            # sheared
    f, uD = data(x)
    with pytest.raises(NotImplementedError):
        PQ.assemble(**{**g, "x": x}, f=f, uD=uD)
    x = g["x"].copy()
    x[30] += [0.05, 0.02]               # one moved vertex
    with pytest.raises(NotImplementedError):
        PQ.assemble(**{**g, "x": x}, f=f, uD=uD)
