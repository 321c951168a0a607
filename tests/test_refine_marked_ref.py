"""The numpy specification of marked refinement (tests/refine_marked_ref.py) checked on its own, without a GPU:
conformity, volume, child counts, the special masks and the shape of the cells over repeated refinement near a point."""
import functools

import numpy as np
import pytest

import partition_ref as PR
import refine_marked_ref as RM
import refine_ref as RR
from datasets import load_mesh

EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def arrays(name):
    if name == "graded_tet_box":
        return ("tetrahedron",) + PR.graded_tet_box()
    if name.startswith("kuhn"):
        return ("tetrahedron",) + RM.kuhn_box(int(name[4:]))
    ctype, x, cells = load_mesh(name)
    return ctype, np.asarray(x, dtype=np.float64), np.asarray(cells, dtype=np.int64)


def points(name):
    """The points the marking gathers around: an interior one; a rim point for the disk; corner and centre for Kuhn."""
    _, x, _ = arrays(name)
    lo, hi = x.min(axis=0), x.max(axis=0)
    if name.startswith("kuhn"):
        return {"corner": lo, "centre": 0.5 * (lo + hi)}
    interior = lo + (hi - lo) * np.array([0.37, 0.58, 0.44][:x.shape[1]])
    if name == "disk":
        cen = 0.5 * (lo + hi)
        return {"interior": interior, "rim": cen + 0.5 * (hi - lo) * np.array([np.cos(0.7), np.sin(0.7)])}
    return {"interior": interior}


CASES = [(n, p) for n in ("disk", "coarse_square", "graded_tet_box", "kuhn2", "kuhn3") for p in points(n)]


def check_mesh(ctype, x, cells, vol0):
    assert np.all(np.isin(RM.facet_cell_counts(ctype, cells), (1, 2))), "a facet with more than two cells"
    vol = np.abs(RM.signed_volumes(x, cells))
    assert np.all(vol > 0.0), "a degenerate cell"
    assert abs(vol.sum() - vol0) <= cells.shape[0] * EPS * vol0


@pytest.mark.parametrize("name,where", CASES)
def test_rounds_near_a_point(name, where):
    ctype, x, cells = arrays(name)
    point = points(name)[where]
    vol0 = np.abs(RM.signed_volumes(x, cells)).sum()
    two_d = ctype == "triangle"
    shape = [RM.min_angle_deg(x, cells) if two_d else RM.tet_quality(x, cells)]
    for rnd in range(6 if two_d else 4):
        r = RM.refine_marked_ref(ctype, x, cells, cell_marks=RM.nearest_mask(x, cells, point))
        hist = np.bincount(np.bincount(r["parent_cells"], minlength=cells.shape[0]))
        assert hist[0] == 0 and len(hist) - 1 <= RM.MAXCHILD[ctype] and hist.sum() == cells.shape[0]
        assert r["x"].shape[0] == x.shape[0] + r["marked"].sum() and np.array_equal(r["x"][:x.shape[0]], x)
        assert np.array_equal(r["parent_cells"], np.sort(r["parent_cells"]))
        x, cells = r["x"], r["cells"]
        check_mesh(ctype, x, cells, vol0)
        shape.append(RM.min_angle_deg(x, cells) if two_d else RM.tet_quality(x, cells))
        print(f"{name}/{where} round {rnd}: {cells.shape[0]} cells, {r['sweeps']} sweeps, children {hist[1:].tolist()}, "
              f"{'min angle' if two_d else 'min |vol|/h^3'} {shape[-1]:.4g}")
    if two_d:
        # longest-edge 4-triangle partitions never fall below half of the coarse mesh's smallest angle
        assert min(shape) >= 0.5 * shape[0]
    else:
        # no bound is known in 3-D (DESIGN.md 7e records the figures): only that the measure stops falling; 1e-12 is
        # for the round-off of the measure itself on similar cells of half the size
        for k in range(3, len(shape)):
            assert shape[k] >= shape[k - 1] * (1.0 - 1e-12)


@pytest.mark.parametrize("name", ["disk", "coarse_square", "graded_tet_box", "kuhn2", "kuhn3"])
def test_all_and_none(name):
    ctype, x, cells = arrays(name)
    nc, nchild = cells.shape[0], RM.MAXCHILD[ctype]
    r = RM.refine_marked_ref(ctype, x, cells, cell_marks=np.ones(nc, dtype=np.uint8))
    assert np.array_equal(np.bincount(r["parent_cells"]), np.full(nc, nchild))
    assert r["marked"].all() and r["x"].shape[0] == x.shape[0] + r["edges"].shape[0]
    assert np.array_equal(r["x"], RR.refine_ref(ctype, x, cells)[0])         # the vertices of uniform refinement
    check_mesh(ctype, r["x"], r["cells"], np.abs(RM.signed_volumes(x, cells)).sum())
    for kw in ({}, {"cell_marks": np.zeros(nc, dtype=np.uint8)}, {"edge_marks": np.zeros(r["edges"].shape[0], dtype=bool)}):
        z = RM.refine_marked_ref(ctype, x, cells, **kw)
        assert np.array_equal(z["x"], x) and np.array_equal(z["cells"], cells) and not z["marked"].any()
        assert np.array_equal(z["parent_cells"], np.arange(nc))
        assert np.array_equal(z["child_nodes"], np.tile(np.arange(cells.shape[1]), (nc, 1)))


@pytest.mark.parametrize("ctype", ["triangle", "tetrahedron"])
def test_single_cell_every_edge_mask(ctype):
    """Every edge mask of one cell: the closure adds the greatest edge (of the cell, of the touched faces), the leaves
    tile the cell, and the mask is independent of the sweep order (least fixed point: closing a closed mask is idle)."""
    x, cells = RR.single_cell(ctype)
    nepc = 3 if ctype == "triangle" else 6
    vol0 = np.abs(RM.signed_volumes(x, cells)).sum()
    for bits in range(1 << nepc):
        em = np.array([(bits >> k) & 1 for k in range(nepc)], dtype=np.uint8)
        r = RM.refine_marked_ref(ctype, x, cells, edge_marks=em)
        assert np.all(r["marked"][em.astype(bool)])
        again = RM.refine_marked_ref(ctype, x, cells, edge_marks=r["marked"])
        assert np.array_equal(again["marked"], r["marked"]) and np.array_equal(again["cells"], r["cells"])
        vol = np.abs(RM.signed_volumes(r["x"], r["cells"]))
        assert np.all(vol > 0.0) and abs(vol.sum() - vol0) <= 8 * EPS * vol0
        assert np.all(np.isin(RM.facet_cell_counts(ctype, r["cells"]), (1, 2)))


def test_transfer_reproduces_polynomials():
    """Degree 1 on the coordinates is the fine coordinate array bit for bit; degree 2 reproduces a quadratic."""
    for name in ("disk", "graded_tet_box"):
        ctype, x, cells = arrays(name)
        r = RM.refine_marked_ref(ctype, x, cells, cell_marks=RM.seeded_mask(cells.shape[0]))
        assert np.array_equal(RM.prolongate_marked_ref(ctype, x, cells, r, x.T, 1), r["x"].T)

        def quad(p):
            return 0.2 + p[:, 0] * p[:, -1] - 0.7 * p[:, 0] ** 2 + 0.4 * p[:, -1] ** 2 + p.sum(axis=1)
        e = r["edges"]
        q = quad(np.concatenate([x, 0.5 * x[e[:, 0]] + 0.5 * x[e[:, 1]]]))
        fe = RR.edge_numbering(ctype, r["cells"])[1]
        qf = quad(np.concatenate([r["x"], 0.5 * r["x"][fe[:, 0]] + 0.5 * r["x"][fe[:, 1]]]))
        assert np.abs(RM.prolongate_marked_ref(ctype, x, cells, r, q, 2) - qf).max() <= 64 * EPS * np.abs(q).max()
