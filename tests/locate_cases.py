"""Meshes and point sets of the point-location tests (TEST INFRASTRUCTURE, no GPU use): shared by
tests/test_hip_evaluate.py (GPU) and tests/test_locate_ref.py, which asserts the input condition on the CPU."""
import functools

import numpy as np

import hub_meshes as HM
import locate_ref as LR
import partition_ref as PR
import refine_ref as RR
from datasets import load_mesh

HUB_3D = min((k for k, c in HM.CASES.items() if c["d"] == 3), key=lambda k: (HM.CASES[k]["nbg"] + sum(h[1] for h in HM.CASES[k]["hubs"]), k))
BOX = ([-1.0, 0.0, 0.5], [1.0, 1.5, 2.0], [3, 4, 5])
CALLER = ["single_triangle", "single_tetrahedron", "single_quadrilateral", "disk", "square_tri", "square_quad",
          "graded_tet_box", "hub_3d", "box_shuffled"]
GENERATED = ["box_3d", "box_2d", "box_slab"]
MESHES = CALLER + GENERATED


def shuffled(x, cells, seed=17):
    rng = np.random.default_rng(seed)
    pv = rng.permutation(x.shape[0])           # new vertex i = old vertex pv[i]
    inv = np.empty_like(pv)
    inv[pv] = np.arange(pv.size)
    pc = rng.permutation(cells.shape[0])
    return np.ascontiguousarray(x[pv]), np.ascontiguousarray(inv[cells[pc]]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def arrays(name):
    """(cell type, x, cells) of a caller-supplied test mesh."""
    if name == "graded_tet_box":
        return ("tetrahedron",) + PR.graded_tet_box()
    if name == "hub_3d":
        x, cells, _ = HM.case_mesh(HUB_3D)
        return "tetrahedron", np.ascontiguousarray(x, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    if name == "box_shuffled":
        from oracle import meshgen
        return ("tetrahedron",) + shuffled(*meshgen.create_box(*BOX))
    if name.startswith("single_"):
        return (name[7:],) + RR.single_cell(name[7:])
    ctype, x, cells = load_mesh(name)
    if name == "square_quad":
        # the file's squares run v0 (0,0), v1 (0,1), v2 (1,0), v3 (1,1): tensor-product order with y first.  The
        # rectangle layer wants x first (phx_q1rect.inc.hip), so the local vertices 1 and 2 change places here; the
        # mesh as loaded is one of the refusals of test_refusals_leave_nothing_behind.
        cells = np.ascontiguousarray(cells[:, [0, 2, 1, 3]])
    return ctype, x, cells


def case_points(ctype, x, cells, lattice=False, nrand=300, seed=23):
    """Every cell centroid, every vertex, every edge midpoint, a seeded random cloud in the bounding box enlarged by
    10 %, and for the boxes points on lattice planes and on all upper faces.  -> (points, number of centroids)."""
    xc = x[cells]
    cen = xc.mean(axis=1)
    pairs = RR.LOCAL_PAIRS[ctype]
    ev = np.unique(np.sort(cells[:, pairs].reshape(-1, 2), axis=1), axis=0)
    mid = 0.5 * (x[ev[:, 0]] + x[ev[:, 1]])
    rng = np.random.default_rng(seed)
    lo, hi = x.min(axis=0), x.max(axis=0)
    cloud = lo - 0.1 * (hi - lo) + 1.2 * (hi - lo) * rng.random((nrand, x.shape[1]))
    parts = [cen, x, mid, cloud]
    if lattice:
        d = x.shape[1]
        planes = [np.unique(x[:, a]) for a in range(d)]
        snap = lo + (hi - lo) * rng.random((200, d))
        for i in range(snap.shape[0]):
            for a in np.flatnonzero(rng.random(d) < 0.5):
                snap[i, a] = rng.choice(planes[a])
        top = lo + (hi - lo) * rng.random((20 * (2 ** d - 1), d))           # every non-empty set of upper faces
        for k in range(1, 2 ** d):
            for a in range(d):
                if (k >> a) & 1:
                    top[20 * (k - 1):20 * k, a] = hi[a]
        parts += [snap, top]
    return np.ascontiguousarray(np.concatenate(parts, axis=0)), cen.shape[0]


def settle_points(ctype, x, cells, pts):
    """The midpoint of an edge is in general no float64 point: 0.5 (x_a + x_b) is ONE of its representable neighbours,
    and seen from a sliver cell (hub meshes: heights of 3e-3) one ulp of a coordinate moves a barycentric coordinate by
    6e-14, across the -1e-14 of the input condition.  A point that misses the condition is replaced by the first of its
    neighbours -- each coordinate one ulp down, kept or one ulp up, in lexicographic order -- that meets it: still the
    edge midpoint to the last bit, and a point no cell sees at the tolerance.  -> (points, number of points moved)."""
    import itertools
    pts = pts.copy()
    bad = LR.unsettled_points(ctype, x, cells, pts)
    for i in bad:
        for step in itertools.product((-1, 0, 1), repeat=pts.shape[1]):
            q = np.array([np.nextafter(c, np.inf * s) if s else c for c, s in zip(pts[i], step)])
            if LR.unsettled_points(ctype, x, cells, q[None]).size == 0:
                pts[i] = q
                break
    return pts, int(bad.size)


@functools.lru_cache(maxsize=None)
def reference_caller(name):
    ctype, x, cells = arrays(name)
    pts, ncen = case_points(ctype, x, cells)
    pts, _ = settle_points(ctype, x, cells, pts)
    return (pts, ncen) + LR.locate_ref(ctype, x, cells, pts) + (LR.input_condition(ctype, x, cells, pts),)


def generated_box_arrays(d):
    """The arrays of the generated box BOX (d = 3) or its 2-D counterpart, as oracle.meshgen restates the generator."""
    from oracle import meshgen
    x, cells = meshgen.create_box(BOX[0][:d], BOX[1][:d], BOX[2][:d])
    return ("tetrahedron" if d == 3 else "triangle"), x, cells.astype(np.int64)


