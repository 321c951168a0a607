"""Meshes, level-sets and nodal fields of the error-indicator tests (TEST INFRASTRUCTURE, no GPU use): shared by
tests/test_hip_estimate.py (GPU) and tests/test_estimate_ref.py, which asserts the input conditions on the CPU.

Every mesh has more than 64 cells and a cell count that is no multiple of 64; the 2-D generated box therefore has
7 x 9 squares (126 triangles) on the extents of locate_cases.BOX, whose own 3 x 4 squares give 24 triangles only.  The
circle / sphere is placed as in demo/weak-dirichlet/refine.py (centre = mean vertex + a small offset, radius = 0.62 x
the smallest half extent), so that cells tagged 1, 2 and 3 all occur and, on the 2-D meshes, no cut cell touches the
mesh boundary.  The 3 x 4 x 5 boxes are too coarse for that radius (the sphere holds no whole tetrahedron): there the
factor is 0.8, and the cut layer reaches the mesh boundary, so boundary facets of cut cells are covered as well.  Nodal data are seeded sums of three sines, not solved solutions: no part is small by cancellation."""
import functools

import numpy as np

import estimate_ref as ER
import locate_cases as LC

MESHES = ["disk", "square_tri", "square_quad", "graded_tet_box", "box_shuffled", "box_2d", "box_3d"]
GENERATED = {"box_2d": 2, "box_3d": 3}
BOX_2D = (LC.BOX[0][:2], LC.BOX[1][:2], [7, 9])
RADIUS_FACTOR = {"box_shuffled": 0.8, "box_3d": 0.8}       # every other mesh: 0.62, as the demo
SUBMESH = ["disk", "box_3d"]
FIELDS = ("u", "p", "phi", "f", "ud")


def degrees(ctype):
    return (1,) if ctype == "quadrilateral" else (1, 2)


@functools.lru_cache(maxsize=None)
def arrays(name):
    """(cell type, x, cells) as the oracle restates them (the generated boxes: oracle.meshgen)."""
    if name == "box_2d":
        from oracle import meshgen
        x, cells = meshgen.create_box(*BOX_2D)
        return "triangle", x, cells.astype(np.int64)
    if name == "box_3d":
        return LC.generated_box_arrays(3)
    ctype, x, cells = LC.arrays(name)
    return ctype, np.ascontiguousarray(x, dtype=np.float64), np.asarray(cells, dtype=np.int64)


def circle(x, factor=0.62):
    """(centre, radius) of demo/weak-dirichlet/refine.py for the vertex array x."""
    d = x.shape[1]
    centre = x.mean(axis=0) + np.array([0.013, -0.007, 0.005][:d])
    radius = factor * 0.5 * (x.max(axis=0) - x.min(axis=0)).min()
    return centre, radius


def levelset(x, pts, factor=0.62):
    centre, radius = circle(x, factor)
    return ((pts - centre) ** 2).sum(axis=1) - radius ** 2


def smooth_field(pts, seed, extent):
    """A seeded sum of three sines with wave lengths of the order of the mesh extent, plus a constant."""
    rng = np.random.default_rng(seed)
    d = pts.shape[1]
    v = np.full(pts.shape[0], rng.uniform(-0.5, 0.5))
    for _ in range(3):
        k = rng.uniform(1.0, 4.0, size=d) * rng.choice([-1.0, 1.0], size=d) / extent
        v = v + rng.uniform(0.3, 1.0) * np.sin(pts @ k + rng.uniform(0.0, 2.0 * np.pi))
    return v


def nodal_fields(x, pts, seed=5, factor=0.62):
    """The five nodal functions at the DoF points `pts` of a mesh with vertices x: u, p, f, u_D seeded smooth fields,
    phi the level-set itself."""
    extent = (x.max(axis=0) - x.min(axis=0)).max()
    out = {k: smooth_field(pts, seed + 11 * i, extent) for i, k in enumerate(FIELDS)}
    out["phi"] = levelset(x, pts, factor)
    return out


def dof_points(ctype, x, cells, degree):
    """DoF points for the CPU tests, with the edge numbering of estimate_ref.edge_numbering: (points, c2e or None)."""
    if degree == 1:
        return x, None
    edges, c2e = ER.edge_numbering(ctype, cells)
    return np.concatenate([x, 0.5 * (x[edges[:, 0]] + x[edges[:, 1]])], axis=0), c2e


@functools.lru_cache(maxsize=None)
def oracle_tags(name):
    """Cell tags of the oracle for the level-set above (P1 nodal, detection degree 1, single-layer cut)."""
    import warnings

    from oracle import tagging as OT
    from oracle.topology import Topology
    ctype, x, cells = arrays(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.asarray(OT.tag_cells_values(Topology(ctype, cells, x.shape[0]), x, OT.NodalP1(levelset(x, x, RADIUS_FACTOR.get(name, 0.62))), 1,
                                              single_layer_cut=True, warn=False)).astype(np.int32)


# ---- Doerfler marking with exact sums: small non-negative integers stored as float64 --------------------------------
MARK_LENGTHS = (1, 63, 64, 65, 1000, 70001)
MARK_THETAS = (0.25, 0.5, 0.999, 1.0)


def integer_indicators(n, kind, seed=3):
    """`ties`: runs of equal values with leading and trailing zeros; `zeros`: all zero."""
    if kind == "zeros":
        return np.zeros(n)
    rng = np.random.default_rng(seed + n)
    v = np.repeat(rng.integers(0, 9, size=n // 3 + 1), 3)[:n].astype(np.float64)    # runs of ties
    if n >= 8:
        v[:2] = 0.0
        v[-3:] = 0.0
        v[n // 2] = 40.0                                                             # one dominant cell
    elif v.sum() == 0.0:
        v[0] = 1.0
    return v
