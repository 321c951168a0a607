"""Meshes, masks and nodal fields of the gradient-recovery tests (TEST INFRASTRUCTURE, no GPU use): shared by
tests/test_hip_recover.py (GPU) and tests/test_recover_ref.py, which asserts the input conditions on the CPU.

The meshes are the seven of tests/estimate_cases.py with their level-sets (radius factor 0.62, on the 3 x 4 x 5 boxes
0.8) and two Delaunay meshes of tests/hub_meshes.py with a vertex of high valence inside the circle / sphere of radius
factor 0.62: `flux_2d` (558 triangles, a star of 80) and `p2_3d` (826 tetrahedra, a star of 76).  Nodal fields are the
seeded sums of sines of estimate_cases.smooth_field, one seed per component."""
import functools
import warnings

import numpy as np

import estimate_cases as EC
import hub_meshes as HM

HUBS = ["flux_2d", "p2_3d"]
MESHES = EC.MESHES + HUBS
VECTOR = ["disk", "box_3d"]            # ncomp = gdim as well
SEED = 5
MARK_THETAS = (0.3, 0.5, 0.8)
MARK_MESHES = [("disk", 1), ("flux_2d", 1)]


def radius_factor(name):
    return EC.RADIUS_FACTOR.get(name, 0.62)


@functools.lru_cache(maxsize=None)
def arrays(name):
    if name in HUBS:
        x, cells, _ = HM.case_mesh(name)
        return ("triangle" if x.shape[1] == 2 else "tetrahedron", np.ascontiguousarray(x, dtype=np.float64),
                np.asarray(cells, dtype=np.int64))
    return EC.arrays(name)


@functools.lru_cache(maxsize=None)
def oracle_tags(name):
    """Cell tags of the oracle for the level-set of estimate_cases.levelset (P1 nodal, single-layer cut)."""
    if name not in HUBS:
        return EC.oracle_tags(name)
    from oracle import tagging as OT
    from oracle.topology import Topology
    ctype, x, cells = arrays(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.asarray(OT.tag_cells_values(Topology(ctype, cells, x.shape[0]), x,
                                              OT.NodalP1(EC.levelset(x, x, radius_factor(name))), 1,
                                              single_layer_cut=True, warn=False)).astype(np.int32)


def field(x, pts, ncomp=None, seed=SEED):
    """(ndofs,) for ncomp None, else (ncomp, ndofs): one seeded smooth field per component."""
    extent = (x.max(axis=0) - x.min(axis=0)).max()
    if ncomp is None:
        return EC.smooth_field(pts, seed, extent)
    return np.stack([EC.smooth_field(pts, seed + 11 * k, extent) for k in range(ncomp)])


def dof_points(ctype, x, cells, degree):
    """DoF points and c2e of the CPU tests (edge numbering of estimate_ref.edge_numbering)."""
    return EC.dof_points(ctype, x, cells, degree)


def sheared_quads():
    """`square_quad` with x -> x + 0.3 y: quadrilaterals the rectangle layer refuses."""
    ctype, x, cells = arrays("square_quad")
    xs = x.copy()
    xs[:, 0] += 0.3 * xs[:, 1]
    return ctype, xs, cells
