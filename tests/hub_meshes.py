"""Delaunay meshes with vertices of high valence ("hubs"), and the oracle systems on them.  No GPU use.

A hub is one vertex at the centre of m points on a small circle (2-D: equispaced) or sphere (3-D: Fibonacci lattice)
of radius r; no other point lies within 2.2 r of it, so the Delaunay mesh joins the hub to exactly those m points.
The row of a hub in a P1 matrix then holds m + 1 stiffness entries (more with the ghost penalty and the p columns of
a hub on the boundary Gamma of the domain), which is what takes the hashed-slot assembly off the paths that meshes
with the connectivity of a Kuhn lattice (at most 6 / 14 neighbours) ever reach: the spill of the 32-key LDS table of
the row kernel, a slot table at load factor 1, the retry with the next capacity and the refusal behind the last one.

The level-set is the unit sphere about CENTRE, as in tests/test_hip_assembly.py.  `CASES` lists the meshes of
tests/test_hip_high_valence.py with the conditions each has to meet; tests/test_hub_meshes.py pins those conditions
on the CPU, against the oracle alone.
"""
import functools
import warnings

import numpy as np
import scipy.sparse as sp
from scipy.spatial import Delaunay

from oracle import assembly as OA
from oracle import assembly_flux as FX
from oracle import assembly_quad as Q
from oracle import assembly_sd as SD
from oracle import elasticity as EL
from oracle import tagging as T
from oracle.points import FACET_VERTS
from oracle.topology import Topology

LO, HI = -1.5, 1.5
CENTRE = np.array([0.03, -0.02, 0.01])
MIN_VOLUME = 1e-10
ROW_LDS_SLOTS = 32          # keys per thread of the row kernel's LDS table (phx_assemble.hip)

# Row-slot capacities each assembler tries, in order, per dimension (the `retry_capacity` calls of the library).
# Interface elasticity: on generated boxes and rectangles the capacity of the rows of cut-cell vertices (the other rows
# hold EL_BOX_BULK_SLOTS); on every other mesh the capacity of every row.
CAPACITIES = {
    "p1": {2: (32, 64, 128), 3: (64, 128, 256)},
    "p2": {2: (128, 256), 3: (256, 512)},
    "sd": {2: (32, 64), 3: (64, 128)},
    "flux": {2: (64, 128), 3: (256, 512)},
    "el": {2: (256, 512, 1024), 3: (256, 512, 1024)},
}


def on_gamma(d, direction):
    """Point of Gamma (the unit sphere about CENTRE) in the given direction."""
    v = np.asarray(direction, dtype=np.float64)[:d]
    return tuple(CENTRE[:d] + v / np.linalg.norm(v))


def ring_points(d, centre, m, radius):
    centre = np.asarray(centre, dtype=np.float64)
    k = np.arange(m)
    if d == 2:
        t = 2.0 * np.pi * (k + 0.25) / m
        unit = np.stack([np.cos(t), np.sin(t)], axis=1)
    else:
        z = 1.0 - (2.0 * k + 1.0) / m
        t = np.pi * (3.0 - np.sqrt(5.0)) * k
        s = np.sqrt(1.0 - z * z)
        unit = np.stack([s * np.cos(t), s * np.sin(t), z], axis=1)
    return centre + radius * unit


def cell_volumes(x, cells):
    e = x[cells[:, 1:]] - x[cells[:, :1]]
    d = x.shape[1]
    return np.abs(np.linalg.det(e)) / (2.0 if d == 2 else 6.0)


def neighbour_counts(nv, cells):
    """Number of vertices each vertex shares a cell with."""
    n = cells.shape[1]
    i, j = np.repeat(cells, n, axis=1).reshape(-1), np.tile(cells, (1, n)).reshape(-1)
    G = sp.csr_matrix((np.ones(i.size), (i, j)), shape=(nv, nv))
    G.sum_duplicates()
    return np.diff(G.indptr) - 1


def build_hub_mesh(d, seed, n_background, hubs):
    """-> x [nv, d], cells [nc, d + 1] (int64), hub vertex indices.  hubs: list of (centre, m, radius)."""
    rng = np.random.default_rng(seed)
    corners = np.array(np.meshgrid(*([[LO, HI]] * d), indexing="ij")).reshape(d, -1).T
    bg = rng.uniform(LO, HI, size=(n_background, d))
    for centre, m, radius in hubs:
        bg = bg[np.linalg.norm(bg - np.asarray(centre)[:d], axis=1) >= 2.2 * radius]
    pts = [corners, bg]
    first_hub = corners.shape[0] + bg.shape[0]
    if hubs:
        pts.append(np.array([np.asarray(c, dtype=np.float64)[:d] for c, _, _ in hubs]))
        pts += [ring_points(d, np.asarray(c, dtype=np.float64)[:d], m, r) for c, m, r in hubs]
    x = np.ascontiguousarray(np.concatenate(pts))
    tri = Delaunay(x)
    cells = tri.simplices.astype(np.int64)
    assert tri.coplanar.size == 0 and np.unique(cells).size == x.shape[0], "qhull dropped points"
    vol = cell_volumes(x, cells)
    assert vol.min() >= MIN_VOLUME, f"sliver cell: volume {vol.min():.3e} (seed {seed})"
    hub_idx = first_hub + np.arange(len(hubs))
    nn = neighbour_counts(x.shape[0], cells)
    for h, (_, m, _) in zip(hub_idx, hubs):
        assert nn[h] == m, f"hub {h} has {nn[h]} neighbours, not {m} (seed {seed})"
    return x, cells, hub_idx


def levelset(pts, sign=1.0):
    d = pts.shape[1]
    return sign * (((pts - CENTRE[:d]) ** 2).sum(axis=1) - 1.0)


def boundary_vertices(topo, ctype):
    """Vertices of the exterior facets (the Dirichlet vertices of the elasticity tests)."""
    f2c = np.asarray(topo.f2c)
    bf = np.flatnonzero(f2c[:, 1] < 0)
    c = f2c[bf, 0]
    c2f = np.asarray(topo.c2f)
    lf = np.argmax(c2f[c] == bf[:, None], axis=1)
    return np.unique(np.take_along_axis(topo.cells[c], FACET_VERTS[ctype][lf], axis=1))


def nodal_data(kind, d, x, V=None, Vp=None):
    """Level-set and nodal inputs of assembler `kind` ("p1" | "p2" | "sd" | "flux" | "el"), as the existing GPU test of
    that assembler chooses them.  V / Vp: oracle spaces of the unknown / the level-set where the kind has some."""
    if kind == "p1":
        uex = np.prod(np.sin(x), axis=1)
        return dict(phi=levelset(x), f=d * uex, ud=uex)
    if kind == "p2":
        pts = V.dof_points(x)
        uex = np.prod(np.sin(pts), axis=1)
        return dict(phi=levelset(Vp.dof_points(x)), f=d * uex, ud=uex)
    if kind == "sd":
        g = 1.0 + 0.5 * x[:, 0] - 0.25 * x[:, 1]
        return dict(phi=levelset(x), f=2.0 * d * g + 4.0 * (0.5 * x[:, 0] - 0.25 * x[:, 1]) + np.sin(x[:, 0]))
    if kind == "flux":
        uex = np.cos(x[:, 0]) * np.sin(x[:, 1] + 0.3) * (np.cos(0.5 * x[:, 2]) if d == 3 else 1.0)
        return dict(phi=levelset(Vp.dof_points(x)), f=(3.0 if d == 2 else 3.25) * uex, g=np.sin(x.sum(axis=1)) + uex)
    if kind == "el":
        rng = np.random.default_rng(5)
        return dict(phi=levelset(x, -1.0), f=np.sin(x @ rng.standard_normal((d, d))) + 0.3,
                    ud=np.cos(x @ rng.standard_normal((d, d))))
    raise ValueError(kind)


FLUX = dict(pen_coef=1.2, stab_coef=0.8, robin_coef=1.0, facet_tag=2, qdeg=10)
SD_STAB = 0.8
EL_E_OUT = 1.0e-3
EL_BOX_BULK_SLOTS = 64


def oracle_assemble(kind, topo, x, cell_tags, facet_tags, ds100, ds101, space=Q.Space):
    """Oracle system of assembler `kind` on tagged arrays -> (A, b, active, data).  `space(topo, degree)` builds the
    oracle spaces (the GPU tests pass one with the library's edge numbering)."""
    d = x.shape[1]
    ctype = "triangle" if d == 2 else "tetrahedron"
    if kind == "p1":
        data = nodal_data(kind, d, x)
        A, b, act = OA.assemble_poisson_wd(topo, x, cell_tags, facet_tags, ds100, data["phi"], data["f"], data["ud"])
    elif kind == "p2":
        V, Vp = space(topo, 2), space(topo, 1)
        data = nodal_data(kind, d, x, V, Vp)
        A, b, act = Q.assemble_poisson_wd_quad(topo, x, cell_tags, facet_tags, ds100, V, Vp, data["phi"], data["f"],
                                               data["ud"])
    elif kind == "sd":
        V = space(topo, 1)
        data = nodal_data(kind, d, x)
        A, b, act = SD.assemble_poisson_sd(topo, x, cell_tags, facet_tags, ds100, V, V, data["phi"], data["f"],
                                           stab_coef=SD_STAB)
    elif kind == "flux":
        Vp = space(topo, 2)
        data = nodal_data(kind, d, x, None, Vp)
        A, b, act = FX.assemble_poisson_flux(topo, x, cell_tags, facet_tags, ds100, Vp, data["phi"], data["f"],
                                             data["g"], **FLUX)
    elif kind == "el":
        data = nodal_data(kind, d, x)
        data["bcv"] = boundary_vertices(topo, ctype)
        A, b, act = EL.assemble_elasticity_if(topo, x, cell_tags, facet_tags, ds100, ds101, data["phi"], data["f"],
                                              data["ud"], data["bcv"], E_in=1.0, E_out=EL_E_OUT)
    else:
        raise ValueError(kind)
    return A, b, act, data


def active_system(A, b, act):
    """-> (active CSR with sorted columns, active rhs, active full indices)."""
    idx = np.flatnonzero(act)
    Ao = A[idx][:, idx].tocsr()
    Ao.sort_indices()
    return Ao, b[idx], idx


def oracle_system(kind, x, cells):
    """The oracle alone: tags (box mode; single-layer cut for the weak-Dirichlet kinds, as their GPU tests), assembly.
    -> dict(A, b, idx: active system; widths: np.diff(indptr); neighbours: per vertex; act, cell_tags, topo)."""
    d = x.shape[1]
    ctype = "triangle" if d == 2 else "tetrahedron"
    topo = Topology(ctype, cells, x.shape[0])
    sign = -1.0 if kind == "el" else 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ct, ft, _, meas, _, _ = T.compute_tags_measures(ctype, x, topo, T.NodalP1(levelset(x, sign)), 1, box_mode=True,
                                                        single_layer_cut=kind in ("p1", "p2"))
    cv = np.zeros(topo.nc, dtype=np.int64)
    cv[ct.indices] = ct.values
    A, b, act, _ = oracle_assemble(kind, topo, x, cv, ft.values, meas(100), meas(101))
    Ao, bo, idx = active_system(A, b, act)
    return dict(A=Ao, b=bo, idx=idx, act=act, widths=np.diff(Ao.indptr), neighbours=neighbour_counts(x.shape[0], cells),
                cell_tags=cv, topo=topo)


def bulk_row_widths(x, cells, cell_tags, idx, widths):
    """Widths of the active rows of DoFs at vertices that belong to no cut cell (cell tag 2)."""
    nv = x.shape[0]
    cutv = np.zeros(nv, dtype=bool)
    cutv[np.unique(cells[np.asarray(cell_tags) == 2])] = True
    return np.asarray(widths)[~cutv[np.asarray(idx) % nv]]


def library_space(mesh, topo, degree):
    """Oracle space of `degree` on a library mesh, with the LIBRARY's edge numbering (`mesh.edges`, `mesh.c2e`)."""
    V = Q.Space.__new__(Q.Space)
    V.topo, V.degree = topo, degree
    if degree == 1:
        V.ndofs, V.cell_dofs, V.edge_vertices = topo.nv, topo.cells, None
    else:
        V.edge_vertices = mesh.edges.astype(np.int64)
        V.ndofs = topo.nv + V.edge_vertices.shape[0]
        V.cell_dofs = np.concatenate([topo.cells, topo.nv + mesh.c2e.astype(np.int64)], axis=1)
    return V


def predicted_capacity(kind, d, widest):
    """First capacity of the assembler that holds a row of `widest` entries; None: beyond the last one."""
    for W in CAPACITIES[kind][d]:
        if widest <= W:
            return W
    return None


# ---------------------------------------------------------------------------------------------------------------
# The cases.  name -> (kind, d, seed, background points, hubs, condition).  A condition is
#   ("widest", lo, hi):  lo <= widest active row <= hi
#   plus, for "spill": the first hub is an interior vertex (u row active, p row inactive) with >= 33 neighbours;
#   for "bulk" (interface elasticity): some row of a vertex that belongs to no cut cell holds more than the 64 slots
#   such rows get on generated boxes (`bulk_row_widths`).
# ---------------------------------------------------------------------------------------------------------------
def _case(kind, d, seed, nbg, hubs, lo, hi, spill=False, bulk=False):
    return dict(kind=kind, d=d, seed=seed, nbg=nbg, hubs=hubs, lo=lo, hi=hi, spill=spill, bulk=bulk)


G2 = on_gamma(2, (0.6, 0.8))
G3 = on_gamma(3, (0.48, 0.6, 0.64))
IN2 = (0.05, 0.1)
IN3 = (0.05, 0.1, -0.05)

R2, R3 = 0.08, 0.12     # ring radii
CASES = {
    # P1 weak Dirichlet, 2-D: capacities 32, 64, 128
    "p1_2d_a_fits": _case("p1", 2, 1, 300, [(G2, 40, R2)], 28, 32),
    "p1_2d_b_full": _case("p1", 2, 1, 300, [(G2, 45, R2)], 32, 32),
    # (a stiffness row of 34 entries cannot fit the first 2-D capacity: the spill is followed by the retry with 64)
    "p1_2d_c_spill": _case("p1", 2, 1, 300, [(IN2, 33, R2)], 34, 64, spill=True),
    "p1_2d_d_retry": _case("p1", 2, 1, 300, [(G2, 70, R2)], 33, 64),
    "p1_2d_d_retry_twice": _case("p1", 2, 1, 300, [(IN2, 100, R2)], 65, 128),
    "p1_2d_e_refusal": _case("p1", 2, 1, 300, [(IN2, 130, R2)], 129, None),
    # P1 weak Dirichlet, 3-D: capacities 64, 128, 256
    "p1_3d_a_fits": _case("p1", 3, 1, 300, [(G3, 30, R3)], 60, 64),
    "p1_3d_b_full": _case("p1", 3, 1, 300, [(G3, 31, R3)], 64, 64),
    "p1_3d_c_spill": _case("p1", 3, 1, 300, [(IN3, 40, R3)], 41, 64, spill=True),
    "p1_3d_d_retry": _case("p1", 3, 1, 300, [(G3, 70, R3)], 65, 128),
    "p1_3d_d_retry_twice": _case("p1", 3, 1, 300, [(IN3, 150, R3)], 129, 256),
    "p1_3d_e_refusal": _case("p1", 3, 1, 300, [(IN3, 260, R3)], 257, None),
    # the other assemblers: widest row in (W1, W2]
    "p2_2d": _case("p2", 2, 1, 200, [(IN2, 60, R2)], 129, 256),
    "p2_3d": _case("p2", 3, 1, 100, [(G3, 40, R3)], 257, 512),
    "sd_2d": _case("sd", 2, 1, 300, [(IN2, 40, R2)], 33, 64),
    "sd_3d": _case("sd", 3, 1, 300, [(IN3, 80, R3)], 65, 128),
    "flux_2d": _case("flux", 2, 1, 200, [(IN2, 80, R2)], 65, 128),
    "flux_3d": _case("flux", 3, 1, 150, [(G3, 80, R3)], 257, 512),
    # 2-D interface elasticity: a hub of 200 ring points on Gamma gives rows of 244 entries, still within the first
    # capacity (256): its retry stays unreached.  (A background vertex outside the ring, away from the cut cells, is
    # joined to 47 ring points: rows of 96 entries.)
    "el_2d": _case("el", 2, 1, 200, [(G2, 200, R2)], 200, 256, bulk=True),
    "el_2d_bulk": _case("el", 2, 1, 200, [(IN2, 40, R2)], 65, 256, bulk=True),      # a hub off Gamma: rows of 82
    "el_3d": _case("el", 3, 1, 150, [(G3, 36, R3), (IN3, 40, R3)], 257, 512, bulk=True),   # and one of 126 off Gamma
    # an ordinary Delaunay mesh of random points, no hub: up to 26 neighbours away from the cut cells, rows of 81
    "el_3d_delaunay": _case("el", 3, 1, 400, [], 257, 512, bulk=True),
}


@functools.lru_cache(maxsize=None)
def case_mesh(name):
    c = CASES[name]
    return build_hub_mesh(c["d"], c["seed"], c["nbg"], c["hubs"])


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    x, cells, _ = case_mesh(name)
    return oracle_system(CASES[name]["kind"], x, cells)
