"""Generated 3-D Kuhn boxes are tagged by kernels that take the connectivity in closed form (one thread per cube,
phx_tag_box.inc.hip).  Everything the tag stage produces is integers, so the closed-form path (PHX_OPT_BOX_TAGS = 1, the
default) must equal the generic kernels (PHX_OPT_BOX_TAGS = 0) element by element: cell and facet tags, histograms,
the one-sided measures, the zero-denominator warning -- and what the P1 weak-Dirichlet assembly derives from the vertex
flags and the per-chunk counts the tagging kernels leave behind (numbering, structural counts, entity lists)."""
import ctypes as C
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOX = ([-1.5] * 3, [1.5] * 3)


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def sphere(centre=(0.0, 0.0, 0.0), radius=1.0):
    c = np.asarray(centre, dtype=np.float64)
    return lambda x: ((x - c) ** 2).sum(axis=1) - radius ** 2


def run(P, mesh, levelset, phi_nodal, deg, single_layer, flag):
    """Tag `mesh` with the closed-form kernels on (flag 1) or off (flag 0), then assemble once; returns all results."""
    from phifem_amd import _lib as L
    from phifem_amd.mesh_scripts import BoundaryMeasure, _tag_cells, _tag_facets
    L.check(L.lib.phx_set_option(mesh._h, L.OPT_BOX_TAGS, flag))
    out = {}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        staged = _tag_cells(mesh, levelset, deg, single_layer_cut=single_layer)
    out["zero_denominator"] = any("zero everywhere on a cell" in str(w.message) for w in caught)
    out["cell_tags_before_facets"] = mesh.cell_tag_values().copy()
    out["facet_error"] = ""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _tag_facets(mesh, staged, deg)
    except L.PartitionError as e:     # phi = 0: the reference's facet sets overlap; the tags are written all the same
        out["facet_error"] = str(e)
    out["cell_tags"] = mesh.cell_tag_values().copy()
    out["facet_tags"] = mesh.facet_tag_values().copy()
    hc, hf = (C.c_int64 * 4)(), (C.c_int64 * 7)()
    L.check(L.lib.phx_mesh_tag_histogram(mesh._h, hc, hf))
    out["cell_hist"], out["facet_hist"] = list(hc), list(hf)
    meas = BoundaryMeasure(mesh, True)
    out["ds100"], out["ds101"] = meas(100).copy(), meas(101).copy()
    # the assembly numbers its DoFs from act_in / act_cut and selects from the chunk counts
    uex = np.prod(np.sin(mesh.x), axis=1)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            s = P.PhiFEMSolver(mesh)
            info = s.assemble(phi_nodal, 3.0 * uex, uex)
        perm = np.zeros(info["n_active"], np.int32)
        L.check(L.lib.phx_system_get_perm(s._sys, L.ptr(perm)[0], None, None, 0))
        out["assembly"] = tuple(info[k] for k in ("n_active", "n_active_u", "nnz", "n_slices"))
        out["perm"] = perm
    except (ValueError, RuntimeError, L.PartitionError) as e:   # e.g. no cell tagged 1 / 2: the same refusal on both paths
        out["assembly"] = (type(e).__name__, str(e))
        out["perm"] = np.zeros(0, np.int32)
    out["ds100_after"], out["ds101_after"] = BoundaryMeasure(mesh, True)(100).copy(), BoundaryMeasure(mesh, True)(101).copy()
    return out


def compare(P, mesh, levelset, phi_nodal, deg=1, single_layer=True):
    new = run(P, mesh, levelset, phi_nodal, deg, single_layer, 1)
    ref = run(P, mesh, levelset, phi_nodal, deg, single_layer, 0)
    assert new.keys() == ref.keys()
    for key in ref:
        a, b = new[key], ref[key]
        if isinstance(b, np.ndarray):
            assert a.shape == b.shape and np.array_equal(a, b), (key, np.flatnonzero(a != b)[:8] if a.shape == b.shape else a.shape)
        else:
            assert a == b, (key, a, b)
    return ref


def nodal_case(P, n, f, deg=1, single_layer=True, **box):
    from phifem_amd.mesh_scripts import NodalFunction
    mesh = P.create_box(BOX[0], BOX[1], list(n), **box)
    phi = f(mesh.x)
    return mesh, compare(P, mesh, NodalFunction(phi), phi, deg, single_layer)


@pytest.mark.parametrize("n,centre", [
    ((1, 1, 1), (0.0, 0.0, 0.0)),        # every facet type at its smallest extent
    ((2, 1, 3), (0.0, 0.0, 0.0)),
    ((5, 4, 3), (0.1, 0.05, -0.05)),     # unequal extents per axis and per facet type
    ((130, 3, 2), (0.0, 0.0, 0.0)),      # two full wavefronts and a tail along x; dword stores at 6 i offsets
    ((23, 17, 9), (0.0, 0.0, 0.0)),      # 21 114 cells: more than ten cell chunks whose boundaries fall inside cubes
])
def test_sphere(P, n, centre):
    mesh, ref = nodal_case(P, n, sphere(centre))
    assert sum(ref["cell_hist"]) == mesh.nc
    if n == (23, 17, 9):
        assert mesh.nc == 21114 and set(np.unique(ref["cell_tags"])) == {1, 2, 3}


@pytest.mark.parametrize("single_layer", [True, False])
def test_band_reaches_a_face(P, single_layer):
    """Sphere centred at (0.55, 0, 0): the band reaches the face x = 1.5 (boundary-cut bit, facet tags 3 / 4)."""
    mesh, ref = nodal_case(P, (16, 16, 16), sphere((0.55, 0.0, 0.0)), single_layer=single_layer)
    assert ref["facet_hist"][3] > 0 and ref["facet_hist"][4] > 0
    assert isinstance(ref["assembly"][0], int) and ref["assembly"][0] > 0


def test_zero_on_a_vertex_plane_and_zero_everywhere(P):
    """phi = x vanishes on a whole vertex plane (exact +-1 compares); phi = 0: den == 0 -> ratio 0.5 and the warning."""
    mesh, ref = nodal_case(P, (12, 12, 12), lambda x: x[:, 0].copy())
    assert not ref["zero_denominator"]
    mesh, ref = nodal_case(P, (12, 12, 12), lambda x: np.zeros(x.shape[0]))
    # every cell is cut; with no inside cell next to them the single layer demotes them all
    assert ref["zero_denominator"] and ref["cell_hist"][3] == mesh.nc and ref["facet_error"]


@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_one_sign(P, sign):
    """No exterior / no interior cells: the `no exterior` argument of the facet rule comes from the histogram."""
    mesh, ref = nodal_case(P, (8, 8, 8), lambda x: np.full(x.shape[0], sign))
    assert ref["cell_hist"][1 if sign < 0 else 3] == mesh.nc


def test_slab_with_cut_faces(P):
    """A slab of a partitioned box: exempt facets, local cube indices against global coordinates."""
    from phifem_amd import _lib as L
    from phifem_amd.mesh_scripts import NodalFunction
    mesh = P.create_box(BOX[0], BOX[1], [6, 5, 3], offset=[0, 0, 2], n_global=[6, 5, 8])
    L.check(L.lib.phx_mesh_set_slab_faces(mesh._h, 1, 1))
    phi = sphere()(mesh.x)
    ref = compare(P, mesh, NodalFunction(phi), phi)
    assert ref["cell_hist"][2] > 0


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_detection_degrees(P, deg):
    """The detection table of degree 1, 2, 3 applied to the register values of a degree-1 level-set."""
    mesh, ref = nodal_case(P, (10, 10, 10), sphere((0.03, -0.02, 0.01)), deg=deg)
    assert set(np.unique(ref["cell_tags"])) == {1, 2, 3}


def test_callable_levelset_mixes_the_paths(P):
    """A callable level-set is sampled at the detection points: the generic cell kernel, followed by the closed-form
    single-layer passes."""
    mesh = P.create_box(BOX[0], BOX[1], [10, 10, 10])

    def f(x):
        return (x[0] - 0.03) ** 2 + (x[1] + 0.02) ** 2 + (x[2] - 0.01) ** 2 - 1.0

    ref = compare(P, mesh, f, f(mesh.x.T), deg=2)
    assert set(np.unique(ref["cell_tags"])) == {1, 2, 3}
