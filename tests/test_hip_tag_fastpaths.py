"""Short paths of the facet tagging and of the ordered selections (phx_tag.hip, phx_tag_box.inc.hip, phx_select.h):
  * the fill pass of a selection leaves a chunk whose scanned count says that it keeps nothing, and asks for all words
    of a chunk before it uses one;
  * a wavefront whose 256 facets (384 / 256 cells) carry one tag takes its counts from one ballot;
  * k_tag_facets asks for the tag bytes of all its cells before it applies the facet rule.
None of them may change a result.  The reference is numpy on the host: the facet rule of oracle/tagging.py on the
exported f2c, the device's cell tags and the `ds` flags of the oracle.  Compared: facet tags, their histogram, and the
three lists the tagging kernels count for (cut cells, ghost-penalty facets, facets tagged 3 / 4) against np.flatnonzero
of their predicates.  "Full" chunks are read as chunks whose wavefronts are uniform: a chunk cannot keep all of its
2048 facets on any of these level-sets.  The closed-form facet -> cells map in the tagging kernel was measured slower
than the f2c loads and is not in the library: what is left of its cases is the generator's map
restated in numpy against the stored f2c; there is no switch to compare across."""
import ctypes as C
import types
import warnings

import numpy as np
import pytest

from oracle import tagging as T

from datasets import load_mesh

pytestmark = pytest.mark.gpu

BOX = ([-1.5] * 3, [1.5] * 3)
CHUNK, WAVE = 2048, 256
BOXES = [(8, 6, 5), (12, 12, 12), (17, 9, 4), (5, 5, 40), (40, 24, 24)]


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0, "no GPU: the HIP path cannot run"
    return phifem_amd


_boxes = {}


def box(P, n):
    if n not in _boxes:
        _boxes[n] = P.create_box(BOX[0], BOX[1], list(n))
    return _boxes[n]


def sphere(centre=(0.0, 0.0, 0.0), radius=1.0):
    c = np.asarray(centre, dtype=np.float64)
    return lambda x: ((x - c[:x.shape[1]]) ** 2).sum(axis=1) - radius ** 2


def plane(x):
    return x[:, 0] + 0.317 * x[:, 1] + 0.113 * x[:, -1] - 0.0437   # through no vertex of these lattices


def device_tags(mesh, phi, has_ext=-1, single_layer=True):
    """Tag on the device; returns cell tags, facet tags, facet histogram and the three lists."""
    from phifem_amd import _lib as L
    from phifem_amd.mesh_scripts import NodalFunction, _tag_cells, _tag_facets
    L.check(L.lib.phx_set_option(mesh._h, L.OPT_HAS_EXTERIOR, has_ext))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        staged = _tag_cells(mesh, NodalFunction(phi), 1, single_layer_cut=single_layer)
        _tag_facets(mesh, staged, 1)
    hc, hf = (C.c_int64 * 4)(), (C.c_int64 * 7)()
    L.check(L.lib.phx_mesh_tag_histogram(mesh._h, hc, hf))
    lists = []
    for which, n in ((0, mesh.nc), (1, mesh.nf), (2, mesh.nf)):
        buf, cnt = np.full(n, -1, dtype=np.int32), C.c_int64(-1)
        L.check(L.lib.phx_mesh_selection(mesh._h, which, buf.ctypes.data_as(C.c_void_p), C.byref(cnt)))
        lists.append(buf[:cnt.value].copy())
    L.check(L.lib.phx_set_option(mesh._h, L.OPT_HAS_EXTERIOR, -1))
    return {"ct": mesh.cell_tag_values(), "ft": mesh.facet_tag_values(), "hist": np.array(list(hf), dtype=np.int64),
            "cut": lists[0], "ghost": lists[1], "t34": lists[2]}


def host_reference(mesh, phi, ct, has_ext=-1, exempt=None):
    """facet_rule on the host from the exported f2c, the cell tags and the boundary-cut flags."""
    f2c = mesh.f2c.astype(np.int64)
    exempt = np.zeros(mesh.nf, dtype=bool) if exempt is None else exempt
    topo = types.SimpleNamespace(cell_type=mesh.cell_type, nc=mesh.nc, nf=mesh.nf, nfpc=mesh.c2f.shape[1],
                                 cells=mesh.cells.astype(np.int64), c2f=mesh.c2f.astype(np.int64), f2c=f2c,
                                 boundary_facets=np.flatnonzero((f2c[:, 1] < 0) & ~exempt))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bcut = T.boundary_cell_cut_flags(topo, mesh.x, T.NodalP1(phi), 1)
    no_ext = (not np.any(ct == 3)) if has_ext < 0 else has_ext == 0
    ft, count = T.tag_facets_values(topo, ct.astype(np.int8), bcut, no_ext)
    assert np.all(count[~exempt] == 1), "the case is degenerate: the reference's facet sets overlap"
    ft = ft.astype(np.int32)
    ft[exempt] = 0
    return {"ft": ft, "hist": np.bincount(ft, minlength=7)[:7].astype(np.int64),
            "cut": np.flatnonzero(ct == 2).astype(np.int32),
            "ghost": np.flatnonzero(((ft == 2) | (ft == 3)) & (f2c[:, 1] >= 0)).astype(np.int32),
            "t34": np.flatnonzero((ft == 3) | (ft == 4)).astype(np.int32)}


def same(a, b, keys):
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), \
            (k, a[k].shape, b[k].shape, np.flatnonzero(a[k] != b[k])[:8] if a[k].shape == b[k].shape else None)


KEYS = ("ft", "hist", "cut", "ghost", "t34")


def check(mesh, phi, has_ext=-1, exempt=None, single_layer=True):
    dev = device_tags(mesh, phi, has_ext, single_layer)
    ref = host_reference(mesh, phi, dev["ct"], has_ext, exempt)
    same(dev, ref, KEYS)
    return dev, ref


def box_f2c_numpy(n):
    """The generator's map restated: facet id = base[type] + index of the anchor inside the type's extent; types
    2a + s lie in planes x_a = const, 6 + c and 9 + a hold the cube's main diagonal.  Returns (nf, 2)."""
    n = np.asarray(n, dtype=np.int64)
    pidx = lambda p0, p1, p2: p0 * 2 + (1 if p1 > p2 else 0)
    out = []
    for t in range(12):
        ext = n.copy()
        if t < 6:
            ext[t // 2] += 1
        o2, o1, o0 = np.meshgrid(np.arange(ext[2]), np.arange(ext[1]), np.arange(ext[0]), indexing="ij")
        o = [o0.reshape(-1), o1.reshape(-1), o2.reshape(-1)]
        cube = lambda q: q[0] + n[0] * (q[1] + n[1] * q[2])
        if t < 6:
            a, s = t // 2, t % 2
            r0, r1 = (1 if a == 0 else 0), (1 if a == 2 else 2)
            s0, s1 = (r1, r0) if s else (r0, r1)
            q = [v.copy() for v in o]
            q[a] -= 1
            lower = np.where(o[a] > 0, cube(q) * 6 + pidx(a, s0, s1), -1)
            upper = np.where(o[a] < n[a], cube(o) * 6 + pidx(s0, s1, a), -1)
            c0 = np.where(lower >= 0, lower, upper)
            c1 = np.where(lower >= 0, upper, -1)
        else:
            a = t - 6 if t < 9 else t - 9
            r0, r1 = (1 if a == 0 else 0), (1 if a == 2 else 2)
            pa, pb = (pidx(r0, r1, a), pidx(r1, r0, a)) if t < 9 else (pidx(a, r0, r1), pidx(a, r1, r0))
            c0, c1 = cube(o) * 6 + pa, cube(o) * 6 + pb
        out.append(np.stack([c0, c1], axis=1))
    return np.concatenate(out, axis=0)


@pytest.mark.parametrize("n", BOXES)
def test_closed_form_map_is_the_stored_f2c(P, n):
    """Every facet, both cells, order included."""
    mesh = box(P, n)
    ref = box_f2c_numpy(n)
    assert ref.shape == (mesh.nf, 2)
    assert np.array_equal(mesh.f2c, ref), np.flatnonzero((mesh.f2c != ref).any(axis=1))[:8]


@pytest.mark.parametrize("n", BOXES)
def test_boxes_unit_sphere(P, n):
    """Facet counts that straddle the paths: nf below one wavefront's worth per type, x extents that are no multiple
    of 4, nf no multiple of 4 or 256, and on 40 x 24 x 24 more than two selection chunks per facet type."""
    mesh = box(P, n)
    dev, ref = check(mesh, sphere()(mesh.x))
    assert ref["cut"].size > 0 and ref["ghost"].size > 0
    if n == (17, 9, 4):
        assert mesh.nf % 4 != 0 and (n[0] + 1) % 4 != 0 and n[0] % 4 != 0
    if n == (40, 24, 24):
        ext = np.array([[n[a] + (1 if t < 6 and t // 2 == a else 0) for a in range(3)] for t in range(12)])
        per_type = ext.prod(axis=1)
        base = np.concatenate([[0], np.cumsum(per_type)])
        assert per_type.min() > 2 * CHUNK
        assert np.any(base[1:-1] % CHUNK != 0) and np.any(base[1:-1] % WAVE != 0)   # type boundaries inside chunks and waves
        nchunks = -(-mesh.nf // CHUNK)
        for key in ("ghost", "t34"):
            kept = np.bincount(ref[key] // CHUNK, minlength=nchunks)
            assert (kept == 0).sum() > 0 and (kept > 0).sum() > 2, key
        kept = np.bincount(ref["cut"] // CHUNK, minlength=-(-mesh.nc // CHUNK))
        assert (kept == 0).sum() > 0 and (kept > 0).sum() > 2
        ft = ref["ft"][:mesh.nf // WAVE * WAVE].reshape(-1, WAVE)
        uniform = (ft == ft[:, :1]).all(axis=1)
        # uniform waves of tag 5 here (the ball is narrower than an x row); of tag 1: test_one_sign
        assert 5 in set(ft[uniform, 0].tolist()) and (~uniform).sum() > 0
        chunk_uniform = uniform[:uniform.size // 8 * 8].reshape(-1, 8).all(axis=1)
        assert chunk_uniform.sum() > 0 and (~chunk_uniform).sum() > 0   # chunks of uniform waves, and mixed ones


def test_small_sphere_one_chunk_of_cut_cells(P):
    """All cut cells in ONE chunk of the cell list: every other chunk leaves the fill pass at once."""
    n = (5, 5, 40)
    mesh = box(P, n)
    dev, ref = check(mesh, sphere((0.0, 0.0, -1.0125), 0.45)(mesh.x))
    assert ref["cut"].size > 0 and np.unique(ref["cut"] // CHUNK).size == 1 and mesh.nc > 2 * CHUNK
    assert (dev["ct"] == 1).sum() > 0


@pytest.mark.parametrize("n", BOXES)
def test_plane_through_the_box(P, n):
    """The level-set cuts the faces of the box: boundary-cut facets, the CB / UB branches of the facet rule.  Without
    the single layer: a cut cell it demotes at a face the level-set crosses lies in two of the reference's facet sets."""
    mesh = box(P, n)
    dev, ref = check(mesh, plane(mesh.x), single_layer=False)
    bnd = mesh.f2c[:, 1] < 0
    assert np.any(bnd & (ref["ft"] == 2)) and ref["t34"].size > 0


@pytest.mark.parametrize("sign", [-1.0, 1.0])
@pytest.mark.parametrize("has_ext", [-1, 0, 1])
def test_one_sign(P, sign, has_ext):
    """All inside / all outside: every wavefront uniform, every chunk empty unless the boundary facets are tagged 4;
    `no exterior` from the histogram and imposed both ways."""
    mesh = box(P, (12, 12, 12))
    dev, ref = check(mesh, np.full(mesh.nv, sign), has_ext=has_ext)
    assert ref["cut"].size == 0 and ref["ghost"].size == 0
    no_ext = (sign < 0) if has_ext < 0 else has_ext == 0
    assert ref["t34"].size == (mesh.nbf if no_ext else 0)
    ft = ref["ft"][:mesh.nf // WAVE * WAVE].reshape(-1, WAVE)
    assert ((ft == (1 if sign < 0 else 5)).all(axis=1)).sum() > 0   # wavefronts uniform in the interior tag


@pytest.mark.parametrize("slab", [0, 1])
def test_two_slabs(P, slab):
    """A two-slab split of 12 x 12 x 12 along z: offsets, the cut plane exempt from tagging."""
    from phifem_amd import _lib as L
    mesh = P.create_box(BOX[0], BOX[1], [12, 12, 6], offset=[0, 0, 6 * slab], n_global=[12, 12, 12])
    L.check(L.lib.phx_mesh_set_slab_faces(mesh._h, 1 if slab == 1 else 0, 1 if slab == 0 else 0))
    k = mesh._facet_vertices() // (13 * 13)
    exempt = (mesh.f2c[:, 1] < 0) & (k == (0 if slab == 1 else 6)).all(axis=1)
    assert exempt.sum() == 2 * 12 * 12
    dev, ref = check(mesh, sphere()(mesh.x), has_ext=1, exempt=exempt)
    assert np.all(dev["ft"][exempt] == 0) and ref["ghost"].size > 0


def test_generic_path_2d_box(P):
    mesh = P.create_box([-1.5, -1.5], [1.5, 1.5], [37, 29])
    dev, ref = check(mesh, sphere()(mesh.x))
    assert ref["cut"].size > 0 and ref["ghost"].size > 0 and mesh.nf > CHUNK
    check(mesh, plane(mesh.x), single_layer=False)


def test_generic_path_unstructured(P):
    ctype, x, cells = load_mesh("disk")
    mesh = P.Mesh.from_arrays(ctype, x, cells)
    r = 0.5 * np.abs(mesh.x).max()
    dev, ref = check(mesh, sphere(radius=r)(mesh.x))
    assert ref["cut"].size > 0 and ref["ghost"].size > 0
