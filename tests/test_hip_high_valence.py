"""GPU parity of the hashed-slot assembly on Delaunay meshes with vertices of high valence (tests/hub_meshes.py)
against the numpy oracles: the branches no mesh with the connectivity of a Kuhn lattice reaches.

 * the spill of the row kernel's 32-key LDS table straight into the row (`RowAcc::add` -> `slot_add_owned`),
 * a slot table that is exactly full (every probe sequence walks the whole row),
 * the retry of the whole assembly with the next capacity (`retry_capacity`), the block-per-row compaction
   (`k_row_fill_block`, `k_row_fill_list`) behind it and the SELL build / SpMV over rows of very different lengths,
 * the refusal behind the last capacity (`MemoryError`), which gives back what it took.

Every case asserts its condition on the oracle matrix first (the widths that tests/test_hub_meshes.py pins on the
CPU), then `info["slot_capacity"]` -- the proof that the assembly took the branch -- the active numbering, the
pattern, values and right-hand side and one SpMV.  Tolerances are the ones of each assembler's own test: P1 1e-12 of
the largest entry (tests/test_hip_assembly.py), the others 1e-11.  The error of each entry relative to the largest
entry of its own row is printed, not asserted.  No solves: these meshes are badly shaped on purpose.
"""
import ctypes as C
import gc
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from oracle.topology import Topology

import hub_meshes as H

pytestmark = pytest.mark.gpu
MAT_TOL = 1e-12          # tests/test_hip_assembly.py
OTHER_TOL = 1e-11        # test_hip_p2 / test_hip_strong_dirichlet / test_hip_flux / test_hip_elasticity


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def live_bytes(P):
    live, cached = C.c_int64(-1), C.c_int64(-1)
    P._lib.check(P._lib.lib.phx_pool_stats(C.byref(live), C.byref(cached)))
    assert live.value >= 0 and cached.value >= 0
    return live.value


def problem(P, name):
    """The mesh of case `name` through the public constructor, tagged by the library, and the oracle system on the
    library's own facet / edge numbering -> (mesh, nodal data, active oracle CSR, active rhs, active full indices)."""
    from phifem_amd.mesh_scripts import NodalFunction
    c = H.CASES[name]
    kind, d = c["kind"], c["d"]
    x, cells, _ = H.case_mesh(name)
    ctype = "triangle" if d == 2 else "tetrahedron"
    mesh = P.Mesh.from_arrays(ctype, x, cells)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, _, meas, _ = P.compute_tags_measures(mesh, NodalFunction(H.levelset(x, -1.0 if kind == "el" else 1.0)), 1,
                                                   box_mode=True, single_layer_cut=kind in ("p1", "p2"))
    topo = Topology(ctype, mesh.cells.astype(np.int64), mesh.nv)
    topo.c2f, topo.f2c, topo.nf = mesh.c2f.astype(np.int64), mesh.f2c.astype(np.int64), mesh.nf
    A, b, act, data = H.oracle_assemble(kind, topo, mesh.x, mesh.cell_tag_values(), mesh.facet_tag_values(), meas(100),
                                        meas(101), space=lambda t, k: H.library_space(mesh, t, k))
    Ao, bo, idx = H.active_system(A, b, act)
    return mesh, data, Ao, bo, idx


def check_condition(name, Ao, mesh=None, idx=None):
    """The case's condition on the oracle matrix the library is compared with -> the capacity it predicts."""
    c = H.CASES[name]
    widths = np.diff(Ao.indptr)
    if c["bulk"]:
        bulk = H.bulk_row_widths(mesh.x, mesh.cells, mesh.cell_tag_values(), idx, widths)
        assert bulk.max() > H.EL_BOX_BULK_SLOTS, (name, int(bulk.max()))
    widest = int(widths.max())
    assert c["lo"] <= widest and (c["hi"] is None or widest <= c["hi"]), (name, widest)
    if c["kind"] == "p1":   # vertex DoFs: the very matrix whose widths the CPU test pins
        assert np.array_equal(widths, H.case_oracle(name)["widths"])
    return H.predicted_capacity(c["kind"], c["d"], widest), widest


def make_solver(P, kind, mesh, **kw):
    if kind == "p1":
        return P.PhiFEMSolver(mesh, **kw)
    if kind == "p2":
        return P.PhiFEMSolver(mesh, degree=2, levelset_degree=1, **kw)
    if kind == "sd":
        return P.StrongDirichletSolver(mesh, stab_coef=H.SD_STAB)
    if kind == "flux":
        return P.NeumannRobinSolver(mesh, pen_coef=H.FLUX["pen_coef"], stab_coef=H.FLUX["stab_coef"],
                                    robin_coef=H.FLUX["robin_coef"], facet_tag=H.FLUX["facet_tag"],
                                    quadrature_degree=H.FLUX["qdeg"])
    return P.InterfaceElasticitySolver(mesh, E_in=1.0, E_out=H.EL_E_OUT)


def assemble(kind, s, data):
    if kind in ("p1", "p2"):
        return s.assemble(data["phi"], data["f"], data["ud"])
    if kind == "sd":
        return s.assemble(data["phi"], data["f"])
    if kind == "flux":
        return s.assemble(data["phi"], data["f"], data["g"])
    return s.assemble(data["phi"], data["f"], data["ud"], data["bcv"])


def compare(name, s, info, Ao, bo, idx, tol, capacity, widest):
    """slot capacity, numbering, pattern, values, right-hand side, SpMV -> the exported matrix and right-hand side"""
    assert info["slot_capacity"] == capacity, (name, info["slot_capacity"], capacity)
    rowptr, col, val, rhs, dof = s.export_csr()
    n = rowptr.size - 1
    Hm = sp.csr_matrix((val, col, rowptr), shape=(n, n))
    assert info["n_active"] == idx.size
    assert np.array_equal(dof, idx), "active DoF numbering differs"
    assert np.array_equal(Hm.indptr, Ao.indptr)
    assert np.array_equal(Hm.indices, Ao.indices)
    scale = np.abs(Ao.data).max()
    err = np.abs(Hm.data - Ao.data)
    rows = np.repeat(np.arange(n), np.diff(Ao.indptr))
    rowmax = np.maximum.reduceat(np.abs(Ao.data), Ao.indptr[:-1])
    per_row = (err / np.maximum(rowmax[rows], 1e-300)).max()
    bscale = max(np.abs(bo).max(), 1e-300)
    rng = np.random.default_rng(0)
    xv = rng.standard_normal(n)
    y = s.spmv(xv)
    yo = Ao @ xv
    spmv_tol = 1e-12 if tol == MAT_TOL else tol
    ratios = {"matrix": err.max() / (tol * scale), "rhs": np.abs(rhs - bo).max() / (tol * bscale),
              "spmv": np.abs(y - yo).max() / (spmv_tol * np.abs(yo).max())}
    print(f"{name}: nv={s.mesh.nv} nc={s.mesh.nc} n_active={n} nnz={Hm.nnz} widest row {widest} "
          f"slot_capacity={info['slot_capacity']} | worst error / bound: matrix {ratios['matrix']:.3g} "
          f"(bound {tol:g} of the largest entry) rhs {ratios['rhs']:.3g} spmv {ratios['spmv']:.3g} | "
          f"worst entry error relative to its row's largest entry {per_row:.3g} (not asserted)")
    assert ratios["matrix"] <= 1.0
    assert ratios["rhs"] <= 1.0
    assert ratios["spmv"] <= 1.0
    return Hm, rhs


P1_PASSING = [n for n, c in H.CASES.items() if c["kind"] == "p1" and c["hi"] is not None]
P1_REFUSED = [n for n, c in H.CASES.items() if c["kind"] == "p1" and c["hi"] is None]
OTHERS = [n for n, c in H.CASES.items() if c["kind"] != "p1"]


@pytest.mark.parametrize("name", P1_PASSING)
def test_p1_matrix_and_rhs_vs_oracle(P, name):
    """(a) fits, (b) full table, (c) LDS spill, (d) retry -- once and twice -- in 2-D and 3-D.  2-D (c): a stiffness
    row of 34 entries cannot fit the first 2-D capacity of 32, so the spill there is followed by the retry with 64."""
    mesh, data, Ao, bo, idx = problem(P, name)
    capacity, widest = check_condition(name, Ao)
    if name.endswith("_b_full"):
        assert np.count_nonzero(np.diff(Ao.indptr) == capacity) >= 1
    s = make_solver(P, "p1", mesh)
    info = assemble("p1", s, data)
    assert info["has_csr"] == 1 and info["stencil_rows"] == 0      # not a box in disguise: the hashed slots
    compare(name, s, info, Ao, bo, idx, MAT_TOL, capacity, widest)


@pytest.mark.parametrize("name", P1_REFUSED)
def test_p1_refusal_behind_the_last_capacity(P, name):
    """(e): a row wider than the last capacity raises the overflow flag in every attempt -- the kernels' designed exit --
    and the assembly is refused with a MemoryError that names the capacity, leaves nothing behind, and does not
    poison the next assembly."""
    mesh, data, Ao, bo, idx = problem(P, name)
    capacity, widest = check_condition(name, Ao)
    assert capacity is None
    last = H.CAPACITIES["p1"][H.CASES[name]["d"]][-1]
    s = make_solver(P, "p1", mesh)
    gc.collect()
    with pytest.raises(MemoryError, match=f"capacity {last} exceeded"):
        assemble("p1", s, data)
    first = live_bytes(P)
    with pytest.raises(MemoryError, match=f"capacity {last} exceeded"):
        assemble("p1", s, data)
    second = live_bytes(P)
    print(f"{name}: nv={mesh.nv} nc={mesh.nc} widest row {widest} > {last}: MemoryError; live bytes after the first "
          f"failure {first}, after the second {second}")
    assert second == first
    ok = name.replace("_e_refusal", "_a_fits")
    mesh2, data2, Ao2, bo2, idx2 = problem(P, ok)
    capacity2, widest2 = check_condition(ok, Ao2)
    s2 = make_solver(P, "p1", mesh2)
    compare(ok + " after the refusal", s2, assemble("p1", s2, data2), Ao2, bo2, idx2, MAT_TOL, capacity2, widest2)


def test_p1_deterministic_retry_3d(P):
    """PHX_OPT_DETERMINISTIC on 3-D case (d): every term goes through `slot_add` (no LDS table), in two passes per
    attempt.  Two assemblies are the same bits, and both match the oracle."""
    name = "p1_3d_d_retry"
    mesh, data, Ao, bo, idx = problem(P, name)
    capacity, widest = check_condition(name, Ao)
    out = []
    for k in range(2):
        s = make_solver(P, "p1", mesh, deterministic=True)
        info = assemble("p1", s, data)
        out.append(compare(f"{name} deterministic #{k}", s, info, Ao, bo, idx, MAT_TOL, capacity, widest))
    (H0, r0), (H1, r1) = out
    assert np.array_equal(H0.data, H1.data) and np.array_equal(r0, r1)


@pytest.mark.parametrize("name", OTHERS)
def test_other_assemblers_vs_oracle(P, name):
    """P2 weak Dirichlet, strong Dirichlet (degree 1), flux and interface elasticity on a hub mesh whose widest row
    lies in (W1, W2]: the retry of each.  2-D interface elasticity: a hub of 200 ring points gives rows of 244
    entries, within W1 = 256 -- its retry stays unreached and `slot_capacity == W1` is asserted instead.  Every
    elasticity mesh also has rows of more than 64 entries at vertices away from the cut cells (a hub off Gamma, or
    plain Delaunay valence in 3-D): such rows hold 64 slots on generated boxes only."""
    kind = H.CASES[name]["kind"]
    mesh, data, Ao, bo, idx = problem(P, name)
    capacity, widest = check_condition(name, Ao, mesh, idx)
    caps = H.CAPACITIES[kind][H.CASES[name]["d"]]
    assert capacity == (caps[0] if name.startswith("el_2d") else caps[1])
    s = make_solver(P, kind, mesh)
    info = assemble(kind, s, data)
    compare(name, s, info, Ao, bo, idx, OTHER_TOL, capacity, widest)
