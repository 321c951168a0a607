"""One application of the coarse-space correction,  out += D R Ac^-1 R^T in  (phx_coarse.inc.hip), through the test aid
`phx_coarse_apply` -- the functions the Krylov loop calls -- against the numpy specification tests/coarse_ref.py, stage
by stage and on the device's own input to each stage, so that a failure names its kernel:

  restriction   (k_cc_restrict_x<false,false> / k_p2c_restrict_x<false>, k_cc_restrict_axis, k_cc_compact)
                |gc - R^T v|_i <= 2 (3 (2 r - 1) + 6) eps (R^T |v|)_i: three nested recursive sums of at most 2 r - 1
                products, each weight with at most three roundings (inv_h, the product, the subtraction); R >= 0, so
                R^T |v| is the condition-free scale.  r is the ratio the kernels use (2 ratio_h for P2).
  gemv          (k_cc_gemv / k_p2c_gemv)  |zc - Ainv gc_dev|_i <= 2 nc eps (|Ainv| |gc_dev|)_i with the exported Ainv.
  prolongation  (k_cc_expand, k_cc_prolong_axis, k_cc_prolong_x_add / k_p2c_prolong_x_add, the scaling dpos)
                |(out - out0) - D R zc_dev|_i <= 32 eps (D R |zc_dev|)_i + eps |out_i|: at most eight products built in
                three passes, and the rounding of the final +=.
  end to end    max |(out - out0) - x_ref| <= 1e-8 max |x_ref|, x_ref = D R (R^T A R)^-1 R^T v from numpy.linalg.solve:
                1e-8 is the project's bound on Ainv Ac - I; a structural error is O(1).

Rows outside the support of R must come back bit for bit; an impulse on a row without a coarse function must give
gc = 0 exactly and leave out untouched.  Every application starts from a seeded random out0; the impulses follow the dense
vector, so nothing an earlier application left in X1 / X2 / X3 may show.  Every case prints its worst ratio to each bound.

Cases: the smallest at which each branch exists.  Which rows reach the edge of the coarse lattice:
  * the sphere of the weak-Dirichlet and P2 problems lies inside the box, so their active rows stay clear of the last
    coarse cell.  In particular elwd-3d-12-H6, where the ratio divides n, has no eligible row on the last lattice point:
    it does NOT reach the `c0 > m - 2` clamp of cc_axis on the device;
  * the interface systems are active on the whole box, but their rows on the box faces are Dirichlet rows (u_in) or
    inactive (u_out) and carry no coarse function: the highest eligible index is n - 1 (asserted).  At 24^2 with H = 5 h
    that is inside the cut-short last cell (20 .. 25); at 11^3 the last eligible index, 10, is itself a node;
  * so no layout has an eligible row on the last lattice point, and the clamp of cc_axis is pinned by the CPU checks of
    the specification (tests/test_coarse_ref.py) alone."""
import types

import numpy as np
import pytest
import scipy.sparse as sp

import coarse_ref as CR
from test_hip_elasticity import setup as if_setup
from test_hip_elasticity_wd import CENTRE, box_case, smooth_data, tag
from test_hip_p2 import setup as p2_setup

pytestmark = pytest.mark.gpu
LD, EPS = CR.LD, CR.EPS
VB_COARSE, BOX_COARSE = "vertex-block-jacobi+coarse", "box-dst+coarse"

CASES = {
    # weak-Dirichlet elasticity
    "elwd-2d-24-H5": ("elwd", (24, 24), 5),             # n no multiple of the ratio
    "elwd-3d-12x10x15-H5": ("elwd", (12, 10, 15), 5),   # three different nf, m and h
    "elwd-3d-12-H6": ("elwd", (12, 12, 12), 6),         # the ratio divides n (the clamp of cc_axis is not reached: see above)
    "elwd-2d-72-H8": ("elwd", (72, 72), 8),             # nf0 = 73 > 64: the strided LDS staging of k_cc_restrict_x
    # interface elasticity (the data of test_elasticity_coarse_correction_vs_direct)
    "if-2d-24-H5": ("interface", (24, 24), 5),
    "if-3d-11-H5": ("interface", (11, 11, 11), 5),
    # P2 weak Dirichlet
    "p2-2d-24-H5": ("p2", (24, 24), 5),
    "p2-3d-10-H5": ("p2", (10, 10, 10), 5),
    "p2-2d-40-H5": ("p2", (40, 40), 5),                 # lattice lines of 81 > 64 points: two ballot rounds of k_p2c_sort
}
IDS = list(CASES)


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


def build(P, name):
    """Assemble and solve once natively, export what the reference needs."""
    layout, ncubes, ratio = CASES[name]
    d = len(ncubes)
    c = types.SimpleNamespace(name=name, layout=layout, d=d, ncubes=ncubes, ratio_h=ratio,
                              r=ratio * CR.steps_per_cube(layout), bcv=None)
    if layout == "elwd":
        if len(set(ncubes)) == 1:
            mesh, _, phi = box_case(d, ncubes[0])
        else:
            mesh = P.create_box([-1.5] * d, [1.5] * d, list(ncubes))
            phi = ((mesh.x - np.asarray(CENTRE)[:d]) ** 2).sum(axis=1) - 1.0
            tag(P, mesh, phi)
        f, uD = smooth_data(mesh.x)
        s = P.ElasticitySolver(mesh, coarse=ratio, deterministic=True)
        s.assemble(phi, f, uD)
        s.solve(rtol=1e-8, max_iter=200000)
        c.pts, c.nent, kind = mesh.x, mesh.nv, VB_COARSE
    elif layout == "interface":
        mesh, topo, x, phi, bcv = if_setup(P, d, ncubes[0], 1.0e-3, centre=[0.02, -0.01, 0.03])
        f = np.stack([np.sin(x[:, 0]) + 0.2, np.cos(x[:, 1]), 0.5 * x[:, -1]][:d], axis=1)
        uD = 0.1 * np.stack([x[:, 0] * x[:, 1], np.sin(x[:, -1]), x[:, 0] - x[:, 1]][:d], axis=1)
        s = P.InterfaceElasticitySolver(mesh, E_in=1.0, E_out=1.0e-3, deterministic=True, coarse=ratio)
        s.assemble(phi, f, uD, bcv)
        s.solve(rtol=1e-8, max_iter=200000)
        c.pts, c.nent, c.bcv, kind = x, mesh.nv, bcv, VB_COARSE
    else:
        work, V, phi, f, uex, *_ = p2_setup(P, d, ncubes[0], 1)
        s = P.PhiFEMSolver(work, degree=2, coarse_space=ratio)
        s.assemble(phi, f, uex)
        s.solve(rtol=1e-8, max_iter=100000)
        c.pts, c.nent, kind = work.p2_dof_points(), V.ndofs, BOX_COARSE
    c.s = s
    # a structured system (P2: the generated 3-D box) is assembled straight into the solver formats and holds no CSR copy
    # (`export_csr` re-assembles one); it is the one that keeps its u columns unscaled
    c.structured = not s.info()["has_csr"]
    assert s.stats["converged"] and s.stats["precond"] == kind, s.stats
    ci = s.coarse_info()
    assert ci["coarse_ratio"] == ratio and ci["coarse_dofs"] > 0, ci
    c.ci = ci
    rowptr, col, val, rhs, dof = s.export_csr()
    c.rowptr, c.dof = rowptr, dof
    c.A = sp.csr_matrix((val, col, rowptr), shape=(dof.size,) * 2)
    L = P._lib
    c.perm = np.empty(dof.size, dtype=np.int32)
    L.check(L.lib.phx_system_get_perm(s._sys, L.ptr(c.perm)[0], None, None, 0))
    assert np.array_equal(np.sort(c.perm), np.arange(dof.size))
    c.node_of, c.ainv = s.coarse_export()
    assert c.node_of.size == ci["coarse_dofs"]
    c.R = CR.restriction(c.pts, dof, c.nent, c.node_of, ncubes, ratio, d, layout, c.bcv)
    c.D = CR.scaling(c.A, dof, c.nent, layout, u_unscaled=c.structured)
    c.Ac = CR.galerkin(c.A, c.R)
    c.blk = dof // c.nent
    c.idx = CR.lattice_index(c.pts[dof % c.nent], ncubes, d, CR.steps_per_cube(layout))
    c.elig = CR.eligible(dof, c.nent, d, layout, c.bcv)
    c.m, c.M = CR.coarse_dims(ncubes, ratio, d)
    return c


@pytest.fixture(scope="module")
def cases(P):
    built = {}

    def get(name):
        if name not in built:
            built[name] = build(P, name)
        return built[name]
    yield get
    for c in built.values():
        c.s._free()


def test_refusals(P):
    """No correction, before the first solve, a null pointer, a vector of another length: ValueError, nothing launched."""
    mesh, _, phi = box_case(2, 12)
    f, uD = smooth_data(mesh.x)
    s0 = P.ElasticitySolver(mesh, coarse=0)
    n = s0.assemble(phi, f, uD)["n_active"]
    s0.solve(rtol=1e-8, max_iter=200000)
    v = np.ones(n)
    with pytest.raises(ValueError, match="no coarse correction"):
        s0.coarse_apply(v, v)
    s0._free()
    with pytest.raises(ValueError):
        s0.coarse_apply(v, v)                                  # no system at all
    s1 = P.ElasticitySolver(mesh, coarse=5)
    s1.assemble(phi, f, uD)
    with pytest.raises(ValueError, match="no coarse correction"):
        s1.coarse_apply(v, v)                                  # built on the first solve
    s1.solve(rtol=1e-8, max_iter=200000)
    assert s1.stats["precond"] == VB_COARSE
    for a, b in ((None, v), (v, None), (v[:-1], v), (v, np.ones(n + 1))):
        with pytest.raises(ValueError):
            s1.coarse_apply(a, b)
    s1._free()


@pytest.mark.parametrize("name", IDS)
def test_exports_and_layout(cases, name):
    """What the reference is built from: the node map is the one the specification derives (k_cc_used / k_p2c_used),
    R is a partition of unity on the eligible rows, and the property the case is there for holds."""
    c = cases(name)
    d, n, r = c.d, c.ncubes, c.ratio_h
    nodes = CR.used_nodes(c.pts, c.dof, c.nent, n, r, d, c.layout, c.bcv)
    assert np.array_equal(c.node_of, nodes)
    rs = np.asarray(c.R.sum(axis=1)).ravel()
    assert np.abs(rs[c.elig] - 1.0).max() <= 8 * EPS and np.all(rs[~c.elig] == 0.0)
    assert c.elig.any() and ((~c.elig).any() or c.layout == "p2")   # every active P2 row carries hats
    nf = [n[a] * CR.steps_per_cube(c.layout) + 1 for a in range(d)]
    if c.layout == "p2":
        assert c.structured == (d == 3)                        # 2-D P2 boxes are assembled row by row
    reach = [int(c.idx[c.elig, a].max()) for a in range(d)]
    print(f"{name}: structured {c.structured}, {c.dof.size} active rows, {c.node_of.size} coarse DoFs, nf {nf}, m {c.m[:d]}, kernel ratio {c.r}, "
          f"highest eligible lattice index per axis {reach}")
    if name == "elwd-2d-24-H5":
        assert all(k % r != 0 and (c.m[a] - 1) * r > k for a, k in enumerate(n))
    if name == "elwd-3d-12x10x15-H5":
        assert len(set(nf)) == 3 and c.m[:3] == [4, 3, 4] and len({nf[a] * c.m[a] for a in range(3)}) == 3
    if name == "elwd-3d-12-H6":
        assert all(k % r == 0 for k in n)
    if name == "elwd-2d-72-H8":
        assert nf[0] == 73 > 64
    if name == "p2-2d-40-H5":
        assert nf[0] == 81 > 64
    if c.layout == "p2":
        assert c.ci["coarse_dofs_u"] > 0 and c.ci["coarse_dofs_p"] > 0
        assert c.ci["coarse_dofs_u"] == np.count_nonzero(c.node_of < c.M)
    if c.layout == "interface":
        # eligibility rule of k_cc_positions: a u_in row with a single entry is a Dirichlet row
        dirichlet = np.flatnonzero((c.blk < d) & np.isin(c.dof % c.nent, c.bcv))
        single = np.flatnonzero((np.diff(c.rowptr) == 1) & (c.blk < d))
        assert dirichlet.size > 0 and np.array_equal(dirichlet, single)
        assert all(reach[a] == n[a] - 1 for a in range(d))     # eligible up to the Dirichlet rows of the box faces
        if name == "if-2d-24-H5":
            assert all(reach[a] > (c.m[a] - 2) * r for a in range(d))   # ... inside the cut-short last cell
        # 2 d blocks, every one with coarse DoFs
        assert set(np.unique(c.node_of // c.M)) == set(range(2 * d))
        # the Galerkin check this layout never had
        rel = np.linalg.norm(c.ainv @ c.Ac - np.eye(c.Ac.shape[0])) / np.sqrt(c.Ac.shape[0])
        print(f"{name}: cond(Ac) {np.linalg.cond(c.Ac):.1e}, |Ac^-1 R^T A R - I|_F / sqrt(nc) = {rel:.2e}")
        assert rel <= 1e-8


def to_pos(c, v_act):
    return np.ascontiguousarray(v_act[c.perm])


def to_act(c, v_pos):
    out = np.empty_like(v_pos)
    out[c.perm] = v_pos
    return out


def worst_ratio(err, bound):
    """max err / bound; an entry with a zero bound must be exact."""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    pos = bound > 0
    if np.any(err[~pos] != 0):
        return np.inf
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def apply_checked(c, v, rng, worst, fails, label):
    """One application of v (active-row order) from a random out0; the four stage ratios go to `worst`."""
    out0 = rng.standard_normal(c.dof.size)
    out_pos, gc, zc = c.s.coarse_apply(to_pos(c, v), to_pos(c, out0))
    out = to_act(c, out_pos)
    nc = c.node_of.size
    ratios = {}
    # restriction, against R^T v
    ratios["restriction"] = worst_ratio(np.abs(gc.astype(LD) - CR.rt_dot(c.R, v)),
                                        2 * (3 * (2 * c.r - 1) + 6) * EPS * CR.rt_dot(c.R, np.abs(v)))
    # gemv, on the device's gc
    ratios["gemv"] = worst_ratio(np.abs(zc.astype(LD) - CR.dense_dot(c.ainv, gc)),
                                 2 * nc * EPS * CR.dense_dot(np.abs(c.ainv), np.abs(gc)))
    # prolongation, on the device's zc
    delta = out.astype(LD) - out0.astype(LD)
    Dl = np.asarray(c.D, dtype=LD)
    ratios["prolongation"] = worst_ratio(np.abs(delta - Dl * CR.r_dot(c.R, zc)),
                                         32 * EPS * np.abs(Dl) * CR.r_dot(c.R, np.abs(zc)) + EPS * np.abs(out).astype(LD))
    # end to end
    gref, zref, xref = CR.apply_ref(c.A, c.R, c.D, v, Ac=c.Ac)
    xmax = float(np.abs(xref).max())
    ratios["end to end"] = float(np.abs(delta - xref).max()) / (1e-8 * xmax) if xmax > 0 else (np.inf if np.abs(delta).max() > 0 else 0.0)
    for k, val in ratios.items():
        worst[k] = max(worst.get(k, 0.0), val)
        if not val <= 1.0:
            fails.append(f"{label}: {k} at {val:.3g} of its bound")
    # rows outside the support of R: bit for bit
    if out[~c.elig].tobytes() != out0[~c.elig].tobytes():
        fails.append(f"{label}: a row outside the support of R was written")
    return out, gc, zc, out0


def impulse_rows(c, blk):
    """Eligible rows of block blk with the lowest and the highest lattice index along each axis."""
    rows = np.flatnonzero(c.elig & (c.blk == blk))
    assert rows.size > 0
    picks = []
    for a in range(c.d):
        picks += [rows[np.argmin(c.idx[rows, a])], rows[np.argmax(c.idx[rows, a])]]
    return picks


def rows_without_hats(c):
    """{label: active row that carries no coarse function}."""
    d = c.d
    if c.layout == "elwd":
        return {"p row": np.flatnonzero(c.blk >= d)[0]}
    if c.layout == "interface":
        ny = 2 * d + 2 * d * d
        return {"p row": np.flatnonzero(c.blk >= ny)[0], "y row": np.flatnonzero((c.blk >= 2 * d) & (c.blk < ny))[0],
                "Dirichlet u_in row": np.flatnonzero((c.blk < d) & ~c.elig)[-1]}
    return {}


@pytest.mark.parametrize("name", IDS)
def test_stages(cases, name):
    c = cases(name)
    rng = np.random.default_rng(2024)
    n = c.dof.size
    worst, fails = {}, []
    apply_checked(c, rng.standard_normal(n), rng, worst, fails, "dense")
    last = CR.blocks_with_hats(c.layout, c.d) - 1
    for blk in (0, last):
        for k, row in enumerate(impulse_rows(c, blk)):
            e = np.zeros(n)
            e[row] = 1.0
            apply_checked(c, e, rng, worst, fails, f"impulse block {blk} axis {k // 2} {'low' if k % 2 == 0 else 'high'} "
                                                   f"(lattice {c.idx[row].tolist()})")
    for label, row in rows_without_hats(c).items():
        e = np.zeros(n)
        e[row] = 1.0
        out, gc, zc, out0 = apply_checked(c, e, rng, worst, fails, label)
        if gc.any() or out.tobytes() != out0.tobytes():
            fails.append(f"impulse on a {label}: gc or out changed")
    print(f"{name}: nc {c.node_of.size}, cond(Ac) {np.linalg.cond(c.Ac):.1e}, worst ratio to the bound: "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", IDS)
def test_reproducible(cases, name):
    """No atomics in any pass: two applications of the same vector give identical bytes."""
    c = cases(name)
    rng = np.random.default_rng(7)
    v, out0 = rng.standard_normal(c.dof.size), rng.standard_normal(c.dof.size)   # position order
    a = c.s.coarse_apply(v, out0)
    e = np.zeros(c.dof.size)
    e[np.flatnonzero(c.elig)[0]] = 1.0
    c.s.coarse_apply(to_pos(c, e), out0)                       # something else in X1 / X2 / X3 in between
    b = c.s.coarse_apply(v, out0)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[0].tobytes() != out0.tobytes()


def test_device_pointers(P, cases):
    """The aid with loc = PHX_DEVICE: in, out, gc and zc on the device give the bytes of the host path."""
    import torch
    c = cases("elwd-2d-24-H5")
    L = P._lib
    rng = np.random.default_rng(9)
    v, out0 = rng.standard_normal(c.dof.size), rng.standard_normal(c.dof.size)
    host = c.s.coarse_apply(v, out0)
    dv, dout = torch.as_tensor(v, device="cuda"), torch.as_tensor(out0, device="cuda")
    dgc, dzc = (torch.empty(c.node_of.size, dtype=torch.float64, device="cuda") for _ in range(2))
    L.check(L.lib.phx_coarse_apply(c.s._sys, L.ptr(dv)[0], L.ptr(dout)[0], L.ptr(dgc)[0], L.ptr(dzc)[0], L.DEVICE))
    for x, y in zip(host, (dout, dgc, dzc)):
        assert x.tobytes() == y.cpu().numpy().tobytes()
    assert dv.cpu().numpy().tobytes() == v.tobytes()
