"""The multilevel reference (tests/multilevel_ref.py) on small hierarchies, and the CPU prototype of the claim the
device code is built on: on the adapted meshes of the Doerfler loop, BiCGStab with M^-1 = R V R^T (+) Jacobi takes
fewer iterations than with Jacobi.  Runs without a GPU."""
import functools
import warnings

import numpy as np
import pytest

import estimate_ref as ER
import multilevel_ref as ML
import refine_marked_ref as RM
import refine_ref as RR
from datasets import load_mesh
from oracle import assembly as OA, tagging as OT

EPS = np.finfo(np.float64).eps


# ---- hierarchies ------------------------------------------------------------------------------------------------------
def marked_hierarchy(ctype, x, cells, rounds, point=None, fraction=0.1, uniform_first=False):
    """Levels of `rounds` marked refinements of the cells nearest `point` (after one uniform round if asked)."""
    x, cells = np.asarray(x, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    levels = [dict(ctype=ctype, x=x, cells=cells, pairs=None)]
    if uniform_first:
        pairs = ML.pairs_uniform(ctype, x, cells)
        x, cells = RR.refine_ref(ctype, x, cells)
        levels.append(dict(ctype=ctype, x=x, cells=cells, pairs=pairs))
    lo, hi = x.min(axis=0), x.max(axis=0)
    point = lo + (hi - lo) * np.array([0.37, 0.58, 0.44][:x.shape[1]]) if point is None else point
    for _ in range(rounds):
        ref = RM.refine_marked_ref(ctype, x, cells, cell_marks=RM.nearest_mask(x, cells, point, fraction))
        x, cells = ref["x"], ref["cells"]
        levels.append(dict(ctype=ctype, x=x, cells=cells, pairs=ML.pairs_marked(ref)))
    return levels


def ball_active(x, frac=0.55):
    """Active u DoFs of a made-up system: the vertices inside a ball around the centre (none on the boundary)."""
    c = 0.5 * (x.min(axis=0) + x.max(axis=0))
    r = frac * 0.5 * (x.max(axis=0) - x.min(axis=0)).min()
    return ((x - c) ** 2).sum(axis=1) < r * r


@functools.lru_cache(maxsize=None)
def small(name):
    if name == "disk3":
        return marked_hierarchy(*load_mesh("disk"), 3)
    if name == "disk_empty":
        ctype, x, cells = load_mesh("disk")
        lv = marked_hierarchy(ctype, x, cells, 1)
        ref = RM.refine_marked_ref(ctype, lv[1]["x"], lv[1]["cells"], cell_marks=np.zeros(lv[1]["cells"].shape[0], np.uint8))
        assert ref["x"].shape[0] == lv[1]["x"].shape[0]
        return lv + [dict(ctype=ctype, x=ref["x"], cells=ref["cells"], pairs=ML.pairs_marked(ref))]
    if name == "kuhn3":
        x, cells = RM.kuhn_box(3)
        return marked_hierarchy("tetrahedron", x, cells, 1, uniform_first=True)
    raise KeyError(name)


SMALL = ["disk3", "disk_empty", "kuhn3"]


# ---- transfer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_restriction_is_the_transpose(name):
    levels = small(name)
    rng = np.random.default_rng(2)
    for l in range(1, len(levels)):
        nv, nvf = levels[l - 1]["x"].shape[0], levels[l]["x"].shape[0]
        P = ML.prolongation_matrix(nv, levels[l]["pairs"])
        assert P.shape == (nvf, nv)
        # P is the degree-1 transfer of the refinement references: it reproduces the fine coordinates bit for bit
        assert np.array_equal(P @ levels[l - 1]["x"], levels[l]["x"])
        r, xc = rng.standard_normal((3, nvf)), rng.standard_normal((3, nv))
        got = ML.restrict_ref(nv, levels[l]["pairs"], r)
        assert got.shape == (3, nv)
        assert np.array_equal(ML.restrict_ref(nv, levels[l]["pairs"], r[1]), got[1])
        lhs, rhs = (got * xc).sum(), (r * (P @ xc.T).T).sum()
        scale = np.abs(got * xc).sum() + np.abs(r * (P @ xc.T).T).sum()
        assert abs(lhs - rhs) <= 1e-13 * scale
        # the order of the additions: a row with the entries 1, 2^60, -2^60 tells left-to-right from any other order
        ptr, idx = ML.restriction_csr(nv, levels[l]["pairs"])
        assert np.all(np.diff(idx.astype(np.int64))[np.setdiff1d(np.arange(idx.size - 1), ptr[1:-1] - 1)] > 0)
        rows = np.flatnonzero(np.diff(ptr) >= 2)
        if rows.size:
            p = rows[0]
            v = np.zeros(nvf)
            v[p], v[idx[ptr[p]]], v[idx[ptr[p] + 1]] = 1.0, 2.0 ** 61, -2.0 ** 61
            assert ML.restrict_ref(nv, levels[l]["pairs"], v)[p] == 0.0     # (1 + 2^60) - 2^60 in float64


# ---- level matrices ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_rediscretisation_is_galerkin(name):
    """P^T K_{l+1} P = K_l: for the unconstrained matrices on every row, for the constrained ones on the unconstrained
    rows that no constrained fine vertex reaches (through P and one row of K_{l+1})."""
    levels = small(name)
    ml = ML.Multilevel(levels, ball_active(levels[-1]["x"]))
    for l in range(1, len(levels)):
        P = ml.P[l]
        Kf, Kc = ML.stiffness_full(levels[l]["x"], levels[l]["cells"]), ML.stiffness_full(levels[l - 1]["x"], levels[l - 1]["cells"])
        E = (P.T @ Kf @ P - Kc).toarray()
        assert np.abs(E).max() <= 1e-13 * np.abs(Kc.toarray()).max()
        cf, cc = ml.cons[l], ml.cons[l - 1]
        Pm = sp_free(cf) @ P @ sp_free(cc)
        E = (Pm.T @ ml.K[l] @ Pm - ml.K[l - 1]).toarray()
        reach = (abs(P).T @ (abs(ml.K[l]) @ cf.astype(float) + cf.astype(float))) > 0
        rows = ~cc & ~np.asarray(reach).reshape(-1)
        assert rows.sum() > 0
        assert np.abs(E[rows]).max() <= 1e-13 * np.abs(ml.K[l - 1].toarray()).max()


def sp_free(cons):
    import scipy.sparse as sp
    return sp.diags((~cons).astype(np.float64))


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("coarse", [0, 1])
def test_vcycle_is_spd_and_contracts(name, coarse):
    levels = small(name)
    ml = ML.Multilevel(levels, ball_active(levels[-1]["x"]), coarse=coarse)
    V = ml.dense()
    assert np.abs(V - V.T).max() <= 1e-13 * np.abs(V).max()
    lam = np.linalg.eigvalsh(0.5 * (V + V.T))
    assert lam.min() > 0.0
    rho = np.abs(np.linalg.eigvals(np.eye(V.shape[0]) - V @ ml.K[-1].toarray())).max()
    print(f"[{name} coarse kind {coarse}] levels {ml.nv}: rho(I - V K_L) = {rho:.4f}, cond(V K) <= {1.0 / (1.0 - rho):.2f}")
    assert rho < 1.0


def test_no_constraint_is_refused():
    levels = small("disk3")
    with pytest.raises(ValueError):
        ML.Multilevel(levels, np.ones(levels[-1]["x"].shape[0], dtype=bool))


# ---- the CPU prototype of the claim -------------------------------------------------------------------------------------
def disk_problem(x):
    ctype, x0, _ = load_mesh("disk")
    cen = x0.mean(axis=0) + np.array([0.013, -0.007])
    r = 0.62 * 0.5 * (x0.max(axis=0) - x0.min(axis=0)).min()
    phi = ((x - cen) ** 2).sum(axis=1) - r ** 2
    uD = np.sin(x[:, 0]) * np.cos(x[:, 1])
    return phi, 2.0 * uD, uD


def wd_system(ctype, x, cells):
    """The weak-Dirichlet system of oracle/assembly.py on the mesh -> dict with the active block in the order
    (u DoFs by vertex, p DoFs by vertex)."""
    phi, f, uD = disk_problem(x)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ct, ft, _, meas, _, topo = OT.compute_tags_measures(ctype, x, cells, OT.NodalP1(phi), 1, box_mode=True,
                                                            single_layer_cut=True, warn=False)
    tags = np.zeros(topo.nc, dtype=np.int32)
    tags[ct.indices] = ct.values
    ftags = np.zeros(topo.nf, dtype=np.int32)
    ftags[ft.indices] = ft.values
    A, b, act = OA.assemble_poisson_wd(topo, x, tags, ftags, meas(100), phi, f, uD)
    nv = x.shape[0]
    idx = np.flatnonzero(act)
    u_vertex = idx[idx < nv]
    Aa = A[idx][:, idx].tocsr()
    return dict(A=Aa, b=b[idx], idx=idx, u_vertex=u_vertex, nu=u_vertex.size, nv=nv, tags=tags, phi=phi, f=f, uD=uD,
                active_u=act[:nv], full=(A, b, act))


@functools.lru_cache(maxsize=None)
def dorfler_loop(rounds=5, theta=0.5):
    """The loop of demo/weak-dirichlet/adapt.py on the CPU -> (levels, systems), one entry per mesh 0 .. rounds."""
    ctype, x, cells = load_mesh("disk")
    x, cells = np.asarray(x, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    levels, systems = [dict(ctype=ctype, x=x, cells=cells, pairs=None)], []
    for rnd in range(rounds + 1):
        S = wd_system(ctype, x, cells)
        systems.append(S)
        if rnd == rounds:
            break
        w = OA.solve_direct(*S["full"])
        nv = x.shape[0]
        parts, _ = ER.estimate_ref(ctype, x, cells, S["tags"], 1, w[:nv], w[nv:], S["phi"], S["f"], S["uD"])
        ref = RM.refine_marked_ref(ctype, x, cells, cell_marks=ER.mark_dorfler_ref(parts.sum(axis=0), theta))
        x, cells = ref["x"], ref["cells"]
        levels.append(dict(ctype=ctype, x=x, cells=cells, pairs=ML.pairs_marked(ref)))
    return levels, systems


def test_cpu_prototype_fewer_iterations_than_jacobi():
    levels, systems = dorfler_loop()
    jac, mlv = [], []
    for l, S in enumerate(systems):
        d = S["A"].diagonal()
        xj, itj, okj = ML.bicgstab(S["A"], S["b"], lambda r: r / d)
        assert okj
        jac.append(itj)
        if l == 0:
            mlv.append(None)                                   # no parent: nothing to build
            continue
        ml = ML.Multilevel(levels[:l + 1], S["active_u"])
        xm, itm, okm = ML.bicgstab(S["A"], S["b"], ML.minv(ml, S["u_vertex"], d[S["nu"]:]))
        assert okm
        for xk in (xj, xm):                                    # the recursive residual has not drifted from the true one
            assert np.linalg.norm(S["b"] - S["A"] @ xk) <= 10 * 1e-8 * np.linalg.norm(S["b"])
        mlv.append(itm)
    print("cells     ", [lv["cells"].shape[0] for lv in levels])
    print("active    ", [S["A"].shape[0] for S in systems])
    print("Jacobi    ", jac)
    print("multilevel", mlv)
    for l in (len(systems) - 2, len(systems) - 1):
        assert mlv[l] < jac[l], (l, mlv, jac)

