"""The specification of the error indicator and of the Doerfler selection (tests/estimate_ref.py) agrees with itself,
and the inputs of tests/test_hip_estimate.py meet the conditions that file relies on.  No GPU."""
import warnings

import numpy as np
import pytest

import estimate_cases as EC
import estimate_ref as ER

CASES = [(name, k) for name in EC.MESHES for k in EC.degrees(EC.arrays(name)[0])]


def setup_case(name, degree, seed=5):
    ctype, x, cells = EC.arrays(name)
    pts, c2e = EC.dof_points(ctype, x, cells, degree)
    return ctype, x, cells, EC.oracle_tags(name), pts, c2e, EC.nodal_fields(x, pts, seed, EC.RADIUS_FACTOR.get(name, 0.62))


def ref(ctype, x, cells, tags, degree, F, c2e, fn=ER.estimate_ref):
    return fn(ctype, x, cells, tags, degree, F["u"], F["p"], F["phi"], F["f"], F["ud"], c2e)


@pytest.mark.parametrize("name", EC.MESHES)
def test_input_condition_tags(name):
    """Every test tagging holds cells tagged 1, 2 and 3; every mesh has more than 64 cells, no multiple of 64."""
    ctype, x, cells = EC.arrays(name)
    tags = EC.oracle_tags(name)
    assert all((tags == t).any() for t in (1, 2, 3)), np.bincount(tags, minlength=4)
    assert cells.shape[0] > 64 and cells.shape[0] % 64 != 0


@pytest.mark.parametrize("name,degree", CASES)
def test_affine_function_has_no_jump(name, degree):
    ctype, x, cells, tags, pts, c2e, F = setup_case(name, degree)
    F["u"] = 0.3 + pts @ (0.7 * np.arange(1, x.shape[1] + 1))
    parts, scales = ref(ctype, x, cells, tags, degree, F, c2e)
    assert scales[1].max() > 0.0
    assert np.abs(parts[1]).max() <= 1e-13 * scales[1].max()


@pytest.mark.parametrize("name,degree", CASES)
def test_boundary_term_vanishes_for_the_constructed_function(name, degree):
    """u_h = phi_h p_h / h_T + u_D on ONE cut cell (p_h a constant, so that the product stays in the space): B = 0."""
    ctype, x, cells, tags, pts, c2e, F = setup_case(name, degree)
    c = int(np.flatnonzero(tags == 2)[0])
    h = ER.cell_diameters(x, cells)[c]
    F["p"] = np.full(pts.shape[0], 0.37)
    F["u"] = F["phi"] * 0.37 / h + F["ud"]        # nodal values: u_h = 0.37 phi_h / h_T + u_D,h since sum N_i = 1
    parts, scales = ref(ctype, x, cells, tags, degree, F, c2e)
    assert scales[2, c] > 0.0 and abs(parts[2, c]) <= 1e-13 * scales[2, c]
    others = np.flatnonzero(tags == 2)[1:]
    assert others.size == 0 or parts[2, others].max() > 0.0       # h_T differs from cell to cell: no accident elsewhere


@pytest.mark.parametrize("name", [n for n in EC.MESHES if EC.arrays(n)[0] != "quadrilateral"])
def test_p1_residual_is_the_mass_matrix_form(name):
    ctype, x, cells, tags, pts, c2e, F = setup_case(name, 1)
    parts, scales = ref(ctype, x, cells, tags, 1, F, c2e)
    _, vol, h = ER.simplex_geometry(x, cells)
    M = ER.p1_mass_matrix(x.shape[1], vol)
    fT = F["f"][cells]
    want = h ** 2 * np.einsum("ci,cij,cj->c", fT, M, fT) * ((tags == 1) | (tags == 2))
    assert np.abs(parts[0] - want).max() <= 1e-13 * scales[0].max()


@pytest.mark.parametrize("name", [n for n in EC.MESHES if EC.arrays(n)[0] != "quadrilateral"])
def test_p1_closed_form_equals_quadrature(name):
    ctype, x, cells, tags, pts, c2e, F = setup_case(name, 1)
    pa, sa = ref(ctype, x, cells, tags, 1, F, c2e, ER.estimate_ref)
    pb, sb = ref(ctype, x, cells, tags, 1, F, c2e, ER.estimate_quadrature)
    for k in range(3):
        assert np.abs(pa[k] - pb[k]).max() <= 1e-13 * sa[k].max()
        assert np.abs(sa[k] - sb[k]).max() <= 1e-13 * sa[k].max()


@pytest.mark.parametrize("name,degree", CASES)
def test_cell_sum_of_jumps_equals_the_facet_sum(name, degree):
    """sum_T J_T = sum over the interior facets of Omega_h of h_F int_F [d_n u_h]^2: one half, twice."""
    ctype, x, cells, tags, pts, c2e, F = setup_case(name, degree)
    parts, scales = ref(ctype, x, cells, tags, degree, F, c2e)
    facetwise = ER.facet_sum_ref(ctype, x, cells, tags, degree, F["u"], c2e)
    assert facetwise > 0.0
    assert abs(parts[1].sum() - facetwise) <= 1e-12 * scales[1].sum()
    # facets towards cells tagged 3 and mesh-boundary facets carry nothing
    T, _, nb, topo = ER.facet_terms(ctype, x, cells, tags, degree, F["u"], c2e)
    other = np.where(topo.f2c[topo.c2f][..., 0] == np.arange(topo.nc)[:, None], topo.f2c[topo.c2f][..., 1],
                     topo.f2c[topo.c2f][..., 0])
    dead = (other < 0) | (tags[np.maximum(other, 0)] == 3) | (tags[np.maximum(other, 0)] == 0) | (tags == 3)[:, None]
    assert dead.any() and np.all(T[dead] == 0.0) and np.all(nb[dead] == -1)


@pytest.mark.parametrize("name,degree", CASES)
def test_doubling_the_data_quadruples_every_part(name, degree):
    """Every part is a square of something linear in (u_h, f_h, u_D) and in the PRODUCT phi_h p_h: doubling u_h, p_h,
    f_h, u_D (the level-set, which is geometry, kept) multiplies every part by 4 exactly -- scaling by 2 commits no
    rounding.  Doubling phi_h as well doubles the product once more: R and J still quadruple exactly, and B is 4 times
    the B of (u_h, 2 p_h, phi_h, f_h, u_D)."""
    ctype, x, cells, tags, pts, c2e, F = setup_case(name, degree)
    parts, _ = ref(ctype, x, cells, tags, degree, F, c2e)
    G = {k: (v if k == "phi" else 2.0 * v) for k, v in F.items()}
    parts2, _ = ref(ctype, x, cells, tags, degree, G, c2e)
    assert np.array_equal(parts2, 4.0 * parts)
    H = {k: 2.0 * v for k, v in F.items()}
    parts3, _ = ref(ctype, x, cells, tags, degree, H, c2e)
    Fp = dict(F, p=2.0 * F["p"])
    parts4, _ = ref(ctype, x, cells, tags, degree, Fp, c2e)
    assert np.array_equal(parts3[:2], 4.0 * parts[:2]) and np.array_equal(parts3[2], 4.0 * parts4[2])
    assert (parts[:, (tags == 3)] == 0.0).all() and (parts[2, tags == 1] == 0.0).all()


# ---- Doerfler ---------------------------------------------------------------------------------------------------------
def test_marking_reference_on_a_hand_example():
    eta2 = np.array([1.0, 4.0, 0.0, 4.0, 1.0])                 # order: 1, 3, 0, 4, 2; sums 4, 8, 9, 10, 10
    assert ER.mark_dorfler_ref(eta2, 0.4).tolist() == [0, 1, 0, 0, 0]
    assert ER.mark_dorfler_ref(eta2, 0.5).tolist() == [0, 1, 0, 1, 0]
    assert ER.mark_dorfler_ref(eta2, 0.85).tolist() == [1, 1, 0, 1, 0]
    assert ER.mark_dorfler_ref(eta2, 1.0).tolist() == [1, 1, 0, 1, 1]
    assert ER.mark_dorfler_ref(np.zeros(4), 0.5).tolist() == [0, 0, 0, 0]
    assert ER.dorfler_margin(eta2, 0.5) == pytest.approx(0.1)
    assert ER.dorfler_margin(np.zeros(3), 0.5) == float("inf")


@pytest.mark.parametrize("n", EC.MARK_LENGTHS)
def test_integer_indicators_are_what_the_gpu_test_says(n):
    v = EC.integer_indicators(n, "ties")
    assert v.shape == (n,) and np.all(v == np.round(v)) and v.min() >= 0.0 and v.sum() > 0.0 and v.sum() < 2 ** 50
    if n >= 8:
        assert v[0] == 0.0 and v[-1] == 0.0 and (np.diff(v) == 0.0).sum() >= n // 2
    for theta in EC.MARK_THETAS:
        m = ER.mark_dorfler_ref(v, theta)
        assert m.sum() >= 1 and not m[v == 0.0].any()
        if theta == 1.0:
            assert np.array_equal(m.astype(bool), v > 0.0)
    assert not ER.mark_dorfler_ref(EC.integer_indicators(n, "zeros"), 0.5).any()


def solved_p1_indicator():
    """The oracle's P1 solve of the demo problem on `disk` and its indicator: the CPU counterpart of the solved case."""
    from oracle import assembly as OA, tagging as OT
    from oracle.topology import Topology
    ctype, x, cells = EC.arrays("disk")
    topo = Topology(ctype, cells, x.shape[0])
    phi = EC.levelset(x, x)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ct, ft, _, meas, _, _ = OT.compute_tags_measures(ctype, x, topo, OT.NodalP1(phi), 1, box_mode=True,
                                                         single_layer_cut=True)
    cv = np.zeros(topo.nc, dtype=np.int64)
    cv[ct.indices] = ct.values
    uex = np.sin(x[:, 0]) * np.cos(x[:, 1])
    A, b, act = OA.assemble_poisson_wd(topo, x, cv, ft.values, meas(100), phi, 2.0 * uex, uex)
    w = OA.solve_direct(A, b, act)
    nv = x.shape[0]
    return ER.estimate_ref(ctype, x, cells, cv, 1, w[:nv], w[nv:], phi, 2.0 * uex, uex), cv


def test_input_condition_margin_of_the_solved_indicator():
    (parts, scales), cv = solved_p1_indicator()
    eta2 = parts.sum(axis=0)
    assert eta2.min() >= 0.0 and (eta2[(cv == 1) | (cv == 2)] > 0.0).all()
    for theta in (0.3, 0.5, 0.8):
        assert ER.dorfler_margin(eta2, theta) > 1e-9
    # the case the scale is for: the boundary term of a solved problem is small against its scale
    cut = cv == 2
    assert parts[2, cut].max() < 1e-2 * scales[2, cut].max()
