"""The specification of gradient recovery (tests/recover_ref.py) and the input conditions of tests/test_hip_recover.py,
on the CPU: reproduction of polynomials, the closed-form indicator against Gauss-Legendre rules, and per mesh and mask
the conditions the GPU tests rely on (cell counts, tags, partly selected stars, long stars, marking margins)."""
import numpy as np
import pytest

import estimate_cases as EC
import estimate_ref as ER
import recover_cases as RC
import recover_ref as RR

TOL = 1e-12


def degrees(name):
    return (1,) if RC.arrays(name)[0] == "quadrilateral" else (1, 2)


CASES = [(n, k) for n in RC.MESHES for k in degrees(n)]


def setup(name, degree):
    ctype, x, cells = RC.arrays(name)
    pts, c2e = RC.dof_points(ctype, x, cells, degree)
    return ctype, x, cells, pts, c2e, RR.omega_mask(RC.oracle_tags(name))


# ---- reproduction -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,degree", CASES)
def test_polynomials_are_reproduced(name, degree):
    """u affine at k = 1, quadratic at k = 2: G = grad u at every vertex with a star, eta2 = 0."""
    ctype, x, cells, pts, c2e, mask = setup(name, degree)
    d = x.shape[1]
    rng = np.random.default_rng(3)
    a = rng.uniform(-1.0, 1.0, size=d)
    H = rng.uniform(-1.0, 1.0, size=(d, d))
    H = 0.5 * (H + H.T) if degree == 2 else np.zeros((d, d))
    u = 0.3 + pts @ a + 0.5 * np.einsum("pi,ij,pj->p", pts, H, pts)
    exact = a + x @ H
    for m in (mask, np.ones_like(mask)):
        r = RR.recover_ref(ctype, x, cells, degree, u, m, c2e)
        star = RR.star_lengths(x.shape[0], cells, m)[0] > 0
        assert star.any() and r.G.shape == (x.shape[0], d)
        assert np.abs(r.G[star] - exact[star]).max() <= TOL * r.G_scale.max()
        assert np.all(r.G[~star] == 0.0)
        assert r.eta2.max() <= TOL * r.eta2_scale.max()
        assert np.all(r.eta2[~m.astype(bool)] == 0.0)


# ---- the independent rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,degree", CASES)
def test_closed_form_agrees_with_gauss_rules(name, degree):
    ctype, x, cells, pts, c2e, mask = setup(name, degree)
    for ncomp in (None, x.shape[1]) if name in RC.VECTOR else (None,):
        u = RC.field(x, pts, ncomp)
        r = RR.recover_ref(ctype, x, cells, degree, u, mask, c2e)
        q = RR.eta2_quadrature(ctype, x, cells, degree, u, mask, r.G, c2e)
        assert r.eta2.max() > 0.0
        assert np.abs(q - r.eta2).max() <= TOL * r.eta2_scale.max()
        assert r.G.shape == (() if ncomp is None else (ncomp,)) + x.shape


def test_vector_fields_are_component_wise():
    ctype, x, cells, pts, c2e, mask = setup("disk", 2)
    u = RC.field(x, pts, 2)
    r = RR.recover_ref(ctype, x, cells, 2, u, mask, c2e)
    parts = [RR.recover_ref(ctype, x, cells, 2, u[k], mask, c2e) for k in range(2)]
    assert np.array_equal(r.G, np.stack([p.G for p in parts]))
    assert np.abs(r.eta2 - (parts[0].eta2 + parts[1].eta2)).max() <= TOL * r.eta2_scale.max()


def test_unsupported_spaces_are_refused():
    ctype, x, cells = RC.arrays("disk")
    with pytest.raises(NotImplementedError):
        RR.recover_ref(ctype, x, cells, 3, np.zeros(x.shape[0]), np.ones(cells.shape[0], dtype=np.uint8))
    ctype, x, cells = RC.arrays("square_quad")
    with pytest.raises(NotImplementedError):
        RR.recover_ref(ctype, x, cells, 2, np.zeros(x.shape[0]), np.ones(cells.shape[0], dtype=np.uint8))


# ---- input conditions of the GPU tests ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.MESHES)
def test_input_conditions(name):
    ctype, x, cells = RC.arrays(name)
    tags = RC.oracle_tags(name)
    mask = RR.omega_mask(tags)
    nc = cells.shape[0]
    assert nc > 64 and nc % 64 != 0
    assert all((tags == t).any() for t in (1, 2, 3))
    sel, full = RR.star_lengths(x.shape[0], cells, mask)
    partly = int(((sel > 0) & (sel < full)).sum())
    print(f"{name}: {nc} cells, {int(mask.sum())} in Omega_h, longest selected star {sel.max()}, {partly} partly selected "
          f"vertices, {int((sel == 0).sum())} vertices without a selected star")
    assert partly > 0, "no vertex whose star is only partly in S"
    assert (sel == 0).any(), "every vertex has a selected star: the exact zeros are not exercised"
    if name in RC.HUBS:
        hub = int(np.argmax(full))
        assert full[hub] > 64 and sel[hub] == full[hub], "the hub's star is not wholly selected"


def test_issue_table():
    """The figures the cases were chosen by."""
    want = {"flux_2d": (558, 80, 36), "p2_3d": (826, 76, 46)}
    for name, (nc, longest, partly) in want.items():
        ctype, x, cells = RC.arrays(name)
        sel, full = RR.star_lengths(x.shape[0], cells, RR.omega_mask(RC.oracle_tags(name)))
        assert (cells.shape[0], int(sel.max()), int(((sel > 0) & (sel < full)).sum())) == (nc, longest, partly)
    for name in EC.MESHES:
        ctype, x, cells = RC.arrays(name)
        sel, full = RR.star_lengths(x.shape[0], cells, RR.omega_mask(RC.oracle_tags(name)))
        assert 20 <= int(((sel > 0) & (sel < full)).sum()) <= 146


@pytest.mark.parametrize("name,degree", RC.MARK_MESHES)
def test_marking_margins(name, degree):
    ctype, x, cells, pts, c2e, mask = setup(name, degree)
    r = RR.recover_ref(ctype, x, cells, degree, RC.field(x, pts), mask, c2e)
    for theta in RC.MARK_THETAS:
        margin = ER.dorfler_margin(r.eta2, theta)
        print(f"{name} k={degree} theta={theta}: margin {margin:.2e}")
        assert margin > 1e-9, "input condition: a partial sum sits at the threshold (change the field's seed)"
