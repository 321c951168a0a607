"""The vector phases and scalar recurrences of the BiCGStab loop, one phase at a time, against tests/krylov_ref.py.

Phase API, mode 1 (`phx_krylov_phase` through `dist_solver.HipBackend`).  After KR_BEGIN / KR_BEGIN2 the workspace and
the scalars belong to the test: all ten vectors are written (a different seeded normal in each, so a read from the wrong
buffer shows), the 16 head scalars too -- in mode 1 `dotv` returns S[R_OFF + q], so the dot products a phase consumes
are the test's choice --, ONE phase runs, and everything is read back and compared with the float64 statement of that
phase.  There is no trajectory, so the bounds are those of single expressions:

  unwritten     every vector the phase does not write keeps its bits, the u rows of phat / shat (pre-set to NaN) included
  ownership     unowned rows of written vectors are exactly 0.0; unowned rows of y keep their bits
  entries       |got - ref| <= 4 eps sum |terms| of that entry's expression (|r_i| + |alpha v_i| for s, |y_i| + |alpha
                phat_i| + |omega shat_i| for y, |r_i| + |beta p_i| + |beta omega v_i| for p, ...): two to four roundings
                of eps / 2 each, with or without FMA contraction, i.e. 2 eps sum |terms|, doubled as in
                test_hip_stencil_paths.py
  RestOut       the rows outside the u block of phat / shat equal the device's own p / s bit for bit
  scalars       one division or one copy: within 1 ulp (eps |ref|); the rest of the head keeps its bits
  dot products  against math.fsum of the reference terms, to sum |a| |delta b| (the entry bounds) + n eps sum |a b|
                (test_spmv_phase_dot_products)
  finish        C y at dof[perm] to 1 ulp (eps |ref|, one rounding for 1 / A_ii and one for the product, against a
                numpy.longdouble reference), exactly 0 elsewhere

Systems: the smallest that reach each branch of `kr_vecs` / `RestOut`; every case first asserts through
`phx_precond_info`, `precond_active()` and `info()` that it did.  The `plane_map` shape of test_hip_stencil_paths.py has
more than 2048 * 256 rows, the cap of `vec_grid`: the grid-stride loops of the vector kernels take a second trip there.
Every other case has n_active % 256 != 0 (a partial last block).  Ownership: all rows, a seeded random half, the upper
half of the solver order unowned; input vectors are zero on unowned rows, as the loop guarantees (y excepted).

Phases 52 - 63 (identity and reduced loop) are refused by the phase API before any launch; that refusal is all this file
asks of them.  The SpMV phases are pinned by test_hip_stencil_paths.py, the preconditioner phases by
test_hip_precond_operator.py, the native loops by test_hip_krylov_loops.py."""
import math

import numpy as np
import pytest

import krylov_ref as K
from test_hip_precond_operator import BOX, SETS, Applied, ball, elasticity_system, weak_system
from test_hip_stencil_paths import SHAPES

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
VEC_GRID_ROWS = 2048 * 256          # vec_grid: at most 2048 blocks of 256 threads
UNASSIGNED_PHASES = (-1, 14, 19, 22, 29, 34, 39, 42, 51, 64)   # next to every run of assigned numbers of KrPhase


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


# ---- systems ------------------------------------------------------------------------------------------------------------
def _expect(kind, hat, rest, structured=None, u_first=None, p2=False):
    return dict(kind=kind, hat=hat, rest=rest, structured=structured, u_first=u_first, p2=p2)


CASES = {
    # phat aliases p, shat aliases s: entries 8 and 9 of the workspace are never touched
    "jacobi_submesh": (lambda P, det: weak_system(P, *BOX, [8] * 3, SETS["sphere"], precond=0, submesh=True,
                                                  deterministic=det),
                       _expect(0, False, False, structured=False)),
    # RestOut with perm == nullptr: rows i >= nu
    "box_p1_lattice": (lambda P, det: weak_system(P, *BOX, [12] * 3, SETS["sphere"], deterministic=det),
                       _expect(1, True, True, structured=True, u_first=True)),
    # RestOut through perm[i] >= nu
    "submesh_lattice": (lambda P, det: weak_system(P, *BOX, [16] * 3, SETS["offset_ellipsoid"], submesh=True,
                                                   deterministic=det),
                        _expect(1, True, True, structured=False, u_first=False)),
    # vertex blocks: phat apart from p, no RestOut
    "elasticity_2d": (lambda P, det: elasticity_system(P, 2, 16, 1.0, False), _expect(2, True, False)),
    # u_p2_block.  Always deterministic: the CSR of a P2 system is a re-assembly, and only then does its diagonal carry
    # the bits of the solver's own (the 1 ulp of `finish` is measured against it)
    "box_p2_lattice": (lambda P, det: weak_system(P, *BOX, [8] * 3, ball([0.03, -0.02, 0.01]), degree=2, kphi=2,
                                                  deterministic=True),
                       _expect(1, True, True, p2=True)),
}
MASKS = {
    "all": None,
    "random_half": lambda ap: np.random.default_rng(12).random(ap.n) < 0.5,
    "upper_half_unowned": lambda ap: np.arange(ap.n) < ap.n // 2,
}


def open_case(P, name, mask, deterministic=False):
    build, ex = CASES[name]
    c = build(P, deterministic)
    ap = Applied(P, c, own_fn=MASKS[mask])
    info = ap.info
    assert ap.kind == ex["kind"] and ap.hat == ex["hat"], (name, ap.kind, ap.hat)
    assert ap.n % 256 != 0, (name, ap.n)
    if ex["kind"] == 1:
        assert ap.vbytes == 8
    if ex["structured"] is not None:
        assert (info["stencil_rows"] > 0) == ex["structured"], (name, info)
    if ex["u_first"] is not None:
        # structured systems keep the u rows first in solver order (RestOut: i >= nu); a sub-mesh does not
        assert np.array_equal(ap.is_u, np.arange(ap.n) < info["n_active_u"]) == ex["u_first"], name
    if ex["p2"]:
        assert c.p2 and (c.ijk[ap.ent[ap.is_u]] % 2 == 1).any()      # edge midpoints among the active u rows
    rest = ~ap.is_u if ex["rest"] else None
    if rest is not None:
        assert rest.any() and not rest.all()
    return ap, rest, ex


# ---- one phase ----------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def make_state(ap, rest, seed, finite_hats):
    """Ten different normals, zero on unowned rows (y keeps its values there).  phat / shat: NaN on the rows no vector
    phase writes (the u rows with RestOut, every row without) unless the phase reads them; where p / s stand in for
    them, entries 8 and 9 of the workspace are NaN throughout."""
    rng = np.random.default_rng(seed)
    own = ap.own_np
    V = {}
    for k in K.NAMES:
        a = rng.standard_normal(ap.n)
        V[k] = a if k == "y" else np.where(own, a, 0.0)
    for k in ("phat", "shat"):
        if not ap.hat:
            V[k] = np.full(ap.n, np.nan)
        elif not finite_hats:
            V[k] = np.where(~rest, np.nan, V[k]) if rest is not None else np.full(ap.n, np.nan)
    return V


def make_head(seed):
    rng = np.random.default_rng(1000 + seed)
    S = np.zeros(K.HEAD)
    S[:] = rng.uniform(0.5, 2.0, K.HEAD) * rng.choice([-1.0, 1.0], K.HEAD)
    S[K.S_MODE] = 1.0
    S[K.S_RESTARTS] = 3.0
    for q in (K.R_TT, K.R_SS, K.R_RR):
        S[K.R_OFF + q] = abs(S[K.R_OFF + q])
    S[K.S_BB], S[K.S_RR] = abs(S[K.S_BB]), abs(S[K.S_RR])
    return S


def run_phase(ap, phase, V0, S0):
    torch = ap.torch
    w = np.concatenate([V0[k] for k in K.NAMES])
    ap.work.copy_(torch.from_numpy(w).to(ap.dev))
    ap.scal[:K.HEAD].copy_(torch.from_numpy(S0).to(ap.dev))
    torch.cuda.synchronize(ap.dev)
    ap.b.phase(phase)
    V1 = ap.read()
    S1 = ap.scal[:K.HEAD].cpu().numpy().copy()
    return V1, S1


def entry_bounds(phase, V0, S0, Sref, hat, restarted):
    """sum |terms| of the expression behind every written entry (without the factor 4 eps)."""
    a = np.abs
    if phase == K.KR_UPDATE_S:
        return {"s": a(V0["r"]) + a(Sref[K.S_ALPHA] * V0["v"])}
    if phase == K.KR_UPDATE_XR:
        ph, sh = (V0["phat"], V0["shat"]) if hat else (V0["p"], V0["s"])
        al, om = S0[K.S_ALPHA], Sref[K.S_OMEGA]
        return {"y": a(V0["y"]) + a(al * ph) + a(om * sh), "r": a(V0["s"]) + a(om * V0["t"])}
    if phase == K.KR_UPDATE_P and not restarted:
        beta = (S0[K.R_OFF + K.R_RHO] / S0[K.S_RHO]) * (S0[K.S_ALPHA] / S0[K.S_OMEGA])
        return {"p": a(V0["r"]) + a(beta * V0["p"]) + a(beta * S0[K.S_OMEGA] * V0["v"])}
    if phase == K.KR_TRUE_RESIDUAL:
        return {"r": a(V0["b"]) + a(V0["t"])}
    return {}      # copies: exact


def check_phase(ap, rest, phase, V0, S0, what, **kw):
    """Runs `phase` on (V0, S0) and holds the outcome against krylov_ref; returns (V1, S1, the reference's scalars, worst ratio to a bound)."""
    own, n = ap.own_np, ap.n
    V1, S1 = run_phase(ap, phase, V0, S0)
    Vr, Sr = K.PHASES[phase](V0, S0, own, rest, ap.hat, **kw)
    wrote = K.written(V0, Vr)
    restarted = Sr[K.S_RESTARTS] != S0[K.S_RESTARTS] and phase == K.KR_UPDATE_P
    bounds = entry_bounds(phase, V0, S0, Sr, ap.hat, restarted)
    worst = 0.0
    delta = {}
    for k in K.NAMES:
        if k not in wrote:
            assert same_bits(V1[k], V0[k]), f"{what}: {k} was written ({np.flatnonzero(bits(V1[k]) != bits(V0[k]))[:8]})"
            continue
        if k in ("phat", "shat"):
            # RestOut: the rows outside the u block hold the device's own p / s bit for bit, the u rows keep theirs
            src = {"phat": "p", "shat": "s"}[k]
            if phase == K.KR_RESTART or restarted:
                src = "r"
            assert same_bits(V1[k][rest], V1[src][rest]), f"{what}: {k} differs from {src} on the RestOut rows"
            assert same_bits(V1[k][~rest], V0[k][~rest]), f"{what}: u rows of {k} were written"
            continue
        if k == "y" and phase != K.KR_BEGIN:
            assert same_bits(V1[k][~own], V0[k][~own]), f"{what}: unowned rows of y changed"
        else:
            assert np.all(V1[k][~own] == 0.0), f"{what}: unowned rows of {k} are not 0.0"
        err = np.abs(V1[k] - Vr[k])
        if k in bounds:
            tol = 4 * EPS * bounds[k]
            bad = np.flatnonzero(~(err <= tol))
            assert bad.size == 0, f"{what}: {k} rows {bad[:8].tolist()} err {err[bad[:4]]} tol {tol[bad[:4]]}"
            worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))
            delta[k] = tol
        else:
            assert same_bits(V1[k], Vr[k]), f"{what}: {k} is a copy and differs ({np.flatnonzero(err != 0)[:8]})"
            delta[k] = np.zeros(n)
    # scalars: the dot products of phases 0, 5, 12 by their own bound, everything else to 1 ulp or untouched
    dots = {}
    if phase == K.KR_BEGIN:
        dots[K.R_RHO] = ("b", "b")
    elif phase == K.KR_UPDATE_XR:
        dots[K.R_RHO], dots[K.R_RR] = ("rhat", "r"), ("r", "r")
    elif phase == K.KR_TRUE_RESIDUAL:
        dots[K.R_RR] = ("r", "r")
    for q, (x, y) in dots.items():
        ax, ay = Vr[x], Vr[y]
        ref = math.fsum((ax * ay).tolist())
        dx = delta.get(x, np.zeros(n))
        dy = delta.get(y, np.zeros(n))
        tol = float(np.abs(ax) @ dy + (np.abs(ay) + dy) @ dx) + n * EPS * float(np.abs(ax) @ np.abs(ay))
        got = S1[K.R_OFF + q]
        assert abs(got - ref) <= tol, f"{what}: R[{q}] = {got!r} vs {ref!r} (tol {tol:.3e})"
        worst = max(worst, abs(got - ref) / tol)
    for i in range(K.HEAD):
        if i - K.R_OFF in dots:
            continue
        if Sr[i] == S0[i] and phase != K.KR_BEGIN:
            assert same_bits(S1[i:i + 1], S0[i:i + 1]), f"{what}: S[{i}] {S0[i]!r} -> {S1[i]!r}"
        else:
            assert abs(S1[i] - Sr[i]) <= EPS * abs(Sr[i]), f"{what}: S[{i}] = {S1[i]!r} vs {Sr[i]!r}"
            if Sr[i] != 0.0:
                worst = max(worst, abs(S1[i] - Sr[i]) / (EPS * abs(Sr[i])))
    return V1, S1, Sr, worst


def all_phases(ap, rest, name, repeat=False):
    """Every vector phase once on inputs of the test's choice; KR_UPDATE_P in its three settings.  repeat: each phase a
    second time from the same inputs, bit for bit (PHX_OPT_DETERMINISTIC)."""
    D = ap.D
    worst = {}
    veto = 0.0 if ap.kind == 1 else 1.0        # box_precond_setup: no veto where the lattice was built
    rhs = ap.rhs[ap.perm]

    def go(tag, phase, V0, S0, **kw):
        V1, S1, Sr, w = check_phase(ap, rest, phase, V0, S0, f"{name} {tag}", **kw)
        worst[tag] = w
        if repeat:
            V2, S2 = run_phase(ap, phase, V0, S0)
            assert all(same_bits(V1[k], V2[k]) for k in K.NAMES) and same_bits(S1, S2), f"{name} {tag}: a second run differs"
        return V1, S1, Sr

    # KR_BEGIN: b = r = rhat = p = rhs[perm] on owned rows, y = 0, (b, b), the veto
    V1, S1, Sr = go("begin", D.KR_BEGIN, make_state(ap, rest, 1, False), make_head(1), rhs=rhs, veto=veto)
    bvec = np.where(ap.own_np, rhs, 0.0)
    for k in ("b", "r", "rhat", "p"):
        assert same_bits(V1[k], bvec), k
    assert np.all(V1["y"] == 0.0) and S1[K.R_OFF + K.R_RR] == veto
    assert np.all(S1[:K.R_OFF] == 0.0), S1
    # KR_BEGIN2 (the head of KR_BEGIN's making, then one of the test's)
    V1, S1, Sr = go("begin2", D.KR_BEGIN2, V1, S1)
    assert S1[K.S_MODE] == 1.0 and S1[K.S_RHO] == S1[K.S_RHO_NEXT] == S1[K.S_BB] == S1[K.S_RR] == S1[K.R_OFF + K.R_RHO]
    S0 = make_head(2)
    S0[K.S_MODE] = 0.0
    _, S1, _ = go("begin2'", D.KR_BEGIN2, make_state(ap, rest, 2, False), S0)
    assert S1[K.S_MODE] == 1.0 and S1[K.S_RHO_NEXT] == S0[K.R_OFF + K.R_RHO]
    # KR_UPDATE_S: the S_RHO_NEXT -> S_RHO hand-over
    S0 = make_head(3)
    _, S1, _ = go("update_s", D.KR_UPDATE_S, make_state(ap, rest, 3, False), S0)
    assert S1[K.S_RHO] == S0[K.S_RHO_NEXT] and S1[K.S_RHO_NEXT] == S0[K.S_RHO_NEXT]
    # KR_UPDATE_XR
    go("update_xr", D.KR_UPDATE_XR, make_state(ap, rest, 4, True), make_head(4))
    # KR_UPDATE_P: a normal step, the collapse threshold from both sides, a beta that is not finite
    S0 = make_head(5)
    _, S1, _ = go("update_p", D.KR_UPDATE_P, make_state(ap, rest, 5, False), S0)
    assert S1[K.S_RESTARTS] == 3.0 and S1[K.S_RHO_NEXT] == S0[K.R_OFF + K.R_RHO] and S1[K.S_RR] == S0[K.R_OFF + K.R_RR]
    for tag, factor, omega, restarts in (("collapse", 0.5e-14, None, True), ("no collapse", 2e-14, None, False),
                                         ("omega = 0", None, 0.0, True)):
        S0 = make_head(6)
        if factor is not None:
            S0[K.R_OFF + K.R_RHO] = factor * S0[K.R_OFF + K.R_RR]
        if omega is not None:
            S0[K.S_OMEGA] = omega
        V1, S1, _ = go(f"update_p, {tag}", D.KR_UPDATE_P, make_state(ap, rest, 6, False), S0)
        if restarts:
            assert same_bits(V1["p"], V1["r"]) and same_bits(V1["rhat"], V1["r"]), tag
            assert S1[K.S_RHO_NEXT] == S0[K.R_OFF + K.R_RR] and S1[K.S_RESTARTS] == 4.0, (tag, S1)
        else:
            assert S1[K.S_RHO_NEXT] == S0[K.R_OFF + K.R_RHO] and S1[K.S_RESTARTS] == 3.0, (tag, S1)
    # KR_TRUE_RESIDUAL, KR_RESTART
    go("true_residual", D.KR_TRUE_RESIDUAL, make_state(ap, rest, 7, False), make_head(7))
    S0 = make_head(8)
    V1, S1, _ = go("restart", D.KR_RESTART, make_state(ap, rest, 8, False), S0)
    assert S1[K.S_RESTARTS] == 4.0 and S1[K.S_ALPHA] == S1[K.S_OMEGA] == 1.0
    assert S1[K.S_RHO] == S1[K.S_RHO_NEXT] == S1[K.S_RR] == S0[K.R_OFF + K.R_RR]
    return worst


def check_finish(ap, name, cs_kind):
    """phx_krylov_finish: x_full[dof[perm[i]]] = C_i y_i (C: 1 on unscaled u columns, 1 / A_ii elsewhere), 0 elsewhere."""
    torch = ap.torch
    nfull = ap.info["n_full"]
    y = np.random.default_rng(31).standard_normal(ap.n)
    ap.put(6, y)
    out = torch.full((nfull,), float("nan"), dtype=torch.float64, device=ap.dev)
    torch.cuda.synchronize(ap.dev)
    ap.b.finish(out)
    torch.cuda.synchronize(ap.dev)
    got = out.cpu().numpy()
    ld = np.longdouble
    c_exact = np.where(ap.is_u, ld(1.0), ld(1.0) / ap.diag.astype(ld)) if cs_kind == "unscaled" else ld(1.0) / ap.diag.astype(ld)
    ref = K.finish(y.astype(ld), ap.perm, ap.dof, c_exact, nfull)
    hit = np.zeros(nfull, dtype=bool)
    hit[ap.dof[ap.perm]] = True
    assert hit.sum() == ap.n
    assert np.all(got[~hit] == 0.0), f"{name}: finish wrote outside the active DoFs"
    err = np.abs(got.astype(ld) - ref)[hit]
    tol = EPS * np.abs(ref[hit])
    assert np.all(err <= tol), f"{name}: finish, rows {np.flatnonzero(err > tol)[:8]}"
    return float((err / tol).max())


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("name", list(CASES))
def test_phase_by_phase(P, name, mask):
    ap, rest, ex = open_case(P, name, mask)
    cs_kind, cs = ap.column_scaling()
    worst = all_phases(ap, rest, f"{name}/{mask}")
    worst["finish"] = check_finish(ap, name, cs_kind)
    print(f"[{name}/{mask}] n={ap.n} (n % 256 = {ap.n % 256}) owned={int(ap.own_np.sum())} kind={ap.kind} hat={ap.hat} "
          f"RestOut rows={0 if rest is None else int(rest.sum())} u first={ex['u_first']} C={cs_kind}: worst ratio to the "
          f"bound " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("name", ["box_p1_lattice", "box_p2_lattice", "jacobi_submesh"])
def test_deterministic_phases_repeat_bit_for_bit(P, name):
    """PHX_OPT_DETERMINISTIC: the same phase from the same inputs gives the same bits, dot products included (the
    partial sums of the blocks are folded in a fixed order)."""
    ap, rest, ex = open_case(P, name, "random_half", deterministic=True)
    worst = all_phases(ap, rest, f"{name}/deterministic", repeat=True)
    print(f"[{name}/deterministic] n={ap.n}: every phase twice, bit for bit; worst ratio {max(worst.values()):.2f}")


def test_grid_stride_of_the_vector_kernels(P):
    """More rows than vec_grid's 2048 blocks of 256 threads cover: the second trip of every GRID_STRIDE loop.  Vector
    phases only; the ownership mask is changed in place (the preconditioner, which the vector phases never touch, is
    the one KR_BEGIN built for all rows)."""
    sh = SHAPES["plane_map"]
    c = weak_system(P, sh["lo"], sh["hi"], sh["n"], sh["phi"])
    ap = Applied(P, c)
    assert ap.n > VEC_GRID_ROWS, ap.n
    assert ap.kind == 1 and ap.hat and ap.vbytes == 8 and ap.info["stencil_rows"] > 0
    assert np.array_equal(ap.is_u, np.arange(ap.n) < ap.info["n_active_u"])
    rest = ~ap.is_u
    cs_kind, cs = ap.column_scaling()
    out = []
    for mask in ("all", "random_half"):
        if MASKS[mask] is not None:
            own = MASKS[mask](ap)
            ap.own.copy_(ap.torch.from_numpy(own.astype(np.uint8)).to(ap.dev))
            ap.own_np = own
            ap.torch.cuda.synchronize(ap.dev)
        worst = all_phases(ap, rest, f"plane_map/{mask}")
        out.append(f"{mask} {max(worst.values()):.2f}")
    fin = check_finish(ap, "plane_map", cs_kind)
    print(f"[plane_map] n={ap.n} > {VEC_GRID_ROWS} ({-(-ap.n // 256)} blocks of rows for 2048 blocks) RestOut rows="
          f"{int(rest.sum())}: worst ratio to the bound " + ", ".join(out) + f", finish {fin:.2f}")


def test_identity_and_reduced_phases_are_refused(P):
    """Phases 52 - 55 need the identity loop and 56 - 63 the reduced loop of a native solve; the phase API never puts
    them in force (kr_cmask and kr_red are not built), so it answers PHX_ERR_VALUE before any launch.  So does every
    number between the assigned phases (the holes of KrPhase), below the first and above the last: "unknown Krylov
    phase", with the workspace and the scalars left as they were."""
    ap, rest, ex = open_case(P, "box_p1_lattice", "all")
    L = ap.b.L
    before = ap.read()
    for phase in (53, 58):
        rc = L.lib.phx_krylov_phase(ap.b.sys, phase)
        assert rc == L.ERR_VALUE, (phase, rc)
        with pytest.raises(ValueError, match="loop"):
            L.check(rc)
    after = ap.read()
    assert all(same_bits(before[k], after[k]) for k in K.NAMES)
    scal = ap.scal.cpu().numpy().copy()
    for phase in UNASSIGNED_PHASES:
        rc = L.lib.phx_krylov_phase(ap.b.sys, phase)
        assert rc == L.ERR_VALUE, (phase, rc)
        with pytest.raises(ValueError, match=f"unknown Krylov phase {phase}$"):
            L.check(rc)
    after = ap.read()
    assert all(same_bits(before[k], after[k]) for k in K.NAMES)
    assert same_bits(scal, ap.scal.cpu().numpy())
