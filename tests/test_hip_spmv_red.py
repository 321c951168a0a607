"""Stored-row product of the reduced BiCGStab loop (k_spmv_red, PHX_OPT_RED_SPMV = 1, the default) against
k_spmv_sell<DOTS, true> (PHX_OPT_RED_SPMV = 0) and against float64 on the host; the z solve of the box preconditioner
(k_tri_z) against recorded values.

Product.  Small structured sphere systems are solved once, which puts the reduced loop in force; then the phases
KR_RED_SPMV_P (57: v_B = (A phat)_B, (v_B, rhat_B)) and KR_RED_SPMV_S (60: t_B = (A shat)_B, (t_B, s_B), (t_B, t_B),
(t_B, rhat_B)) run through `phx_krylov_phase` on seeded normal vectors written with `phx_krylov_reduced_io`.
  y_B           the same bits with the option at 1 and at 0; slots of padding rows (rows = -1) keep theirs; against the
                host product of the exported entries (values of A, p columns divided by their diagonal entry as the SELL
                fill does) each row is within (len + 2) eps sum_j |a_ij x_j|
  dot products  against math.fsum of y_i d_i with y the HOST product: |got - ref| <= 64 eps sum_i |y_i| |d_i| (the order
                of the per-block sums is not fixed; 64 covers the longest stored P1 row)
  deterministic with PHX_OPT_DETERMINISTIC the dot products of two runs are the same bits
Boxes (cubes per axis of [-1.5, 1.5]^3, unit sphere): 10^3, 12^3, 16 x 12 x 10 (anisotropic), 20^3 and 32^3 (8^3, 9^3,
11^3 and 16 x 12 x 8 do not take the reduced loop).  Together they must hold slices of 3, 4, 5 and >= 9 trips (tail only,
an exact round, tail after a round of four, two rounds plus a tail), slices of 8 .. 10 and of 6 .. 7 trips (either side
of the threshold of the round of eight), a last slice with rows = -1 padding, one without, a slice count that is no
multiple of 4 and one that is a multiple of 32 (no idle wavefront in the grid): asserted in
test_systems_cover_the_kernel_paths.  A slice of ONE trip does not exist on these systems: a stored P1 row has at least
five entries, and on 47 sphere systems (8^3 .. 32^3, cubic and anisotropic boxes, radii 0.45 .. 1.3, centred and not) the
shortest slice always had 2 trips; the tail-only path is therefore asserted on the slices of 2 and of 3 trips.

z solve.  `phx_box_poisson_solve` at L = (64, 64, 25) and (64, 64, 183): bit for bit the values the commit before the
spill-free k_tri_z produced for the same seeded input (tests/golden/tri_z_parent.npz: SHA-256 of the result and every
61st value), and within 1e-12 of scipy's DST-I solve (the tolerance of test_hip_precond.py)."""
import ctypes as C
import hashlib
import math
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tri_z_parent.npz")
BOXES = {"10": [10, 10, 10], "12": [12, 12, 12], "16x12x10": [16, 12, 10], "20": [20, 20, 20], "32": [32, 32, 32]}
KR_RED_SPMV_P, KR_RED_SPMV_S = 57, 60
# reduced-loop buffers of phx_krylov_reduced_io
B_RHAT, B_V, B_S, B_T, B_PHAT, B_SHAT, B_SCAL = 1, 3, 4, 5, 8, 9, 10
NSLOT, SLOT_STRIDE, P_OFF = 64, 8, 16


@pytest.fixture(scope="module")
def P():
    import phifem_amd
    assert phifem_amd._lib.device_count() > 0
    return phifem_amd


class System:
    """A solved structured sphere system with its exported stored rows."""

    def __init__(self, P, n, radius=1.0, centre=(0.0, 0.0, 0.0)):
        from phifem_amd import _lib as L
        from phifem_amd.mesh_scripts import NodalFunction
        self.L = L
        self.mesh = P.create_box([-1.5] * 3, [1.5] * 3, n)
        x = self.mesh.x
        phi = ((x - np.asarray(centre)) ** 2).sum(axis=1) - radius ** 2
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            P.compute_tags_measures(self.mesh, NodalFunction(phi), 1, box_mode=True, single_layer_cut=True)
            uex = np.prod(np.sin(x), axis=1)
            self.s = P.PhiFEMSolver(self.mesh)
            self.s.assemble(phi, 3.0 * uex, uex)
            self.s.solve(rtol=1e-6)
        on = C.c_int(0)
        L.check(L.lib.phx_krylov_reduced_loop(self.s._sys, C.byref(on)))
        assert on.value == 1, f"box {n}: the reduced loop is not in force"
        info = self.s.info()
        self.n, self.nu, self.nsl, ne = info["n_active"], info["n_active_u"], info["n_slices"], info["sell_padded_nnz"]
        self.m = 16 * self.nsl
        self.slice_ptr = np.zeros(self.nsl + 1, np.int64)
        self.col = np.zeros(ne, np.int32)
        raw = np.zeros(ne, np.float64)
        self.rows = np.zeros(self.m, np.int32)
        L.check(L.lib.phx_system_export_sell(self.s._sys, L.ptr(self.slice_ptr)[0], L.ptr(self.col)[0], L.ptr(raw)[0],
                                             L.ptr(self.rows)[0]))
        assert self.slice_ptr[-1] == ne
        self.trips = np.diff(self.slice_ptr) // 64
        assert np.array_equal(self.trips * 64, np.diff(self.slice_ptr))
        # slot of every entry: entry k of row r of slice s sits at slice_ptr[s] + 16 k + r
        sl = np.repeat(np.arange(self.nsl), np.diff(self.slice_ptr))
        self.slot = 16 * sl + (np.arange(ne) - self.slice_ptr[sl]) % 16
        # values the product applies: u columns (solver positions < nu) as assembled, p columns over their diagonal entry
        diag = np.ones(self.n)
        self_entry = (self.col == self.rows[self.slot]) & (self.rows[self.slot] >= 0) & (raw != 0.0)
        diag[self.col[self_entry]] = raw[self_entry]
        self.val = np.where(self.col < self.nu, raw, raw / diag[self.col])
        self.live = self.rows >= 0

    def io(self, which, a, put):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.L.check(self.L.lib.phx_krylov_reduced_io(self.s._sys, which, self.L.ptr(a)[0], a.size, int(put)))
        return a

    def get(self, which, count):
        return self.io(which, np.empty(count), False)

    def option(self, opt, value):
        self.L.check(self.L.lib.phx_set_option(self.mesh._h, opt, value))

    def product(self, x):
        """(y, sum_j |a_ij x_j|, entries per row) by SELL slot, float64 on the host."""
        t = self.val * x[self.col]
        y = np.zeros(self.m)
        ab = np.zeros(self.m)
        np.add.at(y, self.slot, t)
        np.add.at(ab, self.slot, np.abs(t))
        return y, ab, np.bincount(self.slot, minlength=self.m)

    def run(self, phase, seed):
        """One SpMV phase on seeded inputs: (y_B, {quantity: dot product}, x, d0, d1)."""
        rng = np.random.default_rng(seed)
        x = rng.standard_normal(self.n)
        d0 = rng.standard_normal(self.m)
        d1 = rng.standard_normal(self.m)
        scal = self.get(B_SCAL, P_OFF + 2 * 8 * NSLOT * SLOT_STRIDE)
        scal[P_OFF:] = 0.0
        self.io(B_SCAL, scal, True)
        self.io(B_RHAT, d1 if phase == KR_RED_SPMV_S else d0, True)
        if phase == KR_RED_SPMV_S:
            self.io(B_S, d0, True)
        self.io(B_PHAT if phase == KR_RED_SPMV_P else B_SHAT, x, True)
        out = B_V if phase == KR_RED_SPMV_P else B_T
        self.io(out, np.full(self.m, np.nan), True)
        self.L.check(self.L.lib.phx_krylov_phase(self.s._sys, phase))
        y = self.get(out, self.m)
        scal = self.get(B_SCAL, scal.size)
        dots = {}
        for q in ((0,) if phase == KR_RED_SPMV_P else (1, 2, 8)):
            base = P_OFF + (q % 8) * NSLOT * SLOT_STRIDE + q // 8
            dots[q] = scal[base:base + NSLOT * SLOT_STRIDE:SLOT_STRIDE].copy()
        return y, dots, x, d0, d1


@pytest.fixture(scope="module")
def systems(P):
    return {k: System(P, n) for k, n in BOXES.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def test_systems_cover_the_kernel_paths(systems):
    trips = np.concatenate([s.trips for s in systems.values()])
    print({k: dict(zip(*np.unique(s.trips, return_counts=True))) for k, s in systems.items()})
    for t in (2, 3, 4, 5):       # 2, 3: tail only (no system has a slice of one trip, see above); 4: a round; 5: round + tail
        assert (trips == t).any(), f"no slice of {t} trips"
    assert (trips >= 9).any()
    assert ((trips >= 8) & (trips <= 11)).any() and ((trips >= 6) & (trips <= 7)).any()
    assert any((~s.live[-16:]).any() for s in systems.values()), "no last slice with padding rows"
    assert any(s.live.all() for s in systems.values()), "no system without padding rows"
    assert any(s.nsl % 4 != 0 for s in systems.values()) and any(s.nsl % 32 == 0 for s in systems.values())
    for s in systems.values():
        assert s.live[:-16].all() and np.all(np.diff(s.trips) <= 0)      # padding in the last slice only; sorted by length


@pytest.mark.parametrize("box", list(BOXES))
def test_product_and_dots(systems, box):
    s = systems[box]
    L = s.L
    for phase in (KR_RED_SPMV_P, KR_RED_SPMV_S):
        s.option(L.OPT_RED_SPMV, 0)
        y0, dots0, x, d0, d1 = s.run(phase, 100 + phase)
        s.option(L.OPT_RED_SPMV, 1)
        y1, dots1, _, _, _ = s.run(phase, 100 + phase)
        assert np.array_equal(bits(y1), bits(y0)), f"{box} phase {phase}: y_B differs from k_spmv_sell"
        assert np.isnan(y1[~s.live]).all() and np.isfinite(y1[s.live]).all()
        yh, ab, cnt = s.product(x)
        err = np.abs(y1 - yh)[s.live]
        tol = ((cnt + 2) * EPS * ab)[s.live]
        assert np.all(err <= tol), f"{box} phase {phase}: rows {np.flatnonzero(err > tol)[:8]}"
        yl = np.where(s.live, yh, 0.0)
        operands = {0: d0} if phase == KR_RED_SPMV_P else {1: d0, 2: yl, 8: d1}
        for q, d in operands.items():
            ref = math.fsum((yl * d).tolist())
            bound = 64 * EPS * float(np.abs(yl) @ np.abs(d))
            for name, dots in (("k_spmv_red", dots1), ("k_spmv_sell", dots0)):
                got = math.fsum(dots[q].tolist())
                print(f"[{box}] phase {phase} quantity {q} {name}: |got - ref| = {abs(got - ref):.3e}, bound {bound:.3e}")
                assert abs(got - ref) <= bound, (box, phase, q, name, got, ref, bound)


def test_deterministic_dots_repeat(systems):
    s = systems["12"]
    L = s.L
    s.option(L.OPT_RED_SPMV, 1)
    s.option(L.OPT_DETERMINISTIC, 1)
    try:
        for phase in (KR_RED_SPMV_P, KR_RED_SPMV_S):
            ya, da, _, _, _ = s.run(phase, 7)
            yb, db, _, _, _ = s.run(phase, 7)
            assert np.array_equal(bits(ya), bits(yb))
            for q in da:
                assert np.array_equal(bits(da[q]), bits(db[q])), (phase, q)
                assert da[q][0] != 0.0 and np.all(da[q][1:] == 0.0)      # folded into slot 0 in a fixed order
    finally:
        s.option(L.OPT_DETERMINISTIC, 0)


# ---- z solve ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L3", [(64, 64, 25), (64, 64, 183)])
def test_tri_z_matches_the_recorded_values(P, L3):
    from phifem_amd import _lib as L
    from test_hip_precond import scipy_box_solve
    h = (0.011, 0.017, 0.013)
    f = np.random.default_rng(1000 + L3[2]).standard_normal((L3[2] - 1, L3[1] - 1, L3[0] - 1))
    u = np.ascontiguousarray(f.copy())
    L.check(L.lib.phx_box_poisson_solve(0, (C.c_int * 3)(*L3), (C.c_double * 3)(*h), 0, u.ctypes.data_as(C.c_void_p)))
    ref = scipy_box_solve(f, L3, h)
    assert np.abs(u - ref).max() <= 1e-12 * np.abs(ref).max()
    g = np.load(GOLDEN)
    key = "x".join(map(str, L3))
    assert np.array_equal(bits(u.ravel()[::61]), bits(g[f"sample_{key}"]))
    assert hashlib.sha256(u.tobytes()).digest() == g[f"sha256_{key}"].tobytes()
