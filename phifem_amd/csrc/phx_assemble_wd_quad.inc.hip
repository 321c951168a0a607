// Weak-Dirichlet phi-FEM Poisson on QUADRILATERALS: mixed (u, p) in Q1 x Q1 with Q1 nodal phi_h, f_h, u_D -- the
// forms of demo/weak-dirichlet/flower/main.py:112-135 (bilinear) and :142-151 (linear), which are independent of the
// cell type, on the second 2-D cell type of mesh_scripts.py:322-325.  Included by phx_assemble.hip after
// phx_q1rect.inc.hip (the rectangle, the Q1 basis, the facet numbering, the Gauss rules: the cell conventions are
// stated there); dispatched to by phx_assemble_poisson_wd.  Restated in tests/poisson_quad_ref.py.
// DoFs, activity and numbering are those of the P1 path (assemble_with_capacity): u at vertex v -> v, p at vertex
// v -> nv + v; u active on the vertices of cells tagged 1 / 2, p on those of cells tagged 2; u rows first.
//
// Every integral is EXACT, so the result equals FFCx's up to round-off:
//  * dx((1,2)) grad u . grad v and f_h v: closed form from the 1-D matrices A1, M1 of linear functions on [0, 1].
//  * dx(2) gamma h^-2 (u - h^-1 phi_h p)(v - h^-1 phi_h q) and its right-hand side with u_D: products of four Q1
//    functions, degree <= 4 in each variable; the 3 x 3 tensor Gauss rule integrates degree 5 per variable exactly.
//  * dx(2) sigma h^2 div(grad u) div(grad v) and -sigma h^2 f_h div(grad v) (main.py:123-128,150) VANISH
//    IDENTICALLY: the Laplacian of a + b x + c y + d x y is zero.  Nothing is launched for them.
//  * ds -(grad u . n) v and dS((2,3)) sigma avg(h) [grad u . n][grad v . n]: along an axis-parallel edge the normal
//    derivative of a Q1 function is linear in the tangential coordinate, the integrands are of degree 2: the 2-point
//    Gauss rule (degree 3) is exact.
// All contributions go through slot_add / slot_rhs_add, so PHX_OPT_DETERMINISTIC (two passes) applies as it does to
// P1 systems on meshes that are not Kuhn boxes.  The kernels are small; the f64 atomics into the slot table bound them.

struct WdqArgs {
  const int32_t *cells, *c2f, *f2c;
  const double *x, *phi, *f, *ud;
  const int32_t *du, *dp;
  int32_t nv;
  double gamma, sigma;
  double *rhs;
  Slots slots;
  int *bad;   // set when a cell is not an axis-parallel rectangle
};

// --- dx((1,2)): main.py:113 grad u . grad v and :143 f_h v; 16 lanes per cell, closed form ----------------------
__global__ void __launch_bounds__(256) k_wdq_bulk(int64_t nlist, const int32_t *__restrict__ list, WdqArgs A) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t e = gid >> 4;
  if (e >= nlist) return;
  const int i = (int)(gid & 15) >> 2, j = (int)(gid & 3);
  RectGeo R;
  if (!rect_load(A.cells, A.x, list[e], R)) { *A.bad = 1; return; }
  const int ix = i & 1, iy = i >> 1, jx = j & 1, jy = j >> 1;
  const double K = (R.hy / R.hx) * a1(ix, jx) * m1(iy, jy) + (R.hx / R.hy) * m1(ix, jx) * a1(iy, jy);
  const int32_t row = A.du[R.v[i]];
  slot_add(A.slots, row, R.v[j], K);
  if (j == 0 && row >= 0) {
    double s = 0.0;
    for (int k = 0; k < 4; ++k) s += m1(ix, k & 1) * m1(iy, k >> 1) * A.f[R.v[k]];
    slot_rhs_add(A.slots, A.rhs, row, R.hx * R.hy * s);
  }
}

// --- dx(2): main.py:115-122 and :144-149; 16 lanes per cut cell ----------------------------------------------------
// The 3 x 3 Gauss tabulation of the Q1 basis on the reference square (the same for every rectangle) is built once
// per workgroup in LDS.  Lane (i, j) forms M_k = int N_i N_j phi_h^k / |K|, k = 0, 1, 2, and writes the four entries
// (u_i, u_j), (u_i, p_j), (p_i, u_j), (p_i, p_j) of the 8 x 8 element tensor; the lanes j = 0 also the two
// right-hand-side entries of vertex i.
__global__ void __launch_bounds__(256) k_wdq_cut(int64_t nlist, const int32_t *__restrict__ list, WdqArgs A) {
  constexpr int NQ = 9;
  __shared__ double sN[NQ][4], sW[NQ];
  if (threadIdx.x < NQ) sW[threadIdx.x] = q1_tab9(threadIdx.x, nullptr, sN[threadIdx.x], nullptr);
  __syncthreads();
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t e = gid >> 4;
  if (e >= nlist) return;
  const int i = (int)(gid & 15) >> 2, j = (int)(gid & 3);
  RectGeo R;
  if (!rect_load(A.cells, A.x, list[e], R)) { *A.bad = 1; return; }
  double ph[4];
  for (int k = 0; k < 4; ++k) ph[k] = A.phi[R.v[k]];
  double M0 = 0.0, M1 = 0.0, M2 = 0.0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double pq = sN[q][0] * ph[0] + sN[q][1] * ph[1] + sN[q][2] * ph[2] + sN[q][3] * ph[3];
    const double w = sW[q] * sN[q][i] * sN[q][j];
    M0 += w; M1 += w * pq; M2 += w * pq * pq;
  }
  const double h1 = 1.0 / R.h, gam = A.gamma * R.hx * R.hy;
  const int32_t ru = A.du[R.v[i]], rp = A.dp[R.v[i]];
  const int32_t cu = R.v[j], cp = A.nv + R.v[j];
  const double up = -gam * h1 * h1 * h1 * M1;
  slot_add(A.slots, ru, cu, gam * h1 * h1 * M0);
  slot_add(A.slots, ru, cp, up);
  slot_add(A.slots, rp, cu, up);
  slot_add(A.slots, rp, cp, gam * h1 * h1 * h1 * h1 * M2);
  if (j == 0) {
    double ud[4];
    for (int k = 0; k < 4; ++k) ud[k] = A.ud[R.v[k]];
    double b0 = 0.0, b1 = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double pq = sN[q][0] * ph[0] + sN[q][1] * ph[1] + sN[q][2] * ph[2] + sN[q][3] * ph[3];
      const double uq = sN[q][0] * ud[0] + sN[q][1] * ud[1] + sN[q][2] * ud[2] + sN[q][3] * ud[3];
      const double w = sW[q] * sN[q][i] * uq;
      b0 += w; b1 += w * pq;
    }
    if (ru >= 0) slot_rhs_add(A.slots, A.rhs, ru, gam * h1 * h1 * b0);
    if (rp >= 0) slot_rhs_add(A.slots, A.rhs, rp, -gam * h1 * h1 * h1 * b1);
  }
}

// --- ds: main.py:114  -int_F (grad u . n) v over (cell, local facet); 16 lanes per entity: row i, column j ---------
// box mode: the packed entities of ds(100); sub-mesh: its boundary facets as (cell, local facet) pairs
__global__ void __launch_bounds__(256) k_wdq_ds(int64_t nent, const int64_t *__restrict__ ent_packed,
                                                const int32_t *__restrict__ ent_pairs, WdqArgs A) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t e = gid >> 4;
  if (e >= nent) return;
  const int i = (int)(gid & 15) >> 2, j = (int)(gid & 3);
  int64_t c;
  int lf;
  if (ent_packed) { c = ent_packed[2 * e + 1] >> 8; lf = (int)(ent_packed[2 * e + 1] & 0xff); }
  else { c = ent_pairs[2 * e]; lf = ent_pairs[2 * e + 1]; }
  RectGeo R;
  if (!rect_load(A.cells, A.x, c, R)) { *A.bad = 1; return; }
  int va, vb, axis;
  double sign;
  quad_facet(lf, &va, &vb, &axis, &sign);
  if (i != va && i != vb) return;   // v vanishes on the facet
  const double fixed = sign > 0.0 ? 1.0 : 0.0, len = axis == 0 ? R.hy : R.hx;
  constexpr Gauss2 g2 = gauss2();
  double acc = 0.0;
  for (int q = 0; q < 2; ++q) {
    const double xi = axis == 0 ? fixed : g2.x[q], eta = axis == 1 ? fixed : g2.x[q];
    double vi, vj, gx, gy, t0, t1;
    q1_at(i, xi, eta, R, &vi, &t0, &t1);
    q1_at(j, xi, eta, R, &vj, &gx, &gy);
    acc += g2.w[q] * vi * sign * (axis == 0 ? gx : gy);
  }
  slot_add(A.slots, A.du[R.v[i]], R.v[j], -len * acc);
}

// --- dS((2,3)): main.py:129-134  sigma avg(h) int_F [grad u . n][grad v . n]; 16 lanes per facet -------------------
// The two rectangles share the two vertices of F: the macro-element has 8 - 2 = 6 distinct vertices (the four of the
// first cell, then the two of the second cell off the facet); the jump coefficient of a shared vertex is the sum of
// its two one-sided normal derivatives.  Both rectangles parametrise the facet in the same direction (tensor-product
// order), so the Gauss points of the two sides coincide.  The 16 lanes walk the 36 entries.
__global__ void __launch_bounds__(256) k_wdq_facets(int64_t nlist, const int32_t *__restrict__ list, WdqArgs A) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t e = gid >> 4;
  if (e >= nlist) return;
  const int l = (int)(gid & 15);
  const int64_t f = list[e];
  constexpr Gauss2 g2 = gauss2();
  int32_t vd[6] = {0, 0, 0, 0, 0, 0};
  double J[2][6] = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}}, hsum = 0.0, len = 0.0;
  int next = 4;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    QuadFacetSide S;
    if (!quad_facet_side(f, side, A.c2f, A.f2c, A.cells, A.x, S)) { *A.bad = 1; return; }
    const RectGeo &R = S.R;
    const int va = S.va, vb = S.vb;
    if (side == 0) len = S.len;
    hsum += R.h;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double Ji[2];
      for (int q = 0; q < 2; ++q) {
        const double xi = S.axis == 0 ? S.fixed : g2.x[q], eta = S.axis == 1 ? S.fixed : g2.x[q];
        double val, gx, gy;
        q1_at(i, xi, eta, R, &val, &gx, &gy);
        Ji[q] = S.sign * (S.axis == 0 ? gx : gy);
      }
      if (side == 0) {
        vd[i] = R.v[i]; J[0][i] = Ji[0]; J[1][i] = Ji[1];
      } else if (i == va || i == vb) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (vd[k] == R.v[i]) { J[0][k] += Ji[0]; J[1][k] += Ji[1]; }
      } else if (next < 6) {
#pragma unroll
        for (int k = 4; k < 6; ++k)
          if (k == next) { vd[k] = R.v[i]; J[0][k] = Ji[0]; J[1][k] = Ji[1]; }
        ++next;
      }
    }
  }
  const double w = A.sigma * 0.5 * hsum * len * 0.5;
  for (int idx = l; idx < 36; idx += 16) {
    const int a = idx / 6, b = idx % 6;
    int32_t va_ = 0, vb_ = 0;
    double Ja0 = 0.0, Ja1 = 0.0, Jb0 = 0.0, Jb1 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {   // without dynamic indexing of the register arrays
      if (k == a) { va_ = vd[k]; Ja0 = J[0][k]; Ja1 = J[1][k]; }
      if (k == b) { vb_ = vd[k]; Jb0 = J[0][k]; Jb1 = J[1][k]; }
    }
    if (A.du[vb_] < 0) continue;   // inactive column (only reachable through user-overwritten tags)
    slot_add(A.slots, A.du[va_], vb_, w * (Ja0 * Jb0 + Ja1 * Jb1));
  }
}

static int assemble_wd_quad_with_capacity(phx_mesh *m, double pen_coef, double stab_coef, const double *dphi,
                                          const double *df, const double *dud, int W, phx_system **out) {
  PHX_REQUIRE(2 * m->nv < INT32_MAX, PHX_ERR_VALUE, "too many DoFs for 32-bit column keys");
  SystemBuild sys(m, m->nv, 2 * m->nv, W);
  DevTemps tmp(m->stream);
  phx_system *s = sys.s;
  Slots &sl = sys.sl;
  s->u_vertex_block = true;
  const dim3 block(256);
  // ---- active numbering (as p1_number, always from the cells)
  uint8_t *fu = nullptr, *fp = nullptr;
  unsigned long long *sup = nullptr;
  PHX_HIP(tmp.alloc(&sup, sizeof(unsigned long long) * (size_t)m->nv));
  PHX_HIP(tmp.alloc(&fu, (size_t)m->nv));
  PHX_HIP(tmp.alloc(&fp, (size_t)m->nv));
  PHX_HIP(hipMemsetAsync(fu, 0, (size_t)m->nv, m->stream));
  PHX_HIP(hipMemsetAsync(fp, 0, (size_t)m->nv, m->stream));
  k_mark_active<4><<<dim3((unsigned)phx_div_up(phx_div_up(m->nc, 4), 256)), block, 0, m->stream>>>(m->nc, m->cells,
                                                                                                   m->cell_tags, fu, fp);
  int32_t nu = 0, np = 0;
  PHX_CHECK(scan_flags_packed(m, fu, fp, sup, &nu, &np, m->nv));
  s->nu = nu;
  s->n = (int64_t)nu + np;
  PHX_REQUIRE(s->n > 0, PHX_ERR_VALUE, "no active DoF: no cell is tagged 1 or 2");
  PHX_HIP(phx_malloc(&s->dof_of_vertex_u, sizeof(int32_t) * (size_t)m->nv));
  PHX_HIP(phx_malloc(&s->dof_of_vertex_p, sizeof(int32_t) * (size_t)m->nv));
  PHX_HIP(phx_malloc(&s->full_of_active, sizeof(int64_t) * (size_t)s->n));
  k_finish_numbering_packed<<<dim3((unsigned)phx_div_up(m->nv, 256)), block, 0, m->stream>>>(
      m->nv, fu, fp, sup, nu, s->dof_of_vertex_u, s->dof_of_vertex_p, s->full_of_active, 0);
  // ---- work lists and integration entities
  int32_t *l_om = nullptr, *l_cut = nullptr, *l_fac = nullptr;
  int64_t n_om = 0, n_cut = 0, n_fac = 0;
  PHX_CHECK(build_list(m, m->nc, SelOmega{m->cell_tags}, &l_om, &n_om));
  tmp.adopt(l_om);
  PHX_CHECK(build_list(m, m->nc, SelCut{m->cell_tags}, &l_cut, &n_cut));
  tmp.adopt(l_cut);
  PHX_CHECK(build_list(m, m->nf, SelGhostFacet{m->facet_tags, m->f2c}, &l_fac, &n_fac));
  tmp.adopt(l_fac);
  DsEntities ds;
  PHX_CHECK(ds_entities(m, &ds));
  PHX_REQUIRE_GRID(n_om * 16, "quadrilateral cell assembly");
  PHX_REQUIRE_GRID(n_fac * 16, "quadrilateral facet assembly");
  PHX_REQUIRE_GRID(ds.n * 16, "quadrilateral boundary assembly");
  // ---- slots
  const int64_t nslots = s->n * W;
  PHX_CHECK(slots_alloc(m, nslots, W, &sl));
  PHX_CHECK(rhs_alloc(m, s));
  WdqArgs A;
  A.cells = m->cells; A.c2f = m->c2f; A.f2c = m->f2c; A.x = m->x;
  A.phi = dphi; A.f = df; A.ud = dud;
  A.du = s->dof_of_vertex_u; A.dp = s->dof_of_vertex_p; A.nv = (int32_t)m->nv;
  A.gamma = pen_coef; A.sigma = stab_coef; A.rhs = s->rhs;
  PHX_CHECK(rect_bad_alloc(m, tmp, &A.bad));
  // ---- element kernels.  PHX_OPT_DETERMINISTIC: exponent pass, then the exact accumulation pass (Slots)
  bool det = false;
  PHX_CHECK(det_alloc(m, sl, nslots, s->n, &det));
  for (int pass = det ? 1 : 0; pass <= (det ? 2 : 0); ++pass) {
    sl.pass = pass;
    A.slots = sl;
    if (n_om) k_wdq_bulk<<<dim3((unsigned)phx_div_up(n_om * 16, 256)), block, 0, m->stream>>>(n_om, l_om, A);
    if (n_cut) k_wdq_cut<<<dim3((unsigned)phx_div_up(n_cut * 16, 256)), block, 0, m->stream>>>(n_cut, l_cut, A);
    if (ds.n) k_wdq_ds<<<dim3((unsigned)phx_div_up(ds.n * 16, 256)), block, 0, m->stream>>>(ds.n, ds.packed, ds.pairs, A);
    if (n_fac) k_wdq_facets<<<dim3((unsigned)phx_div_up(n_fac * 16, 256)), block, 0, m->stream>>>(n_fac, l_fac, A);
    PHX_HIP(hipGetLastError());
  }
  PHX_CHECK(det_finish(m, sl, nslots, s->n, s->rhs));
  PHX_CHECK(rect_bad_check(m, A.bad));
  return sys.finish((int32_t)m->nv, out);
}
