// Neumann / Robin phi-FEM Poisson on QUADRILATERALS: mixed (u, y, p) in Q1 x Q1^2 x DG0 with a Q2 level-set --
// the cell type of demo/neumann/square/main.py:49-50 with its forms :113-158 (and those of demo/robin/square/
// main.py:112-168 with robin_coef != 0).  Included by phx_assemble.hip after phx_assemble_flux.inc.hip (shares
// FxArgs' conventions, slot_add, the work-list builders) and phx_q1rect.inc.hip (the rectangle, the Q1 basis, the
// facet numbering: the cell conventions are stated there).
// Q2 level-set nodal layout: [vertices (nv), edge midpoints by facet id (nf), cell centres (nc)].
// DoFs: u at vertex v -> v, y_k at vertex v -> (1 + k) nv + v, p on cell c -> 3 nv + c.
// Cell integrals of the cut cells: tensor Gauss rule, nq points per direction (|grad phi_h| is not polynomial:
// agreement with FFCx's Gauss-Jacobi rule to quadrature accuracy); bulk cells and edges: closed form / 3-point Gauss.

struct FxqArgs {
  const int32_t *cells, *c2f, *f2c;
  const double *x, *phi, *f, *g;
  const int8_t *ctags;
  const int32_t *dofmap;
  int64_t nv, nf;
  double gamma, sigma, kappa;
  double *rhs;
  Slots slots;
  int nq;
  double gx[8], gw[8];   // Gauss points / weights on [0, 1]
  int *bad;              // set when a cell is not an axis-parallel rectangle
};

__global__ void k_fxq_mark_active(int64_t nc, FxqArgs A, uint8_t *__restrict__ flags) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int t = A.ctags[c] & PHX_TAG_MASK;
  if (t != 1 && t != 2) return;
  for (int i = 0; i < 4; ++i) {
    const int64_t v = A.cells[c * 4 + i];
    flags[v] = 1;
    if (t == 2) { flags[A.nv + v] = 1; flags[2 * A.nv + v] = 1; }
  }
  if (t == 2) flags[3 * A.nv + c] = 1;
}

// --- dx((1,2)): neumann main.py:114 (grad u . grad v + u v) and :144 (f v); 16 lanes per cell, closed form ----
__global__ void __launch_bounds__(256) k_fxq_bulk(int64_t nlist, const int32_t *__restrict__ list, FxqArgs A) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t e = gid / 16;
  const int l = (int)(gid % 16);
  if (e >= nlist) return;
  const int i = l / 4, j = l % 4;
  RectGeo R;
  if (!rect_load(A.cells, A.x, list[e], R)) { *A.bad = 1; return; }
  const int ix = i & 1, iy = i >> 1, jx = j & 1, jy = j >> 1;
  const double K = (R.hy / R.hx) * a1(ix, jx) * m1(iy, jy) + (R.hx / R.hy) * m1(ix, jx) * a1(iy, jy);
  const double Mm = R.hx * R.hy * m1(ix, jx) * m1(iy, jy);
  slot_add(A.slots, A.dofmap[R.v[i]], R.v[j], K + Mm);
  if (j == 0) {
    double s = 0.0;
    for (int k = 0; k < 4; ++k) s += m1(ix, k & 1) * m1(iy, k >> 1) * A.f[R.v[k]];
    unsafeAtomicAdd(&A.rhs[A.dofmap[R.v[i]]], R.hx * R.hy * s);
  }
}

__device__ __forceinline__ void l3_at(double t, double *L, double *dL) {
  L[0] = 2.0 * (t - 0.5) * (t - 1.0); L[1] = 4.0 * t * (1.0 - t); L[2] = 2.0 * t * (t - 0.5);
  dL[0] = 4.0 * t - 3.0; dL[1] = 4.0 - 8.0 * t; dL[2] = 4.0 * t - 1.0;
}
// Q2 level-set and its physical gradient at (xi, eta) from the 9 nodal values (vertices, facet midpoints, centre)
__device__ __forceinline__ void q2_phi_at(const double *ph, double xi, double eta, const RectGeo &R, double *val, double *gx,
                                          double *gy) {
  constexpr int IX[9] = {0, 2, 0, 2, 1, 0, 2, 1, 1}, IY[9] = {0, 0, 2, 2, 0, 1, 1, 2, 1};
  double Lx[3], dLx[3], Ly[3], dLy[3];
  l3_at(xi, Lx, dLx);
  l3_at(eta, Ly, dLy);
  double v = 0.0, a = 0.0, b = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    v += ph[k] * Lx[IX[k]] * Ly[IY[k]];
    a += ph[k] * dLx[IX[k]] * Ly[IY[k]];
    b += ph[k] * Lx[IX[k]] * dLy[IY[k]];
  }
  *val = v; *gx = a / R.hx; *gy = b / R.hy;
}

// functionals of local DoF a (0..3 u_i, 4..11 y_{k,i}, 12 p) at one quadrature point
struct FxqLocal { double U, DY, B, T1[2]; };
__device__ __forceinline__ void fxq_eval(int a, double xi, double eta, const RectGeo &R, double phq, double gpx, double gpy,
                                         double ngp, double kappa, FxqLocal &o) {
  o.U = 0.0; o.DY = 0.0; o.B = 0.0; o.T1[0] = 0.0; o.T1[1] = 0.0;
  double val, gx, gy;
  if (a < 4) {
    q1_at(a, xi, eta, R, &val, &gx, &gy);
    o.U = val; o.T1[0] = gx; o.T1[1] = gy;
    o.B = -kappa * ngp * val;
  } else if (a < 12) {
    const int k = (a - 4) / 4, i = (a - 4) % 4;
    q1_at(i, xi, eta, R, &val, &gx, &gy);
    o.T1[k] = val;
    o.DY = k == 0 ? gx : gy;
    o.B = val * (k == 0 ? gpx : gpy);
  } else {
    o.B = phq / R.h;
  }
}

// --- dx(2): main.py:117-130 and :145-156; one 64-thread block per cut cell walks the 13 x 13 tensor + rhs ----
__global__ void __launch_bounds__(64) k_fxq_cut(int64_t nlist, const int32_t *__restrict__ list, FxqArgs A) {
  constexpr int M = 13;
  const int64_t e = blockIdx.x;
  if (e >= nlist) return;
  const int64_t c = list[e];
  RectGeo R;
  if (!rect_load(A.cells, A.x, c, R)) { *A.bad = 1; return; }
  double ph[9];
  for (int i = 0; i < 4; ++i) ph[i] = A.phi[R.v[i]];
  for (int k = 0; k < 4; ++k) ph[4 + k] = A.phi[A.nv + A.c2f[c * 4 + k]];
  ph[8] = A.phi[A.nv + A.nf + c];
  const double det = R.hx * R.hy, h2 = 1.0 / (R.h * R.h);
  auto full = [&](int a) -> int32_t {
    if (a < 4) return R.v[a];
    if (a < 12) return (int32_t)((1 + (a - 4) / 4) * A.nv + R.v[(a - 4) % 4]);
    return (int32_t)(3 * A.nv + c);
  };
  for (int idx = threadIdx.x; idx < M * M + M; idx += blockDim.x) {
    const bool is_rhs = idx >= M * M;
    const int a = is_rhs ? idx - M * M : idx / M, b = is_rhs ? 0 : idx % M;
    double acc = 0.0;
    for (int qx = 0; qx < A.nq; ++qx)
      for (int qy = 0; qy < A.nq; ++qy) {
        const double xi = A.gx[qx], eta = A.gx[qy], w = A.gw[qx] * A.gw[qy];
        double phq, gpx, gpy;
        q2_phi_at(ph, xi, eta, R, &phq, &gpx, &gpy);
        const double ngp = sqrt(gpx * gpx + gpy * gpy);
        FxqLocal la;
        fxq_eval(a, xi, eta, R, phq, gpx, gpy, ngp, A.kappa, la);
        if (is_rhs) {
          double fq = 0.0, gq = 0.0;
          for (int i = 0; i < 4; ++i) {
            double val, t0, t1;
            q1_at(i, xi, eta, R, &val, &t0, &t1);
            fq += val * A.f[R.v[i]];
            gq += val * A.g[R.v[i]];
          }
          acc += w * (-h2 * gq * ngp * la.B + fq * (la.DY + la.U));
        } else {
          FxqLocal lb;
          fxq_eval(b, xi, eta, R, phq, gpx, gpy, ngp, A.kappa, lb);
          acc += w * (la.T1[0] * lb.T1[0] + la.T1[1] * lb.T1[1] + (la.DY + la.U) * (lb.DY + lb.U) + h2 * la.B * lb.B);
        }
      }
    const double val = A.gamma * det * acc;
    const int32_t row = A.dofmap[full(a)];
    if (is_rhs) unsafeAtomicAdd(&A.rhs[row], val);
    else slot_add(A.slots, row, full(b), val);
  }
}

// --- ds: main.py:115  int_F (y . n) v; 4 lanes per (cell, local facet): (i, j) over the facet's two vertices ----
__global__ void __launch_bounds__(256) k_fxq_ds(int64_t nent, const int64_t *__restrict__ ent_packed,
                                                const int32_t *__restrict__ ent_pairs, FxqArgs A) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t e = gid / 4;
  const int l = (int)(gid % 4);
  if (e >= nent) return;
  int64_t c;
  int lf;
  if (ent_packed) { c = ent_packed[2 * e + 1] >> 8; lf = (int)(ent_packed[2 * e + 1] & 0xff); }
  else { c = ent_pairs[2 * e]; lf = ent_pairs[2 * e + 1]; }
  RectGeo R;
  if (!rect_load(A.cells, A.x, c, R)) { *A.bad = 1; return; }
  int va, vb, axis;
  double sign;
  quad_facet(lf, &va, &vb, &axis, &sign);
  const int ends[2] = {va, vb};
  const int i = l / 2, j = l % 2;
  const double len = axis == 0 ? R.hy : R.hx;   // normal along x: the facet runs along y
  const int32_t col = (int32_t)((1 + axis) * A.nv + R.v[ends[j]]);
  if (A.dofmap[col] < 0) return;  // y lives on cut cells only
  slot_add(A.slots, A.dofmap[R.v[ends[i]]], col, len * m1(i, j) * sign);
}

// --- dS(tag): main.py:132-135  sigma avg(h) int_F [grad u . n][grad v . n]; 64 lanes per facet -----------------
__global__ void __launch_bounds__(256) k_fxq_facets(int64_t nlist, const int32_t *__restrict__ list, FxqArgs A) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t e = gid / 64;
  const int l = (int)(gid % 64);
  if (e >= nlist) return;
  const int a = l / 8, b = l % 8;
  const int64_t f = list[e];
  constexpr Gauss3 g3 = gauss3();
  int32_t dofs[8];
  double J[3][8], hsum = 0.0, len = 0.0;
  for (int side = 0; side < 2; ++side) {
    QuadFacetSide S;
    if (!quad_facet_side(f, side, A.c2f, A.f2c, A.cells, A.x, S)) { *A.bad = 1; return; }
    if (side == 0) len = S.len;
    hsum += S.R.h;
    for (int q = 0; q < 3; ++q) {
      const double xi = S.axis == 0 ? S.fixed : g3.x[q], eta = S.axis == 1 ? S.fixed : g3.x[q];
      for (int i = 0; i < 4; ++i) {
        double val, gx, gy;
        q1_at(i, xi, eta, S.R, &val, &gx, &gy);
        J[q][side * 4 + i] = S.sign * (S.axis == 0 ? gx : gy);
      }
    }
    for (int i = 0; i < 4; ++i) dofs[side * 4 + i] = S.R.v[i];
  }
  double acc = 0.0;
  for (int q = 0; q < 3; ++q) acc += g3.w[q] * J[q][a] * J[q][b];
  slot_add(A.slots, A.dofmap[dofs[a]], dofs[b], A.sigma * 0.5 * hsum * len * acc);
}

static int assemble_flux_quad_with_capacity(phx_mesh *m, const double *params, int facet_tag, int nq,
                                            const double *dphi, const double *df, const double *dg, int W,
                                            phx_system **out) {
  const int64_t nent = 3 * m->nv + m->nc;
  PHX_REQUIRE(nent < INT32_MAX, PHX_ERR_VALUE, "too many DoFs for 32-bit column keys");
  SystemBuild sys(m, nent, nent, W);
  DevTemps tmp(m->stream);
  phx_system *s = sys.s;
  const dim3 block(256);
  FxqArgs A;
  memset(&A, 0, sizeof(A));
  A.cells = m->cells; A.x = m->x; A.ctags = m->cell_tags; A.c2f = m->c2f; A.f2c = m->f2c;
  A.phi = dphi; A.f = df; A.g = dg; A.nv = m->nv; A.nf = m->nf;
  A.gamma = params[0]; A.sigma = params[1]; A.kappa = params[2];
  A.nq = nq;
  {  // Gauss-Legendre points on [0, 1] by Newton iteration on the Legendre polynomial
    for (int i = 0; i < nq; ++i) {
      double z = cos(3.14159265358979323846 * (i + 0.75) / (nq + 0.5)), pp = 1.0;
      for (int it = 0; it < 100; ++it) {
        double p1 = 1.0, p2 = 0.0;
        for (int j = 0; j < nq; ++j) { const double p3 = p2; p2 = p1; p1 = ((2.0 * j + 1.0) * z * p2 - j * p3) / (j + 1.0); }
        pp = nq * (z * p1 - p2) / (z * z - 1.0);
        const double z1 = z;
        z = z1 - p1 / pp;
        if (fabs(z - z1) < 1e-15) break;
      }
      A.gx[i] = 0.5 * (1.0 - z);
      A.gw[i] = 1.0 / ((1.0 - z * z) * pp * pp);
    }
  }
  PHX_CHECK(rect_bad_alloc(m, tmp, &A.bad));
  // ---- active numbering: Jacobi only, as on simplices (phx_assemble_flux.inc.hip)
  uint8_t *flags = nullptr;
  PHX_HIP(tmp.alloc(&flags, (size_t)nent));
  PHX_HIP(hipMemsetAsync(flags, 0, (size_t)nent, m->stream));
  k_fxq_mark_active<<<dim3((unsigned)phx_div_up(m->nc, 256)), block, 0, m->stream>>>(m->nc, A, flags);
  PHX_CHECK(number_single_block(m, s, tmp, flags, nent, "no active DoF: no cell is tagged 1 or 2"));
  A.dofmap = s->dof_of_vertex_u;
  // ---- work lists and integration entities
  int32_t *l_om = nullptr, *l_cut = nullptr, *l_fac = nullptr;
  int64_t n_om = 0, n_cut = 0, n_fac = 0;
  PHX_CHECK(build_list(m, m->nc, SelOmega{m->cell_tags}, &l_om, &n_om));
  tmp.adopt(l_om);
  PHX_CHECK(build_list(m, m->nc, SelCut{m->cell_tags}, &l_cut, &n_cut));
  tmp.adopt(l_cut);
  PHX_CHECK(build_list(m, m->nf, SelFacetTagInterior{m->facet_tags, m->f2c, facet_tag}, &l_fac, &n_fac));
  tmp.adopt(l_fac);
  DsEntities ds;
  PHX_CHECK(ds_entities(m, &ds));
  PHX_REQUIRE_GRID(n_om * 16, "Neumann / Robin cell assembly");
  PHX_REQUIRE_GRID(n_fac * 64, "Neumann / Robin facet assembly");
  // ---- slots
  PHX_CHECK(slots_alloc(m, (int64_t)s->n * W, W, &sys.sl));
  PHX_CHECK(rhs_alloc(m, s));
  A.rhs = s->rhs; A.slots = sys.sl;
  // ---- element kernels
  if (n_om) k_fxq_bulk<<<dim3((unsigned)phx_div_up(n_om * 16, 256)), block, 0, m->stream>>>(n_om, l_om, A);
  if (n_cut) k_fxq_cut<<<dim3((unsigned)n_cut), dim3(64), 0, m->stream>>>(n_cut, l_cut, A);
  if (ds.n) k_fxq_ds<<<dim3((unsigned)phx_div_up(ds.n * 4, 256)), block, 0, m->stream>>>(ds.n, ds.packed, ds.pairs, A);
  if (n_fac) k_fxq_facets<<<dim3((unsigned)phx_div_up(n_fac * 64, 256)), block, 0, m->stream>>>(n_fac, l_fac, A);
  PHX_HIP(hipGetLastError());
  PHX_CHECK(rect_bad_check(m, A.bad));
  return sys.finish((int32_t)nent, out);
}
