// Residual error indicators of the weak-Dirichlet Poisson scheme and the Doerfler selection: included
// by phx_assemble.hip after the assemblers, in front of phx_recover.inc.hip (shares Geo / load_cell / gram, the conical rules, the P2 basis, the Q1-rectangle layer,
// DevTemps / to_device and the fixed-order sums of phx_errors.inc.hip).  For a cell T of Omega_h (cell tag 1 or 2)
//   eta_T^2 = R_T + J_T + B_T
//   R_T = h_T^2 int_T (f_h + Laplace u_h)^2
//   J_T = 1/2 sum_{F of T, other cell T' in Omega_h} h_F int_F [grad u_h . n]^2,   h_F = (h_T + h_T') / 2
//   B_T = h_T^-2 int_T (u_h - phi_h p_h / h_T - u_D)^2   on cut cells (tag 2), else 0
// -- the residuals of the terms the assemblers integrate (main.py:113-151), an indicator for marking and effectivity
// studies, not a proven two-sided bound.  Every rule is exact for its integrand.
// J is a GATHER: a cell walks its own facets through c2f / f2c, loads the neighbour and evaluates the jump itself, so
// every interior facet is evaluated twice and nothing is added atomically: the per-cell numbers and (through per-block
// partial sums folded in a fixed order) the three totals repeat bit for bit.
// The rest of this translation unit is compiled without FMA contraction.
#pragma clang fp contract(off)

#include <float.h>

struct SelOmegaBytes {
  const int8_t *t;
  __host__ __device__ bool operator()(const int32_t &c) const { return test(t[c], c); }
  __host__ __device__ const int8_t *bytes() const { return t; }           // byte fast path of phx_select.h
  __host__ __device__ bool test(int tag, int32_t) const { const int v = tag & PHX_TAG_MASK; return v == 1 || v == 2; }
};

#define EST_THREADS 256
#define EST_MAX_BLOCKS 65536   // grid-stride beyond: the grid and with it the order of the sums depend on the list length only

struct EstArgs {
  const int32_t *cells;
  const double *x;
  const int8_t *ctags;
  const int32_t *c2f, *f2c, *c2e;
  int32_t nvert;
  int64_t nc;
  const double *u, *p, *phi, *f, *ud;
  double *out;          // [3][nc]: R, J, B
  DevRule cut, facet;   // P1: cell rule of degree 4; P2: cell rule of degree 8, facet rule of degree 2
};

// the cell across facet f of cell c when it exists and lies in Omega_h, else -1
__device__ __forceinline__ int64_t est_neighbour(const EstArgs &E, int64_t c, int32_t f) {
  const int32_t a = E.f2c[2 * (int64_t)f], b = E.f2c[2 * (int64_t)f + 1];
  const int32_t o = a == (int32_t)c ? b : a;
  if (o < 0) return -1;
  const int t = E.ctags[o] & PHX_TAG_MASK;
  return (t == 1 || t == 2) ? (int64_t)o : -1;
}

// fixed-order block sums of the three parts (as k_cell_errors): lane tree inside the wave, then the waves in order;
// entry 3 of a block's partial is zero so that k_sum_partials folds them
__device__ __forceinline__ void est_block_sums(const double *s, double *__restrict__ partial) {
  __shared__ double sh[EST_THREADS / 64][3];
  for (int k = 0; k < 3; ++k) {
    double t = s[k];
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = 0.0;
    if (threadIdx.x < 3) for (int wv = 0; wv < EST_THREADS / 64; ++wv) t += sh[wv][threadIdx.x];
    partial[(int64_t)blockIdx.x * 4 + threadIdx.x] = t;
  }
}

// --- P1: one lane per listed cell.  R in closed form (f_h^T M_T f_h), the jump is a constant per facet, B with the
// conical rule of degree 4 ---------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(EST_THREADS)
k_estimate_p1(int64_t nlist, const int32_t *__restrict__ list, EstArgs E, double *__restrict__ partial) {
  constexpr int N = D + 1;
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t e = blockIdx.x * (int64_t)EST_THREADS + threadIdx.x; e < nlist; e += gridDim.x * (int64_t)EST_THREADS) {
    const int64_t c = list[e];
    int32_t v[N];
    double X[N][D];
    load_cell<D>(E.cells, E.x, c, v, X);
    Geo<D> G;
    simplex_geometry<D>(X, G);
    double un[N], gu[D];
    for (int d = 0; d < D; ++d) gu[d] = 0.0;
    double sf = 0.0, sff = 0.0;
    for (int i = 0; i < N; ++i) {
      un[i] = E.u[v[i]];
      const double fi = E.f[v[i]];
      sf += fi; sff += fi * fi;
      for (int d = 0; d < D; ++d) gu[d] += un[i] * G.g[i][d];
    }
    // int_T f_h^2 = |T| / ((D+1)(D+2)) sum_ij (1 + d_ij) f_i f_j
    const double R = G.h * G.h * G.vol * (sf * sf + sff) * (1.0 / ((D + 1) * (D + 2)));
    double J = 0.0;
    for (int lf = 0; lf < N; ++lf) {
      const int64_t o = est_neighbour(E, c, E.c2f[c * N + lf]);
      if (o < 0) continue;
      int32_t v2[N];
      double X2[N][D];
      load_cell<D>(E.cells, E.x, o, v2, X2);
      Geo<D> G2;
      simplex_geometry<D>(X2, G2);
      double gn = 0.0, jump = 0.0;
      for (int d = 0; d < D; ++d) gn += G.g[lf][d] * G.g[lf][d];
      gn = sqrt(gn);
      for (int d = 0; d < D; ++d) {
        double g2 = 0.0;
        for (int i = 0; i < N; ++i) g2 += E.u[v2[i]] * G2.g[i][d];
        jump += (gu[d] - g2) * (-G.g[lf][d] / gn);      // outward normal of facet lf: -g_lf / |g_lf|
      }
      const double area = D * G.vol * gn;
      J += 0.5 * (G.h + G2.h) * area * jump * jump;
    }
    J *= 0.5;
    double B = 0.0;
    if ((E.ctags[c] & PHX_TAG_MASK) == 2) {
      double a[N], ph[N], pp[N];
      for (int i = 0; i < N; ++i) { a[i] = un[i] - E.ud[v[i]]; ph[i] = E.phi[v[i]]; pp[i] = E.p[v[i]]; }
      const double h1 = 1.0 / G.h;
      double acc = 0.0;
      for (int q = 0; q < E.cut.nq; ++q) {
        const double *lam = E.cut.lam + (int64_t)q * N;
        double aq = 0.0, phq = 0.0, ppq = 0.0;
        for (int i = 0; i < N; ++i) { aq += a[i] * lam[i]; phq += ph[i] * lam[i]; ppq += pp[i] * lam[i]; }
        const double g = aq - phq * ppq * h1;
        acc += E.cut.w[q] * g * g;
      }
      B = G.vol * acc * h1 * h1;
    }
    E.out[c] = R; E.out[E.nc + c] = J; E.out[2 * E.nc + c] = B;
    s[0] += R; s[1] += J; s[2] += B;
  }
  est_block_sums(s, partial);
}

// --- Q1 on rectangles: one lane per listed cell.  Laplace u_h = 0; R from the 1-D mass matrices; along a facet the
// normal derivative is linear, so the squared jump takes the 2-point Gauss rule; B the 3 x 3 rule -------------------------
__device__ __forceinline__ double q1_normal_derivative(const double *un, const RectGeo &R, int axis, double t) {
  return axis == 0 ? ((un[1] - un[0]) * (1.0 - t) + (un[3] - un[2]) * t) / R.hx
                   : ((un[2] - un[0]) * (1.0 - t) + (un[3] - un[1]) * t) / R.hy;
}

__global__ void __launch_bounds__(EST_THREADS)
k_estimate_q1(int64_t nlist, const int32_t *__restrict__ list, EstArgs E, double *__restrict__ partial,
              int *__restrict__ bad) {
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t e = blockIdx.x * (int64_t)EST_THREADS + threadIdx.x; e < nlist; e += gridDim.x * (int64_t)EST_THREADS) {
    const int64_t c = list[e];
    RectGeo Rg;
    if (!rect_load(E.cells, E.x, c, Rg)) *bad = 1;
    double un[4], fn[4];
    for (int i = 0; i < 4; ++i) { un[i] = E.u[Rg.v[i]]; fn[i] = E.f[Rg.v[i]]; }
    double ff = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) ff += fn[i] * fn[j] * (m1(i & 1, j & 1) * m1(i >> 1, j >> 1));
    const double R = Rg.h * Rg.h * (Rg.hx * Rg.hy) * ff;
    double J = 0.0;
    for (int lf = 0; lf < 4; ++lf) {
      const int32_t f = E.c2f[c * 4 + lf];
      const int64_t o = est_neighbour(E, c, f);
      if (o < 0) continue;
      RectGeo R2;
      if (!rect_load(E.cells, E.x, o, R2)) *bad = 1;
      int lf2 = 0;
      for (int k = 0; k < 4; ++k) if (E.c2f[o * 4 + k] == f) lf2 = k;
      int va, vb, axis, axis2;
      double sign, sign2;
      quad_facet(lf, &va, &vb, &axis, &sign);
      quad_facet(lf2, &va, &vb, &axis2, &sign2);
      double u2[4];
      for (int i = 0; i < 4; ++i) u2[i] = E.u[R2.v[i]];
      constexpr Gauss2 g = gauss2();
      double acc = 0.0;
      for (int q = 0; q < 2; ++q) {   // both cells parametrise the facet in the same direction
        const double jump = sign * q1_normal_derivative(un, Rg, axis, g.x[q]) +
                            sign2 * q1_normal_derivative(u2, R2, axis2, g.x[q]);
        acc += g.w[q] * jump * jump;
      }
      const double len = axis == 0 ? Rg.hy : Rg.hx;
      J += 0.5 * (Rg.h + R2.h) * len * acc;
    }
    J *= 0.5;
    double B = 0.0;
    if ((E.ctags[c] & PHX_TAG_MASK) == 2) {
      double a[4], ph[4], pp[4];
      for (int i = 0; i < 4; ++i) { a[i] = un[i] - E.ud[Rg.v[i]]; ph[i] = E.phi[Rg.v[i]]; pp[i] = E.p[Rg.v[i]]; }
      const double h1 = 1.0 / Rg.h;
      double acc = 0.0;
      for (int q = 0; q < 9; ++q) {
        double N[4];
        const double w = q1_tab9(q, nullptr, N, nullptr);
        double aq = 0.0, phq = 0.0, ppq = 0.0;
        for (int i = 0; i < 4; ++i) { aq += a[i] * N[i]; phq += ph[i] * N[i]; ppq += pp[i] * N[i]; }
        const double gq = aq - phq * ppq * h1;
        acc += w * gq * gq;
      }
      B = (Rg.hx * Rg.hy) * acc * h1 * h1;
    }
    E.out[c] = R; E.out[E.nc + c] = J; E.out[2 * E.nc + c] = B;
    s[0] += R; s[1] += J; s[2] += B;
  }
  est_block_sums(s, partial);
}

// --- P2: one wavefront per listed cell, four per block, as the P2 element kernels.  The basis values at the points of
// the degree-8 cell rule belong to the RULE: the block tabulates them once in LDS.  Per cell the first NB lanes bring the
// cell's nodal values into LDS, lane = quadrature point evaluates the residual (degree 4) and, on cut cells, the
// boundary term (degree 8), lane = (local facet, facet point) loads the neighbour across that facet and evaluates the
// jump of the normal derivative (degree 2 on the facet); a lane tree adds the wave's contributions in a fixed order.
#define EST_P2_NQMAX(D) ((D) == 3 ? 125 : 25)
#define EST_P2_FACET_NQMAX 4
template <int D>
__global__ void __launch_bounds__(EST_THREADS)
k_estimate_p2(int64_t nlist, const int32_t *__restrict__ list, EstArgs E, double *__restrict__ partial) {
  using B = P2B<D>;
  constexpr int NB = B::NB, N = B::N, NE = B::NE;
  constexpr int NQS = EST_P2_NQMAX(D);   // odd: the rows of the table start in distinct banks
  __shared__ double NqT[NB][NQS], wq[NQS];
  __shared__ double wu[4][NB], wp[4][NB], wph[4][NB], wud[4][NB], wfn[4][NB];
  const int nq = E.cut.nq, nqf = E.facet.nq;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int i = threadIdx.x; i < NB * nq; i += EST_THREADS) {
    const int r = i / nq, q = i - r * nq;
    NqT[r][q] = B::val(r, E.cut.lam + (int64_t)q * N);
  }
  for (int q = threadIdx.x; q < nq; q += EST_THREADS) wq[q] = E.cut.w[q];
  __syncthreads();
  double s[3] = {0.0, 0.0, 0.0};   // lane 0: this wave's totals
  for (int64_t e = blockIdx.x * (int64_t)4 + wave; e < nlist; e += gridDim.x * (int64_t)4) {
    const int64_t c = list[e];
    int32_t v[N];
    double X[N][D];
    load_cell<D>(E.cells, E.x, c, v, X);
    Geo<D> G;
    simplex_geometry<D>(X, G);
    double GG[N][N];
    gram<D>(G, GG);
    const bool cut = (E.ctags[c] & PHX_TAG_MASK) == 2;
    if (lane < NB) {
      const int32_t dl = lane < N ? E.cells[c * N + lane] : E.nvert + E.c2e[c * NE + (lane - N)];
      wu[wave][lane] = E.u[dl];
      wfn[wave][lane] = E.f[dl];
      wp[wave][lane] = cut ? E.p[dl] : 0.0;
      wph[wave][lane] = cut ? E.phi[dl] : 0.0;
      wud[wave][lane] = cut ? E.ud[dl] : 0.0;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double lap = 0.0;                // Laplace u_h, constant on the cell
    for (int b = 0; b < NB; ++b) lap += wu[wave][b] * B::lapl(b, GG);
    const double h1 = 1.0 / G.h;
    double t[3] = {0.0, 0.0, 0.0};
    for (int q = lane; q < nq; q += 64) {
      double fq = 0.0;
      for (int b = 0; b < NB; ++b) fq += wfn[wave][b] * NqT[b][q];
      const double r = fq + lap;
      t[0] += wq[q] * r * r;
      if (cut) {
        double aq = 0.0, phq = 0.0, ppq = 0.0;
        for (int b = 0; b < NB; ++b) {
          const double Nb = NqT[b][q];
          aq += (wu[wave][b] - wud[wave][b]) * Nb; phq += wph[wave][b] * Nb; ppq += wp[wave][b] * Nb;
        }
        const double g = aq - phq * ppq * h1;
        t[2] += wq[q] * g * g;
      }
    }
    t[0] *= G.h * G.h * G.vol;
    t[2] *= G.vol * h1 * h1;
    if (lane < N * nqf) {
      const int lf = lane / nqf, qf = lane - lf * nqf;
      const int64_t o = est_neighbour(E, c, E.c2f[c * N + lf]);
      if (o >= 0) {
        double lam[N], nrm[D], gn = 0.0;
        facet_embed<D>(lf, E.facet.lam + (int64_t)qf * D, lam);
        for (int d = 0; d < D; ++d) {
          double gl = 0.0;
          for (int m = 0; m < N; ++m) gl = m == lf ? G.g[m][d] : gl;
          nrm[d] = gl; gn += gl * gl;
        }
        gn = sqrt(gn);
        for (int d = 0; d < D; ++d) nrm[d] = -nrm[d] / gn;       // outward normal of facet lf
        double dn = 0.0;
        for (int b = 0; b < NB; ++b) {
          double cs[N], gb = 0.0;
          B::gradc(b, lam, cs);
          for (int m = 0; m < N; ++m) {
            double gm = 0.0;
            for (int d = 0; d < D; ++d) gm += G.g[m][d] * nrm[d];
            gb += cs[m] * gm;
          }
          dn += wu[wave][b] * gb;
        }
        // the neighbour: its barycentric coordinates of the same point follow from the shared vertices
        int32_t v2[N];
        double X2[N][D];
        load_cell<D>(E.cells, E.x, o, v2, X2);
        Geo<D> G2;
        simplex_geometry<D>(X2, G2);
        double lam2[N];
        for (int j = 0; j < N; ++j) {
          double l = 0.0;
          for (int i = 0; i < N; ++i) l = v2[j] == v[i] ? lam[i] : l;
          lam2[j] = l;
        }
        double dn2 = 0.0;
        for (int b = 0; b < NB; ++b) {
          const int32_t dl = b < N ? v2[b] : E.nvert + E.c2e[o * NE + (b - N)];
          double cs[N], gb = 0.0;
          B::gradc(b, lam2, cs);
          for (int m = 0; m < N; ++m) {
            double gm = 0.0;
            for (int d = 0; d < D; ++d) gm += G2.g[m][d] * nrm[d];
            gb += cs[m] * gm;
          }
          dn2 += E.u[dl] * gb;
        }
        const double jump = dn - dn2, area = D * G.vol * gn;
        t[1] = 0.5 * (0.5 * (G.h + G2.h)) * area * E.facet.w[qf] * jump * jump;
      }
    }
    for (int k = 0; k < 3; ++k)
      for (int off = 32; off > 0; off >>= 1) t[k] += __shfl_down(t[k], off, 64);
    if (lane == 0) {
      E.out[c] = t[0]; E.out[E.nc + c] = t[1]; E.out[2 * E.nc + c] = t[2];
      s[0] += t[0]; s[1] += t[1]; s[2] += t[2];
    }
    // the next cell overwrites the per-wave tables: every lane is past its reads
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __shared__ double sh[4][3];
  if (lane == 0) for (int k = 0; k < 3; ++k) sh[wave][k] = s[k];
  __syncthreads();
  if (threadIdx.x < 4) {
    double tt = 0.0;
    if (threadIdx.x < 3) for (int wv = 0; wv < 4; ++wv) tt += sh[wv][threadIdx.x];
    partial[(int64_t)blockIdx.x * 4 + threadIdx.x] = tt;
  }
}

template <int D>
static int estimate_simplex(phx_mesh *m, int degree, EstArgs &E, int64_t nlist, const int32_t *list, DevTemps &tmp,
                            double *dsum) {
  hipStream_t st = m->stream;
  double *partial = nullptr;
  if (degree == 1) {
    PHX_CHECK(upload_rule(m, D, 4, &E.cut, tmp));
    const int64_t want = phx_div_up(nlist, (int64_t)EST_THREADS);
    const int64_t nblocks = want < EST_MAX_BLOCKS ? want : EST_MAX_BLOCKS;
    PHX_HIP(tmp.alloc(&partial, sizeof(double) * (size_t)nblocks * 4));
    k_estimate_p1<D><<<dim3((unsigned)nblocks), dim3(EST_THREADS), 0, st>>>(nlist, list, E, partial);
    k_sum_partials<<<dim3(1), dim3(256), 0, st>>>(nblocks, partial, dsum);
  } else {
    PHX_CHECK(upload_rule(m, D, 8, &E.cut, tmp));
    PHX_CHECK(upload_rule(m, D - 1, 2, &E.facet, tmp));   // facet rules carry D barycentric coordinates per point
    PHX_REQUIRE(E.cut.nq <= EST_P2_NQMAX(D), PHX_ERR_VALUE, "cell rule larger than the tables of k_estimate_p2");
    PHX_REQUIRE(E.facet.nq <= EST_P2_FACET_NQMAX, PHX_ERR_VALUE, "facet rule larger than the lanes of k_estimate_p2");
    const int64_t want = phx_div_up(nlist, (int64_t)4);
    const int64_t nblocks = want < EST_MAX_BLOCKS ? want : EST_MAX_BLOCKS;
    PHX_HIP(tmp.alloc(&partial, sizeof(double) * (size_t)nblocks * 4));
    k_estimate_p2<D><<<dim3((unsigned)nblocks), dim3(EST_THREADS), 0, st>>>(nlist, list, E, partial);
    k_sum_partials<<<dim3(1), dim3(256), 0, st>>>(nblocks, partial, dsum);
  }
  PHX_HIP(hipGetLastError());
  return PHX_OK;
}

extern "C" int phx_estimate_poisson_wd(phx_mesh *m, int degree, const double *u, const double *p, const double *phi,
                                       const double *f, const double *u_D, int loc_in, double *eta2_parts, int loc_out,
                                       double *sums3) {
  PHX_REQUIRE(m, PHX_ERR_VALUE, "phx_estimate_poisson_wd: no mesh");
  PHX_HIP(hipSetDevice(m->device));
  const bool quad = m->cell_type == PHX_QUADRILATERAL;
  PHX_REQUIRE((m->cell_type == PHX_TRIANGLE || m->cell_type == PHX_TETRAHEDRON || (quad && m->gdim == 2)) &&
                  (degree == 1 || (degree == 2 && !quad)),
              PHX_ERR_NOT_IMPLEMENTED,
              "estimate: degree 1 on triangles, tetrahedra and rectangles, degree 2 on simplices");
  PHX_REQUIRE(u && p && phi && f && u_D && eta2_parts && sums3, PHX_ERR_VALUE, "phx_estimate_poisson_wd: NULL array");
  PHX_REQUIRE(m->have_cell_tags, PHX_ERR_VALUE,
              "phx_estimate_poisson_wd: the mesh carries no cell tags -- call compute_tags_measures first");
  if (degree == 2) PHX_CHECK(phx_mesh_build_edges(m));
  hipStream_t st = m->stream;
  const int64_t nc = m->nc, nd = degree == 1 ? m->nv : m->nv + m->ne;
  for (int k = 0; k < 3; ++k) sums3[k] = 0.0;
  if (nc == 0) return PHX_OK;
  DevTemps tmp(st);   // staged host inputs, the work list, partial sums, rules: returned on every path out of here
  EstArgs E{};
  PHX_CHECK(to_device(m, u, loc_in, nd, &E.u, tmp));
  PHX_CHECK(to_device(m, p, loc_in, nd, &E.p, tmp));
  PHX_CHECK(to_device(m, phi, loc_in, nd, &E.phi, tmp));
  PHX_CHECK(to_device(m, f, loc_in, nd, &E.f, tmp));
  PHX_CHECK(to_device(m, u_D, loc_in, nd, &E.ud, tmp));
  double *dout = eta2_parts;
  if (loc_out != PHX_DEVICE) PHX_HIP(tmp.alloc(&dout, sizeof(double) * 3 * (size_t)nc));
  PHX_HIP(hipMemsetAsync(dout, 0, sizeof(double) * 3 * (size_t)nc, st));   // cells outside Omega_h: exactly 0
  E.cells = m->cells; E.x = m->x; E.ctags = m->cell_tags; E.c2f = m->c2f; E.f2c = m->f2c; E.c2e = m->c2e;
  E.nvert = (int32_t)m->nv; E.nc = nc; E.out = dout;
  int32_t *list = nullptr;
  int64_t nlist = 0;
  PHX_CHECK(phx_select_indices(st, nc, SelOmegaBytes{m->cell_tags}, &list, &nlist));
  tmp.adopt(list);
  int *bad = nullptr;
  if (nlist > 0) {
    double *dsum = nullptr;
    PHX_HIP(tmp.alloc(&dsum, sizeof(double) * 4));
    if (quad) {
      PHX_CHECK(rect_bad_alloc(m, tmp, &bad));
      double *partial = nullptr;
      const int64_t want = phx_div_up(nlist, (int64_t)EST_THREADS);
      const int64_t nblocks = want < EST_MAX_BLOCKS ? want : EST_MAX_BLOCKS;
      PHX_HIP(tmp.alloc(&partial, sizeof(double) * (size_t)nblocks * 4));
      k_estimate_q1<<<dim3((unsigned)nblocks), dim3(EST_THREADS), 0, st>>>(nlist, list, E, partial, bad);
      k_sum_partials<<<dim3(1), dim3(256), 0, st>>>(nblocks, partial, dsum);
      PHX_HIP(hipGetLastError());
    } else if (m->gdim == 2) {
      PHX_CHECK(estimate_simplex<2>(m, degree, E, nlist, list, tmp, dsum));
    } else {
      PHX_CHECK(estimate_simplex<3>(m, degree, E, nlist, list, tmp, dsum));
    }
    double hsum[4] = {0.0, 0.0, 0.0, 0.0};
    PHX_HIP(hipMemcpyAsync(hsum, dsum, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
    PHX_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < 3; ++k) sums3[k] = hsum[k];
  }
  if (bad) PHX_CHECK(rect_bad_check(m, bad));
  if (loc_out != PHX_DEVICE) {
    PHX_HIP(hipMemcpyAsync(eta2_parts, dout, sizeof(double) * 3 * (size_t)nc, hipMemcpyDeviceToHost, st));
  }
  PHX_HIP(hipStreamSynchronize(st));
  return PHX_OK;
}

// --- Doerfler marking: order the cells by (eta^2 descending, index ascending), S_k the inclusive sums in that order;
// marked are the first k* cells, k* the smallest k with S_k >= theta S_n; nothing when S_n = 0.  A stable radix sort on
// the inverted bit pattern (non-negative doubles order like their bits; -0 counts as 0) carries the index, a scan with
// a fixed order of additions gives S, one kernel writes the mask: position j is marked when S_j-1 < theta S_n.
__global__ void k_dorfler_keys(int64_t n, const double *__restrict__ eta2, unsigned long long *__restrict__ keys,
                               int32_t *__restrict__ idx, int *__restrict__ bad) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += gridDim.x * (int64_t)blockDim.x) {
    const double v = eta2[i];
    if (!(v >= 0.0 && v <= DBL_MAX)) *bad = 1;    // negative, NaN, infinite
    const unsigned long long bits = v == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(v);
    keys[i] = ~bits;
    idx[i] = (int32_t)i;
  }
}

struct DorflerValue {
  __host__ __device__ double operator()(const unsigned long long &k) const {
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)~k);
#else
    const unsigned long long b = ~k;
    double v;
    memcpy(&v, &b, sizeof v);
    return v;
#endif
  }
};

// out[0] = number of marked cells, out[1] = the bad-input flag (one copy brings both to the host)
__global__ void __launch_bounds__(256)
k_dorfler_mask(int64_t n, const double *__restrict__ S, const int32_t *__restrict__ idx, double theta,
               const int *__restrict__ bad, uint8_t *__restrict__ marked, unsigned long long *__restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) out[1] = (unsigned long long)*bad;
  if (*bad) return;
  const double total = S[n - 1], target = theta * total;
  for (int64_t j0 = blockIdx.x * (int64_t)blockDim.x; j0 < n; j0 += gridDim.x * (int64_t)blockDim.x) {
    const int64_t j = j0 + threadIdx.x;
    bool mk = false;
    if (j < n) {
      mk = total > 0.0 && (j == 0 ? 0.0 : S[j - 1]) < target;
      marked[idx[j]] = mk ? 1 : 0;
    }
    const unsigned long long b = __ballot(mk);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&out[0], (unsigned long long)__popcll(b));   // an integer count
  }
}

extern "C" int phx_mark_dorfler(phx_mesh *m, int64_t n, const double *eta2, int loc_in, double theta, uint8_t *marked,
                                int loc_out, int64_t *n_marked) {
  PHX_REQUIRE(m, PHX_ERR_VALUE, "phx_mark_dorfler: no mesh");
  PHX_REQUIRE(n >= 0 && n < INT32_MAX, PHX_ERR_VALUE, "phx_mark_dorfler: %lld entries: 0 .. 2^31 - 2 expected", (long long)n);
  PHX_REQUIRE(theta > 0.0 && theta <= 1.0, PHX_ERR_VALUE, "phx_mark_dorfler: theta must lie in (0, 1]");
  PHX_REQUIRE(n_marked && (n == 0 || (eta2 && marked)), PHX_ERR_VALUE, "phx_mark_dorfler: NULL array");
  *n_marked = 0;
  if (n == 0) return PHX_OK;
  PHX_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  DevTemps tmp(st);
  const double *deta = nullptr;
  PHX_CHECK(to_device(m, eta2, loc_in, n, &deta, tmp));
  unsigned long long *keys = nullptr, *keys2 = nullptr, *dout = nullptr;
  int32_t *idx = nullptr, *idx2 = nullptr;
  double *S = nullptr;
  int *bad = nullptr;
  uint8_t *dmark = marked;
  PHX_HIP(tmp.alloc(&keys, sizeof(unsigned long long) * (size_t)n));
  PHX_HIP(tmp.alloc(&keys2, sizeof(unsigned long long) * (size_t)n));
  PHX_HIP(tmp.alloc(&idx, sizeof(int32_t) * (size_t)n));
  PHX_HIP(tmp.alloc(&idx2, sizeof(int32_t) * (size_t)n));
  PHX_HIP(tmp.alloc(&S, sizeof(double) * (size_t)n));
  PHX_HIP(tmp.alloc(&bad, sizeof(int)));
  PHX_HIP(tmp.alloc(&dout, sizeof(unsigned long long) * 2));
  if (loc_out != PHX_DEVICE) PHX_HIP(tmp.alloc(&dmark, (size_t)n));
  PHX_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
  PHX_HIP(hipMemsetAsync(dout, 0, sizeof(unsigned long long) * 2, st));
  const int64_t want = phx_div_up(n, (int64_t)256);
  const dim3 grid((unsigned)(want < EST_MAX_BLOCKS ? want : EST_MAX_BLOCKS)), block(256);
  k_dorfler_keys<<<grid, block, 0, st>>>(n, deta, keys, idx, bad);
  PHX_HIP(hipGetLastError());
  size_t bsort = 0, bscan = 0;
  PHX_HIP(phx_sort_pairs(nullptr, bsort, keys, keys2, idx, idx2, (size_t)n, 0u, 64u, st));
  const auto vals = rocprim::make_transform_iterator(keys2, DorflerValue());
  PHX_HIP(phx_inclusive_sum(nullptr, bscan, vals, S, (size_t)n, st));
  void *work = nullptr;
  const size_t bwork = bsort > bscan ? bsort : bscan;
  PHX_HIP(tmp.alloc(&work, bwork ? bwork : 16));
  PHX_HIP(phx_sort_pairs(work, bsort, keys, keys2, idx, idx2, (size_t)n, 0u, 64u, st));
  PHX_HIP(phx_inclusive_sum(work, bscan, vals, S, (size_t)n, st));
  k_dorfler_mask<<<grid, block, 0, st>>>(n, S, idx2, theta, bad, dmark, dout);
  PHX_HIP(hipGetLastError());
  unsigned long long hout[2] = {0ull, 0ull};
  PHX_HIP(hipMemcpyAsync(hout, dout, sizeof(hout), hipMemcpyDeviceToHost, st));
  PHX_HIP(hipStreamSynchronize(st));
  PHX_REQUIRE(!hout[1], PHX_ERR_VALUE, "phx_mark_dorfler: eta2 holds a negative, NaN or infinite entry");
  if (loc_out != PHX_DEVICE) {
    PHX_HIP(hipMemcpyAsync(marked, dmark, (size_t)n, hipMemcpyDeviceToHost, st));
    PHX_HIP(hipStreamSynchronize(st));
  }
  *n_marked = (int64_t)hout[0];
  return PHX_OK;
}
