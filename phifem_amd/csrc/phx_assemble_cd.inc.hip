// Convection-diffusion in the P1 x P1 weak-Dirichlet scheme (include of phx_assemble.hip):
//   c u + beta . grad u - div(kappa grad u) = f + c g,  kappa_h nodal P1 > 0,  beta_h nodal P1 [nv][d],  c >= 0,  F = f + c g
// Per cell, g_j = grad N_j:  T_kj = beta_k . g_j,  s_j = grad kappa . g_j,  Q_kj = c delta_kj + T_kj - s_j (the strong
// operator on N_j is sum_k lambda_k Q_kj),  bb_T = mean of beta_k,  ks_T = kb_T + h_T |bb_T|,  tau_T = h_T^2 / ks_T,
// ks_F = kb_F + avg(h) |bb_F|:
//   a = (kappa grad u, grad v)_{dx(1,2)} + c (u, v)_{dx(1,2)} + (beta . grad u, v)_{dx(1,2)} - (kappa d_n u, v)_{ds(100)}
//     + supg tau_T (L u, beta . grad v)_{dx(1,2)}
//     + pen ks_T h_T^-2 (u - phi p / h_T, v - phi q / h_T)_{dx(2)} + stab tau_T (L u, L v)_{dx(2)}
//     + stab avg(h) |F| ks_F ([d_n u], [d_n v])_{dS(2,3)},       L u = c u + beta . grad u - grad kappa . grad u
//   L = (F, v)_{dx(1,2)} + supg tau_T (F, beta . grad v)_{dx(1,2)} + pen ks_T h_T^-2 (u_D, v - phi q / h_T)_{dx(2)}
//     + stab tau_T (F, L v)_{dx(2)}
// Closed forms, with col_j(X) = sum_k X_kj and cN = 1 / ((d+1)(d+2)):
//   (beta . grad N_j, N_i) = |T| cN (col_j(T) + T_ij),   (X N_j, Y N_i) = |T| cN (col_i(Y) col_j(X) + sum_k Y_ki X_kj)
// The boundary term carries no beta (the advection term is not integrated by parts): k_diff_ds is launched as it is.
// Device helpers and host scaffold are shared; the matrix kernels write no right-hand side (k_cd_rhs does, also per time
// step from phx_system_update_rhs).  tests/convection_ref.py restates the forms in numpy.
//
// Compiled without FMA contraction, like the diffusion file before it.
#pragma clang fp contract(off)

struct CdArgs {
  AsmArgs A;
  const double *kappa, *beta;   // [nv], [nv][D]
  double c, supg;
};

// --- beta_h finite everywhere, max |beta_v|, and pe_max = max over the cells of Omega_h of h_T |bb_T| / kb_T.  Fixed-order
// reduction in k_diff_kappa_check's manner: block b reduces its slice of the vertices and its slice of the cells (a tree
// over the block), k_cd_fold folds the block records in index order.  kappa_h has passed diff_check_kappa before. -------
template <int D>
__global__ void __launch_bounds__(256)
k_cd_check(int64_t nv, int64_t nc, const int32_t *__restrict__ cells, const double *__restrict__ x,
           const int8_t *__restrict__ ctags, const double *__restrict__ kappa, const double *__restrict__ beta,
           double *__restrict__ part) {
  __shared__ double cnt[256], lb[256], lpe[256];
  constexpr int N = D + 1;
  double bad = 0.0, bmax = 0.0, pe = 0.0;
  {
    const int64_t per = (nv + gridDim.x - 1) / gridDim.x;
    const int64_t lo = blockIdx.x * per, hi = lo + per < nv ? lo + per : nv;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
      double s = 0.0;
      bool ok = true;
      for (int d = 0; d < D; ++d) {
        const double b = beta[i * D + d];
        ok = ok && fabs(b) <= 1.79e308;          // false for NaN and +-inf
        s += b * b;
      }
      if (ok) bmax = fmax(bmax, sqrt(s));
      else bad += 1.0;
    }
  }
  {
    const int64_t per = (nc + gridDim.x - 1) / gridDim.x;
    const int64_t lo = blockIdx.x * per, hi = lo + per < nc ? lo + per : nc;
    for (int64_t c = lo + threadIdx.x; c < hi; c += 256) {
      const int t = ctags[c] & PHX_TAG_MASK;
      if (t != 1 && t != 2) continue;
      int32_t v[N];
      double X[N][D];
      load_cell<D>(cells, x, c, v, X);
      double h2 = 0.0, sk = 0.0, bb[D];
      for (int d = 0; d < D; ++d) bb[d] = 0.0;
      for (int i = 0; i < N; ++i) {
        sk += kappa[v[i]];
        for (int d = 0; d < D; ++d) bb[d] += beta[(int64_t)v[i] * D + d];
        for (int j = i + 1; j < N; ++j) {
          double s = 0.0;
          for (int d = 0; d < D; ++d) { const double e = X[i][d] - X[j][d]; s += e * e; }
          h2 = fmax(h2, s);
        }
      }
      double s = 0.0;
      for (int d = 0; d < D; ++d) s += bb[d] * bb[d];
      pe = fmax(pe, sqrt(h2) * sqrt(s) / sk);    // the two factors 1 / N cancel; fmax drops a NaN from a bad beta
    }
  }
  cnt[threadIdx.x] = bad; lb[threadIdx.x] = bmax; lpe[threadIdx.x] = pe;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      cnt[threadIdx.x] += cnt[threadIdx.x + s];
      lb[threadIdx.x] = fmax(lb[threadIdx.x], lb[threadIdx.x + s]);
      lpe[threadIdx.x] = fmax(lpe[threadIdx.x], lpe[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { part[3 * blockIdx.x] = cnt[0]; part[3 * blockIdx.x + 1] = lb[0]; part[3 * blockIdx.x + 2] = lpe[0]; }
}
__global__ void k_cd_fold(int nblocks, const double *__restrict__ part, double *__restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double bad = 0.0, bmax = 0.0, pe = 0.0;
  for (int b = 0; b < nblocks; ++b) { bad += part[3 * b]; bmax = fmax(bmax, part[3 * b + 1]); pe = fmax(pe, part[3 * b + 2]); }
  out[0] = bad; out[1] = bmax; out[2] = pe;
}

// PHX_ERR_VALUE unless every entry of beta_h is finite; *bmax = max |beta_v|, *peclet = pe_max
static int cd_check_beta(phx_mesh *m, const double *dkappa, const double *dbeta, double *bmax, double *peclet) {
  DevTemps tmp(m->stream);
  double *part = nullptr;
  const int nblocks = (int)std::min<int64_t>(phx_div_up(std::max<int64_t>(std::max(m->nv, m->nc), 1), 2048), DIFF_CHECK_BLOCKS);
  PHX_HIP(tmp.alloc(&part, sizeof(double) * 3 * (size_t)(nblocks + 1)));
  if (m->gdim == 2)
    k_cd_check<2><<<dim3((unsigned)nblocks), dim3(256), 0, m->stream>>>(m->nv, m->nc, m->cells, m->x, m->cell_tags, dkappa, dbeta, part);
  else
    k_cd_check<3><<<dim3((unsigned)nblocks), dim3(256), 0, m->stream>>>(m->nv, m->nc, m->cells, m->x, m->cell_tags, dkappa, dbeta, part);
  k_cd_fold<<<dim3(1), dim3(64), 0, m->stream>>>(nblocks, part, part + 3 * nblocks);
  PHX_HIP(hipGetLastError());
  double res[3] = {0.0, 0.0, 0.0};
  PHX_HIP(hipMemcpyAsync(res, part + 3 * nblocks, sizeof(res), hipMemcpyDeviceToHost, m->stream));
  PHX_HIP(hipStreamSynchronize(m->stream));
  PHX_REQUIRE(res[0] == 0.0, PHX_ERR_VALUE, "beta_h: %lld of %lld vertices carry an entry that is not finite", (long long)res[0],
              (long long)m->nv);
  *bmax = res[1];
  *peclet = res[2];
  return PHX_OK;
}

// What the element kernels need of one cell beside its geometry: kb_T, ks_T = kb_T + h_T |bb_T|, col_j(T) = (d+1) bb_T . g_j
// and s_j.  Every loop has constant bounds, so the tables stay in registers.
template <int D>
__device__ __forceinline__ void cd_cell(const Geo<D> &G, const double *kap, const double (*bet)[D], double *kb, double *ks,
                                        double *colT, double *s) {
  constexpr int N = D + 1;
  double sk = 0.0, bb[D], b2 = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) bb[d] = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    sk += kap[k];
#pragma unroll
    for (int d = 0; d < D; ++d) bb[d] += bet[k][d];
  }
#pragma unroll
  for (int d = 0; d < D; ++d) b2 += bb[d] * bb[d];
  *kb = sk * (1.0 / N);
  *ks = *kb + G.h * (sqrt(b2) * (1.0 / N));
#pragma unroll
  for (int j = 0; j < N; ++j) {
    colT[j] = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) colT[j] += bb[d] * G.g[j][d];
  }
  diff_slopes<D>(G, kap, s);
}

// entry q of a table of D + 1 values without dynamic indexing.  The chain starts from 0, not from t[0]: a chain that
// equals t[q] for every q is folded back into an indexed load, which puts the table into private memory
template <int N>
__device__ __forceinline__ double cd_pick(const double *t, int q) {
  double r = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) r = k == q ? t[k] : r;
  return r;
}

// --- the terms over dx(1,2): one thread per ACTIVE VERTEX gathers row i of
//   kb |T| g_i . g_j + c |T| M2[i][j] + |T| cN (col_j(T) + T_ij) + supg tau |T| cN (col_i(T) col_j(Q) + sum_k T_ki Q_kj)
// over its star (k_diff_rows' layout: LDS row table, one writer per row).  With Q_kj = c delta_kj + T_kj - s_j the last sum
// is c T_ji + sum_k T_ki T_kj - s_j col_i(T): the lane keeps col(T), s, column i of T and g_i, and forms T_kj = beta_k . g_j
// where it is used -- no 4 x 4 table is held. ----------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(ROW_THREADS)
k_cd_rows(int64_t nv, const int64_t *__restrict__ v2c_ptr, const int32_t *__restrict__ v2c_idx, CdArgs P) {
  __shared__ int32_t lcol[ROW_LDS_SLOTS * ROW_THREADS];
  __shared__ double lval[ROW_LDS_SLOTS * ROW_THREADS];
  const AsmArgs &A = P.A;
  const int64_t vtx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (vtx >= nv) return;
  const int32_t row = A.du[vtx];
  if (row < 0) return;
  RowAcc acc{lcol, lval, (int)threadIdx.x, &A.slots, row};
  for (int k = 0; k < ROW_LDS_SLOTS; ++k) lcol[k * ROW_THREADS + threadIdx.x] = -1;
  constexpr int N = D + 1;
  constexpr double c2 = D == 3 ? 1.0 / 20.0 : 1.0 / 12.0;   // = cN
  const bool det = A.slots.emax != nullptr;
  for (int64_t e = v2c_ptr[vtx]; e < v2c_ptr[vtx + 1]; ++e) {
    const int64_t c = v2c_idx[e];
    const int t = A.ctags[c] & PHX_TAG_MASK;
    if (t != 1 && t != 2) continue;
    int32_t v[N];
    double X[N][D];
    load_cell<D>(A.cells, A.x, c, v, X);
    Geo<D> G;
    simplex_geometry<D>(X, G);
    int i = 0;
    double kap[N], bet[N][D];
#pragma unroll
    for (int q = 0; q < N; ++q) {
      if (v[q] == (int32_t)vtx) i = q;
      kap[q] = P.kappa[v[q]];
#pragma unroll
      for (int d = 0; d < D; ++d) bet[q][d] = P.beta[(int64_t)v[q] * D + d];
    }
    double kb, ks, colT[N], s[N];
    cd_cell<D>(G, kap, bet, &kb, &ks, colT, s);
    const double wsupg = P.supg * (G.h * G.h) / ks * G.vol * c2;
    double gi[D], bi[D], Tki[N];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      gi[d] = 0.0; bi[d] = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) { gi[d] = k == i ? G.g[k][d] : gi[d]; bi[d] = k == i ? bet[k][d] : bi[d]; }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
      Tki[k] = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) Tki[k] += bet[k][d] * gi[d];
    }
    const double colTi = cd_pick<N>(colT, i);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double k = 0.0, Tij = 0.0, tt = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) { k += gi[d] * G.g[j][d]; Tij += bi[d] * G.g[j][d]; }
#pragma unroll
      for (int q = 0; q < N; ++q) {
        double Tqj = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) Tqj += bet[q][d] * G.g[j][d];
        tt += Tki[q] * Tqj;
      }
      const double colQj = P.c + colT[j] - N * s[j];
      const double val = kb * G.vol * k + P.c * G.vol * c2 * (i == j ? 2.0 : 1.0) + G.vol * c2 * (colT[j] + Tij) +
                         wsupg * (colTi * colQj + (P.c * Tki[j] + tt - s[j] * colTi));
      if (det) slot_add(A.slots, row, v[j], val);
      else acc.add(v[j], val);
    }
  }
  if (det) return;
  for (int k = 0; k < ROW_LDS_SLOTS; ++k) {
    const int32_t key = lcol[k * ROW_THREADS + threadIdx.x];
    if (key != -1) slot_add_owned(A.slots, row, key, lval[k * ROW_THREADS + threadIdx.x]);
  }
}

// --- cut cells: 64 lanes per cell, lane = (a, b) of the mixed (u,p) x (u,p) element tensor (k_diff_cut's layout).  Penalty
// blocks weighted by ks_T; the (u,u) lane adds stab tau |T| cN (col_i(Q) col_j(Q) + sum_k Q_ki Q_kj). ------------------
template <int D>
__global__ void __launch_bounds__(256) k_cd_cut(int64_t nlist, const int32_t *__restrict__ list, CdArgs P) {
  const AsmArgs &A = P.A;
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t e = gid >> 6;
  if (e >= nlist) return;
  constexpr int N = D + 1;
  const int a = (int)(gid & 63) >> 3, b = (int)(gid & 7);
  if (a >= 2 * N || b >= 2 * N) return;
  const int64_t c = list[e];
  int32_t v[N];
  double X[N][D];
  load_cell<D>(A.cells, A.x, c, v, X);
  Geo<D> G;
  simplex_geometry<D>(X, G);
  constexpr double c2 = D == 3 ? 1.0 / 20.0 : 1.0 / 12.0;
  constexpr double c3 = D == 3 ? 1.0 / 120.0 : 1.0 / 60.0;
  constexpr double c4 = D == 3 ? 1.0 / 840.0 : 1.0 / 360.0;
  const int i = a % N, j = b % N;
  const bool ap = a >= N, bp = b >= N;
  double ph[N], kap[N], bet[N][D], sp = 0.0;
#pragma unroll
  for (int q = 0; q < N; ++q) {
    ph[q] = A.phi[v[q]]; kap[q] = P.kappa[v[q]]; sp += ph[q];
#pragma unroll
    for (int d = 0; d < D; ++d) bet[q][d] = P.beta[(int64_t)v[q] * D + d];
  }
  double kb, ks, colT[N], s[N];
  cd_cell<D>(G, kap, bet, &kb, &ks, colT, s);
  const double h1 = 1.0 / G.h;
  const double gam = A.gamma * ks * G.vol;
  double val;
  if (!ap && !bp) {
    double gi[D], gj[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      gi[d] = gj[d] = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) { gi[d] = k == i ? G.g[k][d] : gi[d]; gj[d] = k == j ? G.g[k][d] : gj[d]; }
    }
    const double si = cd_pick<N>(s, i), sj = cd_pick<N>(s, j);
    const double colQi = P.c + cd_pick<N>(colT, i) - N * si, colQj = P.c + cd_pick<N>(colT, j) - N * sj;
    double qq = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double Tki = 0.0, Tkj = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) { Tki += bet[k][d] * gi[d]; Tkj += bet[k][d] * gj[d]; }
      qq += ((k == i ? P.c : 0.0) + Tki - si) * ((k == j ? P.c : 0.0) + Tkj - sj);
    }
    val = gam * h1 * h1 * c2 * (i == j ? 2.0 : 1.0) + A.sigma * (G.h * G.h) / ks * G.vol * c2 * (colQi * colQj + qq);
  } else if (ap != bp) {
    const double phi = cd_pick<N>(ph, i), phj = cd_pick<N>(ph, j);
    val = -gam * h1 * h1 * h1 * c3 * (i == j ? 2.0 : 1.0) * (sp + phi + phj);
  } else {
    double m4 = 0.0;
    for (int k = 0; k < N; ++k)
      for (int l = 0; l < N; ++l) m4 += mult4(i, j, k, l) * ph[k] * ph[l];
    val = gam * h1 * h1 * h1 * h1 * c4 * m4;
  }
  const int32_t row = ap ? A.dp[v[i]] : A.du[v[i]];
  const int32_t col = bp ? A.nv + v[j] : v[j];
  slot_add(A.slots, row, col, val);
}

// --- ghost penalty stab avg(h) |F| ks_F ([d_n u], [d_n v]) over the l_fac work list: k_diff_facets with
// ks_F = kb_F + avg(h) |bb_F|.  avg(h) comes from the coordinates of the macro-element's D + 2 vertices (facet_macro hands
// out only the product stab avg(h) |F|). ---------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256) k_cd_facets(int64_t nlist, const int32_t *__restrict__ list, CdArgs P) {
  const AsmArgs &A = P.A;
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= nlist) return;
  constexpr int N = D + 1, M = D + 2;
  const int64_t f = list[e];
  int32_t vd[M];
  double Jd[M], w;
  facet_macro<D>(A, f, vd, Jd, &w);
  // vd[0 .. N-1] are the vertices of the first cell: the facet's are all but the one opposite f; vd[N] is the second
  // cell's vertex opposite f
  const int64_t c0 = A.f2c[2 * f];
  int lf = 0;
#pragma unroll
  for (int k = 0; k < N; ++k)
    if (A.c2f[c0 * N + k] == (int32_t)f) lf = k;
  double Xd[M][D];
#pragma unroll
  for (int a = 0; a < M; ++a)
#pragma unroll
    for (int d = 0; d < D; ++d) Xd[a][d] = A.x[(int64_t)vd[a] * D + d];
  double skf = 0.0, bb[D], h0 = 0.0, h1 = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) bb[d] = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (k != lf) {
      skf += P.kappa[vd[k]];
#pragma unroll
      for (int d = 0; d < D; ++d) bb[d] += P.beta[(int64_t)vd[k] * D + d];
    }
#pragma unroll
    for (int l = k + 1; l < M; ++l) {
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) { const double t = Xd[k][d] - Xd[l][d]; s += t * t; }
      if (l < N) h0 = fmax(h0, s);                                   // a pair of the first cell
      if (k != lf && (l == N || l != lf)) h1 = fmax(h1, s);          // a pair of the second cell: facet vertices and vd[N]
    }
  }
  double b2 = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) b2 += bb[d] * bb[d];
  const double hav = 0.5 * (sqrt(h0) + sqrt(h1));
  w *= skf * (1.0 / D) + hav * (sqrt(b2) * (1.0 / D));
  int32_t rows[M];
#pragma unroll
  for (int a = 0; a < M; ++a) rows[a] = A.du[vd[a]];
#pragma unroll
  for (int a = 0; a < M; ++a)
#pragma unroll
    for (int b = 0; b < M; ++b) slot_add(A.slots, rows[a], vd[b], w * Jd[a] * Jd[b]);
}

struct CdRhsArgs {
  int64_t nu;
  const int64_t *full_of_active;
  const int32_t *dp;
  const int64_t *v2c_ptr;
  const int32_t *v2c_idx;
  const int32_t *cells;
  const double *x;
  const int8_t *ctags;
  const double *kappa, *beta, *phi, *f, *g, *ud;   // g may be null
  double c, gamma, sigma, supg;
  double *rhs;
};

// The linear form as a gather (k_diff_rhs' manner): one lane per active vertex walks its star in v2c order and evaluates
// its u row and its p row from the closed forms.  One writer and one order of additions per row, no atomics.
//   u row: |T| cN (sum F + F_i) + supg tau |T| cN (col_i(T) sum F + sum_k T_ki F_k)
//          on cut cells + stab tau |T| cN (col_i(Q) sum F + c F_i + sum_k T_ki F_k - s_i sum F) + pen ks h^-2 (u_D, N_i)
template <int D>
__global__ void __launch_bounds__(256) k_cd_rhs(CdRhsArgs R) {
  constexpr int N = D + 1;
  constexpr double c2 = D == 3 ? 1.0 / 20.0 : 1.0 / 12.0;
  constexpr double c3 = D == 3 ? 1.0 / 120.0 : 1.0 / 60.0;
  for (int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; a < R.nu; a += (int64_t)gridDim.x * blockDim.x) {
    const int64_t vtx = R.full_of_active[a];
    const int32_t prow = R.dp[vtx];
    double ru = 0.0, rp = 0.0;
    for (int64_t e = R.v2c_ptr[vtx]; e < R.v2c_ptr[vtx + 1]; ++e) {
      const int64_t cell = R.v2c_idx[e];
      const int t = R.ctags[cell] & PHX_TAG_MASK;
      if (t != 1 && t != 2) continue;
      int32_t v[N];
      double X[N][D];
      load_cell<D>(R.cells, R.x, cell, v, X);
      Geo<D> G;
      simplex_geometry<D>(X, G);
      int i = 0;
      double F[N], kap[N], bet[N][D], sF = 0.0;
#pragma unroll
      for (int q = 0; q < N; ++q) {
        if (v[q] == (int32_t)vtx) i = q;
        F[q] = R.g ? R.f[v[q]] + R.c * R.g[v[q]] : R.f[v[q]];
        sF += F[q];
        kap[q] = R.kappa[v[q]];
#pragma unroll
        for (int d = 0; d < D; ++d) bet[q][d] = R.beta[(int64_t)v[q] * D + d];
      }
      double kb, ks, colT[N], s[N];
      cd_cell<D>(G, kap, bet, &kb, &ks, colT, s);
      const double Fi = cd_pick<N>(F, i), colTi = cd_pick<N>(colT, i);
      double gi[D];
#pragma unroll
      for (int d = 0; d < D; ++d) {
        gi[d] = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) gi[d] = k == i ? G.g[k][d] : gi[d];
      }
      double tF = 0.0;     // sum_k T_ki F_k
#pragma unroll
      for (int k = 0; k < N; ++k) {
        double Tki = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) Tki += bet[k][d] * gi[d];
        tF += Tki * F[k];
      }
      const double tau = (G.h * G.h) / ks;
      ru += G.vol * c2 * (sF + Fi);   // int F N_i
      ru += R.supg * tau * G.vol * c2 * (colTi * sF + tF);
      if (t == 1) continue;
      double ph[N], ud[N], sp = 0.0, sud = 0.0;
#pragma unroll
      for (int q = 0; q < N; ++q) { ph[q] = R.phi[v[q]]; ud[q] = R.ud[v[q]]; sp += ph[q]; sud += ud[q]; }
      const double si = cd_pick<N>(s, i), phi_i = cd_pick<N>(ph, i), ud_i = cd_pick<N>(ud, i);
      const double colQi = R.c + colTi - N * si;
      ru += R.sigma * tau * G.vol * c2 * (colQi * sF + (R.c * Fi + tF - si * sF));
      const double h1 = 1.0 / G.h, gam = R.gamma * ks * G.vol;
      ru += gam * h1 * h1 * c2 * (sud + ud_i);
      double bq = 0.0;
#pragma unroll
      for (int q = 0; q < N; ++q) bq += ud[q] * (i == q ? 2.0 : 1.0) * (sp + phi_i + ph[q]);
      rp += -gam * h1 * h1 * h1 * c3 * bq;
    }
    R.rhs[a] = ru;
    if (prow >= 0) R.rhs[prow] = rp;
  }
}

static int cd_update_rhs(phx_system *s, const double *dphi, const double *df, const double *dg, const double *dud) {
  phx_mesh *m = s->mesh;
  PHX_CHECK(build_v2c(m));
  if (s->n == 0) return PHX_OK;
  CdRhsArgs R{s->nu, s->full_of_active, s->dof_of_vertex_p, m->v2c_ptr, m->v2c_idx, m->cells, m->x, m->cell_tags,
              s->diff_kappa, s->cd_beta, dphi, df, dg, dud, s->react_c, s->react_pen, s->react_stab, s->cd_supg, s->rhs};
  const dim3 grid((unsigned)std::min<int64_t>(phx_div_up(std::max<int64_t>(s->nu, 1), 256), 1 << 16));
  if (m->gdim == 2) k_cd_rhs<2><<<grid, dim3(256), 0, m->stream>>>(R);
  else k_cd_rhs<3><<<grid, dim3(256), 0, m->stream>>>(R);
  PHX_HIP(hipGetLastError());
  return PHX_OK;
}

// the element kernels of one pass, in stream order: vertex rows (first: they own their rows on the cleared slots), cut
// cells, boundary term (the diffusion kernel: it carries no beta), ghost penalty
static int cd_launch_pass(phx_mesh *m, const CdArgs &P, const P1Work &w) {
  const int D = m->gdim;
  const dim3 block(256);
  {
    const dim3 g((unsigned)phx_div_up(m->nv, ROW_THREADS)), b(ROW_THREADS);
    if (D == 2) k_cd_rows<2><<<g, b, 0, m->stream>>>(m->nv, m->v2c_ptr, m->v2c_idx, P);
    else k_cd_rows<3><<<g, b, 0, m->stream>>>(m->nv, m->v2c_ptr, m->v2c_idx, P);
  }
  if (w.n_cut > 0) {
    PHX_REQUIRE_GRID(w.n_cut * 64, "cut-cell assembly");
    const dim3 g((unsigned)phx_div_up(w.n_cut * 64, 256));
    if (D == 2) k_cd_cut<2><<<g, block, 0, m->stream>>>(w.n_cut, w.l_cut, P);
    else k_cd_cut<3><<<g, block, 0, m->stream>>>(w.n_cut, w.l_cut, P);
  }
  PHX_HIP(hipGetLastError());
  DsEntities ds;
  PHX_CHECK(ds_entities(m, &ds));
  if (ds.n > 0) {
    const DiffArgs Pd{P.A, P.kappa, P.c};
    const dim3 g((unsigned)phx_div_up(ds.n * 16, 256));
    if (D == 2) k_diff_ds<2><<<g, block, 0, m->stream>>>(ds.n, ds.packed, ds.pairs, Pd);
    else k_diff_ds<3><<<g, block, 0, m->stream>>>(ds.n, ds.packed, ds.pairs, Pd);
  }
  if (w.n_fac > 0) {
    const dim3 g((unsigned)phx_div_up(w.n_fac, 256));
    if (D == 2) k_cd_facets<2><<<g, block, 0, m->stream>>>(w.n_fac, w.l_fac, P);
    else k_cd_facets<3><<<g, block, 0, m->stream>>>(w.n_fac, w.l_fac, P);
  }
  PHX_HIP(hipGetLastError());
  return PHX_OK;
}

struct CdData {
  double pen, stab, supg, c, contrast, bmax, peclet;
  const double *kappa, *beta, *phi, *f, *g, *ud;   // device
};

static int assemble_cd_with_capacity(phx_mesh *m, const CdData &d, int W, phx_system **out) {
  SystemBuild sys(m, m->nv, 2 * m->nv, W);
  phx_system *s = sys.s;
  s->u_vertex_block = true;
  s->react = true;
  s->react_c = d.c; s->react_pen = d.pen; s->react_stab = d.stab;
  s->diff_contrast = d.contrast;
  s->cd_supg = d.supg; s->cd_peclet = d.peclet; s->cd_beta_max = d.bmax;
  // the system's own copies of kappa_h and beta_h: phx_system_update_rhs evaluates the linear form again with them
  PHX_HIP(phx_malloc(&s->diff_kappa, sizeof(double) * (size_t)m->nv));
  PHX_HIP(hipMemcpyAsync(s->diff_kappa, d.kappa, sizeof(double) * (size_t)m->nv, hipMemcpyDeviceToDevice, m->stream));
  PHX_HIP(phx_malloc(&s->cd_beta, sizeof(double) * (size_t)m->nv * m->gdim));
  PHX_HIP(hipMemcpyAsync(s->cd_beta, d.beta, sizeof(double) * (size_t)m->nv * m->gdim, hipMemcpyDeviceToDevice, m->stream));
  CdArgs P;
  AsmArgs &A = P.A;
  A.cells = m->cells; A.x = m->x; A.ctags = m->cell_tags; A.ftags = m->facet_tags;
  A.c2f = m->c2f; A.f2c = m->f2c;
  A.phi = d.phi; A.f = d.f; A.ud = d.ud; A.gamma = d.pen; A.sigma = d.stab;
  A.nv = (int32_t)m->nv;
  P.kappa = s->diff_kappa; P.beta = s->cd_beta; P.c = d.c; P.supg = d.supg;
  {
    DevTemps tmp(m->stream);
    PHX_CHECK(p1_number(m, s, tmp));
    PHX_REQUIRE(s->n > 0, PHX_ERR_VALUE, "no active DoF: no cell is tagged 1 or 2");
    P1Work w;
    PHX_CHECK(p1_work_lists(m, tmp, w));
    PHX_CHECK(rhs_alloc(m, s));
    A.du = s->dof_of_vertex_u; A.dp = s->dof_of_vertex_p; A.rhs = s->rhs;
    const int64_t nslots = s->n * W;
    PHX_CHECK(slots_alloc(m, nslots, W, &sys.sl));
    bool det = false;
    PHX_CHECK(det_alloc(m, sys.sl, nslots, s->n, &det));
    for (int pass = det ? 1 : 0; pass <= (det ? 2 : 0); ++pass) {
      sys.sl.pass = pass;
      A.slots = sys.sl;
      PHX_CHECK(cd_launch_pass(m, P, w));
    }
    PHX_CHECK(det_finish(m, sys.sl, nslots, s->n, s->rhs));
    // the matrix kernels add nothing to the right-hand side: the gather writes every row of it
    PHX_CHECK(cd_update_rhs(s, d.phi, d.f, d.g, d.ud));
  }
  return sys.finish((int32_t)m->nv, out);
}

extern "C" int phx_assemble_convection_wd(phx_mesh *m, double pen_coef, double stab_coef, double supg_coef, double reaction,
                                          const double *kappa_h, const double *beta_h, const double *phi_h, const double *f_h,
                                          const double *g_h, const double *u_D, int loc, phx_system **out) {
  PHX_HIP(hipSetDevice(m->device));
  PHX_REQUIRE(m->cell_type == PHX_TRIANGLE || m->cell_type == PHX_TETRAHEDRON, PHX_ERR_NOT_IMPLEMENTED,
              "convection-diffusion is assembled on triangles and tetrahedra only");
  bool slab = m->facet_exempt != nullptr || m->slab_cut;
  for (int a = 0; a < m->gdim; ++a) slab = slab || (m->box_nglob[a] > 0 && m->box_nglob[a] != m->box_n[a]);
  PHX_REQUIRE(!slab, PHX_ERR_NOT_IMPLEMENTED, "convection-diffusion: slabs and partitioned ranks are not served");
  PHX_REQUIRE(reaction >= 0.0 && reaction <= 1.79e308, PHX_ERR_VALUE, "reaction = %g: a finite value >= 0", reaction);
  PHX_REQUIRE(supg_coef >= 0.0 && supg_coef <= 1.79e308, PHX_ERR_VALUE, "supg_coef = %g: a finite value >= 0", supg_coef);
  PHX_REQUIRE(m->have_cell_tags && m->have_facet_tags, PHX_ERR_VALUE,
              "cell and facet tags must be computed before assembly");
  DevTemps staged(m->stream);
  CdData d{pen_coef, stab_coef, supg_coef, reaction, 1.0, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  PHX_CHECK(to_device(m, kappa_h, loc, m->nv, &d.kappa, staged));
  PHX_CHECK(diff_check_kappa(m, d.kappa, &d.contrast));
  PHX_CHECK(to_device(m, beta_h, loc, m->nv * m->gdim, &d.beta, staged));
  PHX_CHECK(cd_check_beta(m, d.kappa, d.beta, &d.bmax, &d.peclet));
  PHX_CHECK(build_v2c(m));
  PHX_CHECK(to_device(m, phi_h, loc, m->nv, &d.phi, staged));
  PHX_CHECK(to_device(m, f_h, loc, m->nv, &d.f, staged));
  if (g_h) PHX_CHECK(to_device(m, g_h, loc, m->nv, &d.g, staged));
  PHX_CHECK(to_device(m, u_D, loc, m->nv, &d.ud, staged));
  PHX_CHECK(phx_begin_timing(m));
  const auto run = [&](int W) { return assemble_cd_with_capacity(m, d, W, out); };
  int rc = m->gdim == 3 ? retry_capacity({64, 128, 256}, run) : retry_capacity({32, 64, 128}, run);
  if (rc == PHX_OK) rc = phx_end_timing(m, 2);
  return rc;
}

extern "C" int phx_convection_info(const phx_system *s, double *out) {
  PHX_REQUIRE(s != nullptr && s->cd_beta != nullptr && out != nullptr, PHX_ERR_VALUE,
              "phx_convection_info: the system was not built by phx_assemble_convection_wd");
  out[0] = s->cd_peclet; out[1] = s->cd_beta_max; out[2] = s->cd_supg; out[3] = s->diff_contrast;
  return PHX_OK;
}
