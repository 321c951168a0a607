// Variable-coefficient diffusion in the P1 x P1 weak-Dirichlet scheme (include of phx_assemble.hip):
//   c u - div(kappa grad u) = f + c g,  kappa_h nodal P1 > 0,  c >= 0 constant,  F = f + c g,
//   kb_T / kb_F = mean of kappa_h over the vertices of a cell / facet, s_j = grad kappa . grad N_j (constant per cell)
//   a = (kappa grad u, grad v)_{dx(1,2)} + c (u, v)_{dx(1,2)} - (kappa d_n u, v)_{ds(100)}
//     + pen kb_T h_T^-2 (u - phi p / h_T, v - phi q / h_T)_{dx(2)}
//     + stab h_T^2 / kb_T (c u - grad kappa . grad u, c v - grad kappa . grad v)_{dx(2)}
//     + stab avg(h) (kappa [d_n u], [d_n v])_{dS(2,3)}
//   L = (F, v)_{dx(1,2)} + pen kb_T h_T^-2 (u_D, v - phi q / h_T)_{dx(2)} + stab h_T^2 / kb_T (F, c v - grad kappa . grad v)_{dx(2)}
// Every term carries kappa, so the element kernels are this file's own; the device helpers (load_cell, simplex_geometry,
// slot_add, slot_add_owned, RowAcc, mult4, facet_macro) and the host scaffold are shared.  The matrix kernels write no
// right-hand side: it comes from the gather kernel that phx_system_update_rhs runs per time step.
// tests/diffusion_ref.py restates the forms in numpy.
//
// Compiled without FMA contraction, like the reaction file before it.
#pragma clang fp contract(off)

struct DiffArgs {
  AsmArgs A;
  const double *kappa;
  double c;
};

// kappa_h > 0 and finite everywhere, and its smallest and largest entry.  Fixed-order reduction: block b reduces its slice
// of the array (a tree over the block) to {offending entries, min, max of the others}, k_diff_kappa_fold folds the block
// records in index order.
#define DIFF_CHECK_BLOCKS 1024
__global__ void __launch_bounds__(256) k_diff_kappa_check(int64_t n, const double *__restrict__ kappa, double *__restrict__ part) {
  __shared__ double cnt[256], lmin[256], lmax[256];
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
  double bad = 0.0, kmin = 1.79e308, kmax = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const double k = kappa[i];
    if (k > 0.0 && k <= 1.79e308) { kmin = fmin(kmin, k); kmax = fmax(kmax, k); }
    else bad += 1.0;                     // NaN, 0, negative values and +inf
  }
  cnt[threadIdx.x] = bad; lmin[threadIdx.x] = kmin; lmax[threadIdx.x] = kmax;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      cnt[threadIdx.x] += cnt[threadIdx.x + s];
      lmin[threadIdx.x] = fmin(lmin[threadIdx.x], lmin[threadIdx.x + s]);
      lmax[threadIdx.x] = fmax(lmax[threadIdx.x], lmax[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { part[3 * blockIdx.x] = cnt[0]; part[3 * blockIdx.x + 1] = lmin[0]; part[3 * blockIdx.x + 2] = lmax[0]; }
}
__global__ void k_diff_kappa_fold(int nblocks, const double *__restrict__ part, double *__restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double bad = 0.0, kmin = 1.79e308, kmax = 0.0;
  for (int b = 0; b < nblocks; ++b) { bad += part[3 * b]; kmin = fmin(kmin, part[3 * b + 1]); kmax = fmax(kmax, part[3 * b + 2]); }
  out[0] = bad; out[1] = kmin; out[2] = kmax;
}

// PHX_ERR_VALUE unless every entry is finite and > 0; *contrast = max / min
static int diff_check_kappa(phx_mesh *m, const double *dkappa, double *contrast) {
  DevTemps tmp(m->stream);
  double *part = nullptr;
  const int nblocks = (int)std::min<int64_t>(phx_div_up(std::max<int64_t>(m->nv, 1), 2048), DIFF_CHECK_BLOCKS);
  PHX_HIP(tmp.alloc(&part, sizeof(double) * 3 * (size_t)(nblocks + 1)));
  k_diff_kappa_check<<<dim3((unsigned)nblocks), dim3(256), 0, m->stream>>>(m->nv, dkappa, part);
  k_diff_kappa_fold<<<dim3(1), dim3(64), 0, m->stream>>>(nblocks, part, part + 3 * nblocks);
  PHX_HIP(hipGetLastError());
  double res[3] = {0.0, 0.0, 0.0};
  PHX_HIP(hipMemcpyAsync(res, part + 3 * nblocks, sizeof(res), hipMemcpyDeviceToHost, m->stream));
  PHX_HIP(hipStreamSynchronize(m->stream));
  PHX_REQUIRE(res[0] == 0.0, PHX_ERR_VALUE, "kappa_h: %lld of %lld entries are not finite and > 0", (long long)res[0],
              (long long)m->nv);
  *contrast = res[2] / res[1];
  return PHX_OK;
}

// grad kappa = sum_k kappa_k grad N_k, s_j = grad kappa . grad N_j
template <int D>
__device__ __forceinline__ void diff_slopes(const Geo<D> &G, const double *kap, double *s) {
  double gk[D];
  for (int d = 0; d < D; ++d) {
    gk[d] = 0.0;
    for (int k = 0; k <= D; ++k) gk[d] += kap[k] * G.g[k][d];
  }
  for (int j = 0; j <= D; ++j) {
    s[j] = 0.0;
    for (int d = 0; d < D; ++d) s[j] += gk[d] * G.g[j][d];
  }
}

// --- (kappa grad u, grad v) + c (u, v) over dx(1,2): one thread per ACTIVE VERTEX gathers row i of kb_T |T| g_i . g_j +
// c |T| M2[i][j] over its star into a thread-private LDS table and writes the row once (k_assemble_rows' manner: first
// kernel on the cleared slots, one writer per row; deterministic mode goes through the exact accumulation). ------------
template <int D>
__global__ void __launch_bounds__(ROW_THREADS)
k_diff_rows(int64_t nv, const int64_t *__restrict__ v2c_ptr, const int32_t *__restrict__ v2c_idx, DiffArgs P) {
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
  constexpr double c2 = D == 3 ? 1.0 / 20.0 : 1.0 / 12.0;
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
    double sk = 0.0;
    for (int q = 0; q < N; ++q) { if (v[q] == (int32_t)vtx) i = q; sk += P.kappa[v[q]]; }
    const double kb = sk * (1.0 / N);
    for (int j = 0; j < N; ++j) {
      double k = 0.0;
      for (int d = 0; d < D; ++d) k += G.g[i][d] * G.g[j][d];
      const double val = kb * G.vol * k + P.c * G.vol * c2 * (i == j ? 2.0 : 1.0);
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

// --- cut cells: 64 lanes per cell, lane = (a, b) of the mixed (u,p) x (u,p) element tensor (k_assemble_cut's layout).
// Penalty blocks weighted by kb_T; the (u,u) lane adds the residual stabilisation
// stab h^2 / kb |T| (c^2 M2[i][j] - c (s_i + s_j) / (d+1) + s_i s_j). ----------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256) k_diff_cut(int64_t nlist, const int32_t *__restrict__ list, DiffArgs P) {
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
  double ph[N], kap[N], sp = 0.0, sk = 0.0;
  for (int q = 0; q < N; ++q) { ph[q] = A.phi[v[q]]; kap[q] = P.kappa[v[q]]; sp += ph[q]; sk += kap[q]; }
  const double kb = sk * (1.0 / N);
  const double h1 = 1.0 / G.h;
  const double gam = A.gamma * kb * G.vol;
  double val;
  if (!ap && !bp) {
    double s[N];
    diff_slopes<D>(G, kap, s);
    double si = 0.0, sj = 0.0;
    for (int q = 0; q < N; ++q) { si = q == i ? s[q] : si; sj = q == j ? s[q] : sj; }
    const double m2 = c2 * (i == j ? 2.0 : 1.0);
    val = gam * h1 * h1 * m2 +
          A.sigma * (G.h * G.h) / kb * G.vol * (P.c * P.c * m2 - P.c * (si + sj) * (1.0 / N) + si * sj);
  } else if (ap != bp) {
    val = -gam * h1 * h1 * h1 * c3 * (i == j ? 2.0 : 1.0) * (sp + ph[i] + ph[j]);
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

// --- boundary term -(kappa d_n u, v) over ds: 16 lanes per (cell, local facet) entity.  With n = -g_lf / |g_lf|,
// |F| = D |T| |g_lf| and int_F kappa N_i = |F| (sum_{k on F} kappa_k + kappa_i) / (D (D+1)) the entry of row i != lf,
// column j is |T| (g_j . g_lf) (sum_{k on F} kappa_k + kappa_i) / (D+1). -------------------------------------------------
template <int D>
__global__ void k_diff_ds(int64_t nent, const int64_t *__restrict__ ent_packed, const int32_t *__restrict__ ent_pairs,
                          DiffArgs P) {
  const AsmArgs &A = P.A;
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t e = gid >> 4;
  if (e >= nent) return;
  constexpr int N = D + 1;
  const int i = (int)(gid & 15) >> 2, j = (int)(gid & 3);
  if (i >= N || j >= N) return;
  int64_t c;
  int lf;
  if (ent_packed) { c = ent_packed[2 * e + 1] >> 8; lf = (int)(ent_packed[2 * e + 1] & 0xff); }
  else { c = ent_pairs[2 * e]; lf = ent_pairs[2 * e + 1]; }
  if (i == lf || lf < 0 || lf >= N) return;
  int32_t v[N];
  double X[N][D];
  load_cell<D>(A.cells, A.x, c, v, X);
  Geo<D> G;
  simplex_geometry<D>(X, G);
  double k = 0.0, skf = 0.0, ki = 0.0;
  for (int q = 0; q < N; ++q) {
    const double kq = P.kappa[v[q]];
    if (q != lf) skf += kq;
    if (q == i) ki = kq;
    double gq = 0.0;   // g_j . g_q, kept for q == lf
    for (int d = 0; d < D; ++d) gq += G.g[j][d] * G.g[q][d];
    if (q == lf) k = gq;
  }
  slot_add(A.slots, A.du[v[i]], v[j], k * G.vol * ((skf + ki) * (1.0 / N)));
}

// --- ghost penalty stab avg(h) (kappa [d_n u], [d_n v]) over the l_fac work list: one lane per facet (k_assemble_facets'
// layout), the facet tensor w J_a J_b of facet_macro weighted by kb_F. ---------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256) k_diff_facets(int64_t nlist, const int32_t *__restrict__ list, DiffArgs P) {
  const AsmArgs &A = P.A;
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= nlist) return;
  constexpr int N = D + 1, M = D + 2;
  const int64_t f = list[e];
  int32_t vd[M];
  double Jd[M], w;
  facet_macro<D>(A, f, vd, Jd, &w);
  // vd[0 .. N-1] are the vertices of the first cell: the facet's are all but the one opposite f
  const int64_t c0 = A.f2c[2 * f];
  double skf = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k)
    if (A.c2f[c0 * N + k] != (int32_t)f) skf += P.kappa[vd[k]];
  w *= skf * (1.0 / D);
  int32_t rows[M];
#pragma unroll
  for (int a = 0; a < M; ++a) rows[a] = A.du[vd[a]];
#pragma unroll
  for (int a = 0; a < M; ++a)
#pragma unroll
    for (int b = 0; b < M; ++b) slot_add(A.slots, rows[a], vd[b], w * Jd[a] * Jd[b]);
}

struct DiffRhsArgs {
  int64_t nu;
  const int64_t *full_of_active;
  const int32_t *dp;
  const int64_t *v2c_ptr;
  const int32_t *v2c_idx;
  const int32_t *cells;
  const double *x;
  const int8_t *ctags;
  const double *kappa, *phi, *f, *g, *ud;   // g may be null
  double c, gamma, sigma;
  double *rhs;
};

// The linear form as a gather (k_react_rhs' manner): one lane per active vertex walks its star in v2c order and
// evaluates its u row and its p row from the closed forms.  One writer and one order of additions per row.
template <int D>
__global__ void __launch_bounds__(256) k_diff_rhs(DiffRhsArgs R) {
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
      double F[N], sF = 0.0;
      for (int q = 0; q < N; ++q) {
        if (v[q] == (int32_t)vtx) i = q;
        F[q] = R.g ? R.f[v[q]] + R.c * R.g[v[q]] : R.f[v[q]];
        sF += F[q];
      }
      double Fi = 0.0;
      for (int q = 0; q < N; ++q) Fi = q == i ? F[q] : Fi;
      const double mF = G.vol * c2 * (sF + Fi);   // int F N_i
      ru += mF;
      if (t == 1) continue;
      double ph[N], ud[N], kap[N], s[N], sp = 0.0, sud = 0.0, sk = 0.0;
      for (int q = 0; q < N; ++q) {
        ph[q] = R.phi[v[q]]; ud[q] = R.ud[v[q]]; kap[q] = R.kappa[v[q]];
        sp += ph[q]; sud += ud[q]; sk += kap[q];
      }
      const double kb = sk * (1.0 / N);
      diff_slopes<D>(G, kap, s);
      double si = 0.0, phi_i = 0.0, ud_i = 0.0;
      for (int q = 0; q < N; ++q) { si = q == i ? s[q] : si; phi_i = q == i ? ph[q] : phi_i; ud_i = q == i ? ud[q] : ud_i; }
      ru += R.sigma * (G.h * G.h) / kb * (R.c * mF - G.vol * si * (sF * (1.0 / N)));
      const double h1 = 1.0 / G.h, gam = R.gamma * kb * G.vol;
      ru += gam * h1 * h1 * c2 * (sud + ud_i);
      double bq = 0.0;
      for (int q = 0; q < N; ++q) bq += ud[q] * (i == q ? 2.0 : 1.0) * (sp + phi_i + ph[q]);
      rp += -gam * h1 * h1 * h1 * c3 * bq;
    }
    R.rhs[a] = ru;
    if (prow >= 0) R.rhs[prow] = rp;
  }
}

static int diff_update_rhs(phx_system *s, const double *dphi, const double *df, const double *dg, const double *dud) {
  phx_mesh *m = s->mesh;
  PHX_CHECK(build_v2c(m));
  if (s->n == 0) return PHX_OK;
  DiffRhsArgs R{s->nu, s->full_of_active, s->dof_of_vertex_p, m->v2c_ptr, m->v2c_idx, m->cells, m->x, m->cell_tags,
                s->diff_kappa, dphi, df, dg, dud, s->react_c, s->react_pen, s->react_stab, s->rhs};
  const dim3 grid((unsigned)std::min<int64_t>(phx_div_up(std::max<int64_t>(s->nu, 1), 256), 1 << 16));
  if (m->gdim == 2) k_diff_rhs<2><<<grid, dim3(256), 0, m->stream>>>(R);
  else k_diff_rhs<3><<<grid, dim3(256), 0, m->stream>>>(R);
  PHX_HIP(hipGetLastError());
  return PHX_OK;
}

// the element kernels of one pass, in stream order: vertex rows (first: they own their rows on the cleared slots), cut
// cells, boundary term, ghost penalty
static int diff_launch_pass(phx_mesh *m, const DiffArgs &P, const P1Work &w) {
  const int D = m->gdim;
  const dim3 block(256);
  {
    const dim3 g((unsigned)phx_div_up(m->nv, ROW_THREADS)), b(ROW_THREADS);
    if (D == 2) k_diff_rows<2><<<g, b, 0, m->stream>>>(m->nv, m->v2c_ptr, m->v2c_idx, P);
    else k_diff_rows<3><<<g, b, 0, m->stream>>>(m->nv, m->v2c_ptr, m->v2c_idx, P);
  }
  if (w.n_cut > 0) {
    PHX_REQUIRE_GRID(w.n_cut * 64, "cut-cell assembly");
    const dim3 g((unsigned)phx_div_up(w.n_cut * 64, 256));
    if (D == 2) k_diff_cut<2><<<g, block, 0, m->stream>>>(w.n_cut, w.l_cut, P);
    else k_diff_cut<3><<<g, block, 0, m->stream>>>(w.n_cut, w.l_cut, P);
  }
  PHX_HIP(hipGetLastError());
  DsEntities ds;
  PHX_CHECK(ds_entities(m, &ds));
  if (ds.n > 0) {
    const dim3 g((unsigned)phx_div_up(ds.n * 16, 256));
    if (D == 2) k_diff_ds<2><<<g, block, 0, m->stream>>>(ds.n, ds.packed, ds.pairs, P);
    else k_diff_ds<3><<<g, block, 0, m->stream>>>(ds.n, ds.packed, ds.pairs, P);
  }
  if (w.n_fac > 0) {
    const dim3 g((unsigned)phx_div_up(w.n_fac, 256));
    if (D == 2) k_diff_facets<2><<<g, block, 0, m->stream>>>(w.n_fac, w.l_fac, P);
    else k_diff_facets<3><<<g, block, 0, m->stream>>>(w.n_fac, w.l_fac, P);
  }
  PHX_HIP(hipGetLastError());
  return PHX_OK;
}

static int assemble_diff_with_capacity(phx_mesh *m, double pen_coef, double stab_coef, double c, const double *dkappa,
                                       double contrast, const double *dphi, const double *df, const double *dg, const double *dud, int W,
                                       phx_system **out) {
  SystemBuild sys(m, m->nv, 2 * m->nv, W);
  phx_system *s = sys.s;
  s->u_vertex_block = true;
  s->react = true;
  s->react_c = c; s->react_pen = pen_coef; s->react_stab = stab_coef;
  s->diff_contrast = contrast;
  // the system's own copy of kappa_h: phx_system_update_rhs evaluates the linear form again with it
  PHX_HIP(phx_malloc(&s->diff_kappa, sizeof(double) * (size_t)m->nv));
  PHX_HIP(hipMemcpyAsync(s->diff_kappa, dkappa, sizeof(double) * (size_t)m->nv, hipMemcpyDeviceToDevice, m->stream));
  DiffArgs P;
  AsmArgs &A = P.A;
  A.cells = m->cells; A.x = m->x; A.ctags = m->cell_tags; A.ftags = m->facet_tags;
  A.c2f = m->c2f; A.f2c = m->f2c;
  A.phi = dphi; A.f = df; A.ud = dud; A.gamma = pen_coef; A.sigma = stab_coef;
  A.nv = (int32_t)m->nv;
  P.kappa = s->diff_kappa; P.c = c;
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
      PHX_CHECK(diff_launch_pass(m, P, w));
    }
    PHX_CHECK(det_finish(m, sys.sl, nslots, s->n, s->rhs));
    // the matrix kernels add nothing to the right-hand side: the gather writes every row of it
    PHX_CHECK(diff_update_rhs(s, dphi, df, dg, dud));
  }
  return sys.finish((int32_t)m->nv, out);
}

extern "C" int phx_assemble_diffusion_wd(phx_mesh *m, double pen_coef, double stab_coef, double reaction,
                                         const double *kappa_h, const double *phi_h, const double *f_h,
                                         const double *g_h, const double *u_D, int loc, phx_system **out) {
  PHX_HIP(hipSetDevice(m->device));
  PHX_REQUIRE(m->cell_type == PHX_TRIANGLE || m->cell_type == PHX_TETRAHEDRON, PHX_ERR_NOT_IMPLEMENTED,
              "variable-coefficient diffusion is assembled on triangles and tetrahedra only");
  bool slab = m->facet_exempt != nullptr || m->slab_cut;
  for (int a = 0; a < m->gdim; ++a) slab = slab || (m->box_nglob[a] > 0 && m->box_nglob[a] != m->box_n[a]);
  PHX_REQUIRE(!slab, PHX_ERR_NOT_IMPLEMENTED, "variable-coefficient diffusion: slabs and partitioned ranks are not served");
  PHX_REQUIRE(reaction >= 0.0 && reaction <= 1.79e308, PHX_ERR_VALUE, "reaction = %g: a finite value >= 0", reaction);
  PHX_REQUIRE(m->have_cell_tags && m->have_facet_tags, PHX_ERR_VALUE,
              "cell and facet tags must be computed before assembly");
  DevTemps staged(m->stream);
  const double *dkappa, *dphi, *df, *dud, *dg = nullptr;
  PHX_CHECK(to_device(m, kappa_h, loc, m->nv, &dkappa, staged));
  double contrast = 1.0;
  PHX_CHECK(diff_check_kappa(m, dkappa, &contrast));
  PHX_CHECK(build_v2c(m));
  PHX_CHECK(to_device(m, phi_h, loc, m->nv, &dphi, staged));
  PHX_CHECK(to_device(m, f_h, loc, m->nv, &df, staged));
  if (g_h) PHX_CHECK(to_device(m, g_h, loc, m->nv, &dg, staged));
  PHX_CHECK(to_device(m, u_D, loc, m->nv, &dud, staged));
  PHX_CHECK(phx_begin_timing(m));
  const auto run = [&](int W) {
    return assemble_diff_with_capacity(m, pen_coef, stab_coef, reaction, dkappa, contrast, dphi, df, dg, dud, W, out);
  };
  int rc = m->gdim == 3 ? retry_capacity({64, 128, 256}, run) : retry_capacity({32, 64, 128}, run);
  if (rc == PHX_OK) rc = phx_end_timing(m, 2);
  return rc;
}
