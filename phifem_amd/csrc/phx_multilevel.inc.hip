// Multilevel preconditioner of P1 weak-Dirichlet systems on refined simplex meshes (include of phx_solve.hip, after
// phx_coarse.inc.hip): M^-1 = R V R^T on the u block, V one geometric-multigrid V-cycle over the refinement hierarchy
// the mesh carries, Jacobi on the p block (RestOut).  include/phifem_hip.h (phx_multilevel_setup) and DESIGN.md 7f state
// the rules, tests/multilevel_ref.py restates them in numpy.
//
// Level l holds K_l (P1 stiffness of all cells, constrained rows / columns -> identity) in SELL-64 by vertex -- entry k
// of row i at slice_ptr[i >> 6] + 64 k + (i & 63), padding = (column i, value 0) --, 1 / diag, the vectors b, r and two
// iterates (Jacobi sweeps run out of place), and the transfer from level l - 1: the restriction CSR (coarse vertex ->
// new fine vertices, ascending: phx_restrict.inc.hip) and the end vertices of the bisected edges.  All of it is copied
// from the meshes at setup and belongs to the system.  One byte array `cons` serves every level: vertex v of level l
// IS vertex v of level L.
//
// One application (no allocation, no host round trip):
//   gather + first sweep      b_L = R^T p, x = w D^-1 b_L
//   per level, going down     one more sweep; r = b - K x; b_c = restriction of r (0 at constrained), x_c = w D^-1 b_c
//   level 0                   x_0 = K_0^-1 b_0 (dense, one wavefront per row) or 11 more sweeps
//   per level, going up       x += P x_c at free vertices; two sweeps
//   scatter                   phat = (D) x_L at the active vertices
namespace {

#define PHX_ML_OMEGA (2.0 / 3.0)
#define PHX_ML_NU 2
#define PHX_ML_COARSE_SWEEPS 8
#define PHX_ML_DENSE_CAP 2048

struct MlLevel {
  int64_t nv = 0, nslices = 0, sell_nnz = 0;
  int64_t *slice_ptr = nullptr;
  int32_t *col = nullptr;
  double *val = nullptr, *dinv = nullptr;
  double *b = nullptr, *r = nullptr, *xa = nullptr, *xb = nullptr;
  // transfer from the level below (nvc vertices, nm bisected edges: nv = nvc + nm)
  int64_t nvc = 0, nm = 0;
  int32_t *rs_ptr = nullptr, *rs_idx = nullptr, *pairs = nullptr;
};
}  // namespace

struct phx_multilevel {
  std::vector<MlLevel> lv;
  uint8_t *cons = nullptr;     // [nv_L]
  int32_t *vpos = nullptr;     // [nv_L] solver position of the u DoF of the vertex, -1 none
  double *oscale = nullptr;    // [nv_L] what the scatter multiplies by (diag A where the SELL copy holds A D^-1), or nullptr
  double *K0inv = nullptr;     // [n0 * n0] coarse kind 1
  int coarse_kind = 0;
  int64_t points = 0;
};

namespace {
void ml_free(phx_multilevel *ml) {
  if (!ml) return;
  for (MlLevel &l : ml->lv)
    for (void *p : {(void *)l.slice_ptr, (void *)l.col, (void *)l.val, (void *)l.dinv, (void *)l.b, (void *)l.r, (void *)l.xa,
                    (void *)l.xb, (void *)l.rs_ptr, (void *)l.rs_idx, (void *)l.pairs})
      (void)phx_free(p);
  (void)phx_free(ml->cons); (void)phx_free(ml->vpos); (void)phx_free(ml->oscale); (void)phx_free(ml->K0inv);
  delete ml;
}

dim3 ml_grid(int64_t n) { return dim3((unsigned)phx_div_up(n > 0 ? n : 1, 256)); }

// ---- setup: constrained set and maps of level L
__global__ void __launch_bounds__(256)
k_ml_bnd(int64_t nbf, const int32_t *__restrict__ bfacets, const int32_t *__restrict__ cells, phx_cell_info ci,
         uint8_t *__restrict__ bnd) {
  const int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (f >= nbf) return;
  const int64_t c = bfacets[2 * f];
  const int lf = bfacets[2 * f + 1];
  for (int k = 0; k < ci.nvpf; ++k) bnd[cells[c * ci.nvpc + ci.fv[lf][k]]] = 1;
}
__global__ void __launch_bounds__(256)
k_ml_used(int64_t n, const int32_t *__restrict__ cells, uint8_t *__restrict__ used) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) used[cells[i]] = 1;
}
// cons = (boundary and no active u DoF) or vertex of no cell; count[0] += constrained boundary vertices (integer)
__global__ void __launch_bounds__(256)
k_ml_cons(int64_t nv, const uint8_t *__restrict__ bnd, const uint8_t *__restrict__ used, const int32_t *__restrict__ du,
          const int32_t *__restrict__ iperm, const int32_t *__restrict__ perm, const double *__restrict__ diag,
          uint8_t *__restrict__ cons, int32_t *__restrict__ vpos, double *__restrict__ oscale, int32_t *__restrict__ count) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v >= nv) return;
  const int32_t d = du[v];
  const bool cb = bnd[v] && d < 0;
  cons[v] = (cb || !used[v]) ? 1 : 0;
  const int32_t pos = d >= 0 ? iperm[d] : -1;
  vpos[v] = pos;
  if (oscale) oscale[v] = pos >= 0 ? diag[perm[pos]] : 0.0;
  if (cb) atomicAdd(count, 1);
}

// ---- setup: K_l.  One entry per (cell, local pair), key = row << 32 | column
template <int NV>
__global__ void __launch_bounds__(256)
k_ml_entries(int64_t nc, const double *__restrict__ x, const int32_t *__restrict__ cells, uint64_t *__restrict__ key,
             double *__restrict__ val) {
  constexpr int GD = NV - 1;
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  int32_t v[NV];
  double p[NV][GD], g[NV][GD], scale;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    v[i] = cells[c * NV + i];
#pragma unroll
    for (int a = 0; a < GD; ++a) p[i][a] = x[(int64_t)v[i] * GD + a];
  }
  if constexpr (NV == 3) {
    // g_i = rotated edge opposite vertex i (not divided by det): K_ij = g_i . g_j / (2 |det|)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
      g[i][0] = -(p[i2][1] - p[i1][1]);
      g[i][1] = p[i2][0] - p[i1][0];
    }
    const double det = (p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[1][1] - p[0][1]) * (p[2][0] - p[0][0]);
    scale = 0.5 / fabs(det);
  } else {
    double e[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int a = 0; a < 3; ++a) e[k][a] = p[k + 1][a] - p[0][a];
    // gradients times det: b x c, c x a, a x b; the first is minus their sum.  K_ij = g_i . g_j / (6 |det|)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double *u = e[(k + 1) % 3], *w = e[(k + 2) % 3];
      g[k + 1][0] = u[1] * w[2] - u[2] * w[1];
      g[k + 1][1] = u[2] * w[0] - u[0] * w[2];
      g[k + 1][2] = u[0] * w[1] - u[1] * w[0];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) g[0][a] = -(g[1][a] + g[2][a] + g[3][a]);
    const double det = e[0][0] * g[1][0] + e[0][1] * g[1][1] + e[0][2] * g[1][2];
    scale = 1.0 / (6.0 * fabs(det));
  }
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      double d = 0.0;
#pragma unroll
      for (int a = 0; a < GD; ++a) d += g[i][a] * g[j][a];
      const int64_t e_ = (c * NV + i) * NV + j;
      key[e_] = ((uint64_t)(uint32_t)v[i] << 32) | (uint32_t)v[j];
      val[e_] = scale * d;
    }
}

// first sorted entry of row `row`
__device__ __forceinline__ int64_t ml_row_begin(const uint64_t *__restrict__ key, int64_t n, int64_t row) {
  const uint64_t want = (uint64_t)row << 32;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (key[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// len[row] = distinct columns of the row (at least 1: the diagonal of a vertex of no cell)
__global__ void __launch_bounds__(256)
k_ml_rowlen(int64_t nv, int64_t n, const uint64_t *__restrict__ key, int32_t *__restrict__ len) {
  const int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (row >= nv) return;
  int64_t e = ml_row_begin(key, n, row);
  int32_t cnt = 0;
  uint64_t last = ~0ull;
  for (; e < n && (int64_t)(key[e] >> 32) == row; ++e)
    if (key[e] != last) { ++cnt; last = key[e]; }
  len[row] = cnt > 0 ? cnt : 1;
}
// widths[s] = 64 * longest row of slice s, widths[nslices] = 0
__global__ void __launch_bounds__(256)
k_ml_widths(int64_t nslices, int64_t nv, const int32_t *__restrict__ len, int64_t *__restrict__ widths) {
  const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (s > nslices) return;
  int32_t w = 0;
  if (s < nslices)
    for (int64_t i = s * 64; i < s * 64 + 64 && i < nv; ++i) w = max(w, len[i]);
  widths[s] = 64 * (int64_t)w;
}
// the entries of a row are folded in sorted order (stable sort: ascending cell, the same bits on every run)
__global__ void __launch_bounds__(256)
k_ml_fill(int64_t nv, int64_t n, const uint64_t *__restrict__ key, const double *__restrict__ kval,
          const uint8_t *__restrict__ cons, const int64_t *__restrict__ slice_ptr, int32_t *__restrict__ col,
          double *__restrict__ val, double *__restrict__ dinv) {
  const int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t nrow = ((nv + 63) >> 6) << 6;
  if (row >= nrow) return;
  const int64_t base = slice_ptr[row >> 6] + (row & 63);
  const int width = (int)((slice_ptr[(row >> 6) + 1] - slice_ptr[row >> 6]) >> 6);
  int k = 0;
  double diag = 1.0;
  if (row < nv) {
    const bool crow = cons[row] != 0;
    int64_t e = ml_row_begin(key, n, row);
    bool any = false;
    while (e < n && (int64_t)(key[e] >> 32) == row && k < width) {
      const uint64_t kk = key[e];
      double acc = kval[e];
      for (++e; e < n && key[e] == kk; ++e) acc = acc + kval[e];
      const int32_t c = (int32_t)(uint32_t)(kk & 0xffffffffull);
      double v = acc;
      if (crow) v = c == (int32_t)row ? 1.0 : 0.0;
      else if (cons[c]) v = 0.0;
      if (c == (int32_t)row) { diag = v; any = true; }
      col[base + 64 * (int64_t)k] = c;
      val[base + 64 * (int64_t)k] = v;
      ++k;
    }
    if (!any && k < width) {   // vertex of no cell (constrained): the identity row
      col[base] = (int32_t)row;
      val[base] = 1.0;
      k = 1;
    }
    dinv[row] = 1.0 / diag;
  }
  const int32_t self = (int32_t)(row < nv ? row : 0);
  for (; k < width; ++k) {
    col[base + 64 * (int64_t)k] = self;
    val[base + 64 * (int64_t)k] = 0.0;
  }
}

__global__ void __launch_bounds__(256)
k_ml_pairs(int64_t nm, const int32_t *__restrict__ list, const int32_t *__restrict__ edges, int32_t *__restrict__ pairs) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= nm) return;
  const int64_t e = list ? list[r] : r;
  pairs[2 * r] = edges[2 * e];
  pairs[2 * r + 1] = edges[2 * e + 1];
}
// A[row][col] += value over the row's SELL entries (one lane per row: no race; padding adds 0 to the diagonal)
__global__ void __launch_bounds__(256)
k_ml_dense(int64_t nv, const int64_t *__restrict__ slice_ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
           double *__restrict__ A) {
  const int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (row >= nv) return;
  const int64_t base = slice_ptr[row >> 6] + (row & 63);
  const int width = (int)((slice_ptr[(row >> 6) + 1] - slice_ptr[row >> 6]) >> 6);
  for (int k = 0; k < width; ++k) A[row * nv + col[base + 64 * (int64_t)k]] += val[base + 64 * (int64_t)k];
}

// ---- application
// b_L = R^T vin, x = w D^-1 b_L
__global__ void __launch_bounds__(256)
k_ml_gather(int64_t nv, const int32_t *__restrict__ vpos, const double *__restrict__ vin, const double *__restrict__ dinv,
            double *__restrict__ b, double *__restrict__ x) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v >= nv) return;
  const int32_t pos = vpos[v];
  const double bv = pos >= 0 ? vin[pos] : 0.0;
  b[v] = bv;
  x[v] = PHX_ML_OMEGA * dinv[v] * bv;
}
// one pass over the row: RES: out = b - K x (the residual), else out = x + w D^-1 (b - K x) (a sweep)
template <bool RES>
__global__ void __launch_bounds__(256)
k_ml_sweep(int64_t nv, const int64_t *__restrict__ slice_ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
           const double *__restrict__ dinv, const double *__restrict__ b, const double *__restrict__ x,
           double *__restrict__ out) {
  const int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (row >= nv) return;
  const int64_t s0 = slice_ptr[row >> 6];
  const int width = (int)((slice_ptr[(row >> 6) + 1] - s0) >> 6);
  const int64_t base = s0 + (row & 63);
  double acc = 0.0;
  for (int k = 0; k < width; ++k) acc += val[base + 64 * (int64_t)k] * x[col[base + 64 * (int64_t)k]];
  const double res = b[row] - acc;
  out[row] = RES ? res : x[row] + PHX_ML_OMEGA * dinv[row] * res;
}
// b_c[p] = constrained ? 0 : ((r[p] + 0.5 r[m_1]) + 0.5 r[m_2]) + ... (the gather of phx_restrict), x_c = w D_c^-1 b_c
__global__ void __launch_bounds__(256)
k_ml_restrict(int64_t nvc, const int32_t *__restrict__ ptr, const int32_t *__restrict__ idx, const uint8_t *__restrict__ cons,
              const double *__restrict__ r, const double *__restrict__ dinv_c, double *__restrict__ bc, double *__restrict__ xc) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= nvc) return;
  double acc = 0.0;
  if (!cons[p]) {
    acc = r[p];
    const int32_t j1 = ptr[p + 1];
    for (int32_t j = ptr[p]; j < j1; ++j) acc = acc + 0.5 * r[idx[j]];
  }
  bc[p] = acc;
  xc[p] = PHX_ML_OMEGA * dinv_c[p] * acc;
}
// x += P x_c at the free vertices
__global__ void __launch_bounds__(256)
k_ml_prolong_add(int64_t nv, int64_t nvc, const int32_t *__restrict__ pairs, const uint8_t *__restrict__ cons,
                 const double *__restrict__ xc, double *__restrict__ x) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v >= nv || cons[v]) return;
  const double e = v < nvc ? xc[v] : 0.5 * xc[pairs[2 * (v - nvc)]] + 0.5 * xc[pairs[2 * (v - nvc) + 1]];
  x[v] += e;
}
// phat = (D) x_L at the active vertices
__global__ void __launch_bounds__(256)
k_ml_scatter(int64_t nv, const int32_t *__restrict__ vpos, const double *__restrict__ oscale, const double *__restrict__ x,
             double *__restrict__ vout) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v >= nv) return;
  const int32_t pos = vpos[v];
  if (pos >= 0) vout[pos] = oscale ? oscale[v] * x[v] : x[v];
}

// K_l of mesh `m` (its stream is idle; everything runs on `st`)
int ml_build_matrix(phx_mesh *m, const uint8_t *cons, hipStream_t st, MlLevel &l) {
  const int nvpc = m->ci.nvpc;
  const int64_t nv = m->nv, n = m->nc * (int64_t)nvpc * nvpc;
  PHX_REQUIRE_GRID(std::max(m->nc, nv) + 320, "phx_multilevel_setup");
  DevTemps tmp(st);
  uint64_t *key = nullptr, *key2 = nullptr;
  double *val = nullptr, *val2 = nullptr;
  int32_t *len = nullptr;
  PHX_HIP(tmp.alloc(&key, sizeof(uint64_t) * (size_t)n));
  PHX_HIP(tmp.alloc(&key2, sizeof(uint64_t) * (size_t)n));
  PHX_HIP(tmp.alloc(&val, sizeof(double) * (size_t)n));
  PHX_HIP(tmp.alloc(&val2, sizeof(double) * (size_t)n));
  const dim3 block(256);
  if (m->nc > 0) {
    if (nvpc == 3) k_ml_entries<3><<<ml_grid(m->nc), block, 0, st>>>(m->nc, m->x, m->cells, key, val);
    else k_ml_entries<4><<<ml_grid(m->nc), block, 0, st>>>(m->nc, m->x, m->cells, key, val);
    PHX_HIP(hipGetLastError());
    unsigned bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < nv) ++bits;
    size_t bytes = 0;
    void *work = nullptr;
    PHX_HIP(phx_sort_pairs(nullptr, bytes, key, key2, val, val2, (size_t)n, 0u, 32u + bits, st));
    PHX_HIP(tmp.alloc(&work, bytes));
    PHX_HIP(phx_sort_pairs(work, bytes, key, key2, val, val2, (size_t)n, 0u, 32u + bits, st));
  }
  l.nv = nv;
  l.nslices = phx_div_up(nv, 64);
  PHX_HIP(tmp.alloc(&len, sizeof(int32_t) * (size_t)nv));
  PHX_HIP(phx_malloc(&l.slice_ptr, sizeof(int64_t) * (size_t)(l.nslices + 1)));
  k_ml_rowlen<<<ml_grid(nv), block, 0, st>>>(nv, n, key2, len);
  int64_t total = 0;
  PHX_CHECK(slice_offsets(st, tmp, l.nslices, [&](int64_t *widths) {
    k_ml_widths<<<ml_grid(l.nslices + 1), block, 0, st>>>(l.nslices, nv, len, widths);
  }, l.slice_ptr, &total));
  PHX_HIP(hipGetLastError());
  PHX_REQUIRE(total >= 64 * l.nslices && total < ((int64_t)1 << 40), PHX_ERR_HIP, "phx_multilevel_setup: bad SELL size %lld", (long long)total);
  l.sell_nnz = total;
  PHX_HIP(phx_malloc(&l.col, sizeof(int32_t) * (size_t)total));
  PHX_HIP(phx_malloc(&l.val, sizeof(double) * (size_t)total));
  PHX_HIP(phx_malloc(&l.dinv, sizeof(double) * (size_t)nv));
  for (double **q : {&l.b, &l.r, &l.xa, &l.xb}) PHX_HIP(phx_malloc(q, sizeof(double) * (size_t)nv));
  k_ml_fill<<<ml_grid(l.nslices * 64), block, 0, st>>>(nv, n, key2, val2, cons, l.slice_ptr, l.col, l.val, l.dinv);
  PHX_HIP(hipGetLastError());
  PHX_HIP(hipStreamSynchronize(st));   // the temporaries are freed behind their last kernel
  return PHX_OK;
}

// the transfer level l - 1 -> l, copied from the meshes
int ml_build_transfer(phx_mesh *coarse, phx_mesh *fine, hipStream_t st, MlLevel &l) {
  PHX_CHECK(phx_mesh_build_edges(coarse));
  const int64_t nvc = coarse->nv, nm = fine->rm_marked ? fine->rm_nmid : coarse->ne;
  PHX_REQUIRE(fine->nv == nvc + nm && fine->cell_type == coarse->cell_type && fine->device == coarse->device, PHX_ERR_VALUE,
              "phx_multilevel_setup: a mesh of the hierarchy is not the refinement of its parent");
  PHX_CHECK(phx_restrict_csr(coarse, fine));      // on the coarse mesh's stream, synchronised
  l.nvc = nvc; l.nm = nm;
  PHX_HIP(phx_malloc(&l.rs_ptr, sizeof(int32_t) * (size_t)(nvc + 1)));
  PHX_HIP(phx_malloc(&l.rs_idx, sizeof(int32_t) * (size_t)std::max<int64_t>(2 * nm, 1)));
  PHX_HIP(phx_malloc(&l.pairs, sizeof(int32_t) * (size_t)std::max<int64_t>(2 * nm, 1)));
  PHX_HIP(hipMemcpyAsync(l.rs_ptr, fine->rs_ptr, sizeof(int32_t) * (size_t)(nvc + 1), hipMemcpyDeviceToDevice, st));
  if (nm > 0) {
    PHX_HIP(hipMemcpyAsync(l.rs_idx, fine->rs_idx, sizeof(int32_t) * (size_t)(2 * nm), hipMemcpyDeviceToDevice, st));
    k_ml_pairs<<<ml_grid(nm), dim3(256), 0, st>>>(nm, fine->rm_marked ? fine->rm_mid : nullptr, coarse->edges, l.pairs);
    PHX_HIP(hipGetLastError());
  }
  PHX_HIP(hipStreamSynchronize(st));
  return PHX_OK;
}

int ml_build(phx_system *s, phx_multilevel *ml) {
  phx_mesh *m = s->mesh;
  hipStream_t st = m->stream;
  // levels: the chain of living parents
  std::vector<phx_mesh *> chain{m};
  for (phx_mesh *q = m; q->refined_from != 0;) {
    phx_mesh *par = phx_mesh_lookup(q->refined_from);
    if (!par || par->device != m->device) break;
    chain.push_back(par);
    q = par;
  }
  PHX_REQUIRE(chain.size() >= 2, PHX_ERR_VALUE,
              "multilevel preconditioner: the mesh has no living parent (it was not refined, or the coarse mesh is destroyed)");
  std::reverse(chain.begin(), chain.end());
  const int L = (int)chain.size() - 1;
  for (phx_mesh *q : chain) PHX_HIP(hipStreamSynchronize(q->stream));
  const int64_t nv = m->nv;
  PHX_REQUIRE_GRID(std::max(std::max(nv, m->nbf), m->nc * (int64_t)m->ci.nvpc) + 256, "phx_multilevel_setup");
  // constrained set and the maps of level L
  {
    DevTemps tmp(st);
    uint8_t *bnd = nullptr, *used = nullptr;
    int32_t *count = nullptr;
    PHX_HIP(tmp.alloc(&bnd, (size_t)nv));
    PHX_HIP(tmp.alloc(&used, (size_t)nv));
    PHX_HIP(tmp.alloc(&count, sizeof(int32_t)));
    PHX_HIP(phx_malloc(&ml->cons, (size_t)nv));
    PHX_HIP(phx_malloc(&ml->vpos, sizeof(int32_t) * (size_t)nv));
    if (!s->u_unscaled) PHX_HIP(phx_malloc(&ml->oscale, sizeof(double) * (size_t)nv));
    PHX_HIP(hipMemsetAsync(bnd, 0, (size_t)nv, st));
    PHX_HIP(hipMemsetAsync(used, 0, (size_t)nv, st));
    PHX_HIP(hipMemsetAsync(count, 0, sizeof(int32_t), st));
    const dim3 block(256);
    if (m->nbf > 0) k_ml_bnd<<<ml_grid(m->nbf), block, 0, st>>>(m->nbf, m->bfacets, m->cells, m->ci, bnd);
    k_ml_used<<<ml_grid(m->nc * m->ci.nvpc), block, 0, st>>>(m->nc * (int64_t)m->ci.nvpc, m->cells, used);
    k_ml_cons<<<ml_grid(nv), block, 0, st>>>(nv, bnd, used, s->dof_of_vertex_u, s->iperm, s->perm, s->diag, ml->cons, ml->vpos,
                                            ml->oscale, count);
    PHX_HIP(hipGetLastError());
    int32_t hcount = 0;
    PHX_HIP(hipMemcpyAsync(&hcount, count, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    PHX_HIP(hipStreamSynchronize(st));
    PHX_REQUIRE(hcount > 0, PHX_ERR_VALUE,
                "multilevel preconditioner: no constrained boundary vertex (every boundary vertex is active): K is singular");
  }
  ml->lv.resize((size_t)L + 1);
  for (int l = 0; l <= L; ++l) {
    PHX_CHECK(ml_build_matrix(chain[(size_t)l], ml->cons, st, ml->lv[(size_t)l]));
    if (l > 0) PHX_CHECK(ml_build_transfer(chain[(size_t)l - 1], chain[(size_t)l], st, ml->lv[(size_t)l]));
    ml->points += chain[(size_t)l]->nv;
  }
  MlLevel &l0 = ml->lv[0];
  ml->coarse_kind = 0;
  if (l0.nv <= PHX_ML_DENSE_CAP) {
    const size_t bytes = sizeof(double) * (size_t)l0.nv * (size_t)l0.nv;
    PHX_HIP(phx_malloc(&ml->K0inv, bytes));
    PHX_HIP(hipMemsetAsync(ml->K0inv, 0, bytes, st));
    k_ml_dense<<<ml_grid(l0.nv), dim3(256), 0, st>>>(l0.nv, l0.slice_ptr, l0.col, l0.val, ml->K0inv);
    PHX_HIP(hipGetLastError());
    int singular = 0;
    PHX_CHECK(dense_inverse_inplace(ml->K0inv, (int)l0.nv, st, &singular));
    PHX_REQUIRE(!singular, PHX_ERR_VALUE, "multilevel preconditioner: the coarsest level matrix is singular");
    ml->coarse_kind = 1;
  }
  return PHX_OK;
}

// the kind of system PHX_OPT_MULTILEVEL speaks of: P1 weak Dirichlet on triangles or tetrahedra
bool ml_kind_served(const phx_system *s) {
  const phx_mesh *m = s->mesh;
  return (m->cell_type == PHX_TRIANGLE || m->cell_type == PHX_TETRAHEDRON) && !s->u_p2_block && !s->p2s &&
         s->u_vertex_block && !s->u_weighted && s->el_nblk == 0;
}

int ml_setup(phx_system *s) {
  if (s->ml) return PHX_OK;
  phx_mesh *m = s->mesh;
  PHX_REQUIRE(m->cell_type == PHX_TRIANGLE || m->cell_type == PHX_TETRAHEDRON, PHX_ERR_NOT_IMPLEMENTED,
              "multilevel preconditioner: triangles and tetrahedra are implemented");
  PHX_REQUIRE(!s->u_p2_block && !s->p2s, PHX_ERR_NOT_IMPLEMENTED, "multilevel preconditioner: degree 1 is implemented");
  PHX_REQUIRE(!m->is_submesh, PHX_ERR_NOT_IMPLEMENTED, "multilevel preconditioner: sub-meshes are not implemented");
  PHX_REQUIRE(m->p2_coarse == 0, PHX_ERR_NOT_IMPLEMENTED, "multilevel preconditioner: not combined with the coarse-space correction");
  PHX_REQUIRE(s->u_vertex_block && !s->u_weighted && s->el_nblk == 0, PHX_ERR_NOT_IMPLEMENTED,
              "multilevel preconditioner: P1 weak-Dirichlet systems are implemented");
  PHX_REQUIRE(!m->facet_exempt && !m->slab_cut && m->box_nglob[2] == m->box_n[2] && m->box_nglob[1] == m->box_n[1] &&
                  m->box_nglob[0] == m->box_n[0],
              PHX_ERR_VALUE, "multilevel preconditioner: slabs and partitioned ranks are not served");
  PHX_REQUIRE(!s->structured && !s->outer && !m->is_box && !m->on_box_lattice && s->precond_state != 1, PHX_ERR_NOT_IMPLEMENTED,
              "multilevel preconditioner: the lattice preconditioner serves this mesh (a Kuhn box)");
  PHX_REQUIRE(s->n > 0 && s->nu > 0 && s->dof_of_vertex_u && s->iperm && s->diag, PHX_ERR_VALUE,
              "multilevel preconditioner: empty system");
  PHX_HIP(hipSetDevice(m->device));
  phx_multilevel *ml = new phx_multilevel();
  const int rc = ml_build(s, ml);
  if (rc != PHX_OK) {
    (void)hipStreamSynchronize(m->stream);
    ml_free(ml);
    return rc;
  }
  s->ml = ml;
  return PHX_OK;
}

// `n` sweeps from `x` (other buffer `y`); -> where the result is
double *ml_sweeps(const MlLevel &l, hipStream_t st, int n, double *x, double *y) {
  for (int i = 0; i < n; ++i) {
    k_ml_sweep<false><<<ml_grid(l.nv), dim3(256), 0, st>>>(l.nv, l.slice_ptr, l.col, l.val, l.dinv, l.b, x, y);
    std::swap(x, y);
  }
  return x;
}

// vout = P vin on the u rows (the other rows are written by RestOut)
int ml_apply(phx_system *s, const double *vin, double *vout) {
  phx_multilevel *ml = s->ml;
  hipStream_t st = s->mesh->stream;
  const int L = (int)ml->lv.size() - 1;
  const dim3 block(256);
  std::vector<double *> cur((size_t)L + 1);
  {
    MlLevel &t = ml->lv[(size_t)L];
    k_ml_gather<<<ml_grid(t.nv), block, 0, st>>>(t.nv, ml->vpos, vin, t.dinv, t.b, t.xa);
  }
  for (int l = L; l >= 1; --l) {
    MlLevel &f = ml->lv[(size_t)l], &c = ml->lv[(size_t)l - 1];
    double *x = ml_sweeps(f, st, PHX_ML_NU - 1, f.xa, f.xb);
    cur[(size_t)l] = x;
    k_ml_sweep<true><<<ml_grid(f.nv), block, 0, st>>>(f.nv, f.slice_ptr, f.col, f.val, f.dinv, f.b, x, f.r);
    k_ml_restrict<<<ml_grid(c.nv), block, 0, st>>>(c.nv, f.rs_ptr, f.rs_idx, ml->cons, f.r, c.dinv, c.b, c.xa);
  }
  {
    MlLevel &c = ml->lv[0];
    if (ml->coarse_kind == 1) {
      k_cc_gemv<<<dim3((unsigned)phx_div_up(c.nv, 4)), block, 0, st>>>((int)c.nv, ml->K0inv, c.b, c.xb);
      cur[0] = c.xb;
    } else {
      cur[0] = ml_sweeps(c, st, 2 * PHX_ML_NU + PHX_ML_COARSE_SWEEPS - 1, c.xa, c.xb);
    }
  }
  for (int l = 1; l <= L; ++l) {
    MlLevel &f = ml->lv[(size_t)l];
    double *x = cur[(size_t)l], *y = x == f.xa ? f.xb : f.xa;
    k_ml_prolong_add<<<ml_grid(f.nv), block, 0, st>>>(f.nv, f.nvc, f.pairs, ml->cons, cur[(size_t)l - 1], x);
    cur[(size_t)l] = ml_sweeps(f, st, PHX_ML_NU, x, y);
  }
  MlLevel &t = ml->lv[(size_t)L];
  k_ml_scatter<<<ml_grid(t.nv), block, 0, st>>>(t.nv, ml->vpos, ml->oscale, cur[(size_t)L], vout);
  PHX_HIP(hipGetLastError());
  return PHX_OK;
}
}  // namespace

void phx_multilevel_destroy(phx_multilevel *ml) { ml_free(ml); }

extern "C" int phx_multilevel_setup(phx_system *s) {
  PHX_REQUIRE(s && s->mesh, PHX_ERR_VALUE, "phx_multilevel_setup: bad arguments");
  return ml_setup(s);
}
