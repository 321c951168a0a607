// Point location and evaluation of Lagrange nodal functions at arbitrary points (include of phx_submesh.hip:
// -ffp-contract=off, the compares below are exact and the sums run in one stated order).  Stands in for
// dolfinx's Function.eval with a bounding-box tree and for interpolate_nonmatching; tests/locate_ref.py restates
// the rules in numpy.
//
// Reference coordinates: simplices lambda_1 .. lambda_d of the stored vertex order (lambda_0 = 1 - sum); rectangles
// (xi, eta) in tensor-product order.  A cell HOLDS a point when every barycentric coordinate is >= -tol (rectangles:
// xi, eta in [-tol, 1 + tol]).
//
// Two paths:
//  * closed form (generated Kuhn boxes, slabs included): cube = clamped floor((x - lo) / h) corrected against the
//    lattice planes as k_box_coords computes them, simplex = the ordering of the local coordinates, cell id = the
//    generator's numbering (k_box_cells: cube * nper + lexicographic index of the axis permutation).  No search
//    structure, no connectivity is read.  TIE RULES: a point on a lattice plane belongs to the cube ABOVE it, on the
//    upper faces of the box to the last cube; among equal local coordinates the lower axis goes first, which is the
//    lowest-numbered simplex of the cube that holds the point.
//  * bins (every other mesh): a uniform grid over the bounding box with about one bin per cell, (bin, cell) pairs
//    built as count -> scan -> fill with integer atomics and 64-bit offsets; when the pairs exceed
//    PHX_LOC_MAX_PAIRS_PER_CELL * nc the bins per axis are halved and the count runs again.  One lane per point walks
//    its bin.  DETERMINISM RULE: of all cells of the bin that hold the point the one with the SMALLEST cell index wins,
//    whatever the order the atomics filled the bin in.
#define PHX_LOC_MAX_PAIRS_PER_CELL 16

struct phx_locator {
  int64_t n[3] = {1, 1, 1};      // bins per axis
  double lo[3] = {0, 0, 0}, inv[3] = {0, 0, 0};   // bin of coordinate t along a: floor((t - lo[a]) * inv[a]), clamped
  int64_t nbins = 0, npairs = 0;
  int64_t *off = nullptr;        // [nbins + 1]
  int32_t *pairs = nullptr;      // [npairs] cells of bin b at off[b] .. off[b + 1] - 1, in no particular order
  int halvings = 0;
  double tol = 0.0;              // the cell boxes were enlarged for this tolerance
  int64_t bytes = 0;
};
void phx_locator_destroy(phx_locator *l) {
  if (!l) return;
  (void)phx_free(l->off);
  (void)phx_free(l->pairs);
  delete l;
}

namespace {

struct LocGrid { int64_t n[3]; double lo[3], inv[3]; };

__device__ __forceinline__ int64_t loc_bin_axis(const LocGrid &G, int a, double t) {
  const double s = (t - G.lo[a]) * G.inv[a];                      // monotone in t; NaN -> 0
  return s >= (double)G.n[a] ? G.n[a] - 1 : (s > 0.0 ? (int64_t)s : 0);
}

// ---- reference coordinates ----------------------------------------------------------------------------------------
// CT: 0 triangle, 1 rectangle, 2 tetrahedron.  X = the cell's vertex coordinates, r[] = the reference coordinates of p.
template <int CT> struct LocCell;
template <> struct LocCell<0> { static constexpr int NV = 3, D = 2; };
template <> struct LocCell<1> { static constexpr int NV = 4, D = 2; };
template <> struct LocCell<2> { static constexpr int NV = 4, D = 3; };

// gradients of lambda_1 .. lambda_d (rows of the inverse Jacobian)
__device__ __forceinline__ void loc_tri_inv(const double (*X)[3], double (*g)[3]) {
  const double ax = X[1][0] - X[0][0], ay = X[1][1] - X[0][1], bx = X[2][0] - X[0][0], by = X[2][1] - X[0][1];
  const double det = ax * by - bx * ay;
  g[0][0] = by / det; g[0][1] = -bx / det;
  g[1][0] = -ay / det; g[1][1] = ax / det;
}
__device__ __forceinline__ void loc_tet_inv(const double (*X)[3], double (*g)[3]) {
  double e[3][3];
  for (int i = 0; i < 3; ++i)
    for (int a = 0; a < 3; ++a) e[i][a] = X[i + 1][a] - X[0][a];
  double c[3][3];   // c[0] = e1 x e2, c[1] = e2 x e0, c[2] = e0 x e1
  for (int i = 0; i < 3; ++i) {
    const double *u = e[(i + 1) % 3], *v = e[(i + 2) % 3];
    c[i][0] = u[1] * v[2] - u[2] * v[1];
    c[i][1] = u[2] * v[0] - u[0] * v[2];
    c[i][2] = u[0] * v[1] - u[1] * v[0];
  }
  const double det = (e[0][0] * c[0][0] + e[0][1] * c[0][1]) + e[0][2] * c[0][2];
  for (int i = 0; i < 3; ++i)
    for (int a = 0; a < 3; ++a) g[i][a] = c[i][a] / det;
}

// true: the cell holds p
template <int CT>
__device__ __forceinline__ bool loc_ref_coords(const double (*X)[3], const double *p, double tol, double *r) {
  constexpr int D = LocCell<CT>::D;
  if (CT == 1) {
    r[0] = (p[0] - X[0][0]) / (X[1][0] - X[0][0]);
    r[1] = (p[1] - X[0][1]) / (X[2][1] - X[0][1]);
    return r[0] >= -tol && r[0] <= 1.0 + tol && r[1] >= -tol && r[1] <= 1.0 + tol;
  }
  double g[3][3];
  if (CT == 0) loc_tri_inv(X, g); else loc_tet_inv(X, g);
  double sum = 0.0;
  bool in = true;
  for (int i = 0; i < D; ++i) {
    double s = 0.0;
    for (int a = 0; a < D; ++a) s += g[i][a] * (p[a] - X[0][a]);
    r[i] = s;
    sum += s;
    in = in && s >= -tol;
  }
  return in && 1.0 - sum >= -tol;
}

template <int CT>
__device__ __forceinline__ void loc_load_cell(const int32_t *__restrict__ cells, const double *__restrict__ x, int64_t c,
                                              double (*X)[3]) {
  constexpr int NV = LocCell<CT>::NV, D = LocCell<CT>::D;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int64_t v = cells[c * NV + i];
#pragma unroll
    for (int a = 0; a < D; ++a) X[i][a] = x[v * D + a];
  }
}

// ---- bins: bounding box, count, fill, walk ------------------------------------------------------------------------
// per block the min / max of the vertex coordinates: part[block][2 d]; the host folds the blocks
__global__ void __launch_bounds__(256)
k_loc_bbox(int64_t nv, int d, const double *__restrict__ x, double *__restrict__ part) {
  __shared__ double sm[256][6];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x)
    for (int a = 0; a < d; ++a) {
      const double t = x[v * d + a];
      lo[a] = fmin(lo[a], t);
      hi[a] = fmax(hi[a], t);
    }
  for (int a = 0; a < 3; ++a) { sm[threadIdx.x][a] = lo[a]; sm[threadIdx.x][3 + a] = hi[a]; }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int a = 0; a < 3; ++a) {
        sm[threadIdx.x][a] = fmin(sm[threadIdx.x][a], sm[threadIdx.x + s][a]);
        sm[threadIdx.x][3 + a] = fmax(sm[threadIdx.x][3 + a], sm[threadIdx.x + s][3 + a]);
      }
    __syncthreads();
  }
  if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = sm[0][threadIdx.x];
}

// Bin range of a cell: its bounding box enlarged by `mrg` times its largest extent.  A point the cell holds with
// tolerance tol lies within (d + 1) tol extents of the box; mrg = 4 tol + 64 eps leaves room for the round-off of the
// reference coordinates.  loc_bin_axis is monotone, so the bin of such a point lies inside the range.
template <int CT>
__device__ __forceinline__ void loc_cell_range(const LocGrid &G, const int32_t *__restrict__ cells,
                                               const double *__restrict__ x, int64_t c, double mrg, int64_t *b0, int64_t *b1) {
  constexpr int NV = LocCell<CT>::NV, D = LocCell<CT>::D;
  double X[4][3];
  loc_load_cell<CT>(cells, x, c, X);
  double lo[3], hi[3], ext = 0.0;
  for (int a = 0; a < D; ++a) {
    lo[a] = hi[a] = X[0][a];
    for (int i = 1; i < NV; ++i) { lo[a] = fmin(lo[a], X[i][a]); hi[a] = fmax(hi[a], X[i][a]); }
    ext = fmax(ext, hi[a] - lo[a]);
  }
  b0[2] = b1[2] = 0;
  for (int a = 0; a < D; ++a) {
    b0[a] = loc_bin_axis(G, a, lo[a] - mrg * ext);
    b1[a] = loc_bin_axis(G, a, hi[a] + mrg * ext);
  }
}

// FILL = false: cnt[bin] += 1 per overlapped bin; true: the cell takes the next free place of each bin (cnt = cursor)
template <int CT, bool FILL>
__global__ void __launch_bounds__(256)
k_loc_bin_cells(int64_t nc, LocGrid G, const int32_t *__restrict__ cells, const double *__restrict__ x, double mrg,
                uint32_t *__restrict__ cnt, const int64_t *__restrict__ off, int32_t *__restrict__ pairs) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  int64_t b0[3], b1[3];
  loc_cell_range<CT>(G, cells, x, c, mrg, b0, b1);
  for (int64_t k = b0[2]; k <= b1[2]; ++k)
    for (int64_t j = b0[1]; j <= b1[1]; ++j)
      for (int64_t i = b0[0]; i <= b1[0]; ++i) {
        const int64_t b = i + G.n[0] * (j + G.n[1] * k);
        const uint32_t pos = atomicAdd(&cnt[b], 1u);
        if (FILL) pairs[off[b] + pos] = (int32_t)c;
      }
}

__global__ void __launch_bounds__(256)
k_loc_rect_check(int64_t nc, const int32_t *__restrict__ cells, const double *__restrict__ x, int *__restrict__ bad) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  RectGeo R;
  if (!rect_load(cells, x, c, R)) *bad = 1;
}

// sort keys of the points: their bin (bins path) -- points of one bin then sit in one wave and read the same cells
template <int D>
__global__ void __launch_bounds__(256)
k_loc_point_bins(int64_t npts, LocGrid G, const double *__restrict__ pts, uint32_t *__restrict__ key,
                 int32_t *__restrict__ iota) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= npts) return;
  int64_t b = 0, stride = 1;
  for (int a = 0; a < D; ++a) { b += stride * loc_bin_axis(G, a, pts[i * D + a]); stride *= G.n[a]; }
  key[i] = (uint32_t)b;
  iota[i] = (int32_t)i;
}

// one lane per point (order[t] = the point lane t serves, or t itself)
template <int CT>
__global__ void __launch_bounds__(256)
k_loc_walk(int64_t npts, const int32_t *__restrict__ order, const double *__restrict__ pts, LocGrid G,
           const int64_t *__restrict__ off, const int32_t *__restrict__ pairs, const int32_t *__restrict__ cells,
           const double *__restrict__ x, double tol, int32_t *__restrict__ cell_out, double *__restrict__ xref_out) {
  constexpr int D = LocCell<CT>::D;
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= npts) return;
  const int64_t i = order ? order[t] : t;
  double p[3] = {0.0, 0.0, 0.0};
  int64_t b = 0, stride = 1;
  for (int a = 0; a < D; ++a) {
    p[a] = pts[i * D + a];
    b += stride * loc_bin_axis(G, a, p[a]);
    stride *= G.n[a];
  }
  int32_t best = INT32_MAX;
  double br[3] = {0.0, 0.0, 0.0};
  const int64_t k1 = off[b + 1];
  for (int64_t k = off[b]; k < k1; ++k) {
    const int32_t c = pairs[k];
    if (c >= best) continue;
    double X[4][3], r[3];
    loc_load_cell<CT>(cells, x, c, X);
    if (loc_ref_coords<CT>(X, p, tol, r)) {
      best = c;
      for (int a = 0; a < D; ++a) br[a] = r[a];
    }
  }
  cell_out[i] = best == INT32_MAX ? -1 : best;
  for (int a = 0; a < D; ++a) xref_out[i * D + a] = br[a];
}

// ---- closed form on a generated box -----------------------------------------------------------------------------------
struct LocBox {
  int64_t n[3], off[3], nglob[3];
  double lo[3], hi[3], h[3];
};
// lattice plane i of axis a, the arithmetic of k_box_coords
__device__ __forceinline__ double loc_box_plane(const LocBox &B, int a, int64_t i) {
  const double t = (double)(B.off[a] + i) / (double)B.nglob[a];
  return B.lo[a] + (B.hi[a] - B.lo[a]) * t;
}
template <int D>
__global__ void __launch_bounds__(256)
k_loc_box(int64_t npts, LocBox B, const double *__restrict__ pts, double tol, int32_t *__restrict__ cell_out,
          double *__restrict__ xref_out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= npts) return;
  double t[3];
  int64_t o[3] = {0, 0, 0};
  for (int a = 0; a < D; ++a) {
    const double p = pts[i * D + a];
    const double s = (p - loc_box_plane(B, a, 0)) / B.h[a];
    int64_t q = s >= (double)B.n[a] ? B.n[a] - 1 : (s > 0.0 ? (int64_t)s : 0);
    double c0 = loc_box_plane(B, a, q), c1 = loc_box_plane(B, a, q + 1);
    while (q > 0 && p < c0) { --q; c1 = c0; c0 = loc_box_plane(B, a, q); }
    while (q < B.n[a] - 1 && p >= c1) { ++q; c0 = c1; c1 = loc_box_plane(B, a, q + 1); }
    o[a] = q;
    t[a] = (p - c0) / (c1 - c0);
  }
  int pm[3] = {0, 1, 2};
  for (int s = 1; s < D; ++s)       // stable insertion sort, descending: equal coordinates keep the lower axis first
    for (int j = s; j > 0 && t[pm[j - 1]] < t[pm[j]]; --j) { const int w = pm[j]; pm[j] = pm[j - 1]; pm[j - 1] = w; }
  const bool in = 1.0 - t[pm[0]] >= -tol && t[pm[D - 1]] >= -tol;
  const int64_t cube = o[0] + B.n[0] * (o[1] + B.n[1] * o[2]);
  const int simplex = D == 3 ? pm[0] * 2 + (pm[1] > pm[2] ? 1 : 0) : pm[0];   // k_box_cells: c = cube * nper + t
  cell_out[i] = in ? (int32_t)(cube * (D == 3 ? 6 : 2) + simplex) : -1;
  for (int a = 0; a < D; ++a) xref_out[i * D + a] = in ? (a + 1 < D ? t[pm[a]] - t[pm[a + 1]] : t[pm[a]]) : 0.0;
}

// ---- evaluation -------------------------------------------------------------------------------------------------------
// One lane per point.  DEG 1: N_i = lambda_i (rectangles: the Q1 products); DEG 2 (simplices): vertices
// lambda_v (2 lambda_v - 1), then the edges of PHX_ARR_C2E 4 lambda_a lambda_b.  Sums in ascending local DoF order.
template <int CT, int DEG, bool GRAD>
__global__ void __launch_bounds__(256)
k_loc_eval(int64_t npts, int64_t nc, int64_t nv, const int32_t *__restrict__ cells,
           const int32_t *__restrict__ c2e, const double *__restrict__ x, const int32_t *__restrict__ cell_of,
           const double *__restrict__ xref, int ncomp, const double *__restrict__ u, int64_t ld, double fill,
           double *__restrict__ out, double *__restrict__ gout) {
  constexpr int NV = LocCell<CT>::NV, D = LocCell<CT>::D;
  constexpr int NE = DEG == 2 ? (CT == 2 ? 6 : 3) : 0, ND = NV + NE;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= npts) return;
  const int64_t c = cell_of[i];
  if (c < 0 || c >= nc) {
    for (int q = 0; q < ncomp; ++q) {
      out[q * npts + i] = fill;
      if (GRAD)
        for (int a = 0; a < D; ++a) gout[(q * npts + i) * D + a] = fill;
    }
    return;
  }
  int64_t dof[ND];
#pragma unroll
  for (int k = 0; k < NV; ++k) dof[k] = cells[c * NV + k];
#pragma unroll
  for (int k = 0; k < NE; ++k) dof[NV + k] = nv + c2e[c * NE + k];
  double N[ND], G[ND][3];
  double r[3];
  for (int a = 0; a < D; ++a) r[a] = xref[i * D + a];
  double X[4][3];
  if (GRAD) loc_load_cell<CT>(cells, x, c, X);
  if (CT == 1) {
    const double hx = X[1][0] - X[0][0], hy = X[2][1] - X[0][1];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double lx = (k & 1) ? r[0] : 1.0 - r[0], ly = (k >> 1) ? r[1] : 1.0 - r[1];
      N[k] = lx * ly;
      if (GRAD) { G[k][0] = ((k & 1) ? 1.0 : -1.0) * ly / hx; G[k][1] = lx * ((k >> 1) ? 1.0 : -1.0) / hy; }
    }
  } else {
    double lam[NV], gl[NV][3];
    lam[0] = 1.0;
#pragma unroll
    for (int k = 0; k < D; ++k) { lam[k + 1] = r[k]; lam[0] -= r[k]; }
    if (GRAD) {
      double g[3][3];
      if (CT == 0) loc_tri_inv(X, g); else loc_tet_inv(X, g);
      for (int a = 0; a < D; ++a) {
        gl[0][a] = 0.0;
        for (int k = 0; k < D; ++k) { gl[k + 1][a] = g[k][a]; gl[0][a] -= g[k][a]; }
      }
    }
    if (DEG == 1) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        N[k] = lam[k];
        if (GRAD) for (int a = 0; a < D; ++a) G[k][a] = gl[k][a];
      }
    } else {
      constexpr int TE[3][2] = {{1, 2}, {0, 2}, {0, 1}};
      constexpr int KE[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        N[k] = lam[k] * (2.0 * lam[k] - 1.0);
        if (GRAD) for (int a = 0; a < D; ++a) G[k][a] = (4.0 * lam[k] - 1.0) * gl[k][a];
      }
#pragma unroll
      for (int k = 0; k < NE; ++k) {
        const int p = CT == 2 ? KE[k][0] : TE[k % 3][0], q = CT == 2 ? KE[k][1] : TE[k % 3][1];
        N[NV + k] = 4.0 * lam[p] * lam[q];
        if (GRAD) for (int a = 0; a < D; ++a) G[NV + k][a] = 4.0 * (lam[p] * gl[q][a] + lam[q] * gl[p][a]);
      }
    }
  }
  for (int q = 0; q < ncomp; ++q) {
    const double *uq = u + q * ld;
    double val = 0.0, gr[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < ND; ++k) {
      const double w = uq[dof[k]];
      val += N[k] * w;
      if (GRAD) for (int a = 0; a < D; ++a) gr[a] += G[k][a] * w;
    }
    out[q * npts + i] = val;
    if (GRAD) for (int a = 0; a < D; ++a) gout[(q * npts + i) * D + a] = gr[a];
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
// The walk of the bins serves its points sorted by bin (stable radix sort of 32-bit keys; k_loc_walk then serves point
// order[lane]); the evaluation serves them in their own order.  Measured on the MI355X: sorting by
// BIN pays in the walk (10^7 points, 129 k tetrahedra: 12.5 -> 4.0 ms with the sort included), sorting by CELL does not
// pay in the evaluation (0.21 -> 0.84 ms).
dim3 loc_grid(int64_t n) { return dim3((unsigned)phx_div_up(n > 0 ? n : 1, 256)); }

int loc_cell_kind(const phx_mesh *m) {
  return m->cell_type == PHX_TRIANGLE ? 0 : (m->cell_type == PHX_QUADRILATERAL ? 1 : 2);
}

// quadrilaterals: every cell an axis-parallel rectangle in tensor-product order (checked once per mesh)
int loc_require_rect(phx_mesh *m) {
  if (m->cell_type != PHX_QUADRILATERAL || m->rect_checked) return PHX_OK;
  DevTemps tmp(m->stream);
  int *bad = nullptr;
  PHX_CHECK(rect_bad_alloc(m, tmp, &bad));
  k_loc_rect_check<<<loc_grid(m->nc), dim3(256), 0, m->stream>>>(m->nc, m->cells, m->x, bad);
  PHX_HIP(hipGetLastError());
  PHX_CHECK(rect_bad_check(m, bad));
  m->rect_checked = 1;
  return PHX_OK;
}

// order[npts] = the points sorted by key (stable), keys < nkeys
int loc_sort_order(hipStream_t st, DevTemps &tmp, int64_t npts, uint32_t *key, int32_t *iota, uint64_t nkeys,
                   int32_t **order) {
  uint32_t *key2 = nullptr;
  PHX_HIP(tmp.alloc(&key2, sizeof(uint32_t) * (size_t)npts));
  PHX_HIP(tmp.alloc(order, sizeof(int32_t) * (size_t)npts));
  unsigned bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) < nkeys) ++bits;
  size_t bytes = 0;
  PHX_HIP(phx_sort_pairs((void *)nullptr, bytes, key, key2, iota, *order, (size_t)npts, 0u, bits, st));
  char *work = nullptr;
  PHX_HIP(tmp.alloc(&work, bytes ? bytes : 16));
  PHX_HIP(phx_sort_pairs((void *)work, bytes, key, key2, iota, *order, (size_t)npts, 0u, bits, st));
  return PHX_OK;
}

template <int CT>
int loc_build_bins(phx_mesh *m, double tol) {
  constexpr int D = LocCell<CT>::D;
  hipStream_t st = m->stream;
  const double t0 = wall_seconds();
  PHX_CHECK(loc_require_rect(m));
  struct Guard {
    phx_locator *l;
    ~Guard() { phx_locator_destroy(l); }
  } g{new phx_locator()};
  phx_locator *L = g.l;
  L->tol = tol;
  {
    DevTemps tmp(st);
    const int nblk = (int)std::min<int64_t>(256, phx_div_up(m->nv, 256));
    double *part = nullptr;
    PHX_HIP(tmp.alloc(&part, sizeof(double) * 6 * (size_t)nblk));
    k_loc_bbox<<<dim3(nblk), dim3(256), 0, st>>>(m->nv, D, m->x, part);
    PHX_HIP(hipGetLastError());
    std::vector<double> ph((size_t)nblk * 6);
    PHX_HIP(hipMemcpyAsync(ph.data(), part, sizeof(double) * ph.size(), hipMemcpyDeviceToHost, st));
    PHX_HIP(hipStreamSynchronize(st));
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = 0; b < nblk; ++b)
      for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], ph[b * 6 + a]); hi[a] = std::max(hi[a], ph[b * 6 + 3 + a]); }
    double vol = 1.0;
    for (int a = 0; a < D; ++a) {
      PHX_REQUIRE(hi[a] > lo[a] && std::isfinite(hi[a] - lo[a]), PHX_ERR_VALUE,
                  "point location: the mesh has no extent along axis %d (or a coordinate is not finite)", a);
      vol *= hi[a] - lo[a];
    }
    // about one bin per cell: cubes of edge (volume / nc)^(1/d)
    const double edge = pow(vol / (double)m->nc, 1.0 / D);
    for (int a = 0; a < D; ++a) {
      const double q = floor((hi[a] - lo[a]) / edge + 0.5);
      L->n[a] = q < 1.0 ? 1 : (q > 2048.0 * 1024.0 ? 2048 * 1024 : (int64_t)q);
      L->lo[a] = lo[a];
    }
    for (int a = 0; a < D; ++a) L->inv[a] = (double)L->n[a] / (hi[a] - L->lo[a]);
  }
  const double mrg = 4.0 * tol + 64.0 * 2.220446049250313e-16;
  LocGrid G;
  for (;;) {
    L->nbins = L->n[0] * L->n[1] * L->n[2];
    PHX_REQUIRE(L->nbins < ((int64_t)1 << 32), PHX_ERR_VALUE, "point location: %lld bins", (long long)L->nbins);
    for (int a = 0; a < 3; ++a) { G.n[a] = L->n[a]; G.lo[a] = L->lo[a]; G.inv[a] = L->inv[a]; }
    DevTemps tmp(st);
    uint32_t *cnt = nullptr;
    int64_t *off = nullptr;
    PHX_HIP(tmp.alloc(&cnt, sizeof(uint32_t) * (size_t)(L->nbins + 1)));
    PHX_HIP(phx_malloc(&off, sizeof(int64_t) * (size_t)(L->nbins + 1)));
    (void)phx_free(L->off);      // (the offsets of a resolution that was given up)
    L->off = off;
    PHX_HIP(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * (size_t)(L->nbins + 1), st));
    k_loc_bin_cells<CT, false><<<loc_grid(m->nc), dim3(256), 0, st>>>(m->nc, G, m->cells, m->x, mrg, cnt, nullptr, nullptr);
    PHX_HIP(hipGetLastError());
    size_t bytes = 0;
    PHX_HIP(phx_exclusive_sum((void *)nullptr, bytes, cnt, off, (size_t)(L->nbins + 1), st));
    char *work = nullptr;
    PHX_HIP(tmp.alloc(&work, bytes ? bytes : 16));
    PHX_HIP(phx_exclusive_sum((void *)work, bytes, cnt, off, (size_t)(L->nbins + 1), st));
    int64_t total = 0;
    PHX_HIP(hipMemcpyAsync(&total, off + L->nbins, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PHX_HIP(hipStreamSynchronize(st));
    const bool coarsest = L->n[0] == 1 && L->n[1] == 1 && L->n[2] == 1;
    if (total > (int64_t)PHX_LOC_MAX_PAIRS_PER_CELL * m->nc && !coarsest) {
      // too many pairs (large cells of a graded mesh overlap many bins): half the resolution, count again
      for (int a = 0; a < D; ++a) {
        const double len = (double)L->n[a] / L->inv[a];
        L->n[a] = std::max<int64_t>(1, L->n[a] / 2);
        L->inv[a] = (double)L->n[a] / len;
      }
      ++L->halvings;
      continue;
    }
    L->npairs = total;
    PHX_HIP(phx_malloc(&L->pairs, sizeof(int32_t) * (size_t)std::max<int64_t>(total, 1)));
    PHX_HIP(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * (size_t)(L->nbins + 1), st));
    k_loc_bin_cells<CT, true><<<loc_grid(m->nc), dim3(256), 0, st>>>(m->nc, G, m->cells, m->x, mrg, cnt, L->off, L->pairs);
    PHX_HIP(hipGetLastError());
    PHX_HIP(hipStreamSynchronize(st));
    break;
  }
  L->bytes = (int64_t)sizeof(int64_t) * (L->nbins + 1) + (int64_t)sizeof(int32_t) * std::max<int64_t>(L->npairs, 1);
  phx_locator_destroy(m->locator);
  m->locator = L;
  g.l = nullptr;
  m->loc_timings[0] = wall_seconds() - t0;
  return PHX_OK;
}

template <int CT>
int loc_locate_bins(phx_mesh *m, DevTemps &tmp, int64_t npts, const double *pts, double tol, int32_t *cells_d,
                    double *xref_d) {
  constexpr int D = LocCell<CT>::D;
  if (!m->locator || m->locator->tol < tol) PHX_CHECK(loc_build_bins<CT>(m, tol));
  const phx_locator *L = m->locator;
  LocGrid G;
  for (int a = 0; a < 3; ++a) { G.n[a] = L->n[a]; G.lo[a] = L->lo[a]; G.inv[a] = L->inv[a]; }
  hipStream_t st = m->stream;
  int32_t *order = nullptr;
  if (npts > 1) {
    uint32_t *key = nullptr;
    int32_t *iota = nullptr;
    PHX_HIP(tmp.alloc(&key, sizeof(uint32_t) * (size_t)npts));
    PHX_HIP(tmp.alloc(&iota, sizeof(int32_t) * (size_t)npts));
    k_loc_point_bins<D><<<loc_grid(npts), dim3(256), 0, st>>>(npts, G, pts, key, iota);
    PHX_HIP(hipGetLastError());
    PHX_CHECK(loc_sort_order(st, tmp, npts, key, iota, (uint64_t)L->nbins, &order));
  }
  k_loc_walk<CT><<<loc_grid(npts), dim3(256), 0, st>>>(npts, order, pts, G, L->off, L->pairs, m->cells, m->x, tol,
                                                        cells_d, xref_d);
  PHX_HIP(hipGetLastError());
  return PHX_OK;
}

int loc_locate_box(phx_mesh *m, int64_t npts, const double *pts, double tol, int32_t *cells_d, double *xref_d) {
  LocBox B;
  for (int a = 0; a < 3; ++a) {
    B.n[a] = m->box_n[a]; B.off[a] = m->box_off[a]; B.nglob[a] = std::max<int64_t>(m->box_nglob[a], 1);
    B.lo[a] = m->box_lo[a]; B.hi[a] = m->box_hi[a]; B.h[a] = m->box_h[a];
  }
  if (m->gdim == 3)
    k_loc_box<3><<<loc_grid(npts), dim3(256), 0, m->stream>>>(npts, B, pts, tol, cells_d, xref_d);
  else
    k_loc_box<2><<<loc_grid(npts), dim3(256), 0, m->stream>>>(npts, B, pts, tol, cells_d, xref_d);
  PHX_HIP(hipGetLastError());
  return PHX_OK;
}

template <int CT, int DEG>
void loc_launch_eval(phx_mesh *m, bool grad, int64_t npts, const int32_t *cells_d,
                     const double *xref_d, int ncomp, const double *u, int64_t ld, double fill, double *out, double *gout) {
  if (grad)
    k_loc_eval<CT, DEG, true><<<loc_grid(npts), dim3(256), 0, m->stream>>>(npts, m->nc, m->nv, m->cells, m->c2e, m->x,
                                                                          cells_d, xref_d, ncomp, u, ld, fill, out, gout);
  else
    k_loc_eval<CT, DEG, false><<<loc_grid(npts), dim3(256), 0, m->stream>>>(npts, m->nc, m->nv, m->cells, m->c2e, m->x,
                                                                           cells_d, xref_d, ncomp, u, ld, fill, out, gout);
}
}  // namespace

extern "C" int phx_locate_points(phx_mesh *m, int64_t npts, const double *pts, int loc, double tol, int32_t *cells_out,
                                 double *xref_out, int loc_out) {
  PHX_REQUIRE(m && npts >= 0 && (npts == 0 || (pts && cells_out && xref_out)), PHX_ERR_VALUE,
              "phx_locate_points: bad arguments");
  PHX_REQUIRE(tol >= 0.0, PHX_ERR_VALUE, "phx_locate_points: tol must be >= 0");     // (NaN fails as well)
  PHX_REQUIRE(npts < INT32_MAX, PHX_ERR_VALUE, "phx_locate_points: %lld points exceed 32-bit point ids", (long long)npts);
  PHX_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const int D = m->gdim;
  DevTemps tmp(st);
  if (npts == 0) return PHX_OK;
  const double t0 = wall_seconds();
  const double *pd = pts;
  int32_t *cd = cells_out;
  double *xd = xref_out;
  if (loc != PHX_DEVICE) {
    double *b = nullptr;
    PHX_HIP(tmp.alloc(&b, sizeof(double) * (size_t)npts * D));
    PHX_HIP(hipMemcpyAsync(b, pts, sizeof(double) * (size_t)npts * D, hipMemcpyHostToDevice, st));
    pd = b;
  }
  if (loc_out != PHX_DEVICE) {
    PHX_HIP(tmp.alloc(&cd, sizeof(int32_t) * (size_t)npts));
    PHX_HIP(tmp.alloc(&xd, sizeof(double) * (size_t)npts * D));
  }
  double t_build = 0.0;
  if (m->is_box) {
    PHX_CHECK(loc_locate_box(m, npts, pd, tol, cd, xd));
  } else {
    const double b0 = m->loc_timings[0];
    const bool had = m->locator && m->locator->tol >= tol;
    int rc;
    switch (loc_cell_kind(m)) {
      case 0: rc = loc_locate_bins<0>(m, tmp, npts, pd, tol, cd, xd); break;
      case 1: rc = loc_locate_bins<1>(m, tmp, npts, pd, tol, cd, xd); break;
      default: rc = loc_locate_bins<2>(m, tmp, npts, pd, tol, cd, xd); break;
    }
    if (rc != PHX_OK) { (void)hipStreamSynchronize(st); return rc; }
    if (!had) t_build = m->loc_timings[0]; else m->loc_timings[0] = b0;
  }
  if (loc_out != PHX_DEVICE) {
    PHX_HIP(hipMemcpyAsync(cells_out, cd, sizeof(int32_t) * (size_t)npts, hipMemcpyDeviceToHost, st));
    PHX_HIP(hipMemcpyAsync(xref_out, xd, sizeof(double) * (size_t)npts * D, hipMemcpyDeviceToHost, st));
  }
  PHX_HIP(hipStreamSynchronize(st));
  m->loc_timings[1] = wall_seconds() - t0 - t_build;
  return PHX_OK;
}

extern "C" int phx_eval_points(phx_mesh *m, int degree, int ncomp, const double *values, int loc_v, int64_t npts,
                               const int32_t *cells, const double *xref, int loc_p, int want_grad, double fill,
                               double *out, double *grad_out, int loc_out) {
  PHX_REQUIRE(m, PHX_ERR_VALUE, "phx_eval_points: no mesh");
  PHX_REQUIRE(degree == 1 || degree == 2, PHX_ERR_NOT_IMPLEMENTED, "evaluation of degree %d is not implemented", degree);
  const bool quad = m->cell_type == PHX_QUADRILATERAL;
  PHX_REQUIRE(!(quad && degree == 2), PHX_ERR_NOT_IMPLEMENTED, "degree-2 evaluation on quadrilaterals is not implemented");
  PHX_REQUIRE(ncomp >= 1 && npts >= 0 && values && (npts == 0 || (cells && xref && out && (!want_grad || grad_out))),
              PHX_ERR_VALUE, "phx_eval_points: bad arguments");
  PHX_REQUIRE(npts < INT32_MAX, PHX_ERR_VALUE, "phx_eval_points: %lld points exceed 32-bit point ids", (long long)npts);
  PHX_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const int D = m->gdim;
  PHX_CHECK(loc_require_rect(m));
  if (degree == 2) PHX_CHECK(phx_mesh_build_edges(m));
  if (npts == 0) return PHX_OK;
  const double t0 = wall_seconds();
  const int64_t ld = degree == 1 ? m->nv : m->nv + m->ne;
  DevTemps tmp(st);
  const double *ud = values, *xd = xref;
  const int32_t *cd = cells;
  double *od = out, *gd = grad_out;
  if (loc_v != PHX_DEVICE) {
    double *b = nullptr;
    PHX_HIP(tmp.alloc(&b, sizeof(double) * (size_t)ld * ncomp));
    PHX_HIP(hipMemcpyAsync(b, values, sizeof(double) * (size_t)ld * ncomp, hipMemcpyHostToDevice, st));
    ud = b;
  }
  if (loc_p != PHX_DEVICE) {
    int32_t *b = nullptr;
    double *r = nullptr;
    PHX_HIP(tmp.alloc(&b, sizeof(int32_t) * (size_t)npts));
    PHX_HIP(tmp.alloc(&r, sizeof(double) * (size_t)npts * D));
    PHX_HIP(hipMemcpyAsync(b, cells, sizeof(int32_t) * (size_t)npts, hipMemcpyHostToDevice, st));
    PHX_HIP(hipMemcpyAsync(r, xref, sizeof(double) * (size_t)npts * D, hipMemcpyHostToDevice, st));
    cd = b; xd = r;
  }
  if (loc_out != PHX_DEVICE) {
    PHX_HIP(tmp.alloc(&od, sizeof(double) * (size_t)npts * ncomp));
    if (want_grad) PHX_HIP(tmp.alloc(&gd, sizeof(double) * (size_t)npts * ncomp * D));
  }
  const bool grad = want_grad != 0;
  switch (loc_cell_kind(m) * 2 + (degree - 1)) {
    case 0: loc_launch_eval<0, 1>(m, grad, npts, cd, xd, ncomp, ud, ld, fill, od, gd); break;
    case 1: loc_launch_eval<0, 2>(m, grad, npts, cd, xd, ncomp, ud, ld, fill, od, gd); break;
    case 2: loc_launch_eval<1, 1>(m, grad, npts, cd, xd, ncomp, ud, ld, fill, od, gd); break;
    case 4: loc_launch_eval<2, 1>(m, grad, npts, cd, xd, ncomp, ud, ld, fill, od, gd); break;
    default: loc_launch_eval<2, 2>(m, grad, npts, cd, xd, ncomp, ud, ld, fill, od, gd); break;
  }
  PHX_HIP(hipGetLastError());
  if (loc_out != PHX_DEVICE) {
    PHX_HIP(hipMemcpyAsync(out, od, sizeof(double) * (size_t)npts * ncomp, hipMemcpyDeviceToHost, st));
    if (want_grad)
      PHX_HIP(hipMemcpyAsync(grad_out, gd, sizeof(double) * (size_t)npts * ncomp * D, hipMemcpyDeviceToHost, st));
  }
  PHX_HIP(hipStreamSynchronize(st));
  m->loc_timings[2] = wall_seconds() - t0;
  return PHX_OK;
}

extern "C" int phx_locator_info(const phx_mesh *m, int64_t *info) {
  PHX_REQUIRE(m && info, PHX_ERR_VALUE, "phx_locator_info: bad arguments");
  for (int k = 0; k < 8; ++k) info[k] = 0;
  info[0] = m->is_box ? 1 : 2;
  if (const phx_locator *L = m->locator) {
    for (int a = 0; a < m->gdim; ++a) info[1 + a] = L->n[a];
    info[4] = L->npairs; info[5] = L->bytes; info[6] = L->halvings; info[7] = 1;
  }
  return PHX_OK;
}

extern "C" int phx_locate_timings(const phx_mesh *m, double *t) {
  for (int k = 0; k < 3; ++k) t[k] = m->loc_timings[k];
  return PHX_OK;
}
