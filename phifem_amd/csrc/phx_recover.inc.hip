// Recovered gradient and the recovery-based (Zienkiewicz-Zhu) indicator: included LAST by
// phx_assemble.hip (shares Geo / load_cell, the P2 basis, the Q1-rectangle layer, DevTemps / to_device, the ordered
// select and the fixed-order sums of phx_errors.inc.hip / phx_estimate.inc.hip).  With S the selected cells (a byte
// mask, or Omega_h = the cells tagged 1 or 2) and S_v the cells of S that contain the vertex v
//   G(v) = sum_{T in S_v} |T| grad u_h|_T (x_v) / sum_{T in S_v} |T|,      0 exactly where S_v is empty
//   eta_T^2 = sum over the components of int_T |G_h - grad u_h|^2 for T in S, G_h the P1 / Q1 interpolant of G; else 0
// -- an indicator for marking and a post-processed flux: neither a proven bound nor the residual of any scheme.  On
// the rim of S the star of a vertex is one-sided and G is only first-order accurate there.
// Four passes over the WORK LIST (the ascending cells of S, phx_select.h), none over the mesh:
//   1. cells:    one lane per listed cell e stores its record {|T|, grad u_h at its corners} and its (vertex, e N + i)
//                pairs, N corners per cell;
//   2. stars:    a stable radix sort of the pairs by vertex; the positions where the vertex changes (ordered select
//                again) are the segment starts.  Inside a segment the pairs ascend with the listed cell: the adjacency
//                is a function of the connectivity and the mask alone (build_v2c fills by atomics and covers the mesh);
//   3. vertices: one lane per segment walks its pairs in that order and adds |T| and |T| grad -- a loop, so a star of
//                several hundred cells is as correct as one of six;
//   4. eta:      one lane per listed cell takes G at its corners, its own record, and the closed forms
//                  simplices:  |T| / ((d+1)(d+2)) (sum_i d_i . d_i + (sum_i d_i) . (sum_i d_i))
//                  rectangles: hx hy sum_ij d_i (M1 (x) M1)_ij d_j,   M1 = [[1/3, 1/6], [1/6, 1/3]]
//                both exact; per-block partial sums folded in a fixed order give the total.
// No floating-point atomics: the same inputs give the same bits on every run and on every mesh object made from the
// same arrays.  Everything outside the list is cleared by two memsets.
// The rest of this translation unit is compiled without FMA contraction.
#pragma clang fp contract(off)

struct SelMaskBytes {   // a 4-byte aligned mask: four cells per 32-bit load (phx_select.h)
  const int8_t *t;
  __host__ __device__ bool operator()(const int32_t &c) const { return t[c] != 0; }
  __host__ __device__ const int8_t *bytes() const { return t; }
  __host__ __device__ bool test(int tag, int32_t) const { return tag != 0; }
};
struct SelMaskAny {     // any alignment (a view into a caller's tensor)
  const int8_t *t;
  __host__ __device__ bool operator()(const int32_t &c) const { return t[c] != 0; }
};
struct SelSegmentHead { // position j of the sorted pairs starts the star of another vertex
  const uint32_t *k;
  __host__ __device__ bool operator()(const int32_t &j) const { return j == 0 || k[j] != k[j - 1]; }
};

#define REC_P1 0
#define REC_P2 1
#define REC_Q1 2

struct RecArgs {
  const int32_t *cells, *c2e;
  const double *x, *u;
  int32_t nvert;
  int64_t nd;           // nodal values per component
  int ncomp;
  int stride;           // doubles per record: 1 + (gradient sets) * ncomp * gdim
  double *rec;          // [nlist][stride]: |T|, then [corner or 0][component][direction]
  uint32_t *keys;       // [nlist * N] vertex
  int32_t *vals;        // [nlist * N] e * N + local corner
};

// --- 1. records and pairs -----------------------------------------------------------------------------------------------
template <int D, int KIND>
__global__ void __launch_bounds__(EST_THREADS)
k_recover_cells(int64_t nlist, const int32_t *__restrict__ list, RecArgs R, int *__restrict__ bad) {
  constexpr int N = KIND == REC_Q1 ? 4 : D + 1;
  for (int64_t e = blockIdx.x * (int64_t)EST_THREADS + threadIdx.x; e < nlist; e += gridDim.x * (int64_t)EST_THREADS) {
    const int64_t c = list[e];
    double *rec = R.rec + e * R.stride;
    int32_t v[N];
    if constexpr (KIND == REC_Q1) {
      RectGeo Rg;
      if (!rect_load(R.cells, R.x, c, Rg)) *bad = 1;
      for (int i = 0; i < 4; ++i) v[i] = Rg.v[i];
      rec[0] = Rg.hx * Rg.hy;
      for (int cp = 0; cp < R.ncomp; ++cp) {
        double un[4];
        for (int b = 0; b < 4; ++b) un[b] = R.u[cp * R.nd + v[b]];
        for (int i = 0; i < 4; ++i) {
          double gx = 0.0, gy = 0.0;
          for (int b = 0; b < 4; ++b) {
            double val, bx, by;
            q1_at(b, (double)(i & 1), (double)(i >> 1), Rg, &val, &bx, &by);
            gx += un[b] * bx; gy += un[b] * by;
          }
          rec[1 + (i * R.ncomp + cp) * 2] = gx;
          rec[2 + (i * R.ncomp + cp) * 2] = gy;
        }
      }
    } else {
      double X[N][D];
      load_cell<D>(R.cells, R.x, c, v, X);
      Geo<D> G;
      simplex_geometry<D>(X, G);
      rec[0] = G.vol;
      if constexpr (KIND == REC_P1) {
        for (int cp = 0; cp < R.ncomp; ++cp) {
          double gu[D];
          for (int d = 0; d < D; ++d) gu[d] = 0.0;
          for (int i = 0; i < N; ++i) {
            const double ui = R.u[cp * R.nd + v[i]];
            for (int d = 0; d < D; ++d) gu[d] += ui * G.g[i][d];
          }
          for (int d = 0; d < D; ++d) rec[1 + cp * D + d] = gu[d];
        }
      } else {
        using B = P2B<D>;
        int32_t dof[B::NB];
        for (int i = 0; i < N; ++i) dof[i] = v[i];
        for (int k = 0; k < B::NE; ++k) dof[N + k] = R.nvert + R.c2e[c * B::NE + k];
        for (int cp = 0; cp < R.ncomp; ++cp) {
          double un[B::NB];
          for (int b = 0; b < B::NB; ++b) un[b] = R.u[cp * R.nd + dof[b]];
          for (int i = 0; i < N; ++i) {     // the P1 gradient field at corner i: lambda = e_i
            double lam[N], gu[D];
            for (int m = 0; m < N; ++m) lam[m] = m == i ? 1.0 : 0.0;
            for (int d = 0; d < D; ++d) gu[d] = 0.0;
            for (int b = 0; b < B::NB; ++b) {
              double cs[N];
              B::gradc(b, lam, cs);
              for (int d = 0; d < D; ++d) {
                double gb = 0.0;
                for (int m = 0; m < N; ++m) gb += cs[m] * G.g[m][d];
                gu[d] += un[b] * gb;
              }
            }
            for (int d = 0; d < D; ++d) rec[1 + (i * R.ncomp + cp) * D + d] = gu[d];
          }
        }
      }
    }
    for (int i = 0; i < N; ++i) {
      R.keys[e * N + i] = (uint32_t)v[i];
      R.vals[e * N + i] = (int32_t)(e * N + i);
    }
  }
}

// --- 3. one lane per star, in the order of the sorted pairs --------------------------------------------------------------
// records a lane asks for before it adds them (256^3 sphere, DESIGN.md 7g: 1.89 ms one by one, 0.92 with 4, 0.63 with 8)
#define REC_INFLIGHT 8
template <int D>
__global__ void __launch_bounds__(EST_THREADS)
k_recover_vertices(int64_t nseg, const int32_t *__restrict__ seg, int64_t npairs, const uint32_t *__restrict__ keys,
                   const int32_t *__restrict__ vals, const double *__restrict__ rec, int stride, int ncorner, int nsets,
                   int ncomp, int64_t nv, double *__restrict__ grad) {
  for (int64_t s = blockIdx.x * (int64_t)EST_THREADS + threadIdx.x; s < nseg; s += gridDim.x * (int64_t)EST_THREADS) {
    const int64_t j0 = seg[s], j1 = s + 1 < nseg ? (int64_t)seg[s + 1] : npairs;
    const int64_t v = keys[j0];
    for (int cp = 0; cp < ncomp; ++cp) {
      double den = 0.0, num[D];
      for (int d = 0; d < D; ++d) num[d] = 0.0;
      // REC_INFLIGHT records in flight per lane (the loads of a star are independent, its additions are not); the additions
      // keep the order of the pairs
      for (int64_t j = j0; j < j1; j += REC_INFLIGHT) {
        double w[REC_INFLIGHT], g[REC_INFLIGHT][D];
#pragma unroll
        for (int k = 0; k < REC_INFLIGHT; ++k) {
          const int32_t p = vals[j + k < j1 ? j + k : j1 - 1];
          const int64_t e = p / ncorner;
          const int i = nsets == 1 ? 0 : p - (int32_t)e * ncorner;
          const double *r = rec + e * stride;
          w[k] = r[0];
          for (int d = 0; d < D; ++d) g[k][d] = r[1 + (i * ncomp + cp) * D + d];
        }
#pragma unroll
        for (int k = 0; k < REC_INFLIGHT; ++k)
          if (j + k < j1) {
            den += w[k];
            for (int d = 0; d < D; ++d) num[d] += w[k] * g[k][d];
          }
      }
      for (int d = 0; d < D; ++d) grad[((int64_t)cp * nv + v) * D + d] = num[d] / den;
    }
  }
}

// --- 4. the indicator of the listed cells and the block sums of the total ----------------------------------------------
template <int D, bool QUAD>
__global__ void __launch_bounds__(EST_THREADS)
k_recover_eta(int64_t nlist, const int32_t *__restrict__ list, const int32_t *__restrict__ cells,
              const double *__restrict__ rec, int stride, int nsets, int ncomp, int64_t nv,
              const double *__restrict__ grad, double *__restrict__ eta2, double *__restrict__ partial) {
  constexpr int N = QUAD ? 4 : D + 1;
  double total = 0.0;
  for (int64_t e = blockIdx.x * (int64_t)EST_THREADS + threadIdx.x; e < nlist; e += gridDim.x * (int64_t)EST_THREADS) {
    const int64_t c = list[e];
    const double *r = rec + e * stride;
    int32_t v[N];
    for (int i = 0; i < N; ++i) v[i] = cells[c * N + i];
    double acc = 0.0;
    for (int cp = 0; cp < ncomp; ++cp)
      for (int d = 0; d < D; ++d) {
        double dd[N];
        for (int i = 0; i < N; ++i)
          dd[i] = grad[((int64_t)cp * nv + v[i]) * D + d] - r[1 + ((nsets == 1 ? 0 : i) * ncomp + cp) * D + d];
        if constexpr (QUAD) {
          for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) acc += dd[i] * (m1(i & 1, j & 1) * m1(i >> 1, j >> 1)) * dd[j];
        } else {
          double s = 0.0, ss = 0.0;
          for (int i = 0; i < N; ++i) { s += dd[i]; ss += dd[i] * dd[i]; }
          acc += ss + s * s;
        }
      }
    const double eta = QUAD ? r[0] * acc : r[0] * (1.0 / ((D + 1) * (D + 2))) * acc;
    if (eta2) eta2[c] = eta;
    total += eta;
  }
  // fixed-order block sum (as est_block_sums): lane tree inside the wave, then the waves in order; k_sum_partials
  // folds four entries per block
  __shared__ double sh[EST_THREADS / 64];
  for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = total;
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = 0.0;
    if (threadIdx.x == 0) for (int wv = 0; wv < EST_THREADS / 64; ++wv) t += sh[wv];
    partial[(int64_t)blockIdx.x * 4 + threadIdx.x] = t;
  }
}

// grid-stride over a capped grid that depends on the count only.  The eta pass leaves one partial sum per block for ONE
// block to fold: 2048 blocks (eight per CU) keep that fold at a few microseconds (65 536 slots took 0.17 ms).
#define REC_SUM_BLOCKS 2048
static inline dim3 recover_grid(int64_t n, int64_t cap = EST_MAX_BLOCKS) {
  const int64_t want = phx_div_up(n, (int64_t)EST_THREADS);
  return dim3((unsigned)(want < cap ? want : cap));
}

template <int D, int KIND>
static int recover_run(phx_mesh *m, RecArgs &R, int64_t nlist, const int32_t *list, double *dgrad, double *deta,
                       double *sum, DevTemps &tmp) {
  constexpr int N = KIND == REC_Q1 ? 4 : D + 1;
  constexpr int NSETS = KIND == REC_P1 ? 1 : N;
  hipStream_t st = m->stream;
  const int64_t npairs = nlist * N;
  PHX_REQUIRE(npairs < INT32_MAX, PHX_ERR_VALUE, "phx_recover_gradient: %lld (vertex, cell) pairs: fewer than 2^31 - 1 expected",
              (long long)npairs);
  R.stride = 1 + NSETS * R.ncomp * D;
  uint32_t *keys2 = nullptr;
  int32_t *vals2 = nullptr;
  int *bad = nullptr;
  PHX_HIP(tmp.alloc(&R.rec, sizeof(double) * (size_t)nlist * (size_t)R.stride));
  PHX_HIP(tmp.alloc(&R.keys, sizeof(uint32_t) * (size_t)npairs));
  PHX_HIP(tmp.alloc(&keys2, sizeof(uint32_t) * (size_t)npairs));
  PHX_HIP(tmp.alloc(&R.vals, sizeof(int32_t) * (size_t)npairs));
  PHX_HIP(tmp.alloc(&vals2, sizeof(int32_t) * (size_t)npairs));
  if (KIND == REC_Q1) PHX_CHECK(rect_bad_alloc(m, tmp, &bad));
  const dim3 block(EST_THREADS);
  k_recover_cells<D, KIND><<<recover_grid(nlist), block, 0, st>>>(nlist, list, R, bad);
  PHX_HIP(hipGetLastError());
  // stars: stable sort by vertex (the bits a vertex index can have), then the segment starts
  unsigned nbits = 1;
  while (nbits < 32 && ((uint64_t)1 << nbits) < (uint64_t)m->nv) ++nbits;
  size_t bsort = 0;
  PHX_HIP(phx_sort_pairs(nullptr, bsort, R.keys, keys2, R.vals, vals2, (size_t)npairs, 0u, nbits, st));
  void *work = nullptr;
  PHX_HIP(tmp.alloc(&work, bsort ? bsort : 16));
  PHX_HIP(phx_sort_pairs(work, bsort, R.keys, keys2, R.vals, vals2, (size_t)npairs, 0u, nbits, st));
  int32_t *seg = nullptr;
  int64_t nseg = 0;
  PHX_CHECK(phx_select_indices(st, npairs, SelSegmentHead{keys2}, &seg, &nseg));
  tmp.adopt(seg);
  k_recover_vertices<D><<<recover_grid(nseg), block, 0, st>>>(nseg, seg, npairs, keys2, vals2, R.rec, R.stride, N, NSETS,
                                                                R.ncomp, m->nv, dgrad);
  PHX_HIP(hipGetLastError());
  if (deta || sum) {
    const dim3 grid = recover_grid(nlist, REC_SUM_BLOCKS);
    double *partial = nullptr, *dsum = nullptr;
    PHX_HIP(tmp.alloc(&partial, sizeof(double) * (size_t)grid.x * 4));
    PHX_HIP(tmp.alloc(&dsum, sizeof(double) * 4));
    k_recover_eta<D, KIND == REC_Q1><<<grid, block, 0, st>>>(nlist, list, m->cells, R.rec, R.stride, NSETS, R.ncomp,
                                                               m->nv, dgrad, deta, partial);
    k_sum_partials<<<dim3(1), dim3(256), 0, st>>>((int64_t)grid.x, partial, dsum);
    PHX_HIP(hipGetLastError());
    if (sum) {
      double hsum[4] = {0.0, 0.0, 0.0, 0.0};
      PHX_HIP(hipMemcpyAsync(hsum, dsum, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
      PHX_HIP(hipStreamSynchronize(st));
      *sum = hsum[0];
    }
  }
  if (bad) PHX_CHECK(rect_bad_check(m, bad));
  return PHX_OK;
}

extern "C" int phx_recover_gradient(phx_mesh *m, int degree, int ncomp, const double *u, int loc_u,
                                    const uint8_t *cell_mask, int loc_mask, double *grad, double *eta2, int loc_out,
                                    double *sum) {
  PHX_REQUIRE(m, PHX_ERR_VALUE, "phx_recover_gradient: no mesh");
  PHX_HIP(hipSetDevice(m->device));
  const bool quad = m->cell_type == PHX_QUADRILATERAL;
  PHX_REQUIRE((m->cell_type == PHX_TRIANGLE || m->cell_type == PHX_TETRAHEDRON || (quad && m->gdim == 2)) &&
                  (degree == 1 || (degree == 2 && !quad)),
              PHX_ERR_NOT_IMPLEMENTED,
              "recover_gradient: degree 1 on triangles, tetrahedra and rectangles, degree 2 on simplices");
  PHX_REQUIRE(ncomp >= 1, PHX_ERR_VALUE, "phx_recover_gradient: ncomp must be at least 1");
  PHX_REQUIRE(u && grad, PHX_ERR_VALUE, "phx_recover_gradient: NULL array");
  PHX_REQUIRE(cell_mask || m->have_cell_tags, PHX_ERR_VALUE,
              "phx_recover_gradient: no cell mask and the mesh carries no cell tags -- call compute_tags_measures first");
  if (degree == 2) PHX_CHECK(phx_mesh_build_edges(m));
  if (sum) *sum = 0.0;
  hipStream_t st = m->stream;
  const int D = m->gdim;
  const int64_t nc = m->nc, nv = m->nv, nd = degree == 1 ? nv : nv + m->ne;
  if (nc == 0 && nv == 0) return PHX_OK;
  DevTemps tmp(st);   // staged host arrays, the work list, records, pairs, sort room, partial sums: returned on every path
  RecArgs R{};
  PHX_CHECK(to_device(m, u, loc_u, nd * ncomp, &R.u, tmp));
  R.cells = m->cells; R.c2e = m->c2e; R.x = m->x; R.nvert = (int32_t)nv; R.nd = nd; R.ncomp = ncomp;
  const size_t gbytes = sizeof(double) * (size_t)ncomp * (size_t)nv * (size_t)D;
  double *dgrad = grad, *deta = eta2;
  if (loc_out != PHX_DEVICE) {
    PHX_HIP(tmp.alloc(&dgrad, gbytes ? gbytes : 16));
    if (eta2) PHX_HIP(tmp.alloc(&deta, sizeof(double) * (size_t)(nc > 0 ? nc : 1)));
  }
  PHX_HIP(hipMemsetAsync(dgrad, 0, gbytes, st));                                   // vertices with no selected star
  if (deta) PHX_HIP(hipMemsetAsync(deta, 0, sizeof(double) * (size_t)nc, st));     // cells outside S
  int32_t *list = nullptr;
  int64_t nlist = 0;
  if (cell_mask) {
    const int8_t *dmask = reinterpret_cast<const int8_t *>(cell_mask);
    if (loc_mask != PHX_DEVICE) {
      int8_t *copy = nullptr;
      PHX_HIP(tmp.alloc(&copy, (size_t)(nc > 0 ? nc : 1)));
      PHX_HIP(hipMemcpyAsync(copy, cell_mask, (size_t)nc, hipMemcpyHostToDevice, st));
      dmask = copy;
    }
    if (((uintptr_t)dmask & 3u) == 0) PHX_CHECK(phx_select_indices(st, nc, SelMaskBytes{dmask}, &list, &nlist));
    else PHX_CHECK(phx_select_indices(st, nc, SelMaskAny{dmask}, &list, &nlist));
  } else {
    PHX_CHECK(phx_select_indices(st, nc, SelOmegaBytes{m->cell_tags}, &list, &nlist));
  }
  tmp.adopt(list);
  if (nlist > 0) {   // an empty list launches nothing
    if (quad) PHX_CHECK((recover_run<2, REC_Q1>(m, R, nlist, list, dgrad, deta, sum, tmp)));
    else if (D == 2 && degree == 1) PHX_CHECK((recover_run<2, REC_P1>(m, R, nlist, list, dgrad, deta, sum, tmp)));
    else if (D == 2) PHX_CHECK((recover_run<2, REC_P2>(m, R, nlist, list, dgrad, deta, sum, tmp)));
    else if (degree == 1) PHX_CHECK((recover_run<3, REC_P1>(m, R, nlist, list, dgrad, deta, sum, tmp)));
    else PHX_CHECK((recover_run<3, REC_P2>(m, R, nlist, list, dgrad, deta, sum, tmp)));
  }
  if (loc_out != PHX_DEVICE) {
    PHX_HIP(hipMemcpyAsync(grad, dgrad, gbytes, hipMemcpyDeviceToHost, st));
    if (eta2) PHX_HIP(hipMemcpyAsync(eta2, deta, sizeof(double) * (size_t)nc, hipMemcpyDeviceToHost, st));
  }
  PHX_HIP(hipStreamSynchronize(st));
  return PHX_OK;
}
