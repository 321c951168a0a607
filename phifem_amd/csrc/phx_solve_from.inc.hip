// Warm-started solve (include of phx_solve.hip): phx_solve on the correction system A delta = b - A x0.  A wrapper:
// no Krylov loop knows about x0.

#define SF_BLOCKS 512
// partial sums of squares in a fixed order: block k takes the entries k, k + SF_BLOCKS * 256, ... per lane, folds its
// lanes in a tree, and block 0 of the second launch folds the SF_BLOCKS partials the same way
__global__ void __launch_bounds__(256) k_sf_sumsq(int64_t n, const double *__restrict__ v, double *__restrict__ part) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)SF_BLOCKS * 256) a += v[i] * v[i];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
__global__ void __launch_bounds__(256) k_sf_fold(const double *__restrict__ part, double *__restrict__ out) {
  __shared__ double sh[256];
  sh[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + 256];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}
// active entries of a vector in FULL numbering (the inverse of k_scatter_solution's index map)
__global__ void k_sf_gather_full(int64_t n, const int64_t *__restrict__ full_of_active, const int32_t *__restrict__ out_vertex,
                                 int64_t nent, const double *__restrict__ xfull, double *__restrict__ xa) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= n) return;
  int64_t f = full_of_active[r];
  if (out_vertex) { const int64_t blk = f / nent; f = blk * nent + out_vertex[f - blk * nent]; }
  xa[r] = xfull[f];
}
__global__ void k_sf_residual(int64_t n, const double *__restrict__ b, double *__restrict__ ax) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) ax[i] = b[i] - ax[i];
}
__global__ void k_sf_add(int64_t n, const double *__restrict__ x0, double *__restrict__ d) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) d[i] = x0[i] + d[i];
}

// s->rhs points at the residual while the inner solve runs and is put back on every return path
struct SfRhsSwap {
  phx_system *s;
  double *b;
  SfRhsSwap(phx_system *sys, double *r) : s(sys), b(sys->rhs) { s->rhs = r; }
  ~SfRhsSwap() { s->rhs = b; }
};

extern "C" int phx_solve_from(phx_system *s, int method, double rtol, int64_t max_iter, const double *x0, double *x,
                              int loc, double *stats) {
  if (!x0) return phx_solve(s, method, rtol, max_iter, x, loc, stats);
  phx_mesh *m = s->mesh;
  PHX_HIP(hipSetDevice(m->device));
  PHX_REQUIRE(method == PHX_BICGSTAB_JACOBI, PHX_ERR_NOT_IMPLEMENTED, "unknown method %d", method);
  PHX_REQUIRE(!s->kr_work && !s->kr_scal && !s->own, PHX_ERR_NOT_IMPLEMENTED,
              "phx_solve_from serves single-rank systems (Krylov buffers of a multi-rank driver are attached)");
  PHX_REQUIRE(x != nullptr, PHX_ERR_VALUE, "NULL solution array");
  const int64_t n = s->n, nfull = s->nfull;
  if (n == 0) return phx_solve(s, method, rtol, max_iter, x, loc, stats);
  hipStream_t st = m->stream;
  const dim3 block(256), gn((unsigned)phx_div_up(n, 256)), gf((unsigned)phx_div_up(nfull, 256));
  DevTemps tmp(st);
  const double *x0d = x0;
  if (loc != PHX_DEVICE) {
    double *copy = nullptr;
    PHX_HIP(tmp.alloc(&copy, sizeof(double) * (size_t)nfull));
    PHX_HIP(hipMemcpyAsync(copy, x0, sizeof(double) * (size_t)nfull, hipMemcpyHostToDevice, st));
    x0d = copy;
  }
  double *xa = nullptr, *r0 = nullptr, *part = nullptr;
  PHX_HIP(tmp.alloc(&xa, sizeof(double) * (size_t)n));
  PHX_HIP(tmp.alloc(&r0, sizeof(double) * (size_t)n));
  PHX_HIP(tmp.alloc(&part, sizeof(double) * (SF_BLOCKS + 2)));
  k_sf_gather_full<<<gn, block, 0, st>>>(n, s->full_of_active, s->out_vertex, s->nent, x0d, xa);
  PHX_HIP(hipGetLastError());
  PHX_CHECK(phx_spmv(s, xa, r0, PHX_DEVICE));   // the operator phx_spmv applies, original active numbering
  k_sf_residual<<<gn, block, 0, st>>>(n, s->rhs, r0);
  k_sf_sumsq<<<dim3(SF_BLOCKS), block, 0, st>>>(n, s->rhs, part);
  k_sf_fold<<<1, block, 0, st>>>(part, part + SF_BLOCKS);
  k_sf_sumsq<<<dim3(SF_BLOCKS), block, 0, st>>>(n, r0, part);
  k_sf_fold<<<1, block, 0, st>>>(part, part + SF_BLOCKS + 1);
  PHX_HIP(hipGetLastError());
  double nn[2] = {0.0, 0.0};
  PHX_HIP(hipMemcpyAsync(nn, part + SF_BLOCKS, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
  PHX_HIP(hipStreamSynchronize(st));
  const double nb = sqrt(nn[0]), nr = sqrt(nn[1]);
  PHX_REQUIRE(nr == nr && nb == nb, PHX_ERR_VALUE, "phx_solve_from: x0 or the right-hand side is not finite");
  if (nb == 0.0) return phx_solve(s, method, rtol, max_iter, x, loc, stats);   // b = 0: the solution is 0
  if (nr <= rtol * nb) {
    if (x != x0) PHX_HIP(hipMemcpy(x, x0, sizeof(double) * (size_t)nfull,
                                   loc == PHX_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToHost));
    s->kr_ident_used = false;
    s->kr_red_used = false;
    if (stats) {
      for (int k = 0; k < 8; ++k) stats[k] = 0.0;
      stats[1] = nr / nb;
      stats[3] = 1.0;
      stats[6] = 1.0;
    }
    return PHX_OK;
  }
  double *delta = nullptr;
  PHX_HIP(tmp.alloc(&delta, sizeof(double) * (size_t)nfull));
  double inner[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  {
    SfRhsSwap swap(s, r0);
    PHX_CHECK(phx_solve(s, method, rtol * nb / nr, max_iter, delta, PHX_DEVICE, inner));
  }
  k_sf_add<<<gf, block, 0, st>>>(nfull, x0d, delta);
  PHX_HIP(hipGetLastError());
  if (loc == PHX_DEVICE) PHX_HIP(hipMemcpyAsync(x, delta, sizeof(double) * (size_t)nfull, hipMemcpyDeviceToDevice, st));
  else PHX_HIP(hipMemcpyAsync(x, delta, sizeof(double) * (size_t)nfull, hipMemcpyDeviceToHost, st));
  PHX_HIP(hipStreamSynchronize(st));
  if (stats) {
    for (int k = 0; k < 8; ++k) stats[k] = inner[k];
    stats[1] = inner[1] * (nr / nb);
  }
  return PHX_OK;
}
