// Restriction: the transpose of the degree-1 phx_prolongate on triangles and tetrahedra, for fine meshes made by
// phx_mesh_refine and by phx_mesh_refine_marked (include of phx_submesh.hip after phx_refine_marked.inc.hip:
// -ffp-contract=off, the order of the additions is specified).  tests/multilevel_ref.py restates it in numpy.
//
// Prolongation copies at the coarse vertices (fine vertex v < nv IS coarse vertex v) and writes 0.5 u_p + 0.5 u_q at the
// fine vertex nv + r of the r-th bisected coarse edge (p, q).  Its transpose would scatter 0.5 in[nv + r] into out[p]
// and out[q]; it is written as a GATHER instead.  Once per fine mesh an integer CSR "coarse vertex -> the new fine
// vertices that depend on it" is built: the entries (p_r, nv + r), (q_r, nv + r), r ascending, are sorted by their coarse
// vertex with the stable radix sort, so every row lists its fine vertices in ascending id.  Then
//   out[p] = ((in[p] + 0.5 in[m_1]) + 0.5 in[m_2]) + ...      m_1 < m_2 < ... the row of p,
// one lane per coarse vertex, no floating-point atomics: the same bits on every run.
namespace {

// entries 2 r, 2 r + 1 of the r-th bisected edge: `list` = the marked coarse edges (nullptr: every edge, r = e)
__global__ void __launch_bounds__(256)
k_rs_entries(int64_t nm, const int32_t *__restrict__ list, const int32_t *__restrict__ edges, int64_t nv,
             uint32_t *__restrict__ key, int32_t *__restrict__ val) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= nm) return;
  const int64_t e = list ? list[r] : r;
  key[2 * r] = (uint32_t)edges[2 * e];
  key[2 * r + 1] = (uint32_t)edges[2 * e + 1];
  val[2 * r] = val[2 * r + 1] = (int32_t)(nv + r);
}

// ptr[v] = first sorted entry whose coarse vertex is >= v, v = 0 .. nv (ptr[nv] = n)
__global__ void __launch_bounds__(256)
k_rs_ptr(int64_t nv, int64_t n, const uint32_t *__restrict__ key, int32_t *__restrict__ ptr) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v > nv) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)key[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  ptr[v] = (int32_t)lo;
}

__global__ void __launch_bounds__(256)
k_restrict(int64_t nv, const int32_t *__restrict__ ptr, const int32_t *__restrict__ idx, int ncomp,
           const double *__restrict__ in, int64_t ldin, double *__restrict__ out, int64_t ldout) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= nv) return;
  const int32_t j0 = ptr[p], j1 = ptr[p + 1];
  for (int s = 0; s < ncomp; ++s) {
    const double *u = in + s * ldin;
    double acc = u[p];
    for (int32_t j = j0; j < j1; ++j) acc = acc + 0.5 * u[idx[j]];
    out[s * ldout + p] = acc;
  }
}
}  // namespace

// the CSR of `fine` (cached there, freed with it); coarse->edges must exist
int phx_restrict_csr(phx_mesh *coarse, phx_mesh *fine) {
  if (fine->rs_ptr) return PHX_OK;
  const int64_t nv = coarse->nv, nm = fine->rm_marked ? fine->rm_nmid : coarse->ne, n = 2 * nm;
  PHX_REQUIRE(n < INT32_MAX, PHX_ERR_VALUE, "phx_restrict: %lld entries exceed 32-bit offsets", (long long)n);
  PHX_REQUIRE_GRID(nv + nm + 256, "phx_restrict");
  hipStream_t st = coarse->stream;
  DevTemps tmp(st);
  int32_t *ptr = nullptr, *idx = nullptr, *val = nullptr;
  uint32_t *key = nullptr, *key2 = nullptr;
  PHX_HIP(tmp.alloc(&ptr, sizeof(int32_t) * (size_t)(nv + 1)));
  PHX_HIP(tmp.alloc(&idx, sizeof(int32_t) * (size_t)(n + 1)));
  PHX_HIP(tmp.alloc(&val, sizeof(int32_t) * (size_t)(n + 1)));
  PHX_HIP(tmp.alloc(&key, sizeof(uint32_t) * (size_t)(n + 1)));
  PHX_HIP(tmp.alloc(&key2, sizeof(uint32_t) * (size_t)(n + 1)));
  const dim3 block(256);
  if (nm > 0) {
    k_rs_entries<<<rm_grid(nm), block, 0, st>>>(nm, fine->rm_marked ? fine->rm_mid : nullptr, coarse->edges, nv, key, val);
    PHX_HIP(hipGetLastError());
    unsigned bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < nv) ++bits;
    size_t bytes = 0;
    void *work = nullptr;
    PHX_HIP(phx_sort_pairs(nullptr, bytes, key, key2, val, idx, (size_t)n, 0u, bits, st));
    PHX_HIP(tmp.alloc(&work, bytes ? bytes : 16));
    PHX_HIP(phx_sort_pairs(work, bytes, key, key2, val, idx, (size_t)n, 0u, bits, st));
  }
  k_rs_ptr<<<rm_grid(nv + 1), block, 0, st>>>(nv, n, key2, ptr);
  PHX_HIP(hipGetLastError());
  PHX_HIP(hipStreamSynchronize(st));
  fine->rs_ptr = ptr; fine->rs_idx = idx;                                  // they leave the guard
  for (void *q : {(void *)ptr, (void *)idx}) tmp.blocks.erase(std::find(tmp.blocks.begin(), tmp.blocks.end(), q));
  return PHX_OK;
}

extern "C" int phx_restrict(phx_mesh *coarse, phx_mesh *fine, int degree, int ncomp, const double *in, int loc_in,
                            double *out, int loc_out) {
  PHX_REQUIRE(coarse && fine, PHX_ERR_VALUE, "phx_restrict: bad arguments");
  PHX_REQUIRE(coarse->cell_type == PHX_TRIANGLE || coarse->cell_type == PHX_TETRAHEDRON, PHX_ERR_NOT_IMPLEMENTED,
              "restriction serves triangles and tetrahedra");
  PHX_REQUIRE(degree == 1, PHX_ERR_NOT_IMPLEMENTED, "restriction of degree %d is not implemented", degree);
  PHX_REQUIRE(fine != coarse && fine->refined_from == coarse->uid && fine->device == coarse->device &&
                  fine->cell_type == coarse->cell_type,
              PHX_ERR_VALUE, "the fine mesh is not the refinement of the given coarse mesh");
  PHX_REQUIRE(ncomp >= 1 && in && out, PHX_ERR_VALUE, "phx_restrict: bad arguments");
  PHX_HIP(hipSetDevice(coarse->device));
  hipStream_t st = coarse->stream;
  PHX_CHECK(phx_mesh_build_edges(coarse));
  const int64_t nv = coarse->nv, nm = fine->rm_marked ? fine->rm_nmid : coarse->ne;
  PHX_REQUIRE(fine->nv == nv + nm, PHX_ERR_VALUE, "the fine mesh is not the refinement of the given coarse mesh");
  PHX_CHECK(phx_restrict_csr(coarse, fine));
  const int64_t ldin = fine->nv, ldout = nv;
  DevTemps tmp(st);
  const double *din = in;
  double *dout = out;
  if (loc_in != PHX_DEVICE) {
    double *b = nullptr;
    PHX_HIP(tmp.alloc(&b, sizeof(double) * (size_t)ldin * ncomp));
    PHX_HIP(hipMemcpyAsync(b, in, sizeof(double) * (size_t)ldin * ncomp, hipMemcpyHostToDevice, st));
    din = b;
  }
  if (loc_out != PHX_DEVICE) PHX_HIP(tmp.alloc(&dout, sizeof(double) * (size_t)ldout * ncomp));
  k_restrict<<<rm_grid(nv), dim3(256), 0, st>>>(nv, fine->rs_ptr, fine->rs_idx, ncomp, din, ldin, dout, ldout);
  PHX_HIP(hipGetLastError());
  if (loc_out != PHX_DEVICE)
    PHX_HIP(hipMemcpyAsync(out, dout, sizeof(double) * (size_t)ldout * ncomp, hipMemcpyDeviceToHost, st));
  PHX_HIP(hipStreamSynchronize(st));
  return PHX_OK;
}
