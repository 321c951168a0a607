// Partition of an unstructured background mesh over ranks (include of phx_submesh.hip):
//   phx_partition_cells            recursive coordinate bisection of the cell centroids,
//   phx_partition_layout           vertex ownership and the cell layers of one rank,
//   phx_submesh_create_from_flags  the local mesh of a cell flag array with the parent's tags.
// Every rank runs these redundantly on the whole mesh and must obtain the same bits: integer weights, exact
// comparisons, stable sorts, min / max atomics only -- nothing depends on the order threads arrive in.  The rules
// (tie-breaks included) are restated in numpy in tests/partition_ref.py.  No counterpart in the reference (serial,
// src/phifem/mesh_scripts.py:264).
#include <limits.h>

#define PHX_PART_MAX 4096

// order-preserving map of a double onto an unsigned integer (and back)
__host__ __device__ __forceinline__ unsigned long long part_key(double v) {
  unsigned long long u;
  memcpy(&u, &v, sizeof(u));
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double part_unkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  memcpy(&v, &u, sizeof(v));
  return v;
}

// centroid: the vertices summed in local-vertex order, then divided; + 0.0 makes -0.0 and 0.0 one coordinate
__global__ void k_part_centroids(int64_t nc, int nvpc, int gdim, const int32_t *__restrict__ cells,
                                 const double *__restrict__ x, double *__restrict__ cen) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  for (int a = 0; a < gdim; ++a) {
    double s = x[(int64_t)cells[c * nvpc] * gdim + a];
    for (int k = 1; k < nvpc; ++k) s = s + x[(int64_t)cells[c * nvpc + k] * gdim + a];
    cen[c * gdim + a] = s / (double)nvpc + 0.0;
  }
}

__global__ void k_part_mm_init(int n, unsigned long long *__restrict__ mm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) mm[i] = (i & 1) ? 0ull : ~0ull;   // [part][axis][0] min key, [1] max key
}

__device__ __forceinline__ unsigned long long part_shfl_xor(unsigned long long v, int mask) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(v & 0xffffffffull), mask);
  const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), mask);
  return ((unsigned long long)hi << 32) | lo;
}

// segmented min / max of the centroid coordinates, segment = current part of the cell.  A wave whose 64 cells sit in
// one segment (all of them at the first level, most of them later: cells arrive grouped from the mesh generator or
// not at all) reduces with shuffles and issues one pair of atomics per axis; otherwise every lane issues its own.
__global__ void __launch_bounds__(256)
k_part_minmax(int64_t nc, int gdim, const int32_t *__restrict__ part, const double *__restrict__ cen,
              unsigned long long *__restrict__ mm) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool on = c < nc;
  const int p = on ? part[c] : -1;
  const int p0 = __shfl(p, 0);
  const bool uniform = __all(p == p0) && p0 >= 0;
  for (int a = 0; a < gdim; ++a) {
    const unsigned long long key = on ? part_key(cen[c * gdim + a]) : 0ull;
    if (uniform) {
      unsigned long long lo = key, hi = key;
      for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long l2 = part_shfl_xor(lo, s), h2 = part_shfl_xor(hi, s);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
      }
      if ((threadIdx.x & 63) == 0) {
        atomicMin(&mm[((int64_t)p0 * 3 + a) * 2], lo);
        atomicMax(&mm[((int64_t)p0 * 3 + a) * 2 + 1], hi);
      }
    } else if (on) {
      atomicMin(&mm[((int64_t)p * 3 + a) * 2], key);
      atomicMax(&mm[((int64_t)p * 3 + a) * 2 + 1], key);
    }
  }
}

// split axis of every segment: the FIRST axis of largest extent
__global__ void k_part_axis(int nparts, int gdim, const unsigned long long *__restrict__ mm, int32_t *__restrict__ axis) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nparts) return;
  int best = 0;
  double ebest = 0.0;
  for (int a = 0; a < gdim; ++a) {
    const unsigned long long lo = mm[((int64_t)p * 3 + a) * 2], hi = mm[((int64_t)p * 3 + a) * 2 + 1];
    const double e = lo <= hi ? part_unkey(hi) - part_unkey(lo) : 0.0;   // lo > hi: no cell in the segment
    if (a == 0 || e > ebest) { best = a; ebest = e; }
  }
  axis[p] = best;
}

__global__ void k_part_keys(int64_t nc, int gdim, const int32_t *__restrict__ part, const int32_t *__restrict__ axis,
                            const double *__restrict__ cen, unsigned long long *__restrict__ key, int32_t *__restrict__ idx) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  key[c] = part_key(cen[c * gdim + axis[part[c]]]);
  idx[c] = (int32_t)c;
}

__global__ void k_part_gather_part(int64_t nc, const int32_t *__restrict__ idx, const int32_t *__restrict__ part,
                                   uint32_t *__restrict__ pk) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < nc) pk[i] = (uint32_t)part[idx[i]];
}

__global__ void k_part_gather_w(int64_t nc, const int32_t *__restrict__ idx, const int32_t *__restrict__ w,
                                int64_t *__restrict__ wg, int *__restrict__ bad) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nc) return;
  const int32_t v = w ? w[idx[i]] : 1;
  if (v < 0) atomicOr(bad, 1);
  wg[i] = v < 0 ? 0 : v;
}

// ex = exclusive sum of wg over the sorted order: weight in front of the segment / up to its end
__global__ void k_part_bounds(int64_t nc, const uint32_t *__restrict__ pk, const int64_t *__restrict__ wg,
                              const int64_t *__restrict__ ex, int64_t *__restrict__ base, int64_t *__restrict__ end) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nc) return;
  const uint32_t p = pk[i];
  if (i == 0 || pk[i - 1] != p) base[p] = ex[i];
  if (i == nc - 1 || pk[i + 1] != p) end[p] = ex[i] + wg[i];
}

// a cell of the range [p0, p1) stays left while the weight in front of it is short of the share of the left parts
__global__ void k_part_assign(int64_t nc, const uint32_t *__restrict__ pk, const int32_t *__restrict__ idx,
                              const int64_t *__restrict__ ex, const int64_t *__restrict__ base,
                              const int64_t *__restrict__ end, const int32_t *__restrict__ p1_of, int32_t *__restrict__ part) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nc) return;
  const int32_t p0 = (int32_t)pk[i];
  const int64_t np = p1_of[p0] - p0;
  if (np <= 1) return;
  const int64_t nl = np / 2, W = end[p0] - base[p0], before = ex[i] - base[p0];
  if (!(before * np < W * nl)) part[idx[i]] = p0 + (int32_t)nl;
}

extern "C" int phx_partition_cells(phx_mesh *m, int nparts, const int32_t *weights, int32_t *part_out, int loc) {
  PHX_HIP(hipSetDevice(m->device));
  PHX_REQUIRE(nparts >= 1 && nparts <= PHX_PART_MAX, PHX_ERR_VALUE, "nparts = %d: 1 .. %d parts", nparts, PHX_PART_MAX);
  PHX_REQUIRE(part_out != nullptr, PHX_ERR_VALUE, "phx_partition_cells: no output array");
  PHX_REQUIRE(m->ci.nvpc == m->ci.tdim + 1, PHX_ERR_NOT_IMPLEMENTED, "the partitioner serves triangles and tetrahedra");
  hipStream_t st = m->stream;
  const int64_t nc = m->nc;
  const int gdim = m->gdim;
  // the ranges [p0, p1) of every level are known beforehand: p1_of[level][p0] (0 where no range starts)
  std::vector<int32_t> tab;
  int nlevels = 0;
  {
    std::vector<int32_t> cur((size_t)nparts, 0);
    cur[0] = nparts;
    for (;;) {
      bool any = false;
      for (int p = 0; p < nparts; ++p) any = any || cur[p] - p > 1;
      if (!any) break;
      tab.insert(tab.end(), cur.begin(), cur.end());
      ++nlevels;
      std::vector<int32_t> nxt = cur;
      for (int p = 0; p < nparts; ++p)
        if (cur[p] - p > 1) { const int nl = (cur[p] - p) / 2; nxt[p] = p + nl; nxt[p + nl] = cur[p]; }
      cur = nxt;
    }
  }
  int bits = 1;
  while ((1 << bits) < nparts) ++bits;
  double *cen = nullptr;
  int32_t *part = nullptr, *axis = nullptr, *idx = nullptr, *idx2 = nullptr, *p1_of = nullptr, *wdev = nullptr;
  unsigned long long *mm = nullptr, *key = nullptr, *key2 = nullptr;
  uint32_t *pk = nullptr, *pk2 = nullptr;
  int64_t *wg = nullptr, *ex = nullptr, *base = nullptr, *end = nullptr;
  int *bad = nullptr;
  void *tmp = nullptr;
  std::vector<void *> all;
  auto release = [&]() { for (void *q : all) (void)phx_free(q); };
#define PART_ALLOC(ptr, bytes)                                                        \
  do {                                                                                \
    if (phx_malloc(&ptr, (size_t)(bytes)) != hipSuccess) { release(); phx_set_error("partitioner: out of device memory"); return PHX_ERR_HIP; } \
    all.push_back(ptr);                                                               \
  } while (0)
  PART_ALLOC(cen, sizeof(double) * nc * gdim);
  PART_ALLOC(part, sizeof(int32_t) * nc);
  PART_ALLOC(axis, sizeof(int32_t) * nparts);
  PART_ALLOC(idx, sizeof(int32_t) * nc);
  PART_ALLOC(idx2, sizeof(int32_t) * nc);
  PART_ALLOC(p1_of, sizeof(int32_t) * (size_t)nparts * (nlevels > 0 ? nlevels : 1));
  PART_ALLOC(mm, sizeof(unsigned long long) * (size_t)nparts * 6);
  PART_ALLOC(key, sizeof(unsigned long long) * nc);
  PART_ALLOC(key2, sizeof(unsigned long long) * nc);
  PART_ALLOC(pk, sizeof(uint32_t) * nc);
  PART_ALLOC(pk2, sizeof(uint32_t) * nc);
  PART_ALLOC(wg, sizeof(int64_t) * nc);
  PART_ALLOC(ex, sizeof(int64_t) * nc);
  PART_ALLOC(base, sizeof(int64_t) * nparts);
  PART_ALLOC(end, sizeof(int64_t) * nparts);
  PART_ALLOC(bad, sizeof(int));
  size_t b1 = 0, b2 = 0, b3 = 0;
  int rc = PHX_OK;
  auto body = [&]() -> int {
    PHX_HIP(phx_sort_pairs(nullptr, b1, key, key2, idx, idx2, (size_t)nc, 0, 64, st));
    PHX_HIP(phx_sort_pairs(nullptr, b2, pk, pk2, idx2, idx, (size_t)nc, 0, (unsigned)bits, st));
    PHX_HIP(phx_exclusive_sum(nullptr, b3, wg, ex, (size_t)nc, st));
    PHX_HIP(phx_malloc(&tmp, std::max(std::max(b1, b2), std::max(b3, (size_t)16))));
    all.push_back(tmp);
    const int32_t *w = weights;
    if (weights && loc != PHX_DEVICE) {
      PHX_HIP(phx_malloc(&wdev, sizeof(int32_t) * (size_t)nc));
      all.push_back(wdev);
      PHX_HIP(hipMemcpyAsync(wdev, weights, sizeof(int32_t) * (size_t)nc, hipMemcpyHostToDevice, st));
      w = wdev;
    }
    if (nlevels > 0)
      PHX_HIP(hipMemcpyAsync(p1_of, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, st));
    PHX_HIP(hipMemsetAsync(part, 0, sizeof(int32_t) * (size_t)nc, st));
    PHX_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
    const dim3 block(256), grid((unsigned)phx_div_up(nc, 256)), gp((unsigned)phx_div_up(nparts * 6, 256));
    k_part_centroids<<<grid, block, 0, st>>>(nc, m->ci.nvpc, gdim, m->cells, m->x, cen);
    // one pass per level, nothing comes back to the host in between
    for (int l = 0; l < nlevels; ++l) {
      k_part_mm_init<<<gp, block, 0, st>>>(nparts * 6, mm);
      k_part_minmax<<<grid, block, 0, st>>>(nc, gdim, part, cen, mm);
      k_part_axis<<<dim3((unsigned)phx_div_up(nparts, 256)), block, 0, st>>>(nparts, gdim, mm, axis);
      k_part_keys<<<grid, block, 0, st>>>(nc, gdim, part, axis, cen, key, idx);
      // (part, coordinate, cell index): stable sorts, least significant key first; idx starts ascending
      PHX_HIP(phx_sort_pairs(tmp, b1, key, key2, idx, idx2, (size_t)nc, 0, 64, st));
      k_part_gather_part<<<grid, block, 0, st>>>(nc, idx2, part, pk);
      PHX_HIP(phx_sort_pairs(tmp, b2, pk, pk2, idx2, idx, (size_t)nc, 0, (unsigned)bits, st));
      k_part_gather_w<<<grid, block, 0, st>>>(nc, idx, w, wg, bad);
      PHX_HIP(phx_exclusive_sum(tmp, b3, wg, ex, (size_t)nc, st));
      k_part_bounds<<<grid, block, 0, st>>>(nc, pk2, wg, ex, base, end);
      k_part_assign<<<grid, block, 0, st>>>(nc, pk2, idx, ex, base, end, p1_of + (size_t)l * nparts, part);
    }
    PHX_HIP(hipGetLastError());
    int hbad = 0;
    PHX_HIP(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    PHX_HIP(hipMemcpyAsync(part_out, part, sizeof(int32_t) * (size_t)nc,
                           loc == PHX_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    PHX_HIP(hipStreamSynchronize(st));
    PHX_REQUIRE(hbad == 0, PHX_ERR_VALUE, "phx_partition_cells: negative cell weight");
    return PHX_OK;
  };
  rc = body();
  if (rc != PHX_OK) (void)hipStreamSynchronize(st);
  release();
#undef PART_ALLOC
  return rc;
}

// ---- ownership and layers ---------------------------------------------------------------------------------------
__global__ void k_fill_i32(int64_t n, int32_t v, int32_t *__restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) out[i] = v;
}
__global__ void k_own_first(int64_t nc, int nvpc, const int32_t *__restrict__ cells, const int8_t *__restrict__ ctags,
                            int32_t *__restrict__ first) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int t = ctags[c] & PHX_TAG_MASK;
  if (t != 1 && t != 2) return;
  for (int k = 0; k < nvpc; ++k) atomicMin(&first[cells[c * nvpc + k]], (int32_t)c);
}
__global__ void k_own_part(int64_t nv, const int32_t *__restrict__ first, const int32_t *__restrict__ part,
                           int32_t *__restrict__ owner) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v < nv) owner[v] = first[v] == INT_MAX ? -1 : part[first[v]];
}
// layer 1: cells with a vertex the rank owns; `stat[0]` |= 1 when there is one
__global__ void k_layer_one(int64_t nc, int nvpc, const int32_t *__restrict__ cells, const int32_t *__restrict__ owner,
                            int rank, uint8_t *__restrict__ flags, int *__restrict__ stat) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  bool mine = false;
  for (int k = 0; k < nvpc; ++k) mine = mine || owner[cells[c * nvpc + k]] == rank;
  flags[c] = mine ? 1 : 0;
  if (mine) atomicOr(&stat[0], 1);
}
// facet neighbours of the cells flagged `from` that carry no flag yet get `to` (every writer stores the same byte)
__global__ void k_layer_facets(int64_t nc, int nfpc, const int32_t *__restrict__ c2f, const int32_t *__restrict__ f2c,
                               int from, int to, uint8_t *__restrict__ flags) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc || flags[c] != from) return;
  for (int k = 0; k < nfpc; ++k) {
    const int64_t f = c2f[c * nfpc + k];
    for (int j = 0; j < 2; ++j) {
      const int32_t nb = f2c[2 * f + j];
      if (nb >= 0 && nb != c) {
        const uint8_t cur = flags[nb];
        if (cur == 0 || cur == to) flags[nb] = (uint8_t)to;
      }
    }
  }
}
// vertices of the flagged cells
__global__ void k_layer_touch(int64_t nc, int nvpc, const int32_t *__restrict__ cells, const uint8_t *__restrict__ flags,
                              uint8_t *__restrict__ touched) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc || flags[c] == 0) return;
  for (int k = 0; k < nvpc; ++k) touched[cells[c * nvpc + k]] = 1;
}
// layer 3: unflagged cells with a touched vertex
__global__ void k_layer_three(int64_t nc, int nvpc, const int32_t *__restrict__ cells, const uint8_t *__restrict__ touched,
                              uint8_t *__restrict__ flags) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc || flags[c] != 0) return;
  bool any = false;
  for (int k = 0; k < nvpc; ++k) any = any || touched[cells[c * nvpc + k]] != 0;
  if (any) flags[c] = 3;
}
// lowest-numbered cell outside Omega_h (stat[1], INT_MAX: none)
__global__ void k_first_exterior(int64_t nc, const int8_t *__restrict__ ctags, int *__restrict__ stat) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int t = ctags[c] & PHX_TAG_MASK;
  if (t != 1 && t != 2) atomicMin(&stat[1], (int)c);
}

extern "C" int phx_partition_layout(phx_mesh *m, int nparts, const int32_t *part, int rank, int32_t *owner_out,
                                    uint8_t *flags_out, int loc) {
  PHX_HIP(hipSetDevice(m->device));
  PHX_REQUIRE(m->have_cell_tags, PHX_ERR_VALUE, "the cells must be tagged before the partition layout");
  PHX_REQUIRE(part != nullptr && rank >= 0 && rank < nparts, PHX_ERR_VALUE, "phx_partition_layout: rank %d of %d parts", rank, nparts);
  hipStream_t st = m->stream;
  const int64_t nc = m->nc, nv = m->nv;
  int32_t *first = nullptr, *owner = nullptr, *pdev = nullptr;
  uint8_t *flags = nullptr, *touched = nullptr;
  int *stat = nullptr;
  std::vector<void *> all;
  auto body = [&]() -> int {
    PHX_HIP(phx_malloc(&first, sizeof(int32_t) * (size_t)nv)); all.push_back(first);
    PHX_HIP(phx_malloc(&owner, sizeof(int32_t) * (size_t)nv)); all.push_back(owner);
    PHX_HIP(phx_malloc(&flags, (size_t)nc)); all.push_back(flags);
    PHX_HIP(phx_malloc(&touched, (size_t)nv)); all.push_back(touched);
    PHX_HIP(phx_malloc(&stat, sizeof(int) * 2)); all.push_back(stat);
    const int32_t *p = part;
    if (loc != PHX_DEVICE) {
      PHX_HIP(phx_malloc(&pdev, sizeof(int32_t) * (size_t)nc)); all.push_back(pdev);
      PHX_HIP(hipMemcpyAsync(pdev, part, sizeof(int32_t) * (size_t)nc, hipMemcpyHostToDevice, st));
      p = pdev;
    }
    const int hinit[2] = {0, INT_MAX};
    const uint8_t two = 2;
    PHX_HIP(hipMemcpyAsync(stat, hinit, sizeof(hinit), hipMemcpyHostToDevice, st));
    const dim3 block(256), gc((unsigned)phx_div_up(nc, 256)), gv((unsigned)phx_div_up(nv, 256));
    k_fill_i32<<<gv, block, 0, st>>>(nv, INT_MAX, first);
    k_own_first<<<gc, block, 0, st>>>(nc, m->ci.nvpc, m->cells, m->cell_tags, first);
    k_own_part<<<gv, block, 0, st>>>(nv, first, p, owner);
    k_layer_one<<<gc, block, 0, st>>>(nc, m->ci.nvpc, m->cells, owner, rank, flags, stat);
    // layers 1 - 2 complete the owned rows, 3 - 4 the diagonal of every column those rows refer to
    k_layer_facets<<<gc, block, 0, st>>>(nc, m->ci.nfpc, m->c2f, m->f2c, 1, 2, flags);
    PHX_HIP(hipMemsetAsync(touched, 0, (size_t)nv, st));
    k_layer_touch<<<gc, block, 0, st>>>(nc, m->ci.nvpc, m->cells, flags, touched);
    k_layer_three<<<gc, block, 0, st>>>(nc, m->ci.nvpc, m->cells, touched, flags);
    k_layer_facets<<<gc, block, 0, st>>>(nc, m->ci.nfpc, m->c2f, m->f2c, 3, 4, flags);
    k_first_exterior<<<gc, block, 0, st>>>(nc, m->cell_tags, stat);
    PHX_HIP(hipGetLastError());
    int hstat[2] = {0, 0};
    PHX_HIP(hipMemcpyAsync(hstat, stat, sizeof(hstat), hipMemcpyDeviceToHost, st));
    PHX_HIP(hipStreamSynchronize(st));
    if (!(hstat[0] & 1)) {
      // the rank owns nothing: one placeholder cell, so that it has a mesh and joins every collective
      const int64_t c = hstat[1] != INT_MAX ? hstat[1] : 0;
      PHX_HIP(hipMemcpyAsync(flags + c, &two, 1, hipMemcpyHostToDevice, st));
    }
    const hipMemcpyKind kind = loc == PHX_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (owner_out) PHX_HIP(hipMemcpyAsync(owner_out, owner, sizeof(int32_t) * (size_t)nv, kind, st));
    if (flags_out) PHX_HIP(hipMemcpyAsync(flags_out, flags, (size_t)nc, kind, st));
    PHX_HIP(hipStreamSynchronize(st));
    return PHX_OK;
  };
  const int rc = body();
  if (rc != PHX_OK) (void)hipStreamSynchronize(st);
  for (void *q : all) (void)phx_free(q);
  return rc;
}

// Local mesh of a rank: the flagged cells (flags[nc] != 0) as a mesh of their own, cells and vertices ascending in the
// parent's numbering, the parent's cell and facet tags transferred.  NOT a sub-mesh in the sense of box_mode = False: the
// facets on its rim are cuts, not boundary; the P1 assembly takes every integration entity from the tags (ds_bdy(100),
// ghost-penalty facets) and never looks at the boundary-facet list.  Maps through phx_submesh_maps.
extern "C" int phx_submesh_create_from_flags(phx_mesh *m, const uint8_t *flags, int loc, phx_mesh **sub_out) {
  PHX_HIP(hipSetDevice(m->device));
  PHX_REQUIRE(m->have_cell_tags && m->have_facet_tags, PHX_ERR_VALUE,
              "cell and facet tags must be computed before the local mesh");
  PHX_REQUIRE(flags != nullptr, PHX_ERR_VALUE, "phx_submesh_create_from_flags: no flags");
  hipStream_t st = m->stream;
  uint8_t *fdev = nullptr;
  const uint8_t *f = flags;
  if (loc != PHX_DEVICE) {
    PHX_HIP(phx_malloc(&fdev, (size_t)m->nc));
    PHX_HIP(hipMemcpyAsync(fdev, flags, (size_t)m->nc, hipMemcpyHostToDevice, st));
    f = fdev;
  }
  int32_t *c_map = nullptr, *v_map = nullptr, *renum = nullptr;
  int64_t ncs = 0;
  int rc = phx_select_indices(st, m->nc, SelFlag{f}, &c_map, &ncs);
  (void)phx_free(fdev);
  if (rc != PHX_OK) return rc;
  if (ncs == 0) {
    PHX_HIP(phx_free(c_map));
    phx_set_error("no cell is flagged: empty local mesh");
    return PHX_ERR_VALUE;
  }
  phx_mesh *s = nullptr;
  rc = submesh_from_cells(m, c_map, ncs, &s, &v_map, &renum);
  PHX_HIP(phx_free(c_map));
  if (rc != PHX_OK) return rc;
  PHX_HIP(phx_free(v_map)); PHX_HIP(phx_free(renum));
  *sub_out = s;
  return PHX_OK;
}
