// Marked refinement of triangle and tetrahedron meshes: seed, closure, recursive bisection by the greatest marked edge,
// and the nested coarse -> fine transfer onto such a mesh (include of phx_submesh.hip after phx_refine.inc.hip:
// -ffp-contract=off, the edge order compares len2 bit for bit).  Stands in for dolfinx.mesh.refine with marked edges;
// include/phifem_hip.h and DESIGN.md 7e state the rule, tests/refine_marked_ref.py restates it in numpy.
//
// Local degree-2 nodes as in phx_refine.inc.hip: 0 .. nvpc-1 the cell's vertices, nvpc + k the midpoint of local edge
// k.  A sub-simplex is a tuple of nvpc such nodes, packed four bits per position.  Everything a cell needs to know
// about the edge order is the rank of each of its edges among its own (0 = greatest): 3 bits per local edge, `ordpk`.
namespace {

template <int NV> __device__ __forceinline__ int rm_pa(int k) {
  return NV == 3 ? (k == 0 ? 1 : 0) : (k == 0 ? 2 : (k < 3 ? 1 : 0));
}
template <int NV> __device__ __forceinline__ int rm_pb(int k) {
  return NV == 3 ? (k == 2 ? 1 : 2) : ((k == 0 || k == 1 || k == 3) ? 3 : (k == 5 ? 1 : 2));
}

struct SelMarkedEdge {
  const uint8_t *f;
  __host__ __device__ bool operator()(const int32_t &e) const { return f[e] != 0; }
  __host__ __device__ const int8_t *bytes() const { return reinterpret_cast<const int8_t *>(f); }
  __host__ __device__ bool test(int tag, int32_t) const { return tag != 0; }
};

// ---- seed: the given edge mask (or nothing), then every marked cell marks its edges
__global__ void __launch_bounds__(256)
k_rm_seed_cells(int64_t nc, int nepc, const uint8_t *__restrict__ cell_marks, const int32_t *__restrict__ c2e,
                uint8_t *emark) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc || !cell_marks[c]) return;
  for (int k = 0; k < nepc; ++k) emark[c2e[c * nepc + k]] = 1;
}

// ---- the edge order, once per cell: key of edge (p, q), p < q: len2 = ((dx dx + dy dy) + dz dz), d = x[q] - x[p];
// the greater len2 wins, on equal len2 the lexicographically smaller (p, q)
template <int NV>
__global__ void __launch_bounds__(256)
k_rm_order(int64_t nc, const double *__restrict__ x, const int32_t *__restrict__ cells, uint32_t *__restrict__ ordpk) {
  constexpr int NE = NV == 3 ? 3 : 6, GD = NV - 1;
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  int32_t v[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = cells[c * NV + j];
  double len2[NE];
  int32_t p[NE], q[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const int32_t a = v[rm_pa<NV>(k)], b = v[rm_pb<NV>(k)];
    p[k] = a < b ? a : b;
    q[k] = a < b ? b : a;
    const double dx = x[(int64_t)q[k] * GD] - x[(int64_t)p[k] * GD];
    const double dy = x[(int64_t)q[k] * GD + 1] - x[(int64_t)p[k] * GD + 1];
    double l = dx * dx + dy * dy;
    if (NV == 4) {
      const double dz = x[(int64_t)q[k] * GD + 2] - x[(int64_t)p[k] * GD + 2];
      l = l + dz * dz;
    }
    len2[k] = l;
  }
  uint32_t pk = 0;
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    uint32_t r = 0;
#pragma unroll
    for (int l = 0; l < NE; ++l)
      if (l != k && (len2[l] > len2[k] || (len2[l] == len2[k] && (p[l] < p[k] || (p[l] == p[k] && q[l] < q[k]))))) ++r;
    pk |= r << (3 * k);
  }
  ordpk[c] = pk;
}

// ---- closure sweep, one lane per cell: a cell with a marked edge marks its greatest edge, a face with a marked edge
// its greatest (the lane repeats this on its own six bits until they are stable).  Marks are byte stores of 1 and the
// operator is monotone: whatever a lane sees or misses of its neighbours' stores, the fixed point is the least one.
template <int NV>
__global__ void __launch_bounds__(256)
k_rm_sweep(int64_t nc, const int32_t *__restrict__ c2e, const uint32_t *__restrict__ ordpk, uint8_t *emark,
           int32_t *changed) {
  constexpr int NE = NV == 3 ? 3 : 6;
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  int32_t e[NE];
  unsigned mask = 0;
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    e[k] = c2e[c * NE + k];
    mask |= (unsigned)(emark[e[k]] != 0) << k;
  }
  if (!mask) return;
  const uint32_t pk = ordpk[c];
  unsigned want = mask;
#pragma unroll
  for (int k = 0; k < NE; ++k)
    if (((pk >> (3 * k)) & 7u) == 0u) want |= 1u << k;
  if (NV == 4) {
    const unsigned face[4] = {7u, 25u, 42u, 52u};    // local edges of the face opposite vertex 0, 1, 2, 3
    unsigned old;
    do {
      old = want;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        if (!(want & face[f])) continue;
        unsigned best = 0, br = 8;
#pragma unroll
        for (int k = 0; k < NE; ++k) {
          const unsigned r = (pk >> (3 * k)) & 7u;
          if (((face[f] >> k) & 1u) && r < br) { br = r; best = (unsigned)k; }
        }
        want |= 1u << best;
      }
    } while (want != old);
  }
  const unsigned add = want & ~mask;
  if (!add) return;
#pragma unroll
  for (int k = 0; k < NE; ++k)
    if ((add >> k) & 1u) emark[e[k]] = 1;
  *changed = 1;
}

__global__ void __launch_bounds__(256)
k_rm_rank(int64_t nm, const int32_t *__restrict__ list, int32_t *__restrict__ erank) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r < nm) erank[list[r]] = (int32_t)r;
}

// ---- recursive bisection of one cell.  While the tuple holds both end nodes of a marked edge: take the greatest such
// edge, at positions i < j, m its midpoint node; child 0 = position j replaced by m, child 1 = position i replaced by m;
// depth first, child 0 first.  A tuple at depth d holds nvpc - d coarse vertices, so only depths 0 .. 2 split and at
// most 4 tuples of 16 bits wait at a time: the stack is one 64-bit register.  -> number of leaves
template <int NV, typename F>
__device__ __forceinline__ int rm_leaves(unsigned mask, uint32_t pk, F leaf) {
  constexpr int NE = NV == 3 ? 3 : 6;
  unsigned long long stack = NV == 3 ? 0x210ull : 0x3210ull;
  int sp = 1, n = 0;
  while (sp > 0) {
    const uint32_t t = (uint32_t)(stack & 0xffffull);
    stack >>= 16;
    --sp;
    int best = -1, bi = 0, bj = 0;
    unsigned br = 8;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
      if (!((mask >> k) & 1u)) continue;
      int ia = -1, ib = -1;
#pragma unroll
      for (int s = 0; s < NV; ++s) {
        const int node = (int)((t >> (4 * s)) & 15u);
        if (node == rm_pa<NV>(k)) ia = s;
        if (node == rm_pb<NV>(k)) ib = s;
      }
      const unsigned r = (pk >> (3 * k)) & 7u;
      if (ia >= 0 && ib >= 0 && r < br) { br = r; best = k; bi = ia < ib ? ia : ib; bj = ia < ib ? ib : ia; }
    }
    if (best < 0) { leaf(n, t); ++n; continue; }
    const uint32_t m = (uint32_t)(NV + best);
    const uint32_t c0 = (t & ~(15u << (4 * bj))) | (m << (4 * bj)), c1 = (t & ~(15u << (4 * bi))) | (m << (4 * bi));
    stack = (stack << 32) | ((unsigned long long)c1 << 16) | c0;
    sp += 2;
  }
  return n;
}

template <int NV>
__device__ __forceinline__ unsigned rm_cell_mask(int64_t c, const int32_t *__restrict__ c2e, const uint8_t *__restrict__ emark,
                                                 int32_t *e) {
  constexpr int NE = NV == 3 ? 3 : 6;
  unsigned mask = 0;
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    e[k] = c2e[c * NE + k];
    mask |= (unsigned)(emark[e[k]] != 0) << k;
  }
  return mask;
}

// cnt[c] = children of cell c, cnt[nc] = 0 (the exclusive sum over nc + 1 entries ends with the total)
template <int NV>
__global__ void __launch_bounds__(256)
k_rm_count(int64_t nc, const int32_t *__restrict__ c2e, const uint32_t *__restrict__ ordpk,
           const uint8_t *__restrict__ emark, int32_t *__restrict__ cnt) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c > nc) return;
  if (c == nc) { cnt[c] = 0; return; }
  int32_t e[NV == 3 ? 3 : 6];
  const unsigned mask = rm_cell_mask<NV>(c, c2e, emark, e);
  cnt[c] = mask ? rm_leaves<NV>(mask, ordpk[c], [](int, uint32_t) {}) : 1;
}

// one lane per COARSE cell: its children are the fine cells off[c] .. off[c+1]-1, in the order the leaves are reached
template <int NV>
__global__ void __launch_bounds__(256)
k_rm_write(int64_t nc, const int32_t *__restrict__ cells, const int32_t *__restrict__ c2e,
           const uint32_t *__restrict__ ordpk, const uint8_t *__restrict__ emark, const int32_t *__restrict__ erank,
           const int32_t *__restrict__ off, int64_t nv, int32_t *__restrict__ fcells, int32_t *__restrict__ parent,
           int8_t *__restrict__ child) {
  constexpr int NE = NV == 3 ? 3 : 6;
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  int32_t e[NE], g[NV + NE];
  const unsigned mask = rm_cell_mask<NV>(c, c2e, emark, e);
#pragma unroll
  for (int j = 0; j < NV; ++j) g[j] = cells[c * NV + j];
#pragma unroll
  for (int k = 0; k < NE; ++k) g[NV + k] = ((mask >> k) & 1u) ? (int32_t)(nv + erank[e[k]]) : -1;
  const int64_t base = off[c];
  rm_leaves<NV>(mask, ordpk[c], [&](int n, uint32_t t) {
    const int64_t i = base + n;
    parent[i] = (int32_t)c;
#pragma unroll
    for (int s = 0; s < NV; ++s) {
      const int node = (int)((t >> (4 * s)) & 15u);
      int32_t id = -1;
#pragma unroll
      for (int d = 0; d < NV + NE; ++d)
        if (node == d) id = g[d];
      fcells[i * NV + s] = id;
      child[i * NV + s] = (int8_t)node;
    }
  });
}

// fine vertex v < nv is coarse vertex v, fine vertex nv + r the midpoint 0.5 x_p + 0.5 x_q of the r-th marked edge
__global__ void __launch_bounds__(256)
k_rm_coords(int64_t nvf, int64_t nv, int gdim, const double *__restrict__ x, const int32_t *__restrict__ list,
            const int32_t *__restrict__ edges, double *__restrict__ xf) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nvf) return;
  if (i < nv) {
    for (int a = 0; a < gdim; ++a) xf[i * gdim + a] = x[i * gdim + a];
    return;
  }
  const int64_t e = list[i - nv], p = edges[2 * e], q = edges[2 * e + 1];
  for (int a = 0; a < gdim; ++a) xf[i * gdim + a] = 0.5 * x[p * gdim + a] + 0.5 * x[q * gdim + a];
}

// ---- transfer.  Degree 1: the coordinate arithmetic at the new vertices
__global__ void __launch_bounds__(256)
k_rm_prol_mid(int64_t nm, const int32_t *__restrict__ list, const int32_t *__restrict__ edges, int ncomp,
              const double *__restrict__ in, int64_t ldin, double *__restrict__ out, int64_t ldout) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= nm) return;
  const int64_t e = list[r], p = edges[2 * e], q = edges[2 * e + 1];
  for (int s = 0; s < ncomp; ++s) out[s * ldout + r] = 0.5 * in[s * ldin + p] + 0.5 * in[s * ldin + q];
}
// degree 2: fine vertex nv + r copies the coarse edge DoF of the r-th marked edge
__global__ void __launch_bounds__(256)
k_rm_prol_edge_dofs(int64_t nm, const int32_t *__restrict__ list, int ncomp, const double *__restrict__ in, int64_t ldin,
                    double *__restrict__ out, int64_t ldout) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= nm) return;
  for (int s = 0; s < ncomp; ++s) out[s * ldout + r] = in[s * ldin + list[r]];
}
// degree 2, fine edge DoFs: owner[fe] = lowest-numbered parent cell that contains the fine edge (integer atomicMin),
// then that parent writes its P2 function at the fine edge's midpoint.  lambda = mean of the barycentrics of the two
// child_nodes entries (multiples of 1/4: the weights lambda_i (2 lambda_i - 1), 4 lambda_i lambda_j are exact), summed
// over the parent's local DoFs in ascending order, zero weights skipped.  Children of one parent that share a fine
// edge compute the same bits.
__global__ void __launch_bounds__(256)
k_rm_prol2_owner(int64_t n, int nepc, const int32_t *__restrict__ fc2e, const int32_t *__restrict__ parent,
                 int32_t *__restrict__ owner) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  atomicMin(&owner[fc2e[i]], parent[i / nepc]);
}
template <int NV>
__global__ void __launch_bounds__(256)
k_rm_prol2_edges(int64_t ncf, const int32_t *__restrict__ cells, const int32_t *__restrict__ c2e, int64_t nv,
                 const int32_t *__restrict__ parent, const int8_t *__restrict__ child, const int32_t *__restrict__ fc2e,
                 const int32_t *__restrict__ owner, int ncomp, const double *__restrict__ in, int64_t ldin,
                 double *__restrict__ out, int64_t ldout) {
  constexpr int NE = NV == 3 ? 3 : 6, ND = NV + NE;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncf) return;
  const int64_t c = parent[i];
  int64_t g[ND];
#pragma unroll
  for (int d = 0; d < NV; ++d) g[d] = cells[c * NV + d];
#pragma unroll
  for (int k = 0; k < NE; ++k) g[NV + k] = nv + c2e[c * NE + k];
  int t[NV];
#pragma unroll
  for (int s = 0; s < NV; ++s) t[s] = child[i * NV + s];
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    const int64_t fe = fc2e[i * NE + j];
    if (owner[fe] != (int32_t)c) continue;
    const int ends[2] = {t[rm_pa<NV>(j)], t[rm_pb<NV>(j)]};
    double lam[NV];
#pragma unroll
    for (int s = 0; s < NV; ++s) {
      double l2[2];
#pragma unroll
      for (int z = 0; z < 2; ++z) {
        const int node = ends[z];
        l2[z] = node < NV ? (node == s ? 1.0 : 0.0)
                          : ((rm_pa<NV>(node - NV) == s || rm_pb<NV>(node - NV) == s) ? 0.5 : 0.0);
      }
      lam[s] = 0.5 * l2[0] + 0.5 * l2[1];
    }
    double w[ND];
#pragma unroll
    for (int d = 0; d < NV; ++d) w[d] = lam[d] * (2.0 * lam[d] - 1.0);
#pragma unroll
    for (int k = 0; k < NE; ++k) w[NV + k] = 4.0 * lam[rm_pa<NV>(k)] * lam[rm_pb<NV>(k)];
    for (int s = 0; s < ncomp; ++s) {
      const double *u = in + s * ldin;
      double acc = 0.0;
      bool first = true;
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        if (w[d] == 0.0) continue;
        const double v = w[d] * u[g[d]];
        acc = first ? v : acc + v;
        first = false;
      }
      out[s * ldout + fe] = acc;
    }
  }
}

dim3 rm_grid(int64_t n) { return dim3((unsigned)phx_div_up(n > 0 ? n : 1, 256)); }
}  // namespace

extern "C" int phx_mesh_refine_marked(phx_mesh *m, const uint8_t *cell_marks, const uint8_t *edge_marks, int loc,
                                      phx_mesh **fine_out, int64_t *info) {
  PHX_REQUIRE(m && fine_out, PHX_ERR_VALUE, "phx_mesh_refine_marked: bad arguments");
  PHX_REQUIRE(m->cell_type != PHX_QUADRILATERAL, PHX_ERR_NOT_IMPLEMENTED,
              "marked refinement of quadrilaterals is not implemented (it needs hanging nodes)");
  PHX_REQUIRE(m->cell_type == PHX_TRIANGLE || m->cell_type == PHX_TETRAHEDRON, PHX_ERR_NOT_IMPLEMENTED,
              "marked refinement serves triangles and tetrahedra");
  PHX_HIP(hipSetDevice(m->device));
  PHX_REQUIRE(!m->slab_cut, PHX_ERR_VALUE,
              "a slab with declared cut faces cannot be refined: the fine mesh cannot inherit them");
  const bool tri = m->cell_type == PHX_TRIANGLE;
  const int nvpc = tri ? 3 : 4, nepc = tri ? 3 : 6, maxchild = tri ? 4 : 8;
  const double t0 = wall_seconds();
  PHX_CHECK(phx_mesh_build_edges(m));
  const int64_t nc = m->nc, nv = m->nv, ne = m->ne;
  // every count is bounded by the all-marked case, known before anything is allocated
  PHX_REQUIRE(nv + ne < INT32_MAX && nc * (int64_t)maxchild * m->ci.nfpc < INT32_MAX, PHX_ERR_VALUE,
              "refined mesh may be too large for 32-bit local ids (up to %lld vertices, %lld cells)",
              (long long)(nv + ne), (long long)(nc * maxchild));
  PHX_REQUIRE_GRID(nc + 256, "phx_mesh_refine_marked");
  PHX_REQUIRE_GRID(nv + ne + 255, "phx_mesh_refine_marked");
  hipStream_t st = m->stream;
  const dim3 block(256);
  const hipMemcpyKind up = loc == PHX_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  DevTemps tmp(st);
  const double t1 = wall_seconds();
  // ---- 1. seed
  uint8_t *emark = nullptr;
  PHX_HIP(tmp.alloc(&emark, (size_t)ne + 4));
  if (edge_marks) PHX_HIP(hipMemcpyAsync(emark, edge_marks, (size_t)ne, up, st));
  else PHX_HIP(hipMemsetAsync(emark, 0, (size_t)ne, st));
  if (cell_marks) {
    const uint8_t *cm = cell_marks;
    if (loc != PHX_DEVICE) {
      uint8_t *b = nullptr;
      PHX_HIP(tmp.alloc(&b, (size_t)nc));
      PHX_HIP(hipMemcpyAsync(b, cell_marks, (size_t)nc, hipMemcpyHostToDevice, st));
      cm = b;
    }
    k_rm_seed_cells<<<rm_grid(nc), block, 0, st>>>(nc, nepc, cm, m->c2e, emark);
  }
  // ---- 2. closure
  uint32_t *ordpk = nullptr;
  int32_t *changed = nullptr;
  PHX_HIP(tmp.alloc(&ordpk, sizeof(uint32_t) * (size_t)nc));
  PHX_HIP(tmp.alloc(&changed, sizeof(int32_t)));
  if (tri) k_rm_order<3><<<rm_grid(nc), block, 0, st>>>(nc, m->x, m->cells, ordpk);
  else k_rm_order<4><<<rm_grid(nc), block, 0, st>>>(nc, m->x, m->cells, ordpk);
  PHX_HIP(hipGetLastError());
  int64_t sweeps = 0;
  if (cell_marks || edge_marks) {
    for (;;) {
      int32_t ch = 0;
      PHX_HIP(hipMemsetAsync(changed, 0, sizeof(int32_t), st));
      if (tri) k_rm_sweep<3><<<rm_grid(nc), block, 0, st>>>(nc, m->c2e, ordpk, emark, changed);
      else k_rm_sweep<4><<<rm_grid(nc), block, 0, st>>>(nc, m->c2e, ordpk, emark, changed);
      PHX_HIP(hipGetLastError());
      PHX_HIP(hipMemcpyAsync(&ch, changed, sizeof(int32_t), hipMemcpyDeviceToHost, st));
      PHX_HIP(hipStreamSynchronize(st));
      ++sweeps;
      if (!ch) break;
      PHX_REQUIRE(sweeps <= ne + 1, PHX_ERR_HIP, "phx_mesh_refine_marked: the closure does not converge");
    }
  }
  // ---- 3. numbering: midpoints by the ordered select, children by count + exclusive sum
  int32_t *list = nullptr;
  int64_t nm = 0;
  PHX_CHECK(phx_select_indices(st, ne, SelMarkedEdge{emark}, &list, &nm));
  tmp.adopt(list);
  int32_t *erank = nullptr, *cnt = nullptr, *off = nullptr;
  PHX_HIP(tmp.alloc(&erank, sizeof(int32_t) * (size_t)ne));
  PHX_HIP(tmp.alloc(&cnt, sizeof(int32_t) * (size_t)(nc + 1)));
  PHX_HIP(tmp.alloc(&off, sizeof(int32_t) * (size_t)(nc + 1)));
  k_rm_rank<<<rm_grid(nm), block, 0, st>>>(nm, list, erank);
  if (tri) k_rm_count<3><<<rm_grid(nc + 1), block, 0, st>>>(nc, m->c2e, ordpk, emark, cnt);
  else k_rm_count<4><<<rm_grid(nc + 1), block, 0, st>>>(nc, m->c2e, ordpk, emark, cnt);
  PHX_HIP(hipGetLastError());
  size_t sbytes = 0;
  void *stmp = nullptr;
  PHX_HIP(phx_exclusive_sum(nullptr, sbytes, cnt, off, (size_t)(nc + 1), st));
  PHX_HIP(tmp.alloc(&stmp, sbytes ? sbytes : 16));
  PHX_HIP(phx_exclusive_sum(stmp, sbytes, cnt, off, (size_t)(nc + 1), st));
  int32_t total = 0;
  PHX_HIP(hipMemcpyAsync(&total, off + nc, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PHX_HIP(hipStreamSynchronize(st));
  const int64_t ncf = total, nvf = nv + nm;
  PHX_REQUIRE(ncf >= nc && ncf <= nc * (int64_t)maxchild, PHX_ERR_HIP, "phx_mesh_refine_marked: bad child count %lld", (long long)ncf);
  // ---- 4. write
  double *xf = nullptr;
  int32_t *cf = nullptr, *parent = nullptr;
  int8_t *child = nullptr;
  PHX_HIP(tmp.alloc(&xf, sizeof(double) * (size_t)nvf * m->gdim));
  PHX_HIP(tmp.alloc(&cf, sizeof(int32_t) * (size_t)ncf * nvpc));
  PHX_HIP(tmp.alloc(&parent, sizeof(int32_t) * (size_t)ncf));
  PHX_HIP(tmp.alloc(&child, (size_t)ncf * nvpc));
  k_rm_coords<<<rm_grid(nvf), block, 0, st>>>(nvf, nv, m->gdim, m->x, list, m->edges, xf);
  if (tri) k_rm_write<3><<<rm_grid(nc), block, 0, st>>>(nc, m->cells, m->c2e, ordpk, emark, erank, off, nv, cf, parent, child);
  else k_rm_write<4><<<rm_grid(nc), block, 0, st>>>(nc, m->cells, m->c2e, ordpk, emark, erank, off, nv, cf, parent, child);
  PHX_HIP(hipGetLastError());
  // the new mesh copies device sources on ITS stream: everything above has to have run
  PHX_HIP(hipStreamSynchronize(st));
  const double t2 = wall_seconds();
  // ---- 5. the fine mesh: an ordinary untagged mesh, never a lattice, whatever stood behind the coarse one
  phx_mesh *f = nullptr;
  PHX_CHECK(phx_mesh_create_from(m->gdim, m->cell_type, nvf, xf, ncf, cf, PHX_DEVICE, m->device, &f));
  f->refined_from = m->uid;
  f->refine_nchild = 0;
  f->rm_marked = true;
  f->rm_nmid = nm;
  f->rm_parent = parent; f->rm_child = child; f->rm_mid = list;          // they leave the guard
  for (void *q : {(void *)parent, (void *)child, (void *)list}) tmp.blocks.erase(std::find(tmp.blocks.begin(), tmp.blocks.end(), q));
  f->timings[5] = t1 - t0;                 // edge numbering of the coarse mesh (0 when it existed)
  f->timings[6] = t2 - t1;                 // seed, closure, numbering and write
  f->timings[7] = wall_seconds() - t2;     // creation of the fine mesh
  if (info) { info[0] = nm; info[1] = sweeps; info[2] = ncf; }
  *fine_out = f;
  return PHX_OK;
}

int phx_prolongate_marked(phx_mesh *coarse, phx_mesh *fine, int degree, int ncomp, const double *in, int loc_in,
                          double *out, int loc_out) {
  PHX_REQUIRE(coarse->cell_type == PHX_TRIANGLE || coarse->cell_type == PHX_TETRAHEDRON, PHX_ERR_NOT_IMPLEMENTED,
              "marked refinement serves triangles and tetrahedra");
  PHX_REQUIRE(degree == 1 || degree == 2, PHX_ERR_NOT_IMPLEMENTED, "prolongation of degree %d is not implemented", degree);
  PHX_REQUIRE(fine != coarse && fine->refined_from == coarse->uid && fine->device == coarse->device &&
                  fine->nv == coarse->nv + fine->rm_nmid && fine->cell_type == coarse->cell_type,
              PHX_ERR_VALUE, "the fine mesh is not the refinement of the given coarse mesh");
  PHX_REQUIRE(ncomp >= 1 && in && out, PHX_ERR_VALUE, "phx_prolongate: bad arguments");
  PHX_HIP(hipSetDevice(coarse->device));
  hipStream_t st = coarse->stream;
  PHX_CHECK(phx_mesh_build_edges(coarse));
  if (degree == 2) PHX_CHECK(phx_mesh_build_edges(fine));
  const bool tri = coarse->cell_type == PHX_TRIANGLE;
  const int nepc = tri ? 3 : 6;
  const int64_t nv = coarse->nv, nm = fine->rm_nmid;
  const int64_t ldin = degree == 1 ? nv : nv + coarse->ne;
  const int64_t ldout = degree == 1 ? fine->nv : fine->nv + fine->ne;
  PHX_REQUIRE_GRID(fine->nc * (int64_t)nepc + 255, "phx_prolongate");
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
  const dim3 block(256);
  k_prol_copy<<<rm_grid(nv), block, 0, st>>>(nv, ncomp, din, ldin, dout, ldout);
  if (degree == 1) {
    k_rm_prol_mid<<<rm_grid(nm), block, 0, st>>>(nm, fine->rm_mid, coarse->edges, ncomp, din, ldin, dout + nv, ldout);
  } else {
    k_rm_prol_edge_dofs<<<rm_grid(nm), block, 0, st>>>(nm, fine->rm_mid, ncomp, din + nv, ldin, dout + nv, ldout);
    int32_t *owner = nullptr;
    PHX_HIP(tmp.alloc(&owner, sizeof(int32_t) * (size_t)fine->ne));
    PHX_HIP(hipMemsetAsync(owner, 0x7f, sizeof(int32_t) * (size_t)fine->ne, st));
    k_rm_prol2_owner<<<rm_grid(fine->nc * nepc), block, 0, st>>>(fine->nc * nepc, nepc, fine->c2e, fine->rm_parent, owner);
    if (tri)
      k_rm_prol2_edges<3><<<rm_grid(fine->nc), block, 0, st>>>(fine->nc, coarse->cells, coarse->c2e, nv, fine->rm_parent,
                                                               fine->rm_child, fine->c2e, owner, ncomp, din, ldin,
                                                               dout + fine->nv, ldout);
    else
      k_rm_prol2_edges<4><<<rm_grid(fine->nc), block, 0, st>>>(fine->nc, coarse->cells, coarse->c2e, nv, fine->rm_parent,
                                                               fine->rm_child, fine->c2e, owner, ncomp, din, ldin,
                                                               dout + fine->nv, ldout);
  }
  PHX_HIP(hipGetLastError());
  if (loc_out != PHX_DEVICE)
    PHX_HIP(hipMemcpyAsync(out, dout, sizeof(double) * (size_t)ldout * ncomp, hipMemcpyDeviceToHost, st));
  PHX_HIP(hipStreamSynchronize(st));
  return PHX_OK;
}
