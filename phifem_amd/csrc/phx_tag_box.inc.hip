// Tag kernels for generated 3-D Kuhn boxes (included by phx_tag.hip, compiled with -ffp-contract=off).
//
// The connectivity of a generated box is a closed form of (cube, permutation) -- phx_mesh.hip, "Device generator for
// Kuhn boxes": cell c = 6 * cube + t walks o, o + e_p0, o + e_p0 + e_p1, o + e_1 + e_2 + e_3 for the t-th lexicographic
// axis permutation p.  The kernels below take one thread per CUBE, the cubes of one x row in consecutive lanes and
// (j, k) from the block index, and never read `cells`:
//   k_box_tag_cells      8 nodal values per cube (four x rows at i and i + 1) instead of 6 x (16-byte row + 4 gathers),
//                        the arithmetic of k_tag_cells per tet, the wavefront's 384 tag bytes stored as dwords;
//   k_box_mark_inside    6 tag bytes per cube -> the corners of the cube that belong to a cell tagged 1;
//   k_box_demote_count   6 tag bytes per cube -> demotion of isolated cut cells, vertices of the cells that stay cut,
//                        histogram partials, cut cells per chunk of PHX_SEL_CHUNK cells (counted by cell index: a
//                        chunk boundary falls inside a cube, 2048 = 6 * 341 + 2).
// Everything they write is what the generic kernels write, bit for bit (PHX_OPT_BOX_TAGS = 0 keeps those).
struct BoxTagGeo {
  int n0, n1, n2;      // cubes per axis
  int64_t s1, s2;      // vertex strides along y and z: n0 + 1, (n0 + 1) * (n1 + 1)
};

// corners of a cube are numbered dx + 2 dy + 4 dz; path vertex m of tet t
__device__ __forceinline__ constexpr int box_tet_corner(int t, int m) {
  constexpr int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};   // c_perm3
  return m == 0 ? 0 : (m == 1 ? (1 << P[t][0]) : (m == 2 ? ((1 << P[t][0]) | (1 << P[t][1])) : 7));
}
__device__ __forceinline__ constexpr uint32_t box_tet_corners(int t) {
  return (1u << box_tet_corner(t, 0)) | (1u << box_tet_corner(t, 1)) | (1u << box_tet_corner(t, 2)) |
         (1u << box_tet_corner(t, 3));
}
// the corners that belong to one of the tets of the 6-bit set `tm`
__device__ __forceinline__ uint32_t box_corner_mask(uint32_t tm) {
  uint32_t m = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t)
    if ((tm >> t) & 1u) m |= box_tet_corners(t);
  return m;
}
__device__ __forceinline__ int64_t box_corner_vertex(const BoxTagGeo &g, int64_t o, int b) {
  return o + (b & 1) + ((b >> 1) & 1) * g.s1 + (b >> 2) * g.s2;
}

// The second half of the body of k_tag_cells<PHX_PHI_NODAL_P1, 3, 4> for one tet, on register values (ph: phi at the
// four vertices in connectivity order, v: their ids): num / den are the sums of its first loop, `mixed` says that it
// saw samples of both signs -- then the sums are formed again with every term scaled by |det J|, as there.
__device__ __forceinline__ int box_tet_classify(const DetTab &tab, const double ph[4], const int64_t v[4],
                                                const double *__restrict__ x, double num, double den, bool mixed,
                                                bool *zero_den) {
  const double den0 = den;
  if (mixed) {
    double e[3][3];
    for (int a = 0; a < 3; ++a)
      for (int dd = 0; dd < 3; ++dd) e[a][dd] = x[v[a + 1] * 3 + dd] - x[v[0] * 3 + dd];
    const double c0 = e[1][1] * e[2][2] - e[1][2] * e[2][1];
    const double c1 = e[1][0] * e[2][2] - e[1][2] * e[2][0];
    const double c2 = e[1][0] * e[2][1] - e[1][1] * e[2][0];
    const double s = fabs((e[0][0] * c0 - e[0][1] * c1) + e[0][2] * c2);
    num = 0.0;
    den = 0.0;
    for (int q = 0; q < tab.npts; ++q) {
      const double *N = &tab.N[q * tab.nfun];
      double p = N[0] * ph[0];
      for (int i = 1; i < 4; ++i) p = p + N[i] * ph[i];
      const double t = p * s;
      num = num + t;
      den = den + fabs(t);
    }
  }
  const double d = (den > 0.0) ? num / den : 0.5;
  int t = 0;
  if (d > -1.0 && d < 1.0) t = 2;
  if (d == 1.0) t = 3;
  if (d == -1.0) t = 1;
  *zero_den = *zero_den || fabs(den0) <= 1.0e-8;
  return t;
}

// grid: (x blocks, n1, n2), up to 256 threads.  The 6 * 64 tag bytes of a wavefront are contiguous in `tags` and start
// at an even byte (6 * cube): they are staged in LDS at the same offset modulo 4 and leave as aligned dwords, with one
// 2-byte store at either end where the range does not start / end on a dword.
__global__ void __launch_bounds__(256)
k_box_tag_cells(BoxTagGeo g, DetTab tab, const double *__restrict__ phi, const double *__restrict__ x,
                int8_t *__restrict__ tags, int *__restrict__ warn) {
  __shared__ uint32_t st[4][98];   // per wave: 2 + 384 bytes, rounded up
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int j = (int)blockIdx.y, k = (int)blockIdx.z;
  const int64_t row = (int64_t)g.n0 * (j + (int64_t)g.n1 * k);   // first cube of the x row
  const int wi0 = i - lane;                                      // first cube of the wave inside the row
  const int64_t B = 6 * (row + wi0);                             // first tag byte of the wave
  const int pad = (int)(B & 3);                                  // 0 or 2
  uint16_t *st16 = reinterpret_cast<uint16_t *>(st[wv]);
  if (i < g.n0) {
    const int64_t o = i + g.s1 * j + g.s2 * k;
    double pv[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) pv[b] = phi[box_corner_vertex(g, o, b)];
    // first loop of k_tag_cells, the six tets side by side: one read of a table row serves them all, and each tet
    // still sums its own products in connectivity order and its samples in the order of the detection points
    double num[6], den[6];
    uint32_t pos = 0, neg = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) num[t] = den[t] = 0.0;
    for (int q = 0; q < tab.npts; ++q) {
      const double *N = &tab.N[q * tab.nfun];
      const double N0 = N[0], N1 = N[1], N2 = N[2], N3 = N[3];
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        double p = N0 * pv[box_tet_corner(t, 0)];
        p = p + N1 * pv[box_tet_corner(t, 1)];
        p = p + N2 * pv[box_tet_corner(t, 2)];
        p = p + N3 * pv[box_tet_corner(t, 3)];
        num[t] = num[t] + p;
        den[t] = den[t] + fabs(p);
        pos |= (uint32_t)(p > 0.0) << t;
        neg |= (uint32_t)(p < 0.0) << t;
      }
    }
    bool zero_den = false;
    uint32_t tg[6];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      const double ph[4] = {pv[box_tet_corner(t, 0)], pv[box_tet_corner(t, 1)], pv[box_tet_corner(t, 2)],
                            pv[box_tet_corner(t, 3)]};
      const int64_t v[4] = {box_corner_vertex(g, o, box_tet_corner(t, 0)), box_corner_vertex(g, o, box_tet_corner(t, 1)),
                            box_corner_vertex(g, o, box_tet_corner(t, 2)), box_corner_vertex(g, o, box_tet_corner(t, 3))};
      tg[t] = (uint32_t)box_tet_classify(tab, ph, v, x, num[t], den[t], ((pos & neg) >> t) & 1u, &zero_den);
    }
    if (zero_den) atomicOr(warn, 1);
    const int h = (pad >> 1) + 3 * lane;
    st16[h] = (uint16_t)(tg[0] | (tg[1] << 8));
    st16[h + 1] = (uint16_t)(tg[2] | (tg[3] << 8));
    st16[h + 2] = (uint16_t)(tg[4] | (tg[5] << 8));
  }
  __syncthreads();
  if (wi0 >= g.n0) return;
  const int nvalid = min(64, g.n0 - wi0);
  const int64_t A = B + pad;               // first aligned dword of the range
  const int nbytes = 6 * nvalid - pad;     // bytes from A to the end of the range (even, >= 4)
  const int nd = nbytes >> 2, first = pad >> 1;
  uint32_t *g32 = reinterpret_cast<uint32_t *>(tags);
  uint16_t *g16 = reinterpret_cast<uint16_t *>(tags);
  for (int w = lane; w < nd; w += 64) g32[(A >> 2) + w] = st[wv][first + w];
  if (lane == 0 && pad) g16[B >> 1] = st16[1];
  if (lane == 1 && (nbytes & 2)) g16[(A >> 1) + 2 * nd] = st16[2 * (first + nd)];
}

// the six tags of cube `cube` (masked), one per byte pair of three 16-bit loads
__device__ __forceinline__ void box_load_tags(const int8_t *tags, int64_t cube, int t[6]) {
  const uint16_t *t16 = reinterpret_cast<const uint16_t *>(tags) + 3 * cube;
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    const uint32_t w = t16[h];
    t[2 * h] = (int)(w & PHX_TAG_MASK);
    t[2 * h + 1] = (int)((w >> 8) & PHX_TAG_MASK);
  }
}

// touched[v] = 1 for the vertices of the cells tagged 1 (k_mark_inside_vertices; `touched` zeroed by the caller)
__global__ void __launch_bounds__(256)
k_box_mark_inside(BoxTagGeo g, const int8_t *__restrict__ tags, uint8_t *__restrict__ touched) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= g.n0) return;
  const int j = (int)blockIdx.y, k = (int)blockIdx.z;
  const int64_t cube = i + (int64_t)g.n0 * (j + (int64_t)g.n1 * k);
  int t[6];
  box_load_tags(tags, cube, t);
  uint32_t tm = 0;
#pragma unroll
  for (int s = 0; s < 6; ++s) tm |= (uint32_t)(t[s] == 1) << s;
  if (!tm) return;
  const uint32_t cm = box_corner_mask(tm);
  const int64_t o = i + g.s1 * j + g.s2 * k;
#pragma unroll
  for (int b = 0; b < 8; ++b)
    if ((cm >> b) & 1u) touched[box_corner_vertex(g, o, b)] = 1;
}

// k_demote_isolated_cut on cubes.  hist_part[bin][block] with the blocks of the 3-D grid flattened x fastest.
__global__ void __launch_bounds__(256)
k_box_demote_count(BoxTagGeo g, int8_t *__restrict__ tags, const uint8_t *__restrict__ touched,
                   uint32_t *__restrict__ hist_part, int32_t *__restrict__ sel_cut, uint8_t *__restrict__ vcut) {
  __shared__ uint32_t lh[4][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int j = (int)blockIdx.y, k = (int)blockIdx.z;
  const int64_t row = (int64_t)g.n0 * (j + (int64_t)g.n1 * k);
  const int64_t cube = row + i;
  int t[6] = {0x7f, 0x7f, 0x7f, 0x7f, 0x7f, 0x7f};
  if (i < g.n0) {
    box_load_tags(tags, cube, t);
    uint32_t tm = 0;
#pragma unroll
    for (int s = 0; s < 6; ++s) tm |= (uint32_t)(t[s] == 2) << s;
    if (tm && touched) {
      const uint32_t cm = box_corner_mask(tm);
      const int64_t o = i + g.s1 * j + g.s2 * k;
      uint32_t in = 0;
#pragma unroll
      for (int b = 0; b < 8; ++b)
        if ((cm >> b) & 1u) in |= (uint32_t)(touched[box_corner_vertex(g, o, b)] != 0) << b;
      uint32_t stay = 0;
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        if (!((tm >> s) & 1u)) continue;
        if (in & box_tet_corners(s)) stay |= box_tet_corners(s);
        else { tags[6 * cube + s] = 3; t[s] = 3; }
      }
      if (vcut) {
#pragma unroll
        for (int b = 0; b < 8; ++b)
          if ((stay >> b) & 1u) vcut[box_corner_vertex(g, o, b)] = 1;   // vertices of the cells that stay cut
      }
    }
  }
  // ---- counts (wave-uniform: every lane of the block takes part in the ballots)
  const int wi0 = i - lane;
  const int64_t wbase = 6 * (row + wi0);                                          // first cell of the wave
  const int64_t bnd = (wbase / PHX_SEL_CHUNK + 1) * (int64_t)PHX_SEL_CHUNK;       // first cell of the next chunk
  uint32_t cnt[4] = {0, 0, 0, 0}, lo = 0;
  // all 384 cells of the wave carry one tag that is not 2 (away from the interface): one ballot instead of thirty
  const int u0 = __builtin_amdgcn_readfirstlane(t[0]);
  if (u0 != 2 && u0 < 4 &&
      __all(t[0] == u0 && t[1] == u0 && t[2] == u0 && t[3] == u0 && t[4] == u0 && t[5] == u0)) {
#pragma unroll
    for (int b = 0; b < 4; ++b) cnt[b] = u0 == b ? 384u : 0u;
  } else {
#pragma unroll
    for (int s = 0; s < 6; ++s) {
#pragma unroll
      for (int b = 0; b < 4; ++b) cnt[b] += (uint32_t)__popcll(__ballot(t[s] == b));
      lo += (uint32_t)__popcll(__ballot(t[s] == 2 && 6 * cube + s < bnd));
    }
  }
  if (lane == 0) {
    if (wi0 < g.n0) {
      const int64_t chunk = wbase / PHX_SEL_CHUNK;
      if (lo) atomicAdd(&sel_cut[chunk], (int32_t)lo);
      if (cnt[2] - lo) atomicAdd(&sel_cut[chunk + 1], (int32_t)(cnt[2] - lo));   // 384 cells span two chunks at most
    }
    for (int b = 0; b < 4; ++b) lh[wv][b] = cnt[b];
  }
  __syncthreads();
  const int nw = (int)(blockDim.x >> 6);
  if (threadIdx.x < 4) {
    uint32_t a = 0;
    for (int w = 0; w < nw; ++w) a += lh[w][threadIdx.x];
    const size_t nblocks = (size_t)gridDim.x * gridDim.y * gridDim.z;
    const size_t blk = blockIdx.x + (size_t)gridDim.x * (blockIdx.y + (size_t)gridDim.y * blockIdx.z);
    hist_part[(size_t)threadIdx.x * nblocks + blk] = a;
  }
}

// The closed-form kernels serve generated 3-D boxes whose (j, k) fit the grid's y and z extents.
static bool box_tags_apply(const phx_mesh *m) {
  return m->box_tags != 0 && m->is_box && !m->is_submesh && m->gdim == 3 && m->cell_type == PHX_TETRAHEDRON &&
         m->box_n[1] <= 65535 && m->box_n[2] <= 65535;
}

static void box_tag_launch_dims(const phx_mesh *m, BoxTagGeo *g, dim3 *grid, dim3 *block) {
  g->n0 = (int)m->box_n[0]; g->n1 = (int)m->box_n[1]; g->n2 = (int)m->box_n[2];
  g->s1 = m->box_n[0] + 1;
  g->s2 = (m->box_n[0] + 1) * (m->box_n[1] + 1);
  const int threads = (int)std::min<int64_t>(256, phx_div_up(m->box_n[0], 64) * 64);
  *block = dim3((unsigned)threads);
  *grid = dim3((unsigned)phx_div_up(m->box_n[0], threads), (unsigned)m->box_n[1], (unsigned)m->box_n[2]);
}
