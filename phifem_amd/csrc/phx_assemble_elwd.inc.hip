// Weak-Dirichlet linear elasticity, mixed (u, p) in P1^d x P1^d on affine triangles / tetrahedra: included by
// phx_assemble.hip.  The vector analogue of the weak-Dirichlet Poisson scheme above (reference
// demo/weak-dirichlet/flower/main.py:112-135 bilinear form, :142-151 linear form) with the material law of the interface
// demo (data.py:5-36); restated in numpy in tests/elasticity_wd_ref.py:
//   a((u,p),(v,q)) =  int_{dx(1,2)} sigma(u) : eps(v)  -  int_{ds} (sigma(u) n) . v
//                   + pen h^-2 int_{dx(2)} (u - h^-1 phi_h p) . (v - h^-1 phi_h q)
//                   + stab avg(h) int_{dS(2,3)} [sigma(u) n] . [sigma(v) n]
//   L(v,q)         =  int_{dx(1,2)} f_h . v  +  pen h^-2 int_{dx(2)} u_D . (v - h^-1 phi_h q)
// The cell stabilisation stab h^2 (div sigma(u), div sigma(v)) and its right-hand-side partner vanish identically for P1
// (div sigma of a P1 field is zero), as main.py:123-128,150 do for the scalar form.  Every integrand is a polynomial on
// an affine simplex: the closed forms are exact.  The coefficients are not rescaled by E.
// DoF layout: component-major blocks of nv entries, u_a -> a, p_a -> d + a; active: u_a on the vertices of cells tagged
// 1 / 2, p_a on the vertices of cells tagged 2.
//
// Kernel layout: ONE WAVEFRONT per cell / boundary entity / facet (four per 256-thread block), lanes over the entries
// of the element tensor.  The element index is wave-uniform (readfirstlane), so connectivity and coordinates come in
// through scalar loads and the geometry is evaluated once per wavefront; lane 0 leaves it in a per-wave LDS record that
// the lanes index by their (vertex, component) -- no register array is indexed by a lane-dependent value.  The tensors
// are small ((N d)^2 = 36 / 144 for bulk and boundary, d (2N)^2 = 72 / 192 for a cut cell, ((N + 1) d)^2 = 64 / 225 for
// the D + 2 distinct vertices of a facet pair): a 256-thread block per element, as the interface assembler spends,
// would leave three of its four wavefronts without an entry in 2-D and evaluate the geometry four times.

struct ElwdArgs {
  const int32_t *cells;
  const double *x;
  const int32_t *c2f, *f2c;
  const int32_t *dofmap;   // [2 d nv] full DoF -> active row or -1
  const double *phi;       // [nv]
  const double *f;         // [d*nv] component-major
  const double *ud;        // [d*nv]
  double lam, mu, gamma, sigma;
  int32_t nv;
  double *rhs;
  Slots slots;
};

#define ELWD_WAVES 4   // wavefronts (elements) per block

// what lane 0 of a wavefront leaves for the others
template <int D>
struct ElwdCell {
  Geo<D> G;
  int32_t v[D + 1];
  double ph[D + 1];
  double nrm[D];       // outward unit normal of the facet under work
};

__device__ __forceinline__ void elwd_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// wave-uniform element index of this wavefront
__device__ __forceinline__ int64_t elwd_element() {
  return blockIdx.x * (int64_t)ELWD_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

template <int D>
__device__ __forceinline__ void elwd_stage_cell(const ElwdArgs &A, int64_t c, int lane, ElwdCell<D> &L, const double *phi) {
  int32_t v[D + 1];
  double X[D + 1][D];
  load_cell<D>(A.cells, A.x, c, v, X);
  Geo<D> G;
  simplex_geometry<D>(X, G);
  if (lane == 0) {
    L.G = G;
    for (int i = 0; i <= D; ++i) { L.v[i] = v[i]; L.ph[i] = phi ? phi[v[i]] : 0.0; }
  }
}

template <int D>
__global__ void k_elwd_mark_active(int64_t nc, int64_t nv, const int32_t *__restrict__ cells, const int8_t *__restrict__ ctags,
                                   uint8_t *__restrict__ flags) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int t = ctags[c] & PHX_TAG_MASK;
  if (t != 1 && t != 2) return;
  for (int i = 0; i <= D; ++i) {
    const int64_t v = cells[c * (D + 1) + i];
    for (int a = 0; a < D; ++a) {
      flags[(int64_t)a * nv + v] = 1;
      if (t == 2) flags[(int64_t)(D + a) * nv + v] = 1;
    }
  }
}

// --- sigma(u) : eps(v) and f_h . v over the cells of Omega_h ------------------------------------
template <int D>
__global__ void __launch_bounds__(64 * ELWD_WAVES) k_elwd_bulk(int64_t nlist, const int32_t *__restrict__ list, ElwdArgs A) {
  constexpr int N = D + 1, M = N * D;
  constexpr double c2 = D == 3 ? 1.0 / 20.0 : 1.0 / 12.0;
  __shared__ ElwdCell<D> cell[ELWD_WAVES];
  const int64_t e = elwd_element();
  if (e >= nlist) return;   // wave-uniform; only wave-level synchronisation below
  const int lane = threadIdx.x & 63;
  ElwdCell<D> &L = cell[threadIdx.x >> 6];
  elwd_stage_cell<D>(A, list[e], lane, L, nullptr);
  elwd_wave_sync();
  const double vol = L.G.vol;
  for (int idx = lane; idx < M * M; idx += 64) {
    const int r = idx / M, s = idx % M;
    const int a = r / N, i = r % N, cc = s / N, j = s % N;
    // eps(N_i e_a) : sigma(N_j e_c) = sigma(N_j e_c)[a][:] . g_i
    double k = 0.0;
    for (int q = 0; q < D; ++q) k += sig_pq<D>(L.G, A.lam, A.mu, j, cc, a, q) * L.G.g[i][q];
    slot_add(A.slots, A.dofmap[(int64_t)a * A.nv + L.v[i]], cc * A.nv + L.v[j], k * vol);
  }
  if (lane < M) {
    const int a = lane / N, i = lane % N;
    double sf = 0.0;
    for (int q = 0; q < N; ++q) sf += A.f[(int64_t)a * A.nv + L.v[q]];
    slot_rhs_add(A.slots, A.rhs, A.dofmap[(int64_t)a * A.nv + L.v[i]], vol * c2 * (sf + A.f[(int64_t)a * A.nv + L.v[i]]));
  }
}

// --- one-sided boundary term -(sigma(u) n) . v over the (cell, local facet) entities of ds.  With n = -g_lf / |g_lf|,
// |F| = D |K| |g_lf| and int_F N_i = |F| / D (i on F) the entry of row (a, i != lf), column (c, j) is
// |K| sigma(N_j e_c)[a][:] . g_lf. ---------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(64 * ELWD_WAVES) k_elwd_ds(int64_t nent, const int64_t *__restrict__ ent_packed,
                                                              const int32_t *__restrict__ ent_pairs, ElwdArgs A) {
  constexpr int N = D + 1, M = N * D;
  __shared__ ElwdCell<D> cell[ELWD_WAVES];
  const int64_t e = elwd_element();
  if (e >= nent) return;
  const int lane = threadIdx.x & 63;
  ElwdCell<D> &L = cell[threadIdx.x >> 6];
  int64_t c;
  int lf;
  if (ent_packed) { c = ent_packed[2 * e + 1] >> 8; lf = (int)(ent_packed[2 * e + 1] & 0xff); }
  else { c = ent_pairs[2 * e]; lf = ent_pairs[2 * e + 1]; }
  elwd_stage_cell<D>(A, c, lane, L, nullptr);
  elwd_wave_sync();
  const double vol = L.G.vol;
  for (int idx = lane; idx < M * M; idx += 64) {
    const int r = idx / M, s = idx % M;
    const int a = r / N, i = r % N, cc = s / N, j = s % N;
    if (i == lf) continue;
    double k = 0.0;
    for (int q = 0; q < D; ++q) k += sig_pq<D>(L.G, A.lam, A.mu, j, cc, a, q) * L.G.g[lf][q];
    slot_add(A.slots, A.dofmap[(int64_t)a * A.nv + L.v[i]], cc * A.nv + L.v[j], k * vol);
  }
}

// --- penalisation on the cut cells: the scalar (u, p) x (u, p) blocks of k_assemble_cut, once per component a; lane =
// (a, r, s) with r, s = i (u_a at vertex i) or N + i (p_a at vertex i) -----------------------------
template <int D>
__global__ void __launch_bounds__(64 * ELWD_WAVES) k_elwd_cut(int64_t nlist, const int32_t *__restrict__ list, ElwdArgs A) {
  constexpr int N = D + 1, M = 2 * N;
  constexpr double c2 = D == 3 ? 1.0 / 20.0 : 1.0 / 12.0;    // (1 + d_ij) c2 = int N_i N_j / |K|
  constexpr double c3 = D == 3 ? 1.0 / 120.0 : 1.0 / 60.0;   // alpha! c3
  constexpr double c4 = D == 3 ? 1.0 / 840.0 : 1.0 / 360.0;  // alpha! c4
  __shared__ ElwdCell<D> cell[ELWD_WAVES];
  const int64_t e = elwd_element();
  if (e >= nlist) return;
  const int lane = threadIdx.x & 63;
  ElwdCell<D> &L = cell[threadIdx.x >> 6];
  elwd_stage_cell<D>(A, list[e], lane, L, A.phi);
  elwd_wave_sync();
  double sp = 0.0;
  for (int q = 0; q < N; ++q) sp += L.ph[q];
  const double h1 = 1.0 / L.G.h, gam = A.gamma * L.G.vol;
  for (int idx = lane; idx < D * M * M; idx += 64) {
    const int a = idx / (M * M), r = (idx / M) % M, s = idx % M;
    const int i = r % N, j = s % N;
    const bool rp = r >= N, cp = s >= N;
    const double d2 = i == j ? 2.0 : 1.0;
    double val;
    if (!rp && !cp) {
      val = gam * h1 * h1 * c2 * d2;
    } else if (rp != cp) {
      val = -gam * h1 * h1 * h1 * c3 * d2 * (sp + L.ph[i] + L.ph[j]);   // int N_i N_j phi_h = |K| c3 (1 + d_ij)(S + phi_i + phi_j)
    } else {
      double m4 = 0.0;
      for (int k = 0; k < N; ++k)
        for (int l = 0; l < N; ++l) m4 += mult4(i, j, k, l) * L.ph[k] * L.ph[l];
      val = gam * h1 * h1 * h1 * h1 * c4 * m4;
    }
    slot_add(A.slots, A.dofmap[(int64_t)(rp ? D + a : a) * A.nv + L.v[i]], (cp ? D + a : a) * A.nv + L.v[j], val);
  }
  if (lane < D * M) {
    const int a = lane / M, r = lane % M, i = r % N;
    const bool rp = r >= N;
    double ud[N], sud = 0.0;
    for (int q = 0; q < N; ++q) { ud[q] = A.ud[(int64_t)a * A.nv + L.v[q]]; sud += ud[q]; }
    double val;
    if (!rp) {
      val = gam * h1 * h1 * c2 * (sud + A.ud[(int64_t)a * A.nv + L.v[i]]);
    } else {
      double bq = 0.0;
      for (int q = 0; q < N; ++q) bq += ud[q] * (i == q ? 2.0 : 1.0) * (sp + L.ph[i] + L.ph[q]);
      val = -gam * h1 * h1 * h1 * c3 * bq;
    }
    slot_rhs_add(A.slots, A.rhs, A.dofmap[(int64_t)(rp ? D + a : a) * A.nv + L.v[i]], val);
  }
}

// --- stress-jump term stab avg(h) int_F [sigma(u) n] . [sigma(v) n] over the ghost facets.  sigma is constant per
// cell, so the integrand is; with the outward normal of each cell the jump is sigma+ n+ + sigma- n-.  The two cells
// share the D vertices of F: the macro-element has D + 2 distinct vertices (those of the first cell, then the vertex of
// the second cell opposite F) and the traction coefficient of a shared vertex is the sum of its two one-sided ones --
// ((D + 2) D)^2 = 64 / 225 slot updates per facet, not (2 N D)^2 = 144 / 576.  Lanes m * D + a < (D + 2) D first leave
// the traction vector of (macro vertex m, component a) in LDS; an entry is the product of two of them. -------------
template <int D>
__global__ void __launch_bounds__(64 * ELWD_WAVES) k_elwd_facets(int64_t nlist, const int32_t *__restrict__ list, ElwdArgs A) {
  constexpr int N = D + 1, MV = N + 1, M = MV * D;
  __shared__ ElwdCell<D> cell[ELWD_WAVES][2];
  __shared__ int32_t macro_of[ELWD_WAVES][2][N];   // macro vertex of local vertex i of side s
  __shared__ int32_t vd_all[ELWD_WAVES][MV];
  __shared__ double tr_all[ELWD_WAVES][M][D];
  const int64_t e = elwd_element();
  if (e >= nlist) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t f = list[e];
  double hsum = 0.0, area = 0.0;
  int32_t vs[2][N];
  int lfm = 0;
  for (int sd = 0; sd < 2; ++sd) {
    const int64_t c = A.f2c[2 * f + sd];
    double X[N][D];
    load_cell<D>(A.cells, A.x, c, vs[sd], X);
    Geo<D> G;
    simplex_geometry<D>(X, G);
    int lf = 0;
    for (int k = 0; k < N; ++k)
      if (A.c2f[c * N + k] == (int32_t)f) lf = k;
    if (sd == 1) lfm = lf;
    double gl[D], gn = 0.0;
    for (int dd = 0; dd < D; ++dd) {
      gl[dd] = 0.0;
      for (int k = 0; k < N; ++k) gl[dd] = k == lf ? G.g[k][dd] : gl[dd];   // G.g[lf] without dynamic indexing
      gn += gl[dd] * gl[dd];
    }
    gn = sqrt(gn);
    if (sd == 0) area = D * G.vol * gn;
    hsum += G.h;
    if (lane == 0) {
      cell[w][sd].G = G;
      for (int dd = 0; dd < D; ++dd) cell[w][sd].nrm[dd] = -gl[dd] / gn;
    }
  }
  if (lane == 0) {
    for (int i = 0; i < N; ++i) { macro_of[w][0][i] = i; vd_all[w][i] = vs[0][i]; }
    for (int j = 0; j < N; ++j) {
      int mj = N;   // the vertex opposite F
      for (int q = 0; q < N; ++q)
        if (j != lfm && vs[0][q] == vs[1][j]) mj = q;
      macro_of[w][1][j] = mj;
      if (j == lfm) vd_all[w][N] = vs[1][j];
    }
  }
  elwd_wave_sync();
  if (lane < M) {
    const int m = lane / D, a = lane % D;
    double t[D];
    for (int p = 0; p < D; ++p) t[p] = 0.0;
    for (int sd = 0; sd < 2; ++sd)
      for (int i = 0; i < N; ++i) {
        if (macro_of[w][sd][i] != m) continue;
        for (int p = 0; p < D; ++p)
          for (int q = 0; q < D; ++q) t[p] += sig_pq<D>(cell[w][sd].G, A.lam, A.mu, i, a, p, q) * cell[w][sd].nrm[q];
      }
    for (int p = 0; p < D; ++p) tr_all[w][lane][p] = t[p];
  }
  elwd_wave_sync();
  const double wgt = A.sigma * 0.5 * hsum * area;
  for (int idx = lane; idx < M * M; idx += 64) {
    const int r = idx / M, s = idx % M;
    double acc = 0.0;
    for (int p = 0; p < D; ++p) acc += tr_all[w][r][p] * tr_all[w][s][p];
    slot_add(A.slots, A.dofmap[(int64_t)(r % D) * A.nv + vd_all[w][r / D]], (s % D) * A.nv + vd_all[w][s / D], wgt * acc);
  }
}

// Slot capacities (k_el_row_caps), two classes per row.  Rows of DoFs at the vertices of the cut cells and of the two
// cells of every ghost facet -- the u rows with penalty or stress-jump columns, and every p row -- get the capacity W
// under trial: by the numpy specification the longest of them holds 26 entries in 2-D and 83-88 in 3-D (5^3 .. 13^3
// boxes).  Every other row of a generated box holds stiffness and boundary-term columns only, all inside the Kuhn star
// of its vertex: at most 7 x 2 = 14 / 15 x 3 = 45 entries, in 64 slots.  (Left with the cut-cell vertices alone, the
// rows of the inside vertices of a jump facet reach 63 entries at 6^3: too close to 64 to rely on.)  On any other mesh
// the valence is not bounded and every row gets W.
static int assemble_elwd_with_capacity(phx_mesh *m, const double *params, const double *dphi, const double *df,
                                       const double *dud, int W, phx_system **out) {
  const int D = m->gdim;
  const int64_t nent = 2 * (int64_t)D * m->nv;
  PHX_REQUIRE(nent < INT32_MAX, PHX_ERR_VALUE, "too many DoFs for 32-bit column keys");
  SystemBuild sys(m, nent, nent, W);
  DevTemps tmp(m->stream);
  phx_system *s = sys.s;
  Slots &sl = sys.sl;
  s->el_nblk = 2 * D;     // phx_solve: vertex-block Jacobi over the (u, p) DoFs of a vertex
  s->cc_layout = phx_system::PHX_CC_LAYOUT_ELWD;   // coarse functions on the d blocks u_a (phx_coarse.inc.hip)
  s->cc_tried = m->elwd_coarse == 0;               // PHX_OPT_ELWD_COARSE off while assembling: vertex blocks only, for good
  const dim3 block(256);
  ElwdArgs A;
  memset(&A, 0, sizeof(A));
  A.cells = m->cells; A.x = m->x; A.c2f = m->c2f; A.f2c = m->f2c;
  A.phi = dphi; A.f = df; A.ud = dud; A.nv = (int32_t)m->nv;
  // params = {E, nu, pen_coef, stab_coef}; material law data.py:5-10
  A.lam = params[0] * params[1] / (1.0 + params[1]) / (1.0 - 2.0 * params[1]);
  A.mu = params[0] / 2.0 / (1.0 + params[1]);
  A.gamma = params[2]; A.sigma = params[3];
  // ---- active numbering
  {
    DevTemps numbering(m->stream);
    uint8_t *flags = nullptr;
    PHX_HIP(numbering.alloc(&flags, (size_t)nent));
    PHX_HIP(hipMemsetAsync(flags, 0, (size_t)nent, m->stream));
    const dim3 gcells((unsigned)phx_div_up(m->nc, 256));
    if (D == 2) k_elwd_mark_active<2><<<gcells, block, 0, m->stream>>>(m->nc, m->nv, m->cells, m->cell_tags, flags);
    else k_elwd_mark_active<3><<<gcells, block, 0, m->stream>>>(m->nc, m->nv, m->cells, m->cell_tags, flags);
    PHX_CHECK(number_single_block(m, s, numbering, flags, nent, "no active DoF: no cell is tagged 1 or 2"));
  }
  const int32_t n = (int32_t)s->n;
  A.dofmap = s->dof_of_vertex_u;
  // ---- work lists
  int32_t *l_om = nullptr, *l_cut = nullptr, *l_fac = nullptr;
  int64_t n_om = 0, n_cut = 0, n_fac = 0;
  PHX_CHECK(build_list(m, m->nc, SelOmega{m->cell_tags}, &l_om, &n_om));
  tmp.adopt(l_om);
  PHX_CHECK(build_list(m, m->nc, SelCut{m->cell_tags}, &l_cut, &n_cut));
  tmp.adopt(l_cut);
  PHX_CHECK(build_list(m, m->nf, SelGhostFacet{m->facet_tags, m->f2c}, &l_fac, &n_fac));
  tmp.adopt(l_fac);
  DsEntities ds;
  PHX_CHECK(ds_entities(m, &ds));
  // ---- slots: two capacity classes per row
  int64_t total_slots = 0;
  {
    DevTemps caps(m->stream);
    uint8_t *cutv = nullptr;
    int64_t *cap = nullptr;
    PHX_HIP(caps.alloc(&cutv, (size_t)m->nv));
    const bool bulk64 = m->is_box && !m->is_submesh;
    PHX_HIP(hipMemsetAsync(cutv, bulk64 ? 0 : 1, (size_t)m->nv, m->stream));
    if (bulk64 && n_cut > 0) {
      const dim3 g((unsigned)phx_div_up(n_cut, 256));
      if (D == 2) k_mark_cells<3><<<g, block, 0, m->stream>>>(n_cut, l_cut, m->cells, cutv);
      else k_mark_cells<4><<<g, block, 0, m->stream>>>(n_cut, l_cut, m->cells, cutv);
    }
    if (bulk64 && n_fac > 0) {
      const dim3 g((unsigned)phx_div_up(n_fac, 256));
      if (D == 2) k_mark_facet_cells<3><<<g, block, 0, m->stream>>>(n_fac, l_fac, m->f2c, m->cells, cutv);
      else k_mark_facet_cells<4><<<g, block, 0, m->stream>>>(n_fac, l_fac, m->f2c, m->cells, cutv);
    }
    int wbig = 0;
    while ((1 << wbig) < W) ++wbig;
    uint8_t *wlog = nullptr;   // the slot table owns wlog and off (free_slots)
    int64_t *off = nullptr;
    PHX_HIP(phx_malloc(&wlog, (size_t)n));
    sl.wlog = wlog;
    PHX_HIP(caps.alloc(&cap, sizeof(int64_t) * (size_t)(n + 1)));
    PHX_HIP(phx_malloc(&off, sizeof(int64_t) * (size_t)(n + 1)));
    sl.off = off;
    k_el_row_caps<<<dim3((unsigned)phx_div_up((int64_t)n + 1, 256)), block, 0, m->stream>>>(
        n, s->full_of_active, m->nv, cutv, wbig, wlog, cap);
    PHX_CHECK(exclusive_sum<int64_t>(m, cap, off, (int64_t)n + 1));
    PHX_HIP(hipMemcpy(&total_slots, off + n, sizeof(int64_t), hipMemcpyDeviceToHost));
  }
  PHX_CHECK(slots_alloc(m, total_slots, W, &sl));
  PHX_CHECK(rhs_alloc(m, s));
  A.rhs = s->rhs;
  PHX_REQUIRE_GRID(phx_div_up(n_om, ELWD_WAVES) * 256, "elasticity bulk assembly");
  PHX_REQUIRE_GRID(phx_div_up(n_fac, ELWD_WAVES) * 256, "elasticity facet assembly");
  // PHX_OPT_DETERMINISTIC: every kernel that adds into the slots or the right-hand side runs twice (Slots)
  bool det = false;
  PHX_CHECK(det_alloc(m, sl, total_slots, n, &det));
  const auto grid = [](int64_t nelem) { return dim3((unsigned)phx_div_up(nelem, ELWD_WAVES)); };
  for (int pass = det ? 1 : 0; pass <= (det ? 2 : 0); ++pass) {
    sl.pass = pass;
    A.slots = sl;
    if (D == 2) {
      if (n_om) k_elwd_bulk<2><<<grid(n_om), block, 0, m->stream>>>(n_om, l_om, A);
      if (ds.n) k_elwd_ds<2><<<grid(ds.n), block, 0, m->stream>>>(ds.n, ds.packed, ds.pairs, A);
      if (n_cut) k_elwd_cut<2><<<grid(n_cut), block, 0, m->stream>>>(n_cut, l_cut, A);
      if (n_fac) k_elwd_facets<2><<<grid(n_fac), block, 0, m->stream>>>(n_fac, l_fac, A);
    } else {
      if (n_om) k_elwd_bulk<3><<<grid(n_om), block, 0, m->stream>>>(n_om, l_om, A);
      if (ds.n) k_elwd_ds<3><<<grid(ds.n), block, 0, m->stream>>>(ds.n, ds.packed, ds.pairs, A);
      if (n_cut) k_elwd_cut<3><<<grid(n_cut), block, 0, m->stream>>>(n_cut, l_cut, A);
      if (n_fac) k_elwd_facets<3><<<grid(n_fac), block, 0, m->stream>>>(n_fac, l_fac, A);
    }
    PHX_HIP(hipGetLastError());
  }
  PHX_CHECK(det_finish(m, sl, total_slots, n, s->rhs));
  return sys.finish((int32_t)nent, out);
}

extern "C" int phx_assemble_elasticity_wd(phx_mesh *m, const double *params, const double *phi_h, const double *f_h,
                                          const double *u_D, int loc, phx_system **out) {
  PHX_HIP(hipSetDevice(m->device));
  PHX_REQUIRE(m->cell_type == PHX_TRIANGLE || m->cell_type == PHX_TETRAHEDRON, PHX_ERR_NOT_IMPLEMENTED,
              "weak-Dirichlet elasticity is assembled on triangles and tetrahedra only");
  bool slab = m->facet_exempt != nullptr || m->slab_cut;
  for (int a = 0; a < m->gdim; ++a) slab = slab || (m->box_nglob[a] > 0 && m->box_nglob[a] != m->box_n[a]);
  PHX_REQUIRE(!slab, PHX_ERR_NOT_IMPLEMENTED, "weak-Dirichlet elasticity: slabs and partitioned ranks are not served");
  PHX_REQUIRE(params != nullptr, PHX_ERR_VALUE, "NULL params");
  PHX_REQUIRE(m->have_cell_tags && m->have_facet_tags, PHX_ERR_VALUE,
              "cell and facet tags must be computed before assembly");
  const int D = m->gdim;
  DevTemps staged(m->stream);
  const double *dphi, *df, *dud;
  PHX_CHECK(to_device(m, phi_h, loc, m->nv, &dphi, staged));
  PHX_CHECK(to_device(m, f_h, loc, (int64_t)D * m->nv, &df, staged));
  PHX_CHECK(to_device(m, u_D, loc, (int64_t)D * m->nv, &dud, staged));
  PHX_CHECK(phx_begin_timing(m));
  const auto run = [&](int W) { return assemble_elwd_with_capacity(m, params, dphi, df, dud, W, out); };
  // W: capacity of the rows of cut-cell vertices on a generated box, of every row elsewhere.  The first one holds every
  // row of a mesh with the connectivity of a Kuhn lattice; the later ones are for caller-supplied meshes with vertices
  // of high valence.  Behind the last one the assembly is refused (PHX_ERR_CAPACITY).
  int rc = D == 3 ? retry_capacity({128, 256, 512}, run) : retry_capacity({64, 128, 256}, run);
  if (rc == PHX_OK) rc = phx_end_timing(m, 2);
  return rc;
}
