// Reaction term of the P1 x P1 weak-Dirichlet scheme (include of phx_assemble.hip): c u - Lap u = f + c g, one implicit
// step of the heat equation.
//   a = a_Poisson + c (u, v)_{dx(1,2)} + stab c^2 h_T^2 (u, v)_{dx(2)}
//   L = L_Poisson(f + c g; u_D) + stab c h_T^2 (f + c g, v)_{dx(2)}
// The Poisson element kernels of phx_assemble.hip run as they are (the generic ones: vertex rows over v2c, cut cells,
// boundary term, ghost penalty), the mass terms are one more element kernel of the pass, and the right-hand side comes
// from the gather kernel that phx_system_update_rhs runs per time step.  tests/heat_ref.py restates both in numpy.
//
// The rest of this translation unit is compiled without FMA contraction.
#pragma clang fp contract(off)

// mass terms: 16 lanes per cell of Omega_h, lane = (i, j) of the element tensor w |T| (1 + d_ij) / ((d+1)(d+2)),
// w = c on cells tagged 1 and c (1 + stab c h_T^2) on cut cells
template <int D>
__global__ void __launch_bounds__(256) k_react_mass(int64_t nlist, const int32_t *__restrict__ list, AsmArgs A, double c) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t e = gid >> 4;
  if (e >= nlist) return;
  constexpr int N = D + 1;
  const int i = (int)(gid & 15) >> 2, j = (int)(gid & 3);
  if (i >= N || j >= N) return;
  const int64_t cell = list[e];
  int32_t v[N];
  double X[N][D];
  load_cell<D>(A.cells, A.x, cell, v, X);
  Geo<D> G;
  simplex_geometry<D>(X, G);
  constexpr double c2 = D == 3 ? 1.0 / 20.0 : 1.0 / 12.0;
  double w = c;
  if ((A.ctags[cell] & PHX_TAG_MASK) == 2) w = c * (1.0 + A.sigma * c * (G.h * G.h));
  slot_add(A.slots, A.du[v[i]], v[j], w * G.vol * c2 * (i == j ? 2.0 : 1.0));
}

struct ReactRhsArgs {
  int64_t nu;
  const int64_t *full_of_active;
  const int32_t *dp;
  const int64_t *v2c_ptr;
  const int32_t *v2c_idx;
  const int32_t *cells;
  const double *x;
  const int8_t *ctags;
  const double *phi, *f, *g, *ud;   // g may be null
  double c, gamma, sigma;
  double *rhs;
};

// The linear form as a gather: one lane per active vertex walks its star in v2c order and evaluates its u row and its p
// row from the closed forms (mass matrix; third-order barycentric tensor for the phi u_D term).  Every row has one
// writer and one order of additions: the same data give the same bytes.
template <int D>
__global__ void __launch_bounds__(256) k_react_rhs(ReactRhsArgs R) {
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
      const double mF = G.vol * c2 * (sF + F[i]);   // int (f + c g) N_i
      if (t == 1) { ru += mF; continue; }
      ru += mF * (1.0 + R.sigma * R.c * (G.h * G.h));
      double ph[N], ud[N], sp = 0.0, sud = 0.0;
      for (int q = 0; q < N; ++q) { ph[q] = R.phi[v[q]]; ud[q] = R.ud[v[q]]; sp += ph[q]; sud += ud[q]; }
      const double h1 = 1.0 / G.h, gam = R.gamma * G.vol;
      ru += gam * h1 * h1 * c2 * (sud + ud[i]);
      double bq = 0.0;
      for (int q = 0; q < N; ++q) bq += ud[q] * (i == q ? 2.0 : 1.0) * (sp + ph[i] + ph[q]);
      rp += -gam * h1 * h1 * h1 * c3 * bq;
    }
    R.rhs[a] = ru;
    if (prow >= 0) R.rhs[prow] = rp;
  }
}

static int react_update_rhs(phx_system *s, const double *dphi, const double *df, const double *dg, const double *dud) {
  phx_mesh *m = s->mesh;
  PHX_CHECK(build_v2c(m));
  if (s->n == 0) return PHX_OK;
  ReactRhsArgs R{s->nu, s->full_of_active, s->dof_of_vertex_p, m->v2c_ptr, m->v2c_idx, m->cells, m->x, m->cell_tags,
                 dphi, df, dg, dud, s->react_c, s->react_pen, s->react_stab, s->rhs};
  const dim3 grid((unsigned)std::min<int64_t>(phx_div_up(std::max<int64_t>(s->nu, 1), 256), 1 << 16));
  if (m->gdim == 2) k_react_rhs<2><<<grid, dim3(256), 0, m->stream>>>(R);
  else k_react_rhs<3><<<grid, dim3(256), 0, m->stream>>>(R);
  PHX_HIP(hipGetLastError());
  return PHX_OK;
}

// systems with a conductivity (phx_assemble_diff.inc.hip, included after this file)
static int diff_update_rhs(phx_system *s, const double *dphi, const double *df, const double *dg, const double *dud);
// systems with a conductivity and a velocity (phx_assemble_cd.inc.hip)
static int cd_update_rhs(phx_system *s, const double *dphi, const double *df, const double *dg, const double *dud);

extern "C" int phx_system_update_rhs(phx_system *s, const double *phi_h, const double *f_h, const double *g_h,
                                     const double *u_D, int loc) {
  PHX_REQUIRE(s != nullptr && s->react, PHX_ERR_VALUE,
              "phx_system_update_rhs: the system was not built by phx_assemble_reaction_wd, phx_assemble_diffusion_wd or "
              "phx_assemble_convection_wd");
  phx_mesh *m = s->mesh;
  PHX_HIP(hipSetDevice(m->device));
  PHX_REQUIRE(m->have_cell_tags, PHX_ERR_VALUE, "cell tags must be computed before the right-hand side");
  DevTemps staged(m->stream);
  const double *dphi, *df, *dud, *dg = nullptr;
  PHX_CHECK(to_device(m, phi_h, loc, m->nv, &dphi, staged));
  PHX_CHECK(to_device(m, f_h, loc, m->nv, &df, staged));
  if (g_h) PHX_CHECK(to_device(m, g_h, loc, m->nv, &dg, staged));
  PHX_CHECK(to_device(m, u_D, loc, m->nv, &dud, staged));
  PHX_CHECK(s->cd_beta      ? cd_update_rhs(s, dphi, df, dg, dud)
            : s->diff_kappa ? diff_update_rhs(s, dphi, df, dg, dud)
                            : react_update_rhs(s, dphi, df, dg, dud));
  PHX_HIP(hipStreamSynchronize(m->stream));   // the caller may overwrite its arrays when this returns
  return PHX_OK;
}

// the element kernels of one pass, in stream order: vertex rows (first: they own their rows on the cleared slots), cut
// cells, boundary term, ghost penalty -- the generic kernels of phx_assemble.hip on every mesh -- and the mass terms
static int react_launch_pass(phx_mesh *m, const AsmArgs &A, const P1Work &w, const int32_t *l_om, int64_t n_om, double c) {
  const int D = m->gdim;
  const dim3 block(256);
  {
    const dim3 g((unsigned)phx_div_up(m->nv, ROW_THREADS)), b(ROW_THREADS);
    if (D == 2) k_assemble_rows<2><<<g, b, 0, m->stream>>>(m->nv, m->v2c_ptr, m->v2c_idx, A);
    else k_assemble_rows<3><<<g, b, 0, m->stream>>>(m->nv, m->v2c_ptr, m->v2c_idx, A);
  }
  if (w.n_cut > 0) {
    PHX_REQUIRE_GRID(w.n_cut * 64, "cut-cell assembly");
    const dim3 g((unsigned)phx_div_up(w.n_cut * 64, 256));
    if (D == 2) k_assemble_cut<2><<<g, block, 0, m->stream>>>(w.n_cut, w.l_cut, A);
    else k_assemble_cut<3><<<g, block, 0, m->stream>>>(w.n_cut, w.l_cut, A);
  }
  PHX_HIP(hipGetLastError());
  DsEntities ds;
  PHX_CHECK(ds_entities(m, &ds));
  if (ds.n > 0) {
    const dim3 g((unsigned)phx_div_up(ds.n * 16, 256));
    if (D == 2) k_assemble_ds<2><<<g, block, 0, m->stream>>>(ds.n, ds.packed, ds.pairs, A);
    else k_assemble_ds<3><<<g, block, 0, m->stream>>>(ds.n, ds.packed, ds.pairs, A);
  }
  if (w.n_fac > 0) {
    const dim3 g((unsigned)phx_div_up(w.n_fac, 256));
    if (D == 2) k_assemble_facets<2><<<g, block, 0, m->stream>>>(w.n_fac, w.l_fac, A);
    else k_assemble_facets<3><<<g, block, 0, m->stream>>>(w.n_fac, w.l_fac, A);
  }
  if (n_om > 0) {
    PHX_REQUIRE_GRID(n_om * 16, "mass-term assembly");
    const dim3 g((unsigned)phx_div_up(n_om * 16, 256));
    if (D == 2) k_react_mass<2><<<g, block, 0, m->stream>>>(n_om, l_om, A, c);
    else k_react_mass<3><<<g, block, 0, m->stream>>>(n_om, l_om, A, c);
  }
  PHX_HIP(hipGetLastError());
  return PHX_OK;
}

static int assemble_react_with_capacity(phx_mesh *m, double pen_coef, double stab_coef, double c, const double *dphi,
                                        const double *df, const double *dg, const double *dud, int W, phx_system **out) {
  SystemBuild sys(m, m->nv, 2 * m->nv, W);
  phx_system *s = sys.s;
  s->u_vertex_block = true;
  s->react = true;
  s->react_c = c; s->react_pen = pen_coef; s->react_stab = stab_coef;
  AsmArgs A;
  A.cells = m->cells; A.x = m->x; A.ctags = m->cell_tags; A.ftags = m->facet_tags;
  A.c2f = m->c2f; A.f2c = m->f2c;
  A.phi = dphi; A.f = df; A.ud = dud; A.gamma = pen_coef; A.sigma = stab_coef;
  A.nv = (int32_t)m->nv;
  {
    DevTemps tmp(m->stream);
    PHX_CHECK(p1_number(m, s, tmp));
    PHX_REQUIRE(s->n > 0, PHX_ERR_VALUE, "no active DoF: no cell is tagged 1 or 2");
    P1Work w;
    PHX_CHECK(p1_work_lists(m, tmp, w));
    int32_t *l_om = nullptr;
    int64_t n_om = 0;
    PHX_CHECK(build_list(m, m->nc, SelOmega{m->cell_tags}, &l_om, &n_om));
    tmp.adopt(l_om);
    PHX_CHECK(rhs_alloc(m, s));
    A.du = s->dof_of_vertex_u; A.dp = s->dof_of_vertex_p; A.rhs = s->rhs;
    const int64_t nslots = s->n * W;
    PHX_CHECK(slots_alloc(m, nslots, W, &sys.sl));
    bool det = false;
    PHX_CHECK(det_alloc(m, sys.sl, nslots, s->n, &det));
    for (int pass = det ? 1 : 0; pass <= (det ? 2 : 0); ++pass) {
      sys.sl.pass = pass;
      A.slots = sys.sl;
      PHX_CHECK(react_launch_pass(m, A, w, l_om, n_om, c));
    }
    PHX_CHECK(det_finish(m, sys.sl, nslots, s->n, s->rhs));
    // the right-hand side the Poisson kernels left is replaced by the gather's: a refresh with the same data is a no-op
    PHX_CHECK(react_update_rhs(s, dphi, df, dg, dud));
  }
  return sys.finish((int32_t)m->nv, out);
}

extern "C" int phx_assemble_reaction_wd(phx_mesh *m, double pen_coef, double stab_coef, double reaction,
                                        const double *phi_h, const double *f_h, const double *g_h, const double *u_D,
                                        int loc, phx_system **out) {
  PHX_HIP(hipSetDevice(m->device));
  PHX_REQUIRE(m->cell_type == PHX_TRIANGLE || m->cell_type == PHX_TETRAHEDRON, PHX_ERR_NOT_IMPLEMENTED,
              "the reaction term is assembled on triangles and tetrahedra only");
  bool slab = m->facet_exempt != nullptr || m->slab_cut;
  for (int a = 0; a < m->gdim; ++a) slab = slab || (m->box_nglob[a] > 0 && m->box_nglob[a] != m->box_n[a]);
  PHX_REQUIRE(!slab, PHX_ERR_NOT_IMPLEMENTED, "reaction term: slabs and partitioned ranks are not served");
  PHX_REQUIRE(reaction >= 0.0 && reaction <= 1.79e308, PHX_ERR_VALUE, "reaction = %g: a finite value >= 0", reaction);
  PHX_REQUIRE(m->have_cell_tags && m->have_facet_tags, PHX_ERR_VALUE,
              "cell and facet tags must be computed before assembly");
  PHX_CHECK(build_v2c(m));
  DevTemps staged(m->stream);
  const double *dphi, *df, *dud, *dg = nullptr;
  PHX_CHECK(to_device(m, phi_h, loc, m->nv, &dphi, staged));
  PHX_CHECK(to_device(m, f_h, loc, m->nv, &df, staged));
  if (g_h) PHX_CHECK(to_device(m, g_h, loc, m->nv, &dg, staged));
  PHX_CHECK(to_device(m, u_D, loc, m->nv, &dud, staged));
  PHX_CHECK(phx_begin_timing(m));
  const auto run = [&](int W) { return assemble_react_with_capacity(m, pen_coef, stab_coef, reaction, dphi, df, dg, dud, W, out); };
  int rc = m->gdim == 3 ? retry_capacity({64, 128, 256}, run) : retry_capacity({32, 64, 128}, run);
  if (rc == PHX_OK) rc = phx_end_timing(m, 2);
  return rc;
}
