// Interface linear elasticity on QUADRILATERALS: the 5-field mixed phi-FEM of phx_assemble_el.inc.hip
// (u_in, u_out, y_in, y_out, p) in Q1^2 x Q1^2 x Q1^{2x2} x Q1^{2x2} x Q1^2 with a Q1 nodal level-set -- the
// cell_type "quadrilateral" of demo/interface-elasticity/main.py:99-108 with the forms :179-235 (bilinear),
// :255-269 (linear) and the Dirichlet rows of u_in :158-177,237-239,271-277.  Included by phx_assemble.hip after
// phx_assemble_el.inc.hip (ElArgs, ElB<2>, el_add / el_rhs: the DoF layout, the Dirichlet lifting and the
// deterministic Slots passes) and phx_q1rect.inc.hip (the rectangle, the Q1 basis, the facet numbering, the Gauss
// rules: the cell conventions are stated there).
// f_h, u_D: Q1 nodal vector fields, as on simplices (oracle/elasticity.py).  Restated in tests/elasticity_quad_ref.py.
//
// Quadrature is EXACT, so the result equals FFCx's up to round-off:
//  * cell integrands are products of Q1 functions and their derivatives (degree <= 1 in each variable; a derivative
//    lowers its own variable's degree to 0) with the Q1 phi_h, grad(phi_h) and f_h.  The worst terms are
//    h^-4 (p phi_h)(q phi_h) and h^-2 (y . grad phi_h)(z . grad phi_h): degree <= 4 in each variable.  The 3 x 3
//    tensor Gauss rule integrates degree 5 per variable exactly.
//  * facet integrands: (y . n) v and jump(sigma(u), n) . jump(sigma(v), n) are of degree <= 2 along the facet
//    (sigma of a Q1 field is linear along an axis-parallel facet): the 2-point Gauss rule (degree 3) is exact.
//  * the bulk stiffness and the source term use the closed-form 1-D integrals of linear functions on [0, 1].

// int_K d_p N_i d_q N_j on a rectangle (closed form, tensor products of 1-D integrals)
__device__ __forceinline__ double elq_dd(const RectGeo &R, int p, int i, int q, int j) {
  const int ix = i & 1, iy = i >> 1, jx = j & 1, jy = j >> 1;
  if (p == 0 && q == 0) return (R.hy / R.hx) * a1(ix, jx) * m1(iy, jy);
  if (p == 1 && q == 1) return (R.hx / R.hy) * m1(ix, jx) * a1(iy, jy);
  if (p == 0) return c1(ix, jx) * c1(jy, iy);   // int L_ix' L_jx  int L_iy L_jy'
  return c1(jx, ix) * c1(iy, jy);
}

// sigma(N e_b)[p][q] for a basis function with physical gradient g
__device__ __forceinline__ double elq_sig(const double *g, double lam, double mu, int b, int p, int q) {
  return (p == q ? lam * g[b] : 0.0) + mu * ((p == b ? g[q] : 0.0) + (q == b ? g[p] : 0.0));
}

__device__ __forceinline__ bool elq_side_on(int side, int t) {
  return side == 0 ? (t == 1 || t == 2) : (t == 2 || t == 3);
}

// --- stiffness main.py:185-186,226-227 on dx((1,2)) / dx((2,3)) + source :263-264; 128 lanes per cell ------------
// lane = (side, row (a, i), column (c, j)) of the two 8 x 8 displacement blocks; lanes 0..15 also write the rhs
__global__ void __launch_bounds__(128) k_elq_bulk(int64_t nc, ElArgs A) {
  using B = ElB<2>;
  const int64_t c = blockIdx.x;
  if (c >= nc) return;
  const int t = A.ctags[c] & PHX_TAG_MASK;
  if (t < 1 || t > 3) return;
  RectGeo R;
  if (!rect_load(A.cells, A.x, c, R)) { if (threadIdx.x == 0) *A.bad = 1; return; }
  const int side = threadIdx.x / 64, r = (threadIdx.x / 8) % 8, s = threadIdx.x % 8;
  if (elq_side_on(side, t)) {
    const int a = r / 4, i = r % 4, cc = s / 4, j = s % 4;
    // eps(N_i e_a) : sigma(N_j e_c) = lam d_c N_j d_a N_i + mu (delta_ac grad N_j . grad N_i + d_a N_j d_c N_i)
    const double lam = A.lam[side], mu = A.mu[side];
    double k = lam * elq_dd(R, a, i, cc, j) + mu * elq_dd(R, cc, i, a, j);
    if (a == cc) k += mu * (elq_dd(R, 0, i, 0, j) + elq_dd(R, 1, i, 1, j));
    el_add<2>(A, B::ublk(side, a) * A.nv + R.v[i], B::ublk(side, cc) * A.nv + R.v[j], k);
  }
  if (threadIdx.x < 16) {
    const int sd = threadIdx.x / 8, a = (threadIdx.x / 4) % 2, i = threadIdx.x % 4;
    if (!elq_side_on(sd, t)) return;
    const int ix = i & 1, iy = i >> 1;
    double sf = 0.0;
    for (int k = 0; k < 4; ++k) sf += m1(ix, k & 1) * m1(iy, k >> 1) * A.f[(int64_t)a * A.nv + R.v[k]];
    el_rhs<2>(A, B::ublk(sd, a) * A.nv + R.v[i], R.hx * R.hy * sf);
  }
}

// --- cut cells: penalization main.py:188-203, cell stabilisation :211-217, rhs :255-260; one workgroup per cell ----
// The 3 x 3 Gauss tabulation of the Q1 basis (values, physical gradients), phi_h, grad(phi_h) and f_h live in LDS;
// the lanes walk the entries of the present block pairs of the 56 x 56 element tensor (el_cut_pair_present<2>).
__global__ void __launch_bounds__(256) k_elq_cut(int64_t nlist, const int32_t *__restrict__ list, ElArgs A) {
  using B = ElB<2>;
  constexpr int NQ = 9;
  const int64_t e = blockIdx.x;
  if (e >= nlist) return;
  __shared__ uint16_t present[B::C * B::C];
  __shared__ int npresent;
  __shared__ double sN[NQ][4], sG[NQ][4][2], sW[NQ], sPh[NQ], sGp[NQ][2], sF[NQ][2];
  const int64_t c = list[e];
  RectGeo R;
  if (!rect_load(A.cells, A.x, c, R)) { if (threadIdx.x == 0) *A.bad = 1; return; }   // uniform across the workgroup
  if (threadIdx.x == 0) npresent = 0;
  __syncthreads();
  for (int pi = threadIdx.x; pi < B::C * B::C; pi += blockDim.x)
    if (el_cut_pair_present<2>(pi / B::C, pi % B::C)) present[atomicAdd(&npresent, 1)] = (uint16_t)pi;
  if (threadIdx.x < NQ) {
    sW[threadIdx.x] = q1_tab9(threadIdx.x, &R, sN[threadIdx.x], sG[threadIdx.x]);
    double ph = 0.0, gpx = 0.0, gpy = 0.0, f0 = 0.0, f1 = 0.0;
    for (int i = 0; i < 4; ++i) {
      const double val = sN[threadIdx.x][i], tx = sG[threadIdx.x][i][0], ty = sG[threadIdx.x][i][1];
      const double pv = A.phi[R.v[i]];
      ph += pv * val; gpx += pv * tx; gpy += pv * ty;
      f0 += A.f[R.v[i]] * val;
      f1 += A.f[A.nv + R.v[i]] * val;
    }
    sPh[threadIdx.x] = ph; sGp[threadIdx.x][0] = gpx; sGp[threadIdx.x][1] = gpy;
    sF[threadIdx.x][0] = f0; sF[threadIdx.x][1] = f1;
  }
  __syncthreads();
  const int nent = npresent * 16;
  const double h1 = 1.0 / R.h, gam = A.gamma;
  const double sgn[2] = {1.0, -1.0};
  for (int idx = threadIdx.x; idx < nent; idx += blockDim.x) {
    const int pair = present[idx / 16], ij = idx % 16;
    const int rb = pair / B::C, cb = pair % B::C, i = ij / 4, j = ij % 4;
    int kr, ar, br, kc, ac, bc;
    B::decode(rb, kr, ar, br);
    B::decode(cb, kc, ac, bc);
    double val = 0.0;
    bool has = false;
#pragma unroll 1
    for (int q = 0; q < NQ; ++q) {
      const double w = sW[q], Ni = sN[q][i], Nj = sN[q][j];
      const double *gi = sG[q][i], *gj = sG[q][j];
      const double Mij = w * Ni * Nj;
      if (kr <= 1 && kc <= 1) {                       // u_s - u_t
        if (kr == kc) {                               // (y + sigma(u)):(z + sigma(v)), v-u part
          const double lam = A.lam[kr], mu = A.mu[kr];
          double t = 0.0;
          for (int p = 0; p < 2; ++p)
            for (int qq = 0; qq < 2; ++qq) t += elq_sig(gi, lam, mu, ar, p, qq) * elq_sig(gj, lam, mu, ac, p, qq);
          val += gam * A.coefW[kr] * w * t;
          has = true;
        }
        if (ar == ac) { val += gam * sgn[kr] * sgn[kc] * h1 * h1 * Mij; has = true; }
      } else if (kr <= 1 && (kc == 2 || kc == 3)) {   // u_s - y_t : v-y part
        if (kr == kc - 2) { val += gam * A.coefW[kr] * w * Nj * elq_sig(gi, A.lam[kr], A.mu[kr], ar, ac, bc); has = true; }
      } else if ((kr == 2 || kr == 3) && kc <= 1) {   // y_s - u_t : z-u part
        if (kc == kr - 2) { val += gam * A.coefW[kc] * w * Ni * elq_sig(gj, A.lam[kc], A.mu[kc], ac, ar, br); has = true; }
      } else if ((kr == 2 || kr == 3) && (kc == 2 || kc == 3)) {  // y_s - y_t
        const int sr = kr - 2, sc = kc - 2;
        if (ar == ac) {
          val += gam * sgn[sr] * sgn[sc] * h1 * h1 * sGp[q][br] * sGp[q][bc] * Mij;   // main.py:193-197
          has = true;
          if (sr == sc) {
            val += A.sigma * R.h * R.h * w * gi[br] * gj[bc];                          // main.py:211-217
            if (br == bc) val += gam * A.coefW[sr] * Mij;                              // z-y part
          }
        }
      } else if (kr <= 1 && kc == 4) {                // u_s - p
        if (ar == ac) { val += gam * sgn[kr] * h1 * h1 * h1 * Mij * sPh[q]; has = true; }
      } else if (kr == 4 && kc <= 1) {                // p - u_t
        if (ar == ac) { val += gam * sgn[kc] * h1 * h1 * h1 * Mij * sPh[q]; has = true; }
      } else if (kr == 4 && kc == 4) {
        if (ar == ac) { val += gam * h1 * h1 * h1 * h1 * Mij * sPh[q] * sPh[q]; has = true; }
      }
    }
    if (has) el_add<2>(A, rb * A.nv + R.v[i], cb * A.nv + R.v[j], val);
  }
  // rhs: sigma h^2 f . div(z), z = N_i E_ab  ->  sigma h^2 int f_a d_b N_i
  if (threadIdx.x < 32) {
    const int side = threadIdx.x / 16, a = (threadIdx.x / 8) % 2, b = (threadIdx.x / 4) % 2, i = threadIdx.x % 4;
    double acc = 0.0;
    for (int q = 0; q < NQ; ++q) acc += sW[q] * sF[q][a] * sG[q][i][b];
    el_rhs<2>(A, B::yblk(side, a, b) * A.nv + R.v[i], A.sigma * R.h * R.h * acc);
  }
}

// --- one-sided boundary terms main.py:182-183: (y_s n) . v_s over d_bdry(100) / d_bdry(101); 8 lanes per entity ---
// n = sign e_axis on the local facet; int_F N_i N_j = |F| m1 over the facet's two vertices
__global__ void __launch_bounds__(256) k_elq_ds(int64_t nent, const int64_t *__restrict__ ent_packed, int side, ElArgs A) {
  using B = ElB<2>;
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t e = gid / 8;
  const int l = (int)(gid % 8);
  if (e >= nent) return;
  const int64_t c = ent_packed[2 * e + 1] >> 8;
  const int lf = (int)(ent_packed[2 * e + 1] & 0xff);
  RectGeo R;
  if (!rect_load(A.cells, A.x, c, R)) { *A.bad = 1; return; }
  int va, vb, axis;
  double sign;
  quad_facet(lf, &va, &vb, &axis, &sign);
  const int ends[2] = {va, vb};
  const int a = l / 4, i = (l / 2) % 2, j = l % 2;
  const double len = axis == 0 ? R.hy : R.hx;   // normal along x: the facet runs along y
  const int32_t row = B::ublk(side, a) * A.nv + R.v[ends[i]], col = B::yblk(side, a, axis) * A.nv + R.v[ends[j]];
  if (A.dofmap[row] < 0 || A.dofmap[col] < 0) return;   // y lives on cut cells only
  el_add<2>(A, row, col, len * m1(i, j) * sign);
}

// --- facet stabilisation main.py:205-209 (dS(3), in) and :219-223 (dS(4), out); one workgroup per facet ----------
// entry (r, s) over the 16 local functions (cell side, component a, vertex i) of the two cells; 2-point Gauss on
// the facet, which both rectangles parametrise in the same direction (tensor-product order)
__global__ void __launch_bounds__(256) k_elq_facets(int64_t nlist, const int32_t *__restrict__ list, int side, ElArgs A) {
  using B = ElB<2>;
  const int64_t e = blockIdx.x;
  if (e >= nlist) return;
  const int64_t f = list[e];
  constexpr Gauss2 g2 = gauss2();
  QuadFacetSide S[2];
  double hsum = 0.0;
  for (int sd = 0; sd < 2; ++sd) {
    if (!quad_facet_side(f, sd, A.c2f, A.f2c, A.cells, A.x, S[sd])) { if (threadIdx.x == 0) *A.bad = 1; return; }
    hsum += S[sd].R.h;
  }
  const double len = S[0].len;
  const double wgt = A.sigma * 0.5 * hsum * len;
  const double lam = A.lam[side], mu = A.mu[side];
  const int r = threadIdx.x / 16, s = threadIdx.x % 16;
  const int sr = r / 8, ar = (r / 4) % 2, i = r % 4;
  const int sc = s / 8, ac = (s / 4) % 2, j = s % 4;
  double acc = 0.0;
  for (int q = 0; q < 2; ++q) {
    double J[2][2];   // (sigma(N e) n)_p of the row and the column function
    for (int k = 0; k < 2; ++k) {
      const int sd = k == 0 ? sr : sc, vi = k == 0 ? i : j, comp = k == 0 ? ar : ac;
      const QuadFacetSide &F = S[sd];
      const double xi = F.axis == 0 ? F.fixed : g2.x[q], eta = F.axis == 1 ? F.fixed : g2.x[q];
      double val, g[2];
      q1_at(vi, xi, eta, F.R, &val, &g[0], &g[1]);
      for (int p = 0; p < 2; ++p) J[k][p] = F.sign * elq_sig(g, lam, mu, comp, p, F.axis);
    }
    acc += g2.w[q] * (J[0][0] * J[1][0] + J[0][1] * J[1][1]);
  }
  el_add<2>(A, B::ublk(side, ar) * A.nv + S[sr].R.v[i], B::ublk(side, ac) * A.nv + S[sc].R.v[j], wgt * acc);
}

// launched by assemble_el_with_capacity (phx_assemble_el.inc.hip) in place of the simplex element kernels
static int el_quad_launch(phx_mesh *m, const ElArgs &A, int64_t n_cut, const int32_t *l_cut, int64_t n_f3,
                          const int32_t *l_f3, int64_t n_f4, const int32_t *l_f4) {
  const dim3 block(256);
  k_elq_bulk<<<dim3((unsigned)m->nc), dim3(128), 0, m->stream>>>(m->nc, A);
  if (n_cut) k_elq_cut<<<dim3((unsigned)n_cut), block, 0, m->stream>>>(n_cut, l_cut, A);
  for (int sd = 0; sd < 2; ++sd)
    if (m->ent_count[sd])
      k_elq_ds<<<dim3((unsigned)phx_div_up(m->ent_count[sd] * 8, 256)), block, 0, m->stream>>>(
          m->ent_count[sd], m->ent_buf[sd], sd, A);
  if (n_f3) k_elq_facets<<<dim3((unsigned)n_f3), block, 0, m->stream>>>(n_f3, l_f3, 0, A);
  if (n_f4) k_elq_facets<<<dim3((unsigned)n_f4), block, 0, m->stream>>>(n_f4, l_f4, 1, A);
  PHX_HIP(hipGetLastError());
  return PHX_OK;
}
