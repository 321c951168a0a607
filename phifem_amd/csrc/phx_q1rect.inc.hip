// Q1 on a rectangle: the element layer shared by the quadrilateral assemblers (phx_assemble_flux_quad.inc.hip,
// phx_assemble_el_quad.inc.hip, phx_assemble_wd_quad.inc.hip) and the quadrilateral error norms (phx_errors.inc.hip).
// Included by phx_assemble.hip in front of them and of phx_assemble_el.inc.hip (its host function serves both cell
// kinds).
// Conventions, stated here once:
//  * cells are axis-parallel rectangles in tensor-product vertex order v0 (0,0), v1 (1,0), v2 (0,1), v3 (1,1) -- what
//    dolfinx.mesh.create_rectangle builds;
//  * local facets in basix numbering f0 (v0,v1), f1 (v0,v2), f2 (v1,v3), f3 (v2,v3);
//  * h_T = the diagonal (ufl.CellDiameter), avg(h_T) over an interior facet = the mean of the two diagonals;
//  * both cells of an interior facet parametrise it in the same direction, so the Gauss points of the two sides coincide.
// A cell that is not such a rectangle sets a device flag (rect_bad_alloc); the host then fails with
// PHX_ERR_NOT_IMPLEMENTED (rect_bad_check).

struct RectGeo { double hx, hy, h; int32_t v[4]; };
__device__ __forceinline__ bool rect_load(const int32_t *__restrict__ cells, const double *__restrict__ x, int64_t c,
                                          RectGeo &R) {
  double X[4][2];
  for (int i = 0; i < 4; ++i) {
    R.v[i] = cells[c * 4 + i];
    X[i][0] = x[2 * (int64_t)R.v[i]];
    X[i][1] = x[2 * (int64_t)R.v[i] + 1];
  }
  R.hx = X[1][0] - X[0][0];
  R.hy = X[2][1] - X[0][1];
  R.h = sqrt(R.hx * R.hx + R.hy * R.hy);
  const double tx = 1e-12 * fabs(R.hx), ty = 1e-12 * fabs(R.hy);
  return R.hx > 0.0 && R.hy > 0.0 && fabs(X[1][1] - X[0][1]) <= tx && fabs(X[2][0] - X[0][0]) <= ty &&
         fabs(X[3][0] - X[1][0]) <= tx && fabs(X[3][1] - X[2][1]) <= ty;
}

// 1-D linear element integrals on [0, 1]: stiffness A1 = [[1,-1],[-1,1]], mass M1 = [[2,1],[1,2]] / 6,
// C1 = int L_i' L_j = -+ 1/2 for L_0 = 1 - t, L_1 = t
__device__ __forceinline__ double a1(int i, int j) { return i == j ? 1.0 : -1.0; }
__device__ __forceinline__ double m1(int i, int j) { return (i == j ? 2.0 : 1.0) / 6.0; }
__device__ __forceinline__ double c1(int i, int j) { (void)j; return i ? 0.5 : -0.5; }

// Q1 value / physical gradient of vertex function i at reference (xi, eta)
__device__ __forceinline__ void q1_at(int i, double xi, double eta, const RectGeo &R, double *val, double *gx, double *gy) {
  const double lx = (i & 1) ? xi : 1.0 - xi, ly = (i >> 1) ? eta : 1.0 - eta;
  const double dx = (i & 1) ? 1.0 : -1.0, dy = (i >> 1) ? 1.0 : -1.0;
  *val = lx * ly;
  *gx = dx * ly / R.hx;
  *gy = lx * dy / R.hy;
}

// Gauss-Legendre points and weights on [0, 1]
struct Gauss2 { double x[2], w[2]; };
struct Gauss3 { double x[3], w[3]; };
__host__ __device__ constexpr Gauss2 gauss2() {
  constexpr double s3 = 0.5 / 1.7320508075688772;
  return {{0.5 - s3, 0.5 + s3}, {0.5, 0.5}};
}
__host__ __device__ constexpr Gauss3 gauss3() {
  constexpr double s15 = 0.7745966692414834 * 0.5;
  return {{0.5 - s15, 0.5, 0.5 + s15}, {5.0 / 18.0, 8.0 / 18.0, 5.0 / 18.0}};
}

// Point q = 3 qx + qy of the 3 x 3 tensor Gauss rule: the four Q1 values N[i] and the weight w[qx] w[qy].  With a
// rectangle R also the physical gradients G[i][0..1], and the weight is scaled by |K| = hx hy.  The cut-cell kernels
// let their first nine lanes fill a shared-memory table with it.
__device__ __forceinline__ double q1_tab9(int q, const RectGeo *R, double *N, double (*G)[2]) {
  constexpr Gauss3 g = gauss3();
  const double xi = g.x[q / 3], eta = g.x[q % 3];
  const RectGeo unit{1.0, 1.0, 0.0, {0, 0, 0, 0}};   // reference square: the values do not depend on the rectangle
  const RectGeo &Q = R ? *R : unit;
  for (int i = 0; i < 4; ++i) {
    double gx, gy;
    q1_at(i, xi, eta, Q, &N[i], &gx, &gy);
    if (G) { G[i][0] = gx; G[i][1] = gy; }
  }
  const double w = g.w[q / 3] * g.w[q % 3];
  return R ? w * R->hx * R->hy : w;
}

// local facet lf of a rectangle: its two vertices, the axis of its outward normal and the sign
__device__ __forceinline__ void quad_facet(int lf, int *va, int *vb, int *axis, double *sign) {
  constexpr int FA[4] = {0, 0, 1, 2}, FB[4] = {1, 2, 3, 3}, AX[4] = {1, 0, 0, 1};
  constexpr double SG[4] = {-1.0, -1.0, 1.0, 1.0};
  *va = FA[lf]; *vb = FB[lf]; *axis = AX[lf]; *sign = SG[lf];
}

// One side of interior facet f: the cell f2c[2 f + side], where f sits in it (local facet, its two vertices, normal
// sign e_axis), the reference coordinate `fixed` (0 or 1) of the facet along `axis` and its length.  false: the cell
// is not a rectangle.
struct QuadFacetSide {
  RectGeo R;
  int lf, va, vb, axis;
  double sign, fixed, len;
};
__device__ __forceinline__ bool quad_facet_side(int64_t f, int side, const int32_t *__restrict__ c2f,
                                                const int32_t *__restrict__ f2c, const int32_t *__restrict__ cells,
                                                const double *__restrict__ x, QuadFacetSide &S) {
  const int64_t c = f2c[2 * f + side];
  if (!rect_load(cells, x, c, S.R)) return false;
  S.lf = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c2f[c * 4 + k] == (int32_t)f) S.lf = k;
  quad_facet(S.lf, &S.va, &S.vb, &S.axis, &S.sign);
  S.fixed = S.sign > 0.0 ? 1.0 : 0.0;
  S.len = S.axis == 0 ? S.R.hy : S.R.hx;   // normal along x: the facet runs along y
  return true;
}

// The device flag the kernels set on a cell that is not a rectangle, and the one place that reports it.
static int rect_bad_alloc(phx_mesh *m, DevTemps &tmp, int **bad) {
  PHX_HIP(tmp.alloc(bad, sizeof(int)));
  PHX_HIP(hipMemsetAsync(*bad, 0, sizeof(int), m->stream));
  return PHX_OK;
}
// reads the flag back (synchronises the stream)
static int rect_bad_check(phx_mesh *m, const int *bad) {
  int hbad = 0;
  PHX_HIP(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, m->stream));
  PHX_HIP(hipStreamSynchronize(m->stream));
  PHX_REQUIRE(!hbad, PHX_ERR_NOT_IMPLEMENTED,
              "quadrilateral cells must be axis-parallel rectangles in tensor-product vertex order");
  return PHX_OK;
}
