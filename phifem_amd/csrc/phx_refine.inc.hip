// Uniform regular refinement and the nested coarse -> fine transfer of Lagrange nodal functions (include of
// phx_submesh.hip: -ffp-contract=off, the transfer arithmetic is specified bit for bit).  Stands in for
// dolfinx.mesh.refine (demo/interface-elasticity/main.py:390) with red / Bey refinement; tests/refine_ref.py restates
// every rule in numpy.  Purely topological: nothing here compares floats.
//
// Local degree-2 nodes of a cell: 0 .. nvpc-1 its vertices, nvpc + k its local edge k (simplices, basix order) or
// local facet k (quadrilaterals), last the quadrilateral's centre.  The fine vertex of local node d of cell c is
// cells[c][d], nv + c2e[c][k] (quadrilaterals: nv + c2f[c][k]), nv + nf + c.
namespace {

struct RefineTables {
  int nvpc = 0, nchild = 0, nmid = 0, nepc = 0, ndof2 = 0;
  int8_t child[8][4] = {};
  double w[8][6][10] = {};   // simplices: P2 weights of child k, child edge j (basix local order), parent local DoF d
};

// local vertex pairs of the local edges (simplices, basix) / local facets (quadrilaterals)
const int kTriEdge[3][2] = {{1, 2}, {0, 2}, {0, 1}};
const int kTetEdge[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};
const int kQuadFacet[4][2] = {{0, 1}, {0, 2}, {1, 3}, {2, 3}};

int refine_tables(int cell_type, RefineTables &T) {
  T = RefineTables();
  // children as pairs (i, j) of parent vertices: i == j the vertex, otherwise the midpoint of (i, j); 9 = the centre
  static const int tri[4][3][2] = {{{0, 0}, {0, 1}, {0, 2}}, {{0, 1}, {1, 1}, {1, 2}}, {{0, 2}, {1, 2}, {2, 2}},
                                   {{1, 2}, {0, 2}, {0, 1}}};
  static const int tet[8][4][2] = {   // Bey, interior diagonal m02 - m13
      {{0, 0}, {0, 1}, {0, 2}, {0, 3}}, {{0, 1}, {1, 1}, {1, 2}, {1, 3}}, {{0, 2}, {1, 2}, {2, 2}, {2, 3}},
      {{0, 3}, {1, 3}, {2, 3}, {3, 3}}, {{0, 1}, {0, 2}, {0, 3}, {1, 3}}, {{0, 1}, {0, 2}, {1, 2}, {1, 3}},
      {{0, 2}, {0, 3}, {1, 3}, {2, 3}}, {{0, 2}, {1, 2}, {1, 3}, {2, 3}}};
  static const int quad[4][4][2] = {{{0, 0}, {0, 1}, {0, 2}, {9, 9}}, {{0, 1}, {1, 1}, {9, 9}, {1, 3}},
                                    {{0, 2}, {9, 9}, {2, 2}, {2, 3}}, {{9, 9}, {1, 3}, {2, 3}, {3, 3}}};
  const int (*mid)[2];
  if (cell_type == PHX_TRIANGLE) { T.nvpc = 3; T.nchild = 4; T.nmid = 3; T.nepc = 3; mid = kTriEdge; }
  else if (cell_type == PHX_TETRAHEDRON) { T.nvpc = 4; T.nchild = 8; T.nmid = 6; T.nepc = 6; mid = kTetEdge; }
  else if (cell_type == PHX_QUADRILATERAL) { T.nvpc = 4; T.nchild = 4; T.nmid = 4; T.nepc = 0; mid = kQuadFacet; }
  else {
    phx_set_error("refinement serves triangles, tetrahedra and quadrilaterals");
    return PHX_ERR_NOT_IMPLEMENTED;
  }
  T.ndof2 = T.nvpc + T.nmid + (cell_type == PHX_QUADRILATERAL ? 1 : 0);
  for (int k = 0; k < T.nchild; ++k)
    for (int j = 0; j < T.nvpc; ++j) {
      const int *p = cell_type == PHX_TRIANGLE ? tri[k][j] : (cell_type == PHX_TETRAHEDRON ? tet[k][j] : quad[k][j]);
      int node = -1;
      if (p[0] == 9) node = T.nvpc + T.nmid;
      else if (p[0] == p[1]) node = p[0];
      else
        for (int e = 0; e < T.nmid; ++e)
          if (mid[e][0] == p[0] && mid[e][1] == p[1]) node = T.nvpc + e;
      T.child[k][j] = (int8_t)node;
    }
  if (cell_type == PHX_QUADRILATERAL) return PHX_OK;
  // P2 basis of the parent at the midpoint of every child edge, in barycentric coordinates (all values dyadic)
  for (int k = 0; k < T.nchild; ++k)
    for (int j = 0; j < T.nepc; ++j) {
      double lam[4] = {0, 0, 0, 0};
      for (int s = 0; s < 2; ++s) {
        const int node = T.child[k][mid[j][s]];
        if (node < T.nvpc) lam[node] += 0.5;
        else { lam[mid[node - T.nvpc][0]] += 0.25; lam[mid[node - T.nvpc][1]] += 0.25; }
      }
      for (int d = 0; d < T.nvpc; ++d) T.w[k][j][d] = lam[d] * (2.0 * lam[d] - 1.0);
      for (int e = 0; e < T.nmid; ++e) T.w[k][j][T.nvpc + e] = 4.0 * lam[mid[e][0]] * lam[mid[e][1]];
    }
  return PHX_OK;
}

struct ChildTab { int nvpc, nchild, nmid; int8_t child[8][4]; };

// one thread per FINE cell: child k of coarse cell c is fine cell nchild c + k
__global__ void __launch_bounds__(256)
k_refine_cells(int64_t ncf, ChildTab T, const int32_t *__restrict__ cells, const int32_t *__restrict__ c2m, int64_t nv,
               int64_t ctr_base, int32_t *__restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncf) return;
  const int64_t c = i / T.nchild;
  const int k = (int)(i - c * T.nchild);
  for (int j = 0; j < T.nvpc; ++j) {
    const int node = T.child[k][j];
    int64_t id;
    if (node < T.nvpc) id = cells[c * T.nvpc + node];
    else if (node < T.nvpc + T.nmid) id = nv + c2m[c * T.nmid + (node - T.nvpc)];
    else id = ctr_base + c;
    out[i * T.nvpc + j] = (int32_t)id;
  }
}

// facet -> its two vertices (quadrilaterals), read from the facet's first cell
__global__ void __launch_bounds__(256)
k_refine_facet_pairs(int64_t nf, const int32_t *__restrict__ f2c, const int32_t *__restrict__ c2f,
                     const int32_t *__restrict__ cells, int32_t *__restrict__ pairs) {
  const int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const int64_t c = f2c[2 * f];
  int lf = 0;
  for (int k = 0; k < 4; ++k)
    if (c2f[c * 4 + k] == f) lf = k;
  const int a = lf < 2 ? 0 : lf - 1, b = lf == 0 ? 1 : (lf == 3 ? 3 : lf + 1);   // (0,1) (0,2) (1,3) (2,3)
  pairs[2 * f] = cells[c * 4 + a];
  pairs[2 * f + 1] = cells[c * 4 + b];
}

// ---- degree 1: copy at the coarse vertices, 0.5 u_p + 0.5 u_q at midpoints, ((u0/4 + u1/4) + u2/4) + u3/4 at centres
__global__ void __launch_bounds__(256)
k_prol_copy(int64_t n, int ncomp, const double *__restrict__ in, int64_t ldin, double *__restrict__ out, int64_t ldout) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int q = 0; q < ncomp; ++q) out[q * ldout + i] = in[q * ldin + i];
}
__global__ void __launch_bounds__(256)
k_prol_mid(int64_t n, const int32_t *__restrict__ pairs, int ncomp, const double *__restrict__ in, int64_t ldin,
           double *__restrict__ out, int64_t ldout) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t p = pairs[2 * i], q = pairs[2 * i + 1];
  for (int s = 0; s < ncomp; ++s) out[s * ldout + i] = 0.5 * in[s * ldin + p] + 0.5 * in[s * ldin + q];
}
__global__ void __launch_bounds__(256)
k_prol_centre(int64_t nc, const int32_t *__restrict__ cells, int ncomp, const double *__restrict__ in, int64_t ldin,
              double *__restrict__ out, int64_t ldout) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int64_t v0 = cells[4 * c], v1 = cells[4 * c + 1], v2 = cells[4 * c + 2], v3 = cells[4 * c + 3];
  for (int s = 0; s < ncomp; ++s) {
    const double *u = in + s * ldin;
    out[s * ldout + c] = ((0.25 * u[v0] + 0.25 * u[v1]) + 0.25 * u[v2]) + 0.25 * u[v3];
  }
}

// ---- degree 2 on simplices: the fine edge DoFs.  Pass 1: owner[fe] = lowest-numbered parent cell that contains the
// fine edge (integer atomicMin); pass 2: that parent writes.  Children of ONE parent that share a fine edge evaluate
// the same table row in the same order, so their stores carry the same bits.
__global__ void __launch_bounds__(256)
k_prol2_owner(int64_t ncf, int nchild, int nepc, const int32_t *__restrict__ fc2e, int32_t *__restrict__ owner) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncf * nepc) return;
  atomicMin(&owner[fc2e[i]], (int32_t)((i / nepc) / nchild));
}
__global__ void __launch_bounds__(256)
k_prol2_edges(int64_t ncf, int nvpc, int nchild, int nepc, const int32_t *__restrict__ cells,
              const int32_t *__restrict__ c2e, int64_t nv, const int32_t *__restrict__ fc2e,
              const int32_t *__restrict__ owner, const double *__restrict__ w, int ncomp, const double *__restrict__ in,
              int64_t ldin, double *__restrict__ out, int64_t ldout) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncf) return;
  const int64_t c = i / nchild;
  const int k = (int)(i - c * nchild);
  const int ndof2 = nvpc + nepc;
  int64_t g[10];
  for (int d = 0; d < nvpc; ++d) g[d] = cells[c * nvpc + d];
  for (int e = 0; e < nepc; ++e) g[nvpc + e] = nv + c2e[c * nepc + e];
  for (int j = 0; j < nepc; ++j) {
    const int64_t fe = fc2e[i * nepc + j];
    if (owner[fe] != (int32_t)c) continue;
    const double *wr = w + (k * nepc + j) * ndof2;
    for (int s = 0; s < ncomp; ++s) {
      const double *u = in + s * ldin;
      double acc = 0.0;
      bool first = true;
      for (int d = 0; d < ndof2; ++d) {     // ascending parent-local DoF, zero weights skipped
        if (wr[d] == 0.0) continue;
        const double t = wr[d] * u[g[d]];
        acc = first ? t : acc + t;
        first = false;
      }
      out[s * ldout + fe] = acc;
    }
  }
}

double wall_seconds() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

extern "C" int phx_refine_tables(int cell_type, int32_t *children, int *nchild, double *p2_weights) {
  RefineTables T;
  PHX_CHECK(refine_tables(cell_type, T));
  if (nchild) *nchild = T.nchild;
  if (children)
    for (int k = 0; k < T.nchild; ++k)
      for (int j = 0; j < T.nvpc; ++j) children[k * T.nvpc + j] = T.child[k][j];
  if (p2_weights && T.nepc > 0)
    for (int k = 0; k < T.nchild; ++k)
      for (int j = 0; j < T.nepc; ++j)
        for (int d = 0; d < T.ndof2; ++d) p2_weights[(k * T.nepc + j) * T.ndof2 + d] = T.w[k][j][d];
  return PHX_OK;
}

extern "C" int phx_mesh_refine(phx_mesh *m, phx_mesh **fine_out) {
  RefineTables T;
  PHX_CHECK(refine_tables(m->cell_type, T));
  PHX_HIP(hipSetDevice(m->device));
  PHX_REQUIRE(!m->slab_cut, PHX_ERR_VALUE,
              "a slab with declared cut faces cannot be refined: the fine mesh cannot inherit them");
  const bool quad = m->cell_type == PHX_QUADRILATERAL;
  const double t0 = wall_seconds();
  if (!quad) PHX_CHECK(phx_mesh_build_edges(m));
  const int64_t nmidg = quad ? m->nf : m->ne;
  const int64_t nvf = m->nv + nmidg + (quad ? m->nc : 0), ncf = m->nc * (int64_t)T.nchild;
  PHX_REQUIRE(nvf < INT32_MAX && ncf * (int64_t)m->ci.nfpc < INT32_MAX, PHX_ERR_VALUE,
              "refined mesh too large for 32-bit local ids (%lld vertices, %lld cells)", (long long)nvf, (long long)ncf);
  PHX_REQUIRE_GRID(ncf + 255, "phx_mesh_refine");
  DevTemps tmp(m->stream);
  double *xf = nullptr;
  int32_t *cf = nullptr;
  PHX_HIP(tmp.alloc(&xf, sizeof(double) * (size_t)nvf * m->gdim));
  PHX_HIP(tmp.alloc(&cf, sizeof(int32_t) * (size_t)ncf * T.nvpc));
  const double t1 = wall_seconds();
  // fine vertices = the degree-2 Lagrange DoF points, by the kernel Mesh.lagrange_dof_points(2) runs
  PHX_CHECK(phx_lagrange_dof_points(m, 2, xf));
  ChildTab C;
  C.nvpc = T.nvpc; C.nchild = T.nchild; C.nmid = T.nmid;
  memcpy(C.child, T.child, sizeof(C.child));
  k_refine_cells<<<dim3((unsigned)phx_div_up(ncf, 256)), dim3(256), 0, m->stream>>>(
      ncf, C, m->cells, quad ? m->c2f : m->c2e, m->nv, m->nv + nmidg, cf);
  PHX_HIP(hipGetLastError());
  // the new mesh copies device sources on ITS stream: everything above has to have run
  PHX_HIP(hipStreamSynchronize(m->stream));
  const double t2 = wall_seconds();
  phx_mesh *f = nullptr;
  if (m->is_box || (m->on_box_lattice && !m->is_submesh)) {
    // a lattice stands behind the coarse mesh: the fine one is what phx_mesh_create makes of the same arrays (host
    // lattice detection, generated box or lattice copy behind it) -- one read-back, as a caller's arrays would cost
    std::vector<double> xh((size_t)nvf * m->gdim);
    std::vector<int32_t> ch((size_t)ncf * T.nvpc);
    PHX_HIP(hipMemcpy(xh.data(), xf, sizeof(double) * xh.size(), hipMemcpyDeviceToHost));
    PHX_HIP(hipMemcpy(ch.data(), cf, sizeof(int32_t) * ch.size(), hipMemcpyDeviceToHost));
    PHX_CHECK(phx_mesh_create_from(m->gdim, m->cell_type, nvf, xh.data(), ncf, ch.data(), PHX_HOST, m->device, &f));
  } else {
    PHX_CHECK(phx_mesh_create_from(m->gdim, m->cell_type, nvf, xf, ncf, cf, PHX_DEVICE, m->device, &f));
  }
  f->refined_from = m->uid;
  f->refine_nchild = T.nchild;
  f->timings[5] = t1 - t0;                 // edge numbering of the coarse mesh (0 when it existed)
  f->timings[6] = t2 - t1;                 // refinement kernels
  f->timings[7] = wall_seconds() - t2;     // creation of the fine mesh (topology, boundary list, lattice detection)
  *fine_out = f;
  return PHX_OK;
}

extern "C" int phx_prolongate(phx_mesh *coarse, phx_mesh *fine, int degree, int ncomp, const double *in, int loc_in,
                              double *out, int loc_out) {
  if (fine && fine->rm_marked) return phx_prolongate_marked(coarse, fine, degree, ncomp, in, loc_in, out, loc_out);
  RefineTables T;
  PHX_CHECK(refine_tables(coarse->cell_type, T));
  const bool quad = coarse->cell_type == PHX_QUADRILATERAL;
  PHX_REQUIRE(degree == 1 || degree == 2, PHX_ERR_NOT_IMPLEMENTED, "prolongation of degree %d is not implemented", degree);
  PHX_REQUIRE(!(quad && degree == 2), PHX_ERR_NOT_IMPLEMENTED, "degree-2 prolongation on quadrilaterals is not implemented");
  PHX_REQUIRE(fine != coarse && fine->refined_from == coarse->uid && fine->device == coarse->device &&
                  fine->nc == coarse->nc * (int64_t)T.nchild,
              PHX_ERR_VALUE, "the fine mesh is not the refinement of the given coarse mesh");
  PHX_REQUIRE(ncomp >= 1 && in && out, PHX_ERR_VALUE, "phx_prolongate: bad arguments");
  PHX_HIP(hipSetDevice(coarse->device));
  hipStream_t st = coarse->stream;
  if (!quad) PHX_CHECK(phx_mesh_build_edges(coarse));
  if (degree == 2) PHX_CHECK(phx_mesh_build_edges(fine));
  const int64_t nv = coarse->nv, nmidg = quad ? coarse->nf : coarse->ne;
  const int64_t ldin = degree == 1 ? nv : nv + coarse->ne;
  const int64_t ldout = degree == 1 ? fine->nv : fine->nv + fine->ne;
  PHX_REQUIRE(fine->nv == nv + nmidg + (quad ? coarse->nc : 0), PHX_ERR_VALUE,
              "the fine mesh is not the refinement of the given coarse mesh");
  PHX_REQUIRE_GRID(fine->nc * (int64_t)(T.nepc > 0 ? T.nepc : 1) + 255, "phx_prolongate");
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
  auto grid = [](int64_t n) { return dim3((unsigned)phx_div_up(n > 0 ? n : 1, 256)); };
  if (degree == 1) {
    k_prol_copy<<<grid(nv), block, 0, st>>>(nv, ncomp, din, ldin, dout, ldout);
    const int32_t *pairs = coarse->edges;
    if (quad) {
      int32_t *fp = nullptr;
      PHX_HIP(tmp.alloc(&fp, sizeof(int32_t) * 2 * (size_t)coarse->nf));
      k_refine_facet_pairs<<<grid(coarse->nf), block, 0, st>>>(coarse->nf, coarse->f2c, coarse->c2f, coarse->cells, fp);
      pairs = fp;
    }
    k_prol_mid<<<grid(nmidg), block, 0, st>>>(nmidg, pairs, ncomp, din, ldin, dout + nv, ldout);
    if (quad)
      k_prol_centre<<<grid(coarse->nc), block, 0, st>>>(coarse->nc, coarse->cells, ncomp, din, ldin, dout + nv + nmidg, ldout);
  } else {
    // fine vertex v < nv is coarse vertex v, fine vertex nv + e is the node of coarse edge e: the first nv + ne values
    // are copies.  Fine edge DoFs: the parent's P2 function at the fine edge's midpoint, written by the fine edge's
    // lowest-numbered parent cell.
    k_prol_copy<<<grid(ldin), block, 0, st>>>(ldin, ncomp, din, ldin, dout, ldout);
    int32_t *owner = nullptr;
    double *w = nullptr;
    PHX_HIP(tmp.alloc(&owner, sizeof(int32_t) * (size_t)fine->ne));
    PHX_HIP(tmp.alloc(&w, sizeof(T.w)));
    std::vector<double> wh((size_t)T.nchild * T.nepc * T.ndof2);
    for (int k = 0; k < T.nchild; ++k)
      for (int j = 0; j < T.nepc; ++j)
        for (int d = 0; d < T.ndof2; ++d) wh[(size_t)(k * T.nepc + j) * T.ndof2 + d] = T.w[k][j][d];
    PHX_HIP(hipMemcpyAsync(w, wh.data(), sizeof(double) * wh.size(), hipMemcpyHostToDevice, st));
    PHX_HIP(hipMemsetAsync(owner, 0x7f, sizeof(int32_t) * (size_t)fine->ne, st));
    k_prol2_owner<<<grid(fine->nc * T.nepc), block, 0, st>>>(fine->nc, T.nchild, T.nepc, fine->c2e, owner);
    k_prol2_edges<<<grid(fine->nc), block, 0, st>>>(fine->nc, T.nvpc, T.nchild, T.nepc, coarse->cells, coarse->c2e, nv,
                                                    fine->c2e, owner, w, ncomp, din, ldin, dout + fine->nv, ldout);
    PHX_HIP(hipGetLastError());
    PHX_HIP(hipStreamSynchronize(st));    // `wh` goes out of scope
  }
  PHX_HIP(hipGetLastError());
  if (loc_out != PHX_DEVICE)
    PHX_HIP(hipMemcpyAsync(out, dout, sizeof(double) * (size_t)ldout * ncomp, hipMemcpyDeviceToHost, st));
  PHX_HIP(hipStreamSynchronize(st));
  return PHX_OK;
}
