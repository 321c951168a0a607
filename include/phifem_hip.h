/* phifem_hip.h -- C ABI of the MI355X-native phi-FEM hot path (libphifem_hip.so).
 *
 * The reference (PhiFEM/phiFEM v0.7.0) has no FFI: its boundary is the Python call
 *   compute_tags_measures(mesh, discrete_levelset, detection_degree, box_mode,
 *                         single_layer_cut, overwrite_tags)      src/phifem/mesh_scripts.py:571-653
 * followed, in every demo, by dolfinx `assemble_matrix` / `assemble_vector` and a PETSc/MUMPS
 * solve (demo/weak-dirichlet/flower/main.py:137-139,153-154,162-182).  Each entry point below
 * names the reference lines it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every buffer it passes in;
 *   - every function returns 0 on success or a negative phx_status; phx_last_error() gives
 *     the message of the last failure on the calling thread;
 *   - arguments called `loc` say where a buffer lives: PHX_HOST or PHX_DEVICE (a device
 *     pointer of the mesh's GPU, e.g. a torch tensor's data_ptr);
 *   - one mesh handle is bound to one GPU and one HIP stream; handles are not thread-safe,
 *     different handles may be used concurrently;
 *   - there is NO CPU fallback: without a usable GPU the device entry points fail with
 *     PHX_ERR_HIP.  The few host-only helpers are marked [host].
 *
 * Numbering contract (also restated in oracle/topology.py and oracle/meshgen.py)
 *   cells/vertices keep caller order; simplex local facet i is opposite local vertex i;
 *   quadrilateral vertices are in tensor-product order, facets (0,1),(0,2),(1,3),(2,3);
 *   u-DoF of vertex v is v, p-DoF is nv + v.
 */
#ifndef PHIFEM_HIP_H
#define PHIFEM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phx_mesh phx_mesh;     /* mesh + topology + current tags, resident in HBM */
typedef struct phx_system phx_system; /* assembled matrix + rhs + solver workspace       */

enum phx_status {
  PHX_OK = 0,
  PHX_ERR_VALUE = -1,          /* -> ValueError            (mesh_scripts.py:242,262,609,614) */
  PHX_ERR_NOT_IMPLEMENTED = -2,/* -> NotImplementedError   (mesh_scripts.py:326-329)         */
  PHX_ERR_HIP = -3,            /* -> RuntimeError: HIP runtime failure / no GPU              */
  PHX_ERR_PARTITION = -4,      /* -> ValueError: facet tag sets overlap (dolfinx MeshTags
                                     rejects duplicated entities, mesh_scripts.py:554-556)    */
  PHX_ERR_CAPACITY = -5,       /* row-slot capacity exceeded during assembly; retry larger   */
  PHX_ERR_BREAKDOWN = -6,      /* Krylov breakdown (rho or omega vanished)                   */
  PHX_ERR_TIMEOUT = -7         /* multi-GPU: a collective did not complete within PHX_DIST_TIMEOUT_S (a rank
                                  never arrived); the stream is wedged -- the process must exit        */
};

enum phx_loc { PHX_HOST = 0, PHX_DEVICE = 1 };

enum phx_cell_type { PHX_TRIANGLE = 0, PHX_QUADRILATERAL = 1, PHX_TETRAHEDRON = 2 };

/* How the level-set reaches the tagging kernels (mesh_scripts.py:571-574: a P_k Function or a
 * UFL expression). */
enum phx_phi_kind {
  PHX_PHI_NODAL_P1 = 0, /* phi[nv]: values at the mesh vertices                               */
  PHX_PHI_POINTS = 1,   /* phi_cells[nc*npts_cell] then phi_bfacets[nbf*npts_facet]: values the
                           host evaluated at the physical detection points (expression mode)  */
  PHX_PHI_QUADRIC = 2   /* 7 doubles {cx,cy,cz, sx,sy,sz, c0}: sum_a (s_a x_a - c_a)^2 + c0,
                           evaluated on the device at the physical detection points           */
};

enum phx_array {          /* phx_mesh_get_array selectors */
  PHX_ARR_COORDS = 0,     /* f64 [nv*gdim]                                */
  PHX_ARR_CELLS = 1,      /* i32 [nc*nvpc]                                */
  PHX_ARR_C2F = 2,        /* i32 [nc*nfpc]                                */
  PHX_ARR_F2C = 3,        /* i32 [nf*2], ascending cell index, -1 padded  */
  PHX_ARR_CELL_TAGS = 4,  /* i32 [nc]  values 1,2,3 (0 = unclassified)    */
  PHX_ARR_FACET_TAGS = 5, /* i32 [nf]  values 1..6                        */
  PHX_ARR_BFACETS = 6,    /* i32 [nbf*2] (cell, local facet) of the background-boundary facets,
                             ascending facet index                        */
  PHX_ARR_C2E = 7,        /* i32 [nc*nepc] cell -> edges (P2 DoFs), local edge order of basix:
                             triangle (1,2),(0,2),(0,1); tetrahedron (2,3),(1,3),(1,2),(0,3),(0,2),(0,1) */
  PHX_ARR_EDGES = 8,      /* i32 [ne*2] vertex pair of every edge, ascending */
  PHX_ARR_PARENT_CELLS = 9, /* i32 [nc]     meshes made by phx_mesh_refine_marked: coarse cell of every cell      */
  PHX_ARR_CHILD_NODES = 10  /* i8 [nc*nvpc] the same: local degree-2 nodes of the parent, the cell's leaf tuple  */
};

/* ------------------------------------------------------------------ misc ------------- */
int phx_version(void);                     /* [host] ABI version (1) */
const char *phx_last_error(void);          /* [host] */
int phx_device_count(int *n);              /* [host] 0 GPUs is not an error here */
/* Return the device memory cached by the library's allocator to the driver. */
int phx_pool_release(void);
/* [host] Bytes the allocator has handed out and not got back (all devices) / bytes it keeps cached.  A call that
 * fails must leave live_bytes where it found it. */
int phx_pool_stats(int64_t *live_bytes, int64_t *cached_bytes);

/* [host] Detection points on the reference cell / reference facet: restates
 * _reference_{segment,triangle_boundary,square_boundary}_points (mesh_scripts.py:28-92) and
 * extends them to the tetrahedron.  which = 0: cell points (tdim coords each), 1: facet points
 * (tdim-1 coords each).  Count-then-fill: call with out == NULL to get *npts. */
int phx_detection_points(int cell_type, int degree, int which, double *out, int64_t *npts);

/* Level-sets that are neither P1-nodal nor a quadric reach phx_tag_cells / phx_tag_facets as PHX_PHI_POINTS: one
 * value per detection point, the cells first ([nc][points per cell]), then the background-boundary facets in
 * ascending facet id ([nbf][points per facet]); *count = the number of values (doubles) of that layout.
 * phx_levelset_eval_points: a DEGREE-2 nodal level-set (mesh_scripts.py:95-134 with a P2 `discrete_levelset`, the
 * Robin / Neumann demos' phi_h) evaluated on the device -- nodal[nv + ne] (vertices, then edges) on simplices,
 * nodal[nv + nf + nc] (vertices, facets, cells) on quadrilaterals, at `loc`; out_device[count].
 * phx_detection_points_physical: the physical detection points x_q themselves, out_device[count][gdim], so that a
 * caller's expression (the "UFL expression" mode of tests/test_compute_meshtags.py:159-161) can be evaluated on
 * device arrays without a host round trip. */
int phx_levelset_points_count(phx_mesh *m, int detection_degree, int64_t *count);
int phx_levelset_eval_points(phx_mesh *m, int detection_degree, const double *nodal, int loc,
                             double *out_device);
int phx_detection_points_physical(phx_mesh *m, int detection_degree, double *out_device);

/* Lagrange level-sets of degree 1, 2 and 3 -- the `discretize=True` input of tests/test_compute_meshtags.py:153-158,
 * which interpolates phi into basix.ufl.element("Lagrange", cell, detection_degree) (dolfinx `Function.interpolate`,
 * :157) before src/phifem/mesh_scripts.py:95-134 evaluates it at the detection points.
 *
 * Reference element: basix's default (GLL-warped) Lagrange nodes in basix's local order -- vertices; per edge (basix
 * edge order; a quadrilateral's edges are its local facets) k - 1 nodes from its first to its second local vertex, at
 * the Gauss-Lobatto-Legendre parameters (1 -+ 1/sqrt5)/2 for k = 3; then at k = 3 the triangle's centroid, the
 * tetrahedron's 4 face centroids (face f opposite vertex f), the quadrilateral's 4 interior nodes (tensor product of
 * the 1-D GLL points, x fastest).  The degree-1 and -2 tables are those of phx_tag_cells and phx_levelset_eval_points.
 *
 * Global DoF layout of a nodal level-set (`NodalFunction(values, degree)`):
 *   degree 1  nv                  vertices
 *   degree 2  nv + ne             vertices, edges (PHX_ARR_EDGES)                       (simplices)
 *             nv + nf + nc        vertices, facets, cells                               (quadrilaterals)
 *   degree 3  nv + 2 ne + nc      vertices, 2 per edge, 1 per cell                      (triangles)
 *             nv + 2 ne + nf      vertices, 2 per edge, 1 per face (facet id)           (tetrahedra)
 *             nv + 2 nf + 4 nc    vertices, 2 per facet, 4 per cell (interior order)    (quadrilaterals)
 * The pair of an edge (facet) e is nodal[nv + 2e], nodal[nv + 2e + 1]: first the node nearer its LOWER global vertex.
 * ne: phx_mesh_edge_count; nv, nc, nf: phx_mesh_counts.
 *
 * [host] phx_lagrange_nodes: the reference-cell nodes, out[n][tdim]; count-then-fill (out == NULL -> *n).
 * [host] phx_lagrange_tabulate: the basis at npts reference points pts[npts][tdim], out[npts][ndof] (local order).
 * phx_levelset_eval_points_deg: phx_levelset_eval_points for a nodal level-set of degree `levelset_degree` (1, 2 or
 * 3, laid out as above, at `loc`); degree 2 IS phx_levelset_eval_points.  out_device: phx_levelset_points_count values.
 * phx_lagrange_dof_points: physical coordinates of every global DoF of degree 1-3, out_device[ndofs][gdim] (the
 * interpolation points of `Function.interpolate`); quadrilateral nodes through the bilinear geometry map. */
int phx_lagrange_nodes(int cell_type, int degree, double *out, int64_t *n);
int phx_lagrange_tabulate(int cell_type, int degree, int64_t npts, const double *pts, double *out);
int phx_levelset_eval_points_deg(phx_mesh *m, int detection_degree, int levelset_degree, const double *nodal,
                                 int loc, double *out_device);
int phx_lagrange_dof_points(phx_mesh *m, int degree, double *out_device);

/* [host] Facet numbering and connectivities of an unstructured mesh: stands in for dolfinx
 * create_connectivity (mesh_scripts.py:151-153,419-422) and locate_entities_boundary (:430).
 * c2f[nc*nfpc], f2c[(max)nc*nfpc*2] are caller buffers; *nf receives the facet count. */
int phx_topology_build_host(int cell_type, int64_t nv, int64_t nc, const int32_t *cells,
                            int32_t *c2f, int32_t *f2c, int64_t *nf);

/* ------------------------------------------------------------------ mesh ------------- */
/* Unstructured mesh from caller arrays (host): replaces XDMFFile.read_mesh + connectivities
 * (tests/test_compute_meshtags.py:136-137).  Quadrilaterals in tensor-product order. */
int phx_mesh_create(int gdim, int cell_type, int64_t nv, const double *coords, int64_t nc,
                    const int32_t *cells, int device, phx_mesh **out);

/* Structured Kuhn/Freudenthal simplicial box generated ON THE DEVICE: replaces
 * dolfinx.mesh.create_rectangle / create_box (demo/weak-dirichlet/flower/main.py:45-46).
 * n[gdim] cubes per axis in this (sub-)box; vertex (i,j,k) sits at
 *   lo[a] + (hi[a]-lo[a]) * (double)(offset[a]+i) / (double)n_global[a]
 * so that a slab of a larger box (multi-GPU partition) reproduces the global coordinates bit
 * for bit.  offset/n_global may be NULL (= 0 / n). */
int phx_mesh_create_box(int gdim, const double *lo, const double *hi, const int64_t *n,
                        const int64_t *offset, const int64_t *n_global, int device,
                        phx_mesh **out);

/* Multi-GPU slabs: declare that the lower / upper end plane of the LAST axis of a device-generated
 * box is a cut through the global mesh, not part of its boundary.  Facets on such a plane stay
 * untagged (0) and take no part in the `ds` detection of mesh_scripts.py:434-461. */
int phx_mesh_set_slab_faces(phx_mesh *m, int lower_is_cut, int upper_is_cut);
int phx_mesh_destroy(phx_mesh *m);
/* Number of edges (builds the edge numbering on first use; needed for P2 spaces). */
int phx_mesh_edge_count(phx_mesh *m, int64_t *ne);
/* counts[6] = {gdim, cell_type, nv, nc, nf, nbf} */
int phx_mesh_counts(const phx_mesh *m, int64_t *counts);
/* Copy a mesh array out (to host or to a device buffer of the same GPU). */
int phx_mesh_get_array(phx_mesh *m, int which, void *out, int loc);
/* The HIP stream all work of this mesh is enqueued on (as uintptr). */
int phx_mesh_stream(phx_mesh *m, uint64_t *stream);
int phx_mesh_synchronize(phx_mesh *m);
/* Enqueue all further work of this mesh on a caller stream (e.g. torch's current stream, so that
 * torch.distributed collectives and the kernels order without extra synchronisation). */
int phx_mesh_set_stream(phx_mesh *m, uint64_t stream);
enum phx_option {
  PHX_OPT_PROFILE_SPMV = 1, /* k > 0: bracket every k-th SpMV launch of a solve with HIP events  */
  PHX_OPT_HAS_EXTERIOR = 2, /* -1: `len(exterior_cells) == 0` (mesh_scripts.py:469) is decided
                               from this mesh's tags; 0/1: imposed by a multi-GPU driver that
                               reduced it over all slabs                                        */
  PHX_OPT_SPMV_XCD_GROUP = 3, /* G > 0: SpMV blocks are regrouped so that each XCD (blockIdx % 8)
                               walks runs of G consecutive blocks; 0: plain order (default)      */
  PHX_OPT_PRECOND = 5, /* 1 (default): P1 Poisson systems on Kuhn boxes (2-D, 3-D) are preconditioned with the
                               lattice Laplacian of a box around the active vertices, inverted by f64 sine
                               transforms (u block; p block: Jacobi); 2: the same with f32 transforms -- 25 %
                               faster per application, but the half-length sine transform amplifies rounding
                               by O(L) and BiCGStab is not a flexible method: erratic on some problems
                               (2-D flower: 100-580 iterations against 38); 0: Jacobi everywhere          */
  PHX_OPT_EXPORT_CSR = 7, /* 1: systems assembled from now on ALSO keep the CSR copy phx_system_export
                               hands out (sorted columns, dolfinx sparsity pattern with its explicit zeros).
                               Default 0: the solver formats are built straight from the row slots and the CSR
                               is never formed for P1 weak-Dirichlet systems on Kuhn boxes -- export then
                               returns PHX_ERR_VALUE and the host re-assembles with this option set         */
  PHX_OPT_STRUCTURED = 8, /* 1 (default): P1 weak-Dirichlet systems on Kuhn boxes apply their
                               translation-invariant interior rows from a 7-point stencil over runs of
                               consecutive rows (no stored columns or values); only the rows near Gamma_h keep
                               SELL storage; P2 weak-Dirichlet systems on 3-D Kuhn boxes likewise (eight class
                               stencils, interior rows never assembled).  0: every row stored (SELL)          */
  PHX_OPT_DETERMINISTIC = 9, /* 1: bit-reproducible results for the scattering assemblies (P2 weak Dirichlet,
                               interface elasticity, P1 weak Dirichlet on meshes that are no Kuhn boxes -- boxes keep
                               plain atomics at P1) and the Krylov solve: the element kernels run twice and
                               accumulate exactly (per-slot exponent, two accumulators), the dot products are
                               summed in a fixed order.  Costs one more pass of the element kernels and 12 bytes
                               per row slot while assembling (skipped beyond PHX_DET_LIMIT_GB, default a fifth of the device memory).
                               Default 0: f64 atomics in arrival order (results equal to round-off)           */
  PHX_OPT_EL_COARSE = 10, /* coarse-space correction of the interface-elasticity solve on generated boxes (one rank):
                               Galerkin problem on trilinear functions of spacing H = value * h per displacement
                               block, added to the vertex-block Jacobi (the iteration count then follows H / h
                               instead of growing with the box).  -1 (default): on from 80 cubes per axis with
                               H ~ n / 8 (H = 16 h beyond 128 cubes); 0: off; >= 5: this ratio.  The dense inverse
                               of the coarse matrix is the library's own (phx_dense_inverse)                   */
  PHX_OPT_STENCIL_PLANE_ROWS = 11, /* structured P1 systems on 3-D boxes: from this many interior rows per lattice
                               plane on (default 32768: three planes of the vector no longer fit an XCD's L2 next to the
                               streams) the stencil blocks of the SpMV walk the k-th eighth of EVERY plane on XCD k
                               instead of the k-th eighth of all rows; 0: never.  Placement only: same product   */
  PHX_OPT_P2_COARSE = 12, /* two-level preconditioner of P2 weak-Dirichlet systems on generated Kuhn boxes (one rank):
                               the additive Galerkin correction R Ac^-1 R^T (multilinear functions of spacing H = value * h,
                               one set per field, Ac = R^T A R probed through the solver's own operator) on top of the
                               h/2-lattice sine transform on u and Jacobi on p.  0 (default): off; -1: automatic (ratio
                               and on/off chosen by the library); >= 5: this ratio; 1..4: PHX_ERR_VALUE.
                               Built on the first solve of a system; phx_coarse_info reports it            */
  PHX_OPT_BOX_TAGS = 13, /* 1 (default): generated 3-D Kuhn boxes are tagged by kernels that take one thread per cube
                               and the connectivity in closed form (cells, single-layer passes); 0: the generic
                               kernels that stream `cells` run on them too.  Same tags, bit for bit: 0 is the
                               reference path of tests/test_box_closed_form_tags.py                          */
  PHX_OPT_MULTILEVEL = 14, /* 1: P1 weak-Dirichlet systems of this mesh (triangles, tetrahedra; one rank) are
                               preconditioned with one geometric-multigrid V-cycle over the refinement hierarchy the
                               mesh carries (phx_mesh_refine / phx_mesh_refine_marked, down to the first mesh without a
                               living parent) on the u block and Jacobi on the p block: see phx_multilevel_setup.
                               Systems of any other kind on this mesh (degree 2, strong Dirichlet, elasticity,
                               quadrilaterals) are solved as without the option; a P1 weak-Dirichlet system that
                               cannot be served (no living parent, Kuhn box, sub-mesh, slab, ...) fails its solve
                               with the status phx_multilevel_setup reports.  0 (default): off, nothing changes  */
  PHX_OPT_ELWD_COARSE = 15, /* coarse-space correction of the weak-Dirichlet elasticity solve
                               (phx_assemble_elasticity_wd) on generated simplicial boxes, 2-D and 3-D, one rank: the
                               Galerkin problem of PHX_OPT_EL_COARSE on multilinear functions of spacing H = value * h,
                               one set per displacement component u_a (the p blocks have no coarse part), added to the
                               vertex-block Jacobi.  0 (default): off, vertex blocks alone; -1: automatic (ratio and
                               on/off chosen by the library); >= 5: this ratio; 1..4: PHX_ERR_VALUE.  Read
                               when a system is assembled (0: that system never builds one) and on its first solve;
                               phx_coarse_info reports the correction or why it was not built.  Independent of
                               PHX_OPT_EL_COARSE, which speaks of interface-elasticity systems only             */
  PHX_OPT_BOX_FACET_ROWS = 16, /* 1 (default): where a P1 weak-Dirichlet assembly on a Kuhn box addresses its stored rows
                               by lattice offset code (structured system, no CSR copy, not deterministic), the ghost
                               penalty is gathered per stored row from the facet tags, the per-type tables of
                               phx_box_facet_tables and the vertex coordinates, without atomics; 0: the facet kernel that scatters with f64
                               atomics runs there too.  Same matrix to round-off: 0 is the reference path of
                               tests/test_box_facet_rows.py                                                      */
  PHX_OPT_RED_SPMV = 17, /* 1 (default): the two stored-row products of the reduced BiCGStab loop (phases 57 / 60) run
                               k_spmv_red, a kernel that holds the stored-row branch of the SpMV alone; 0: k_spmv_sell
                               runs there too.  Same y_B, bit for bit, and dot-product partials of the same composition:
                               0 is the reference path of tests/test_hip_spmv_red.py                          */
  PHX_OPT_ALLOW_EMPTY = 6, /* 1: phx_assemble_poisson_wd returns an EMPTY system (n_active = 0) when no cell
                               is tagged 1 / 2 instead of PHX_ERR_VALUE: a slab of a partitioned box that
                               does not touch the domain still joins every collective of the solve          */
  PHX_OPT_SPMV_VALUE_INDEX = 4 /* 1 (default): systems assembled from now on store SELL slices whose
                               values take <= 64 distinct doubles as dictionary + byte codes
                               (bit-identical products, 5 instead of 12 bytes per entry); 0: raw */
};
int phx_set_option(phx_mesh *m, int option, int64_t value);
/* Direct solve of the 7-point lattice Laplacian K = sum_a (h_b h_c / h_a) tridiag(-1, 2, -1)_a with
 * homogeneous Dirichlet faces on an (L0-1) x (L1-1) x (L2-1) interior lattice (x fastest), by type-I sine
 * transforms on the device (f32 != 0: lattice array and transforms in single precision);
 * L_a in {64, 128, 192, 256, 384, 512, 768, 1024}.  u overwrites f (host).
 * This is the kernel sequence of the fictitious-domain preconditioner (PHX_OPT_PRECOND), exposed for tests. */
int phx_box_poisson_solve(int device, const int *L, const double *h, int f32, double *f_host);
/* Timing aid: average microseconds of the x, y and z (forward + divide + inverse) transform passes on an
 * (L0-1) x (L1-1) x (L2-1) lattice (tools/dst_bench.py). */
int phx_box_dst_bench(int device, const int *L, int f32, int reps, double *out_us3);
/* a_host (n x n, row-major, n <= 20000) := its inverse: the library's own dense inverse (blocked Gauss-Jordan elimination
 * with partial pivoting, phx_dense.inc.hip) that the elasticity coarse correction applies to its Galerkin matrix -- exposed
 * for tests.  *singular = 1: a pivot column vanished (a_host is then undefined).  The reference has no counterpart (MUMPS
 * factorises the whole system, demo/interface-elasticity/main.py:283-289). */
int phx_dense_inverse(int device, int64_t n, double *a_host, int *singular);
/* Mean elapsed time of an empty HIP event pair on the mesh stream: the cost the bracketing of
 * PHX_OPT_PROFILE_SPMV adds to each timed launch (measurement aid of bench.py). */
int phx_event_pair_overhead(phx_mesh *m, double *seconds);
/* Tag counts of the current tagging: cells4[t] for t = 0..3, facets7[t] for t = 0..6. */
int phx_mesh_tag_histogram(const phx_mesh *m, int64_t *cells4, int64_t *facets7);

/* ------------------------------------------------------------------ tagging ---------- */
/* _tag_cells (mesh_scripts.py:284-390) incl. _compute_detection_vector (:95-134):
 * tags 1 inside / 2 cut / 3 outside, optional single-layer demotion (:349-358).
 * warn_zero_denominator (may be NULL) receives 1 when some cell's denominator is ~0 (the
 * RuntimeWarning of :129-133). */
int phx_tag_cells(phx_mesh *m, int phi_kind, const double *phi, int loc, int detection_degree,
                  int single_layer_cut, int *warn_zero_denominator);

/* _tag_facets (mesh_scripts.py:393-558), tags 1..6, from the cell tags currently held by the
 * mesh; the `ds` detection of the background-boundary facets (:434-461) uses the same phi.
 * Fails with PHX_ERR_PARTITION when the reference's sets do not partition the facets. */
int phx_tag_facets(phx_mesh *m, int phi_kind, const double *phi, int loc, int detection_degree);

/* User overwrite of tags (_overwrite_tags, mesh_scripts.py:561-568, value checks :606-615). */
int phx_overwrite_tags(phx_mesh *m, int entity_is_facet, int64_t n, const int32_t *indices,
                       const int32_t *values);
/* Install externally computed dense tags (tests, multi-GPU ghost exchange). */
int phx_set_tags(phx_mesh *m, int entity_is_facet, const int32_t *values, int loc);

/* [host] The three selections whose per-chunk counts the tagging kernels leave behind, as the assembly and the entity
 * collection make them: which = 0 cut cells (tag 2), 1 ghost-penalty facets (tag 2 / 3 with two cells), 2 facets tagged
 * 3 / 4.  Ascending entity indices; out may be NULL to ask for *count alone (at most nc resp. nf entries). */
int phx_mesh_selection(phx_mesh *m, int which, int32_t *out, int64_t *count);
/* _compute_integration_entities (mesh_scripts.py:137-192) for the two one-sided measures of
 * compute_tags_measures (:617-626): which = 100 -> facets tagged 4 seen from cells {1,2};
 * which = 101 -> facets tagged 3 seen from cells {2,3}.  Flat [cell, local facet, ...] in the
 * reference's order.  Count-then-fill on *n_pairs (out may be NULL). */
int phx_integration_entities(phx_mesh *m, int which, int32_t *out, int64_t *n_pairs);

/* Sub-mesh of the cells tagged 1 or 2 with transferred tags: dolfinx create_submesh +
 * _transfer_tags (mesh_scripts.py:217-281,636-645).  c_map[ncs], v_map[nvs] are count-then-fill
 * (pass NULL first, sizes come back in counts of *sub). */
int phx_submesh_create(phx_mesh *m, phx_mesh **sub);
int phx_submesh_maps(phx_mesh *sub, int32_t *c_map, int32_t *v_map);

/* --- partition of an unstructured background mesh over ranks (triangles, tetrahedra) ---------
 * No counterpart in the reference (serial, src/phifem/mesh_scripts.py:264).  Every rank holds the WHOLE mesh, calls
 * these redundantly and obtains the same bits; tests/partition_ref.py restates the rules in numpy.
 *
 * Recursive coordinate bisection of the cell centroids into nparts <= 4096 parts: part[nc] (int32).  weights[nc]:
 * non-negative int32, NULL = all ones.  Centroid = vertex coordinates summed in local-vertex order, then divided by the
 * vertex count.  A part range [p0, p1) over its cells S splits along the first axis of largest centroid extent; S is
 * ordered by (coordinate, cell index) and the left (p1 - p0) / 2 parts take the shortest prefix whose weight w satisfies
 * w (p1 - p0) >= W (p1 - p0) / 2 (integer arithmetic, W = weight of S).  One pass per level on the device: segmented
 * min / max, two stable radix sorts, one weighted scan; nothing returns to the host in between.  loc: where weights and
 * part live. */
int phx_partition_cells(phx_mesh *m, int nparts, const int32_t *weights, int32_t *part, int loc);
/* Ownership and local cells of `rank` for a partition of the TAGGED mesh.  owner[nv] (int32): part of the
 * lowest-numbered cell tagged 1 or 2 that contains the vertex, -1 for vertices of exterior cells only.  flags[nc]
 * (uint8), the first layer that takes the cell: 1 = a cell with a vertex the rank owns; 2 = a facet neighbour of a
 * layer-1 cell (a ghost-penalty facet couples all DoFs of its two cells, so the rows of owned vertices reach that far);
 * 3 = a cell with a vertex of layers 1 - 2; 4 = a facet neighbour of a layer-3 cell (the solver scales every column by
 * its diagonal entry, so the diagonal of each column an owned row refers to has to be complete as well); 0 = not local.
 * A rank that owns nothing gets one placeholder cell (flag 2): the lowest-numbered cell not tagged 1 / 2, else cell 0.
 * Either output may be NULL.  loc: where part, owner and flags live. */
int phx_partition_layout(phx_mesh *m, int nparts, const int32_t *part, int rank, int32_t *owner, uint8_t *flags, int loc);
/* Local mesh of the cells with flags[nc] != 0: cells and vertices ascending in the parent's numbering (maps through
 * phx_submesh_maps), the parent's cell and facet tags transferred, never recomputed.  Unlike phx_submesh_create the
 * result is a BOX-MODE mesh: the facets on its rim are cuts, not boundary -- assemble with the transferred tags. */
int phx_submesh_create_from_flags(phx_mesh *m, const uint8_t *flags, int loc, phx_mesh **sub);

/* --- uniform regular refinement and the nested coarse -> fine transfer ----------------------
 * Stands in for dolfinx.mesh.refine (demo/interface-elasticity/main.py:390) with red (2-D) / Bey (3-D) refinement;
 * tests/refine_ref.py restates the rules in numpy.  Purely topological: no float is compared.
 *
 * Fine vertices = the degree-2 Lagrange DoF points of the coarse mesh in the layout above, computed by the kernel of
 * phx_lagrange_dof_points(m, 2): coarse vertex v stays v; simplices: the midpoint of edge e is nv + e; quadrilaterals:
 * the midpoint of facet f is nv + f, the centre of cell c is nv + nf + c.
 * Child k of coarse cell c is fine cell nchild * c + k (parent of a fine cell = cell / nchild).  Children in LOCAL
 * degree-2 nodes -- 0 .. nvpc-1 the cell's vertices as stored, nvpc + k its local edge k (basix order, PHX_ARR_C2E) or
 * local facet k (quadrilaterals), last the quadrilateral's centre; m_ij = node of the edge (i, j):
 *   triangle       (v0, m01, m02) (m01, v1, m12) (m02, m12, v2) (m12, m02, m01)
 *   tetrahedron    Bey's rule, interior diagonal m02 - m13:
 *                  (v0, m01, m02, m03) (m01, v1, m12, m13) (m02, m12, v2, m23) (m03, m13, m23, v3)
 *                  (m01, m02, m03, m13) (m01, m02, m12, m13) (m02, m03, m13, m23) (m02, m12, m13, m23)
 *   quadrilateral  b, l, r, t = midpoints of local facets 0..3, ctr the centre (tensor-product order kept):
 *                  (v0, b, l, ctr) (b, v1, ctr, r) (l, ctr, v2, t) (ctr, r, t, v3)
 * Children need not keep the parent's orientation sign.
 *
 * phx_mesh_refine: *fine is an ordinary untagged mesh with its own stream, facet numbering and boundary list,
 * remembering which mesh it was refined from.  When a lattice stands behind the coarse mesh (generated boxes, caller
 * meshes recognised as lattices) the fine arrays are read back once and the fine mesh is what phx_mesh_create makes of
 * them (same lattice detection, same generated box or lattice copy behind it); for every other mesh no mesh array
 * returns to the host in this call.  PHX_ERR_VALUE: slab with declared cut faces (phx_mesh_set_slab_faces), fine
 * counts beyond the 32-bit id limits (checked before anything is allocated); PHX_ERR_NOT_IMPLEMENTED: other cell types.
 *
 * phx_prolongate: in[ncomp][coarse ndofs(degree)] -> out[ncomp][fine ndofs(degree)], component-major, at loc_in /
 * loc_out.  The Lagrange spaces are nested: the fine function equals the coarse one pointwise.  `fine` must be the
 * direct result of phx_mesh_refine(coarse), else PHX_ERR_VALUE.
 *   degree 1 (all three cell types): copy at coarse vertices, 0.5 u_p + 0.5 u_q at midpoints,
 *     ((0.25 u0 + 0.25 u1) + 0.25 u2) + 0.25 u3 at quadrilateral centres -- bit for bit the coordinate arithmetic.
 *   degree 2 (simplices): fine vertex DoFs are copies of the coarse vertex / edge DoFs; a fine edge DoF is the parent
 *     cell's P2 function at the fine edge's midpoint, sum_d w[d] u[dof d of the parent] over the parent's local DoFs d
 *     in ascending LOCAL order with zero weights skipped (weights 0, -1/8, 1/4, 3/8, 1/2, 3/4).
 *     DETERMINISM RULE: a fine edge seen from several parent cells is written by the LOWEST-NUMBERED parent cell (an
 *     integer min pass, then one write pass; no floating-point atomics), so every run gives the same bits.
 *   PHX_ERR_NOT_IMPLEMENTED: degree 2 on quadrilaterals, degree 3.
 * Both calls release every temporary on failure (phx_pool_stats live bytes return to where they were).
 *
 * [host] phx_refine_tables: children[nchild][nvpc] in the local nodes above, *nchild, and for simplices
 * p2_weights[nchild][nepc][ndof2] (ndof2 = nvpc + nepc): the weights of child k's local edge j (basix order on the
 * child's vertices).  Any output may be NULL. */
int phx_mesh_refine(phx_mesh *m, phx_mesh **fine);
int phx_prolongate(phx_mesh *coarse, phx_mesh *fine, int degree, int ncomp, const double *in, int loc_in,
                   double *out, int loc_out);
int phx_refine_tables(int cell_type, int32_t *children, int *nchild, double *p2_weights);

/* --- marked refinement of triangle and tetrahedron meshes ------------------------------------
 * Stands in for dolfinx.mesh.refine with marked edges (longest-edge bisection with closure); tests/refine_marked_ref.py
 * restates the rule in numpy, and the device result equals it bit for bit.
 *
 * cell_marks[nc], edge_marks[ne] (uint8, non-zero = marked, at `loc`; edge ids as PHX_ARR_EDGES / PHX_ARR_C2E, in 2-D
 * the edges are the facets); either may be NULL.  Both NULL: a copy, one child per cell.
 *
 * EDGE ORDER, strict and total: the key of edge (p, q), p < q, is len2 = ((dx dx + dy dy) + dz dz), d = x[q] - x[p],
 * evaluated without contraction.  The greater len2 wins; on equal len2 the lexicographically smaller (p, q) wins.  It
 * depends on coordinates and vertex ids only.
 *   1. Seed: a marked cell marks all its edges; the edge mask is OR-ed in.
 *   2. Closure, the least fixed point of: every cell with a marked edge gets its greatest edge marked; in 3-D every
 *      face with a marked edge gets its greatest edge marked.  (Monotone: independent of sweep order and races.  One
 *      lane per cell and sweep, marks are byte stores of 1, the host reads one 4-byte flag per sweep.)
 *   3. Subdivision: a sub-simplex is a tuple of nvpc local degree-2 nodes of the coarse cell (0 .. nvpc-1 its vertices,
 *      nvpc + k the midpoint of local edge k), starting with (0, .., nvpc-1).  While it holds both end nodes of a
 *      marked coarse edge: take the greatest such edge, at positions i < j, m its midpoint node; child 0 is the tuple
 *      with position j replaced by m, child 1 with position i replaced by m.  Depth first, child 0 first; the leaves in
 *      the order reached are the children: 1-4 per triangle, 1-8 per tetrahedron.  How a face is split depends only on
 *      its own marked edges and the order, so neighbours agree: the result is conforming.  Orientation signs are not
 *      kept.
 *   4. Numbering: fine vertex v < nv is coarse vertex v; the midpoint 0.5 x_p + 0.5 x_q of marked edge e is nv + rank(e),
 *      the rank among the marked edges by ascending id.  The children of cell c are the fine cells off[c] .. off[c+1]-1,
 *      off the exclusive sum of the child counts.
 *   5. *fine is an ordinary untagged mesh (never a lattice, whatever stood behind the coarse one) that remembers the
 *      mesh it came from and carries PHX_ARR_PARENT_CELLS and PHX_ARR_CHILD_NODES (the leaf tuples).
 * info (nullable) = {marked edges after the closure, closure sweeps run, fine cells}.
 * PHX_ERR_NOT_IMPLEMENTED: quadrilaterals (hanging nodes); PHX_ERR_VALUE: slab with declared cut faces, counts of the
 * all-marked case beyond the 32-bit id limits (checked before anything is allocated).  Temporaries are released on
 * every exit (phx_pool_stats live bytes return to where they were).
 *
 * phx_prolongate accepts such a fine mesh (simplices, degree 1 and 2):
 *   degree 1: copy at the coarse vertices, 0.5 u_p + 0.5 u_q at the new ones -- the coordinate arithmetic.
 *   degree 2: the first nv values are copies, fine vertex nv + rank(e) copies the coarse edge DoF of e; a fine edge DoF
 *     is the parent's P2 function at the fine edge's midpoint: lambda = mean of the barycentrics of its two child
 *     nodes, weights lambda_i (2 lambda_i - 1), 4 lambda_i lambda_j (exact: all lambda are multiples of 1/4), summed
 *     over the parent's local DoFs in ascending order with zero weights skipped.  The LOWEST-NUMBERED parent cell that
 *     contains the fine edge writes it (integer min pass, then a write pass): the same bits on every run. */
int phx_mesh_refine_marked(phx_mesh *m, const uint8_t *cell_marks, const uint8_t *edge_marks, int loc, phx_mesh **fine,
                           int64_t *info);

/* --- restriction: the transpose of the degree-1 phx_prolongate -------------------------------
 * in[ncomp][fine nv] -> out[ncomp][coarse nv], component-major, at loc_in / loc_out: <phx_restrict(r), x> =
 * <r, phx_prolongate(x)>.  Triangles and tetrahedra, `fine` the direct result of phx_mesh_refine(coarse) or of
 * phx_mesh_refine_marked(coarse) (fine vertex v < nv is coarse vertex v in both; a uniformly refined lattice mesh is
 * re-created through phx_mesh_create and keeps that numbering).
 *   ORDER RULE: out[p] = ((in[p] + 0.5 in[m_1]) + 0.5 in[m_2]) + ..., m_1 < m_2 < ... the new fine vertices on the
 *   bisected coarse edges that end in p, by ascending fine vertex id, added left to right without contraction.  It is a
 *   gather through an integer CSR (coarse vertex -> dependent fine vertices) built once per fine mesh with the stable
 *   radix sort and freed with the fine mesh; no floating-point atomics: the same bits on every run, and bit for bit
 *   tests/multilevel_ref.py.
 * PHX_ERR_NOT_IMPLEMENTED: degree 2, quadrilaterals; PHX_ERR_VALUE: `fine` is not the direct child of `coarse`.
 * Temporaries are released on every exit. */
int phx_restrict(phx_mesh *coarse, phx_mesh *fine, int degree, int ncomp, const double *in, int loc_in, double *out,
                 int loc_out);

/* --- point location and evaluation of Lagrange functions at arbitrary points -----------------
 * Stands in for dolfinx's Function.eval with a bounding-box tree and for interpolate_nonmatching;
 * tests/locate_ref.py restates the rules in numpy.
 *
 * Reference coordinates of a point in a cell: simplices lambda_1 .. lambda_d of the STORED vertex order (lambda_0 =
 * 1 - sum); axis-parallel rectangles (xi, eta) in tensor-product order.  A cell holds a point when every barycentric
 * coordinate is >= -tol (rectangles: xi, eta in [-tol, 1 + tol]).
 *
 * phx_locate_points: pts[npts][gdim] at `loc` -> cells_out[npts] (-1: no cell holds the point) and
 * xref_out[npts][tdim] (zeros where the cell is -1; callers must not rely on that) at loc_out.
 *   Generated boxes (phx_mesh_create_box, slabs included) take a CLOSED FORM: cube = clamped floor((x - lo) / h)
 *   corrected against the lattice planes, simplex = the ordering of the local coordinates, cell id = the generator's
 *   numbering.  No search structure is built, no connectivity is read.  Tie rules: a point on a lattice plane belongs
 *   to the cube above it, on the upper faces of the box to the last cube; among equal local coordinates the lower axis
 *   goes first (the lowest-numbered simplex of that cube that holds the point).
 *   Every other mesh (rectangles included) is searched through BINS: a uniform grid over the bounding box with about
 *   one bin per cell, (bin, cell) pairs built as count -> scan -> fill with integer atomics and 64-bit offsets.  When the
 *   pairs exceed 16 nc the bins per axis are halved and the count runs again (deterministic).  The structure belongs to
 *   the mesh: built on first use on the mesh's stream (again when a call asks for a larger tol), freed with the mesh.
 *   DETERMINISM RULE: of all cells that hold the point the one with the SMALLEST cell index wins; the result depends
 *   neither on the fill order of the bins nor on the order of the points.
 *   PHX_ERR_VALUE: tol < 0; PHX_ERR_NOT_IMPLEMENTED: a quadrilateral that is no axis-parallel rectangle in
 *   tensor-product order.
 *
 * phx_eval_points: values[ncomp][ndofs(degree)] at loc_v (the layout phx_solve returns per field), cells[npts] and
 * xref[npts][tdim] at loc_p as phx_locate_points wrote them -> out[ncomp][npts] and, with want_grad, the physical
 * gradient in that cell grad_out[ncomp][npts][gdim], at loc_out; `fill` where the cell is -1 (or out of range).
 *   degree 1: triangles, tetrahedra, rectangles (Q1); degree 2: simplices, vertices then the edges of PHX_ARR_C2E.
 *   One lane per point; sums run in ascending local DoF order, so results repeat bit for bit.
 *   PHX_ERR_NOT_IMPLEMENTED: degree 2 on quadrilaterals, degree 3, non-rectangular quadrilaterals.
 *
 * Both calls release every temporary on failure (phx_pool_stats live bytes return to where they were); what stays
 * after a successful phx_locate_points is the locator, reported by phx_locator_info.
 *
 * [host] phx_locator_info: info[8] = {path: 1 closed form / 2 bins, bins along x, y, z, stored (bin, cell) pairs,
 * device bytes held, halvings of the resolution, 1 when the bins are built}; a closed-form mesh reports zeros after
 * the path.
 * [host] phx_locate_timings: t[3] = wall seconds of the last locator build, of the last phx_locate_points without
 * the build, and of the last phx_eval_points (each call ends with the stream synchronised). */
int phx_locate_points(phx_mesh *m, int64_t npts, const double *pts, int loc, double tol, int32_t *cells_out,
                      double *xref_out, int loc_out);
int phx_eval_points(phx_mesh *m, int degree, int ncomp, const double *values, int loc_v, int64_t npts,
                    const int32_t *cells, const double *xref, int loc_p, int want_grad, double fill, double *out,
                    double *grad_out, int loc_out);
int phx_locator_info(const phx_mesh *m, int64_t *info);
int phx_locate_timings(const phx_mesh *m, double *t);

/* ------------------------------------------------------------------ assembly --------- */
/* Weak-Dirichlet phi-FEM Poisson, mixed (u,p) in P1 x P1: bilinear form
 * demo/weak-dirichlet/flower/main.py:112-135 + assemble_matrix :137-139, linear form :142-151 +
 * assemble_vector :153-154, on the tags currently held by the mesh (dx((1,2)), dx(2), dS((2,3)),
 * ds = ds(100) in box mode or all exterior facets on a sub-mesh).
 * phi_h, f_h, u_D: nodal P1 arrays [nv].  Only the active DoFs (rows touched by an integral)
 * are stored.  Quadrilateral meshes: Q1 x Q1 with Q1 nodal arrays [nv] on axis-parallel rectangles in
 * tensor-product vertex order (same DoF layout and active set); any other quadrilateral returns
 * PHX_ERR_NOT_IMPLEMENTED. */
int phx_assemble_poisson_wd(phx_mesh *m, double pen_coef, double stab_coef, const double *phi_h,
                            const double *f_h, const double *u_D, int loc, phx_system **out);
/* [host] The facet classes of a Kuhn box of uniform spacings h[gdim] behind PHX_OPT_BOX_FACET_ROWS: *ntypes = 12 (3-D)
 * or 3 (2-D) facet types in the generator's numbering (facet id = base[type] + anchor index).  cells and offsets are the
 * tables the row kernel walks; J and w are what its closed form gives where every cube has the spacings h (the kernel
 * takes each facet's spacings from the vertex coordinates, as the scattering kernel does).  Per type t:
 *   cells[2 t + side]                 the two simplices of the facet as axis-permutation indices (cell = cube * nper +
 *                                     index); the first one lies in the cube below the anchor for the types in a
 *                                     plane x_a = const, in the anchor cube otherwise, the second one in the anchor cube
 *   offsets[(t (gdim + 2) + l) gdim + a]  the gdim + 2 vertices of the macro-element as lattice offsets from the anchor:
 *                                     the gdim + 1 vertices of the first cell, then the vertex of the second cell
 *                                     opposite the facet
 *   J[t (gdim + 2) + l]               jump of the normal derivative of the hat function of vertex l across the facet
 *                                     (a shared vertex carries both one-sided terms; exactly 0.0 where it vanishes)
 *   w[t]                              stab_coef avg(h) |F| with h the cell diameter (main.py:129-134)
 * Entry (l, m) of the facet tensor is w[t] J[l] J[m].  Any output may be NULL.  PHX_ERR_VALUE if the tables do not
 * fit the lattice offset codes of the row slots (a library defect). */
int phx_box_facet_tables(int gdim, const double *h, double stab_coef, int *ntypes, int32_t *cells, int32_t *offsets,
                         double *J, double *w);
/* The same forms with primal_degree = auxiliary_degree = 2 (BASELINE configs[2]); the
 * div(grad(.)) terms of main.py:123-128,150 are live.  DoFs per field: vertex v -> v, edge e ->
 * nv + e (PHX_ARR_EDGES / PHX_ARR_C2E), p block shifted by nv + ne.  f_h, u_D: nodal P2 arrays
 * [nv + ne]; phi_h: [nv] if phi_degree == 1, [nv + ne] if 2. */
int phx_assemble_poisson_wd_p2(phx_mesh *m, double pen_coef, double stab_coef, const double *phi_h,
                               int phi_degree, const double *f_h, const double *u_D, int loc,
                               phx_system **out);
/* Strong-Dirichlet ("direct") phi-FEM Poisson, u_h = phi_h w_h, one scalar field w of Lagrange
 * degree 1 or 2: bilinear form demo/strong-dirichlet/flower/main.py:104-117 + assemble_matrix
 * :120-121, linear form :125-129, on the tags held by the mesh (dx((1,2)), dx(2), dS((2,3)), ds =
 * ds_bdy(100) on the background mesh :60-65 or all exterior facets of a sub-mesh :70).  f_h: nodal
 * array of the w space ([nv], or [nv + ne] at degree 2); phi_h: [nv] if phi_degree == 1, [nv + ne]
 * if 2.  The system holds the active w DoFs only (n_active_u == n_active, n_full = DoFs of the
 * space); the caller forms u_h = w_h phi_h at the nodes of its solution space (main.py:176-182). */
int phx_assemble_poisson_sd(phx_mesh *m, double stab_coef, int degree, const double *phi_h,
                            int phi_degree, const double *f_h, int loc, phx_system **out);
/* Neumann / Robin phi-FEM Poisson (-lap u + u = f, du/dn + kappa u = g on the boundary), mixed (u, y, p) in
 * P1 x P1^d x DG0 with a P2 level-set, on simplices: forms demo/robin/square/main.py:112-168 + assemble_matrix /
 * assemble_vector :145-147,167-168; kappa = 0 with facet_tag = 3 is the formulation of
 * demo/neumann/square/main.py:113-158.  QUADRILATERAL meshes (the cell type of that demo, :49-50; axis-parallel
 * rectangles in tensor-product vertex order, else PHX_ERR_NOT_IMPLEMENTED) are assembled as Q1 x Q1^2 x DG0 with a Q2
 * level-set: phi_h[nv + nf + nc] = vertex values, edge-midpoint values by facet id, cell-centre values; the cut-cell
 * integrals then use a tensor Gauss rule of quadrature_degree / 2 + 1 points per direction.
 * params = {pen_coef, stab_coef, robin_coef}; facet_tag: the interior facets carrying the gradient-jump term
 * (2 in the Robin demo :140, 3 in the Neumann demo :134); quadrature_degree: degree of the cut-cell rule
 * (|grad phi_h| is not polynomial; 10 = UFL's estimate for the Robin integrand).  phi_h: [nv + ne] (P2: vertex
 * values, then edge values), f_h, g_h (u_N / u_R): [nv].  DoFs in the full numbering: u at vertex v -> v,
 * y_k at vertex v -> (1 + k) nv + v, p on cell c -> (1 + gdim) nv + c; n_full = (1 + gdim) nv + nc. */
int phx_assemble_poisson_flux(phx_mesh *m, const double *params, int facet_tag, int quadrature_degree,
                              const double *phi_h, const double *f_h, const double *g_h, int loc,
                              phx_system **out);
/* Interface linear elasticity, 5-field mixed phi-FEM (u_in, u_out, y_in, y_out, p), all P1:
 * demo/interface-elasticity/main.py:179-235 (bilinear form) + assemble_matrix(bcs) :237-239, linear
 * form :255-269 + apply_lifting / bc.set :271-277, material law data.py:5-36, on the tags held by
 * the mesh (box mode: dx((1,2)), dx((2,3)), dx(2), dS(3), dS(4), d_bdry(100), d_bdry(101)).
 *   params[6] = {E_in, nu_in, E_out, nu_out, penalization_coefficient, stabilization_coefficient}
 *   phi_h[nv]; f_h, u_D: [d*nv] component-major nodal vector fields; bc_vertices[nbc]: vertices
 *   where u_in = u_D is imposed (main.py:158-177).
 * DoF layout: component-major blocks of nv: u_in[a] -> a, u_out[a] -> d+a, y_in[a][b] -> 2d+a d+b,
 * y_out[a][b] -> 2d+d^2+a d+b, p[a] -> 2d+2d^2+a; phx_solve returns x[(2d+2d^2+d)*nv]. */
int phx_assemble_elasticity_if(phx_mesh *m, const double *params, const double *phi_h,
                               const double *f_h, const double *u_D, const int32_t *bc_vertices,
                               int64_t nbc, int loc, phx_system **out);
/* Weak-Dirichlet linear elasticity, one material, displacement prescribed on {phi = 0}: mixed (u, p) in
 * P1^d x P1^d on triangles / tetrahedra, the vector analogue of phx_assemble_poisson_wd (forms
 * demo/weak-dirichlet/flower/main.py:112-135, 142-151 with sigma(u) : eps(v), (sigma(u) n) . v and the jump of
 * sigma(u) n in place of the gradient terms; material law demo/interface-elasticity/data.py:5-36, plane strain in
 * 2-D), on the tags held by the mesh (dx((1,2)), dx(2), dS((2,3)), ds = ds_bdy(100) in box mode or every exterior
 * facet of a sub-mesh).  The coefficients are not rescaled by E.
 *   params[4] = {E, nu, pen_coef, stab_coef}
 *   phi_h[nv]; f_h, u_D: [d*nv] component-major nodal vector fields (host or device, `loc`).
 * DoF layout: component-major blocks of nv: u[a] -> a, p[a] -> d+a; n_full = 2 d nv.  Active: u on the vertices of
 * cells tagged 1 / 2, p on the vertices of cells tagged 2.  phx_solve preconditions with the vertex blocks.
 * Quadrilateral meshes, slabs and partitioned ranks: PHX_ERR_NOT_IMPLEMENTED.  Rows longer than the last slot
 * capacity (2-D: 64, 128, 256; 3-D: 128, 256, 512): PHX_ERR_CAPACITY. */
int phx_assemble_elasticity_wd(phx_mesh *m, const double *params, const double *phi_h, const double *f_h,
                               const double *u_D, int loc, phx_system **out);
/* Reaction-diffusion c u - Lap u = f + c g in the P1 x P1 weak-Dirichlet scheme of phx_assemble_poisson_wd (same
 * tags, DoF layout, active set, "inactive DoFs = 0"), c = `reaction` >= 0 a constant -- one implicit time step of the
 * heat equation (backward Euler: c = 1 / dt, g = u^n; BDF2: c = 3 / (2 dt), g = (4 u^n - u^{n-1}) / 3):
 *   a = a_Poisson + c (u, v)_{dx(1,2)} + stab c^2 h_T^2 (u, v)_{dx(2)}
 *   L = L_Poisson(f + c g; u_D) + stab c h_T^2 (f + c g, v)_{dx(2)}
 * with the consistent mass (1 + delta_ij) |T| / ((d+1)(d+2)).  g_h may be NULL (= 0).  The system stores every row
 * (never stencil-coded, no detour over the generated box behind a caller-supplied Kuhn mesh) and keeps (reaction,
 * pen_coef, stab_coef) for phx_system_update_rhs, which also produced its right-hand side.  phx_solve treats it as a
 * P1 Poisson system that is not stencil-coded (lattice preconditioner where the mesh has a lattice, else Jacobi).
 * reaction < 0 or not finite: PHX_ERR_VALUE.  Quadrilaterals, slabs and partitioned ranks: PHX_ERR_NOT_IMPLEMENTED. */
int phx_assemble_reaction_wd(phx_mesh *m, double pen_coef, double stab_coef, double reaction, const double *phi_h,
                             const double *f_h, const double *g_h, const double *u_D, int loc, phx_system **out);
/* Overwrites the right-hand side of a phx_assemble_reaction_wd system with L above for new data (on the tags the mesh
 * holds) and leaves the matrix alone: one lane per active vertex gathers its u and p row over the vertex star in a
 * fixed order, no atomics -- the same data give the same bytes.  Serves phx_assemble_diffusion_wd and phx_assemble_convection_wd systems too
 * (with the kappa_h / beta_h of their assembly).  Any other system: PHX_ERR_VALUE. */
int phx_system_update_rhs(phx_system *s, const double *phi_h, const double *f_h, const double *g_h,
                          const double *u_D, int loc);
/* Variable-coefficient diffusion c u - div(kappa grad u) = f + c g in the same P1 x P1 weak-Dirichlet setting (tags,
 * DoF layout, active set, "inactive DoFs = 0" of phx_assemble_poisson_wd / phx_assemble_reaction_wd).  kappa_h is a
 * nodal P1 field, finite and > 0 (checked on the device before anything is built: PHX_ERR_VALUE), c = `reaction` >= 0 a
 * constant, F = f + c g, kb_T / kb_F the mean of kappa_h over the vertices of a cell / facet:
 *   a = (kappa grad u, grad v)_{dx(1,2)} + c (u, v)_{dx(1,2)} - (kappa d_n u, v)_{ds(100)}
 *     + pen kb_T h_T^-2 (u - phi p / h_T, v - phi q / h_T)_{dx(2)}
 *     + stab h_T^2 / kb_T (c u - grad kappa . grad u, c v - grad kappa . grad v)_{dx(2)}
 *     + stab avg(h) (kappa [d_n u], [d_n v])_{dS(2,3)}
 *   L = (F, v)_{dx(1,2)} + pen kb_T h_T^-2 (u_D, v - phi q / h_T)_{dx(2)}
 *     + stab h_T^2 / kb_T (F, c v - grad kappa . grad v)_{dx(2)}
 * kappa_h = 1 gives the system of phx_assemble_reaction_wd.  g_h may be NULL (= 0).  Every row is stored; the system
 * keeps a device copy of kappa_h (released with it) and serves phx_system_update_rhs, which also produced its
 * right-hand side.  phx_solve: lattice preconditioner (plain lattice Laplacian) where the mesh has a lattice and
 * max kappa_h / min kappa_h <= 50, else Jacobi.  Quadrilaterals, slabs and partitioned ranks: PHX_ERR_NOT_IMPLEMENTED. */
int phx_assemble_diffusion_wd(phx_mesh *m, double pen_coef, double stab_coef, double reaction, const double *kappa_h,
                              const double *phi_h, const double *f_h, const double *g_h, const double *u_D, int loc,
                              phx_system **out);
/* Convection-diffusion c u + beta . grad u - div(kappa grad u) = f + c g in the same P1 x P1 weak-Dirichlet setting (tags,
 * DoF layout, active set, "inactive DoFs = 0" of phx_assemble_diffusion_wd).  beta_h[nv][d] is a nodal P1 vector field,
 * vertex-major like the coordinates, finite (checked on the device before anything is built: PHX_ERR_VALUE); kappa_h as
 * for phx_assemble_diffusion_wd; c = `reaction` >= 0 and supg_coef >= 0 constants (else PHX_ERR_VALUE).  With
 * L u = c u + beta . grad u - grad kappa . grad u, bb_T / bb_F the mean of beta_h over the vertices of a cell / facet,
 * ks_T = kb_T + h_T |bb_T|, ks_F = kb_F + avg(h) |bb_F| and tau_T = h_T^2 / ks_T:
 *   a = (kappa grad u, grad v)_{dx(1,2)} + c (u, v)_{dx(1,2)} + (beta . grad u, v)_{dx(1,2)} - (kappa d_n u, v)_{ds(100)}
 *     + supg tau_T (L u, beta . grad v)_{dx(1,2)}
 *     + pen ks_T h_T^-2 (u - phi p / h_T, v - phi q / h_T)_{dx(2)} + stab tau_T (L u, L v)_{dx(2)}
 *     + stab avg(h) |F| ks_F ([d_n u], [d_n v])_{dS(2,3)}
 *   L = (F, v)_{dx(1,2)} + supg tau_T (F, beta . grad v)_{dx(1,2)} + pen ks_T h_T^-2 (u_D, v - phi q / h_T)_{dx(2)}
 *     + stab tau_T (F, L v)_{dx(2)}
 * beta_h = 0 gives the system of phx_assemble_diffusion_wd for any supg_coef.  g_h may be NULL (= 0).  Every row is
 * stored; the system keeps device copies of kappa_h and beta_h (released with it) and serves phx_system_update_rhs, which
 * also produced its right-hand side.  phx_solve: lattice preconditioner where the mesh has a lattice,
 * max kappa_h / min kappa_h <= 50 and pe_max = max_T h_T |bb_T| / kb_T <= PHX_CD_LATTICE_MAX_PECLET, else Jacobi.
 * Quadrilaterals, slabs and partitioned ranks: PHX_ERR_NOT_IMPLEMENTED. */
int phx_assemble_convection_wd(phx_mesh *m, double pen_coef, double stab_coef, double supg_coef, double reaction,
                               const double *kappa_h, const double *beta_h, const double *phi_h, const double *f_h,
                               const double *g_h, const double *u_D, int loc, phx_system **out);
/* out[4] = {pe_max, max |beta_v|, supg_coef, max kappa_h / min kappa_h} of a phx_assemble_convection_wd system; any other
 * system: PHX_ERR_VALUE. */
int phx_convection_info(const phx_system *s, double *out);
int phx_system_destroy(phx_system *s);
/* info[14] = {n_active, n_active_u, nnz (structural, CSR), n_full (= 2*nv), sell_padded_nnz,
 *             slot_capacity, sell_nnz (explicit zeros dropped), n_slices, value-indexed slices,
 *             matrix bytes one SpMV of the solve streams (columns + value stream + slice table),
 *             value-indexed slices whose dictionary exceeds 64 entries (LDS look-up),
 *             rows applied from the stencil (structured systems, else 0), stencil runs,
 *             1 if the system holds its CSR copy (phx_system_export can return the matrix)} */
int phx_system_info(const phx_system *s, int64_t *info);
/* CSR of the active system in ORIGINAL active numbering (sorted columns) + the map active row ->
 * full DoF index; host buffers: rowptr[n_active+1], col[nnz], val[nnz], rhs[n_active],
 * dof[n_active].  Any pointer may be NULL. */
int phx_system_export(phx_system *s, int64_t *rowptr, int32_t *col, double *val, double *rhs,
                      int64_t *dof);
/* SELL-16 copy of the stored rows of a structured P1 system (Kuhn box), as the SpMV reads it; host buffers:
 * slice_ptr[n_slices+1], col[sell_padded_nnz] (solver positions), val[sell_padded_nnz] (entries of A),
 * rows[16*n_slices] (solver position of each slice row, -1: padding).  Any pointer may be NULL. */
int phx_system_export_sell(phx_system *s, int64_t *slice_ptr, int32_t *col, double *val, int32_t *rows);

/* ------------------------------------------------------------------ solve ------------ */
enum phx_method { PHX_BICGSTAB_JACOBI = 0 };
/* Replaces KSP preonly + LU/MUMPS with null-pivot detection (main.py:162-182): solves the active
 * system, returns x in FULL numbering [2*nv] with inactive DoFs = 0 (what ICNTL(24)=1 yields).
 * stats[8] = {iterations, relative residual ||b-Ax||/||b||, seconds, spmv_count,
 *            average SpMV seconds and launches timed (PHX_OPT_PROFILE_SPMV),
 *            converged (1: relative residual <= rtol; 0: max_iter reached -- the reference solves directly,
 *            its callers assume an accurate x: treat 0 as a failure), breakdown restarts}.
 * Returns PHX_OK also when max_iter was reached: check stats[6].
 * The residual that is reported (and tested against rtol) is the TRUE one: when the recurrences announce
 * convergence, b - A x is evaluated once and, if it does not meet rtol (drift after thousands of iterations on
 * ill-conditioned systems), the iteration restarts from it. */
int phx_solve(phx_system *s, int method, double rtol, int64_t max_iter, double *x, int loc,
              double *stats);
/* phx_solve started from x0 (FULL numbering, same `loc` as x, may be x itself; NULL: phx_solve).  r0 = b - A x0 on
 * the active rows; ||r0|| <= rtol ||b||: x = x0 with 0 iterations; else phx_solve on A delta = r0 with the tolerance
 * rtol ||b|| / ||r0|| and x = x0 + delta.  stats[1] = ||b - A x|| / ||b||, the other entries are the inner solve's.
 * Single-rank systems only (externally attached Krylov buffers: PHX_ERR_NOT_IMPLEMENTED). */
int phx_solve_from(phx_system *s, int method, double rtol, int64_t max_iter, const double *x0, double *x, int loc,
                   double *stats);

/* --- pieces of the solve for externally driven (multi-GPU) iterations ------------------------
 * The driver owns the loop, does the halo exchange of the SpMV inputs before phases 2 / 4 and
 * all-reduces the 8 reduction scalars (scal[8..15]) after phases 0, 2, 4 and 5.  Vectors are in SOLVER
 * order (row i of the solver = active row perm[i]).
 *   work: 10 vectors of n doubles {r, rhat, p, v, s, t, y, b, phat, shat};  scal: 8208 doubles (16
 *         scalars + 2 x 8 x 64 dot-product slots of 64 B)
 *   own : n bytes in solver order, 1 = this rank owns the row (NULL = all)
 * SpMV inputs: p / s, or -- when phx_krylov_precond_active says 1 after phase 0 -- phat / shat, which
 * phases 7 / 8 compute from p / s (rank-local block preconditioner on the owned rows). */
int phx_krylov_attach(phx_system *s, double *work, double *scal, const uint8_t *own);
int phx_krylov_precond_active(const phx_system *s, int *active);
/* --- slab-exact preconditioner of a z-partitioned box -----------------------------------------------------
 * Every rank holds whole x-y planes of ONE global lattice box around the active vertices of ALL ranks: sine
 * transforms in x and y stay rank-local, the tridiagonal z solves continue across ranks through two carries per
 * lattice column and rank (one all-gather per application).  Protocol, after phx_krylov_attach:
 *   phx_precond_local_bbox   -> out6 = min / max GLOBAL vertex indices of this rank's owned active u DoFs
 *                               (INT64_MAX / -1 when it owns none); the driver reduces MIN / MAX over the ranks
 *   phx_precond_setup_global -> builds this rank's share; zb[nranks + 1]: rank r owns the global vertex planes
 *                               [zb[r], zb[r+1]);  *ncol = 0: not applicable (every rank gets the same answer)
 *   phx_precond_set_carry_buffers -> send[2 ncol], recv[nranks * 2 ncol] doubles on the device (caller-owned)
 *   per application: phase 7 (or 8), all-gather send -> recv over the ranks, phase 9 (or 10).
 * phx_precond_dist_info: out4 = {active, doubles per rank in the all-gather, planes held here, planes of the
 * global column}. */
int phx_precond_local_bbox(phx_system *s, int64_t *out6);
int phx_precond_setup_global(phx_system *s, const int64_t *bbox6, int nranks, int rank, const int64_t *zb,
                             int64_t *ncol);
int phx_precond_set_carry_buffers(phx_system *s, double *send, double *recv);
int phx_precond_dist_info(const phx_system *s, int64_t *out4);
/* Multi-GPU drivers choose the preconditioner collectively: phase 0 leaves this rank's veto in scal[8 + 5]
 * (1: box preconditioner configured out or impossible here; 0: built, or the rank owns no u row); the driver
 * all-reduces scal[8 + 4 .. 8 + 5] (SUM) after phase 0 and, when the vetoes add up to > 0, calls this on
 * every rank before the first iteration: Jacobi everywhere, same vectors exchanged, same check cadence. */
int phx_krylov_precond_disable(phx_system *s);
/* After a solve: out[8] = {preconditioner (0: Jacobi, 1: lattice solve, 2: vertex-block Jacobi of the
 * elasticity system, 3: 2 with the coarse correction, 4: 1 with the P2 coarse correction), transform lengths L0, L1, L2, lattice points of
 * the box, sampled average seconds of one y-pass launch of the sine transforms (PHX_OPT_PROFILE_SPMV),
 * launches sampled, bytes per lattice value (4: f32 transforms, 8: f64)}. */
int phx_precond_info(phx_system *s, double *out);
/* Multilevel preconditioner (PHX_OPT_MULTILEVEL; tests/multilevel_ref.py restates it in numpy).
 * M^-1 = R V R^T on the u block, Jacobi on the p block: R^T places the u rows at their vertices of the system's mesh
 * (level L, zeros elsewhere), V is ONE V-cycle for K_L, R reads the active vertices back.
 *   Levels 0 .. L: the chain of phx_mesh_refine / phx_mesh_refine_marked parents of the system's mesh, down to the first
 *   mesh that has no parent or whose parent has been destroyed.
 *   Constrained vertices: on level L a vertex of a mesh-boundary facet that is no active u DoF of the system (active
 *   boundary vertices stay free: phi-FEM imposes nothing there), and a vertex that belongs to no cell; on level l < L a
 *   vertex is constrained when its image on level L (the same id) is.
 *   K_l: the P1 stiffness matrix of ALL cells of level l, constrained rows and columns replaced by the identity, in
 *   SELL-64 by vertex, built by a stable sort of one entry per (cell, local pair) and an in-order fold: no
 *   floating-point atomics, the same bits on every run.
 *   Smoother: damped Jacobi x <- x + w D^-1 (b - K x), w = 2/3, 2 sweeps before and after, zero initial guess (the first
 *   sweep is x = w D^-1 b).  Transfers: phx_restrict's gather with constrained coarse entries set to zero, the degree-1
 *   prolongation with constrained fine entries left alone.  V is symmetric and one fixed linear operator.
 *   Coarsest level: n_0 <= 2048: the dense inverse of K_0 (kind 1); otherwise 2 * 2 + 8 sweeps from zero (kind 0).  (A
 *   lattice solve on a Kuhn-box level 0, kind 2, is not built.)
 * phx_multilevel_setup builds it for `s` now (phx_solve builds it on the first solve when the option is set) and reports:
 *   PHX_ERR_VALUE: the system's mesh has no living parent; no constrained boundary vertex (K would be singular); slab or
 *     partitioned rank;
 *   PHX_ERR_NOT_IMPLEMENTED: degree 2, quadrilaterals, sub-meshes, systems other than P1 weak Dirichlet, systems that
 *     the lattice preconditioner serves (Kuhn boxes and meshes recognised as such), P2 coarse-space correction asked for.
 * It copies what it needs from the coarser meshes: they may be destroyed afterwards.  Everything is freed with the system.
 * phx_precond_info then reports {5, levels, n_0, coarse kind, sum of the level sizes, 0, 0, 8}. */
int phx_multilevel_setup(phx_system *s);
/* After a solve, the coarse-space correction of the system (P2: PHX_OPT_P2_COARSE; elasticity: PHX_OPT_EL_COARSE):
 * out[6] = {ratio H / h, coarse DoFs of the first field (P2: u; elasticity: all), coarse DoFs of the second field (P2: p;
 * elasticity: 0), build seconds, operator products of the probing, bytes the dense apply streams (nc^2 * 8)}.  No
 * correction: out[1] = out[2] = 0, and out[0] = -reason when one was asked for and could not be built (1: not a single-rank
 * generated box with the lattice preconditioner, 2: box smaller than 2 H, 3: more coarse DoFs than the dense inverse takes
 * (20000), 4: singular coarse matrix, 5: the check |Ac Ac^-1 v - v| failed, 6: automatic choice: the correction does not pay at
 * this box size). */
int phx_coarse_info(phx_system *s, double *out);
/* Test aid: node_of[nc] = field * M + node of each compact coarse DoF (M = m0 m1 m2 coarse nodes per field, node =
 * i + m0 (j + m1 k), node (i, j, k) at the lattice point (i, j, k) * H) and ainv[nc * nc] = Ac^-1, row-major.  Either
 * pointer may be null.  PHX_ERR_VALUE when the system has no coarse correction. */
int phx_coarse_export(phx_system *s, int32_t *node_of, double *ainv);
/* Test aid: one application of the correction, out += D R Ac^-1 R^T in, through the functions the Krylov loop calls
 * (restriction, dense product, prolongation with the scaling D), exactly as the loop adds it to phat.  in[n] and out[n]
 * are in the solver's position order (phx_system_get_perm: position -> active row); nothing is permuted here.  out is
 * read and accumulated into.  gc[nc] receives the restricted vector R^T in and zc[nc] the coarse solution Ac^-1 gc;
 * either may be null.  The stream is synchronised before the call returns.  PHX_ERR_VALUE, before anything is launched:
 * no coarse correction (not solved yet, or none built), no active row, the correction of a partitioned box (its
 * restriction is all-reduced between phases 30-33), a null in or out. */
int phx_coarse_apply(phx_system *s, const double *in, double *out, double *gc, double *zc, int loc);
/* After phx_solve: *on = 1 when the solve ran the identity loop (structured P1 system with the f64 lattice
 * preconditioner: SpMVs over the stored rows only, A K_box^-1 = I on the stencil rows), 0 for the standard loop.
 * PHX_KR_IDENTITY=0 in the environment forces the standard loop. */
int phx_krylov_identity_loop(const phx_system *s, int *on);
/* After phx_solve: *on = 1 when the identity loop ran on compact vectors over the stored rows (started from
 * x0 = M^-1 E_C b_C, so that every Krylov vector vanishes on the stencil rows).  PHX_KR_REDUCED=0 in the environment
 * keeps the full-length identity loop. */
int phx_krylov_reduced_loop(const phx_system *s, int *on);
/* Test aid, after a phx_solve that ran the reduced loop (PHX_ERR_VALUE otherwise): copies one buffer of that loop from
 * (put != 0) or to `host`.  which 0 .. 6: the compact stored-row vectors r, rhat, p, v, s, t, u_B (16 doubles per SELL
 * slice, indexed by SELL slot); 7: u in solver order (n_active); 8 / 9: phat / shat (n_active); 10: the scalars and
 * dot-product slots (16 + 2 * 8 * 64 * 8 doubles; quantity q of parity par: slot k at 16 + ((8 par + q % 8) * 64 + k) * 8
 * + q / 8).  count must be the length of the buffer.  While the loop stays in force phx_krylov_phase accepts its phases:
 * 57 KR_RED_SPMV_P v_B = (A phat)_B with (v_B, rhat_B) into quantity 0, 60 KR_RED_SPMV_S t_B = (A shat)_B with
 * (t_B, s_B), (t_B, t_B), (t_B, rhat_B) into quantities 1, 2, 8, parity 0, added to what the slots hold. */
int phx_krylov_reduced_io(phx_system *s, int which, double *host, int64_t count, int put);
/* Phases (the KrPhase names of phx_solve.hip): 0 KR_BEGIN, 1 KR_BEGIN2, 2 KR_SPMV_P v = A phat, 3 KR_UPDATE_S
 * s-update, 4 KR_SPMV_S t = A shat, 5 KR_UPDATE_XR x/r-update, 6 KR_UPDATE_P p-update + roll, 7 KR_PRECOND_P phat = P p,
 * 8 KR_PRECOND_S shat = P s (no-ops without a preconditioner); with the slab-exact preconditioner
 * (phx_precond_setup_global) 7 / 8 run its first half and 9 KR_EXACT_P / 10 KR_EXACT_S the second, the driver
 * all-gathering the carry buffer in between.  Multi-GPU overlap: 20 KR_SPMV_P_INNER | 21 KR_SPMV_P_HALO
 * (40 KR_SPMV_S_INNER | 41 KR_SPMV_S_HALO) = phase 2 (4) in two launches -- the rows that read no halo entry, then
 * (after the driver has unpacked the halo) the rows that do; they need the row flags phx_solve_distributed builds.
 * True-residual verification: 11 KR_TRUE_SPMV t = A y (after a halo exchange of y), 12 KR_TRUE_RESIDUAL r = b - t and
 * (r, r) -> scal[8 + 5] (all-reduced by the driver), 13 KR_RESTART restart of the recurrences from r.  Partitioned
 * coarse correction: 30 KR_CC_RESTRICT_P / 32 KR_CC_RESTRICT_S restrict p / s, 31 KR_CC_ADD_P / 33 KR_CC_ADD_S add the
 * prolonged correction.  52-55 (KR_ID_SPMV_P, KR_ID_UPDATE_S, KR_ID_SPMV_S, KR_ID_UPDATE_XRP) belong to the identity
 * loop of phx_solve and 56-63 to its reduced loop; their workspaces are built by phx_solve alone (phase 0 of this API
 * never puts those loops in force), so they are refused with PHX_ERR_VALUE before anything is launched. */
int phx_krylov_phase(phx_system *s, int phase);
int phx_krylov_finish(phx_system *s, double *x, int loc);
/* reset != 0: arm the SpMV event profile; else collect {average seconds, launches timed}. */
int phx_krylov_profile(phx_system *s, int reset, double *avg_seconds, int64_t *count);
/* perm[n] (solver position -> active row), dof_u[nv] / dof_p[nv] (vertex -> active row or -1). */
int phx_system_get_perm(phx_system *s, int32_t *perm, int32_t *dof_u, int32_t *dof_p, int loc);

/* --- native multi-GPU solve: RCCL on the solver's stream (bound with dlopen at run time) -------
 * One communicator per process; the 128-byte id comes from rank 0 (phx_comm_unique_id) and is
 * broadcast by the host (torch.distributed).  phx_solve_distributed runs the same phase sequence
 * as phx_solve with a point-to-point halo of p and s (ncclSend/ncclRecv with up to nranks - 1 peers, on the communicator's
 * own stream, overlapped with the rows of the SpMV that read no halo entry; PHX_DIST_OVERLAP=0: in series) and
 * three all-reduces of 1, 2, 2 doubles per iteration.  Convergence checks are scheduled as in phx_solve; relres /
 * converged refer to the TRUE residual (one more halo exchange + SpMV + all-reduce, restart when it misses rtol).
 * Every host wait is bounded by PHX_DIST_TIMEOUT_S (default 300 s) -> PHX_ERR_TIMEOUT.
 * Interface-elasticity systems (PHX_OPT_EL_COARSE): the coarse correction is built collectively before the first
 * iteration (all-reduces of the used-node flags, of a veto and of the coarse matrix: every rank restricts the rows it
 * owns), and every application adds one all-reduce of the coarse right-hand side (phases 30 / 32 restrict p / s,
 * 31 / 33 add the prolonged correction to phat / shat).  The phase API alone keeps the vertex blocks.
 * Buffers attached with phx_krylov_attach.
 *   peers[npeers]; counts[2*npeers] = {n_send, n_recv}; idx[2*npeers] = device int64 arrays
 *   {send positions, recv positions} in solver order. */
typedef struct phx_comm phx_comm;
int phx_comm_unique_id(void *out128);
int phx_comm_create(int nranks, int rank, const void *uid128, int device, phx_comm **out);
int phx_comm_destroy(phx_comm *c);
/* Path of the shared object the ten RCCL entry points were bound from (dladdr of ncclAllReduce), zero-terminated into
 * out[len].  The library binds RCCL at run time (librccl.so.1 of the process; PHX_RCCL_LIB names another file -- the
 * one-GPU tests load a host-staged stand-in that way -- and says so on stderr): a driver prints this next to its
 * result so that what carried the collectives is on record.  No counterpart in the reference (serial). */
int phx_comm_library(char *out, int64_t len);
/* *out = 1 when phx_solve_distributed overlaps the halo exchanges of this communicator with the SpMV rows that read no
 * halo entry (second stream, two events): phx_halo_selftest has then seen the overlapped exchange deliver, bit for bit, what
 * the exchange in series delivers, and PHX_DIST_OVERLAP is not 0.  Otherwise the exchanges stay on the solver stream. */
int phx_comm_overlap(const phx_comm *c, int *out);
int phx_solve_distributed(phx_system *s, phx_comm *c, int npeers, const int *peers,
                          const int64_t *counts, const int64_t *const *idx, double rtol,
                          int64_t max_iter, double *x, int loc, double *stats);
/* stats[8] as phx_solve, except stats[7] = 1 when all ranks kept the box preconditioner, 0 when one vetoed it. */
/* One halo exchange of `vec` (solver order) through the solver's own code path: wiring test. */
int phx_halo_selftest(phx_system *s, phx_comm *c, int npeers, const int *peers,
                      const int64_t *counts, const int64_t *const *idx, double *vec);

/* y = A x on the active system (solver ordering is internal; x, y are in active numbering).
 * For tests and halo-exchange driven (multi-GPU) solvers. */
int phx_spmv(phx_system *s, const double *x, double *y, int loc);
/* Cell-wise discretisation errors, demo/interface-elasticity/main.py:327-383: the exact solution
 * and u_h are interpolated into the Lagrange space of degree 3 (= primal_degree + 2 for P1, basix's default
 * GLL-warped variant [3P]), e = I(u_ex) - u_h, and per listed cell K
 *   l2_local[i]  = int_K e . e            (main.py:369-377)      h10_local[i] = int_K grad e : grad e   (:347-356)
 * norms[4] = { sum l2_local, sum h10_local, int |I u_ex|^2 (:363-367), int |grad I u_ex|^2 (:339-345) } over the
 * listed cells, summed in a fixed order.  u_h: component-major nodal values [ncomp][nv] (degree_h 1) or
 * [ncomp][nv + ne] (2); u_ref: the exact solution at the reference nodes of each listed cell,
 * [ncells][n_nodes][ncomp], nodes as `phx_reference_nodes` lists them (physical point = sum_m bary[m] x_vertex_m);
 * cell_list: ncells cell indices, or NULL for all cells (ncells == nc).  All arrays live at `loc`. */
int phx_reference_nodes(int gdim, int degree, double *bary, int *n_nodes);
int phx_cell_errors(phx_mesh *m, int ncomp, int degree_h, const double *u_h, const double *u_ref,
                    int64_t ncells, const int32_t *cell_list, int loc, double *l2_local,
                    double *h10_local, double *norms);
/* --- a posteriori error indicators and Doerfler marking ----------------------------------------
 * The reference has no counterpart (dolfinx users write the residual forms in UFL); tests/estimate_ref.py restates
 * the definition in numpy.
 *
 * phx_estimate_poisson_wd: residual indicator of the weak-Dirichlet Poisson scheme (phx_assemble_poisson_wd*) on the
 * cell tags currently held by the mesh.  u, p, phi, f, u_D: nodal arrays of ONE degree at loc_in, [nv] (degree 1) or
 * [nv + ne] (degree 2, vertices then the edges of PHX_ARR_C2E), the layout phx_solve returns per field.  With h_T the
 * cell diameter of the assemblers and Omega_h the cells tagged 1 or 2, for T in Omega_h
 *   R_T = h_T^2 int_T (f_h + Laplace u_h)^2
 *   J_T = 1/2 sum over the facets F of T whose other cell T' exists and lies in Omega_h of
 *         h_F int_F [grad u_h . n]^2,   h_F = (h_T + h_T') / 2        (cell tags and f2c only, no facet tags)
 *   B_T = h_T^-2 int_T (u_h - phi_h p_h / h_T - u_D)^2   if T is tagged 2, else 0
 * -> eta2_parts[3][nc] at loc_out (rows R, J, B; cells outside Omega_h exactly 0) and sums3[3] on the host, the
 * totals of the rows.  These are the residuals of the discrete scheme's own terms: an indicator for marking and for
 * effectivity studies, not a proven two-sided bound.
 *   degree 1: triangles, tetrahedra, rectangles (Q1); degree 2: simplices.  Every rule is exact for its integrand.
 *   DETERMINISM RULE: J is a gather -- a cell evaluates the jumps over its own facets, so an interior facet is
 *   evaluated twice and nothing is added atomically; the totals are per-block partial sums folded in a fixed order.
 *   The same inputs give the same bits on every run.
 *   PHX_ERR_VALUE: the mesh carries no cell tags (call compute_tags_measures first), a NULL array;
 *   PHX_ERR_NOT_IMPLEMENTED: degree 2 on quadrilaterals, degree 3, non-rectangular quadrilaterals.
 *
 * phx_mark_dorfler: eta2[n] at loc_in -> marked[n] (0 / 1) at loc_out and *n_marked.  Order the entries by (eta2
 * descending, index ascending), let S_k be the inclusive sums in that order: marked are the first k* entries, k* the
 * smallest k with S_k >= theta S_n; nothing is marked when S_n = 0.  A stable radix sort, a scan with a fixed order of
 * additions and one mask kernel on the mesh's device and stream; nothing but n_marked returns to the host.
 *   PHX_ERR_VALUE: theta outside (0, 1]; a negative, NaN or infinite entry.
 *
 * Both calls release every temporary on failure (phx_pool_stats live bytes return to where they were). */
int phx_estimate_poisson_wd(phx_mesh *m, int degree, const double *u, const double *p, const double *phi,
                            const double *f, const double *u_D, int loc_in, double *eta2_parts, int loc_out,
                            double *sums3);
int phx_mark_dorfler(phx_mesh *m, int64_t n, const double *eta2, int loc_in, double theta, uint8_t *marked,
                     int loc_out, int64_t *n_marked);
/* --- recovered gradient and the recovery-based (Zienkiewicz-Zhu) indicator ---------------------
 * u: nodal values of `degree`, component-major [ncomp][nv] (degree 1) or [ncomp][nv + ne] (degree 2, vertices then
 * the edges of PHX_ARR_C2E) at loc_u.  S = the cells whose byte of cell_mask[nc] (at loc_mask) is not 0; cell_mask
 * NULL: the cells tagged 1 or 2 (tag & 0x7f) on the cell tags the mesh holds.  With S_v the cells of S that contain v
 *   G(v) = sum_{T in S_v} |T| grad u_h|_T (x_v) / sum_{T in S_v} |T|        (exactly 0 where S_v is empty)
 * -> grad[ncomp][nv][gdim] at loc_out; |T| the cell volume, grad u_h|_T (x_v) the gradient of T's own polynomial at
 * its corner v.  eta2 (NULL: not wanted): [nc] at loc_out,
 *   eta_T^2 = sum over the components of int_T |G_h - grad u_h|^2 for T in S,   exactly 0 for T not in S,
 * G_h the P1 / Q1 interpolant of G; closed forms, exact for degrees 1 and 2.  sum (NULL: not wanted): the total of
 * eta2 on the host.  An indicator for marking and a post-processed flux: neither a proven bound nor the residual of
 * any scheme; at the rim of S the stars are one-sided and G is first-order accurate only.
 *   degree 1: triangles, tetrahedra, rectangles (Q1); degree 2: simplices.
 *   DETERMINISM RULE: the cells of S are listed in ascending order, the (vertex, listed cell) pairs sorted by a stable
 *   radix sort, every vertex adds its star in that order and the total is folded from per-block slots in a fixed
 *   order: no floating-point atomics.  The same mesh arrays, mask and values give the same bits on every run and on
 *   every mesh object.  Work and temporaries scale with |S| (two memsets clear the rest of the outputs).
 *   PHX_ERR_VALUE: no mask and no cell tags on the mesh (call compute_tags_measures first), a NULL array, ncomp < 1,
 *   2^31 - 1 or more pairs; PHX_ERR_NOT_IMPLEMENTED: degree 2 on quadrilaterals, degree 3, non-rectangular
 *   quadrilaterals.  Every temporary is released on every return (phx_pool_stats). */
int phx_recover_gradient(phx_mesh *m, int degree, int ncomp, const double *u, int loc_u, const uint8_t *cell_mask,
                         int loc_mask, double *grad, double *eta2, int loc_out, double *sum);

/* Times `reps` launches of the SpMV kernel with HIP events on the mesh's stream.
 * out[3] = {avg ms per launch, algorithmic bytes per launch (12 nnz + 20 n), padded bytes}. */
int phx_spmv_bench(phx_system *s, int reps, double *out);

/* Per-stage device seconds of the last calls, measured with HIP events on the mesh's stream:
 * t[8] = {tag_cells, tag_facets, assemble, solve, spmv_avg, n/a, n/a, n/a}. */
int phx_last_timings(const phx_mesh *m, double *t);

#ifdef __cplusplus
}
#endif
#endif /* PHIFEM_HIP_H */
