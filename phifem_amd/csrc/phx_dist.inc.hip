// Native multi-GPU Krylov loop: RCCL (ncclSend/ncclRecv halo + ncclAllReduce of the batched dot
// products) on the solver's HIP stream; included by phx_solve.hip.  RCCL is bound at run time with
// dlopen (the process already holds PyTorch's librccl; a C host may hold /opt/rocm's), so the
// library itself has no link-time dependency on it.  SURVEY 8(e): slabs talk point-to-point to at
// most two neighbours over dedicated xGMI links, the parts of a general partition to up to nranks - 1 peers;
// the scalar all-reduces carry 1, 2 and 2 doubles.
#include <dlfcn.h>
#include <time.h>

typedef struct { char internal[128]; } phx_nccl_uid;
typedef void *phx_nccl_comm;
struct NcclApi {
  int (*GetUniqueId)(phx_nccl_uid *);
  int (*CommInitRank)(phx_nccl_comm *, int, phx_nccl_uid, int);
  int (*CommDestroy)(phx_nccl_comm);
  int (*Send)(const void *, size_t, int, int, phx_nccl_comm, hipStream_t);
  int (*Recv)(void *, size_t, int, int, phx_nccl_comm, hipStream_t);
  int (*AllReduce)(const void *, void *, size_t, int, int, phx_nccl_comm, hipStream_t);
  int (*AllGather)(const void *, void *, size_t, int, phx_nccl_comm, hipStream_t);
  int (*GroupStart)();
  int (*GroupEnd)();
  const char *(*GetErrorString)(int);
  bool ok = false;
};
static NcclApi g_nccl;
static char g_nccl_path[512] = "";   // file the ten entry points were bound from (phx_comm_library)
enum { PHX_NCCL_FLOAT64 = 8, PHX_NCCL_SUM = 0 };  // ncclDataType_t / ncclRedOp_t values of nccl.h

static int nccl_bind() {
  if (g_nccl.ok) return PHX_OK;
  void *h = nullptr;
  // PHX_RCCL_LIB: an explicit library path (the tests load a host-staged stand-in that lets several ranks share
  // the one GPU of the test box, which RCCL itself refuses)
  const char *names[] = {phx_sw_rccl_lib(), "librccl.so.1", "librccl.so", "libnccl.so.2"};
  for (const char *n : names) { if (!n || !*n) continue; h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
  PHX_REQUIRE(h != nullptr, PHX_ERR_HIP, "librccl not found: %s", dlerror());
#define BIND(field, sym) \
  *(void **)(&g_nccl.field) = dlsym(h, sym); \
  PHX_REQUIRE(g_nccl.field != nullptr, PHX_ERR_HIP, "librccl lacks %s", sym)
  BIND(GetUniqueId, "ncclGetUniqueId");
  BIND(CommInitRank, "ncclCommInitRank");
  BIND(CommDestroy, "ncclCommDestroy");
  BIND(Send, "ncclSend");
  BIND(Recv, "ncclRecv");
  BIND(AllReduce, "ncclAllReduce");
  BIND(AllGather, "ncclAllGather");
  BIND(GroupStart, "ncclGroupStart");
  BIND(GroupEnd, "ncclGroupEnd");
  BIND(GetErrorString, "ncclGetErrorString");
#undef BIND
  {
    // which file the symbols really come from (a soname says little): the object that holds ncclAllReduce.  Said once on
    // stderr when PHX_RCCL_LIB substituted the collective library, so that a stand-in is never bound silently.
    Dl_info di;
    if (dladdr((void *)g_nccl.AllReduce, &di) && di.dli_fname) snprintf(g_nccl_path, sizeof(g_nccl_path), "%s", di.dli_fname);
    const char *e = phx_sw_rccl_lib();
    if (e && *e) fprintf(stderr, "phifem_hip: collective library taken from PHX_RCCL_LIB: %s\n", g_nccl_path[0] ? g_nccl_path : e);
  }
  g_nccl.ok = true;
  return PHX_OK;
}

// Path of the library the RCCL entry points are bound to (binds them if that has not happened yet).
extern "C" int phx_comm_library(char *out, int64_t len) {
  PHX_CHECK(nccl_bind());
  PHX_REQUIRE(out != nullptr && len > 0, PHX_ERR_VALUE, "phx_comm_library: no buffer");
  snprintf(out, (size_t)len, "%s", g_nccl_path);
  return PHX_OK;
}

#define PHX_NCCL(expr)                                                                     \
  do {                                                                                     \
    int e_ = (expr);                                                                       \
    if (e_ != 0) {                                                                         \
      phx_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, g_nccl.GetErrorString(e_)); \
      return PHX_ERR_HIP;                                                                  \
    }                                                                                      \
  } while (0)

struct phx_comm {
  phx_nccl_comm comm = nullptr;
  int nranks = 1, rank = 0, device = 0;
  // halo exchanges run on their own stream so that the rows of the SpMV that read no halo entry overlap with them
  hipStream_t cs = nullptr;
  hipEvent_t ev_packed = nullptr, ev_recvd = nullptr;
  // the overlapped exchange (second stream, two events) is used once phx_halo_selftest has seen it deliver, on THIS
  // communicator, what the exchange in series delivers (never validated on hardware with several GPUs before)
  bool overlap_ok = false;
};

extern "C" int phx_comm_unique_id(void *out128) {
  PHX_CHECK(nccl_bind());
  phx_nccl_uid id;
  PHX_NCCL(g_nccl.GetUniqueId(&id));
  memcpy(out128, &id, sizeof(id));
  return PHX_OK;
}

extern "C" int phx_comm_create(int nranks, int rank, const void *uid128, int device, phx_comm **out) {
  PHX_CHECK(nccl_bind());
  PHX_HIP(hipSetDevice(device));
  phx_nccl_uid id;
  memcpy(&id, uid128, sizeof(id));
  phx_comm *c = new phx_comm();
  c->nranks = nranks; c->rank = rank; c->device = device;
  const int e = g_nccl.CommInitRank(&c->comm, nranks, id, rank);
  if (e != 0) {
    phx_set_error("ncclCommInitRank failed: %s", g_nccl.GetErrorString(e));
    delete c;
    return PHX_ERR_HIP;
  }
  if (hipStreamCreateWithFlags(&c->cs, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_packed, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_recvd, hipEventDisableTiming) != hipSuccess) {
    phx_set_error("communication stream / events could not be created");
    g_nccl.CommDestroy(c->comm);
    delete c;
    return PHX_ERR_HIP;
  }
  *out = c;
  return PHX_OK;
}

extern "C" int phx_comm_destroy(phx_comm *c) {
  if (!c) return PHX_OK;
  if (c->cs) { (void)hipStreamSynchronize(c->cs); }
  if (c->comm && g_nccl.ok) g_nccl.CommDestroy(c->comm);
  if (c->ev_packed) (void)hipEventDestroy(c->ev_packed);
  if (c->ev_recvd) (void)hipEventDestroy(c->ev_recvd);
  if (c->cs) (void)hipStreamDestroy(c->cs);
  delete c;
  return PHX_OK;
}

// 1 when the halo exchanges of this communicator run overlapped with the SpMV (self-test passed and PHX_DIST_OVERLAP != 0)
extern "C" int phx_comm_overlap(const phx_comm *c, int *out) {
  PHX_REQUIRE(c != nullptr && out != nullptr, PHX_ERR_VALUE, "phx_comm_overlap: null argument");
  *out = (phx_sw_dist_overlap() && c->overlap_ok) ? 1 : 0;
  return PHX_OK;
}

__global__ void k_halo_pack(int64_t n, const int64_t *__restrict__ idx, const double *__restrict__ v,
                            double *__restrict__ buf) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) buf[i] = v[idx[i]];
}
__global__ void k_halo_unpack(int64_t n, const int64_t *__restrict__ idx, const double *__restrict__ buf,
                              double *__restrict__ v) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) v[idx[i]] = buf[i];
}

// entries that differ bit for bit (NaN-safe) between the vector and a snapshot
__global__ void k_halo_compare(int64_t n, const int64_t *__restrict__ idx, const double *__restrict__ v,
                               const double *__restrict__ snap, unsigned long long *__restrict__ bad) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n && __double_as_longlong(v[idx[i]]) != __double_as_longlong(snap[i])) atomicAdd(bad, 1ull);
}

// Peer lists of one rank.  Up to two peers (slabs) keep one pack and one unpack launch per peer; with more (a general
// partition) the index lists are concatenated and the buffers are slices, in peer order, of ONE
// send and ONE receive arena, so that a single pack and a single unpack launch serve all peers (seven peers would
// otherwise put 14 tiny kernels into every SpMV).  PHX_DIST_FUSED_PACK=0 keeps the launches per peer (A/B aid).
struct HaloSpec {
  int npeers = 0;
  std::vector<int> peer;
  std::vector<int64_t> nsend, nrecv;
  std::vector<const int64_t *> send_idx, recv_idx;
  std::vector<double *> sbuf, rbuf;
  bool fused = false;
  int64_t tot_send = 0, tot_recv = 0;
  int64_t *send_cat = nullptr, *recv_cat = nullptr;     // [tot_send], [tot_recv] concatenated positions (fused)
  double *send_arena = nullptr, *recv_arena = nullptr;  // [tot_send], [tot_recv]
};

static void halo_free(HaloSpec &H) {
  (void)phx_free(H.send_arena); (void)phx_free(H.recv_arena);
  (void)phx_free(H.send_cat); (void)phx_free(H.recv_cat);
  H.send_arena = H.recv_arena = nullptr;
  H.send_cat = H.recv_cat = nullptr;
}

// peers[npeers], counts[2 npeers] = {nsend, nrecv}, idx[2 npeers] = {send_idx, recv_idx} as phx_solve_distributed
static int halo_setup(HaloSpec &H, const phx_comm *c, int npeers, const int *peers, const int64_t *counts,
                      const int64_t *const *idx, hipStream_t st) {
  // (two peers are accepted on any communicator, as before the cap was lifted: a one-rank communicator exchanging with
  // itself is how the wiring is tested on one GPU)
  const int cap = c->nranks - 1 > 2 ? c->nranks - 1 : 2;
  PHX_REQUIRE(npeers >= 0 && npeers <= cap, PHX_ERR_VALUE, "%d peers: a rank of %d has at most %d", npeers, c->nranks, cap);
  H.npeers = npeers;
  for (int p = 0; p < npeers; ++p) {
    PHX_REQUIRE(peers[p] >= 0 && peers[p] < c->nranks, PHX_ERR_VALUE, "peer %d is no rank of the communicator", peers[p]);
    PHX_REQUIRE(counts[2 * p] >= 0 && counts[2 * p + 1] >= 0, PHX_ERR_VALUE, "negative halo count");
    H.peer.push_back(peers[p]);
    H.nsend.push_back(counts[2 * p]); H.nrecv.push_back(counts[2 * p + 1]);
    H.send_idx.push_back(idx[2 * p]); H.recv_idx.push_back(idx[2 * p + 1]);
    H.tot_send += counts[2 * p]; H.tot_recv += counts[2 * p + 1];
  }
  H.fused = npeers > 2 && phx_sw_dist_fused_pack();
  // (+ one entry per peer: every slice has an address of its own, also an empty one)
  PHX_HIP(phx_malloc(&H.send_arena, sizeof(double) * (size_t)(H.tot_send + npeers + 1)));
  PHX_HIP(phx_malloc(&H.recv_arena, sizeof(double) * (size_t)(H.tot_recv + npeers + 1)));
  if (H.fused) {
    PHX_HIP(phx_malloc(&H.send_cat, sizeof(int64_t) * (size_t)(H.tot_send + 1)));
    PHX_HIP(phx_malloc(&H.recv_cat, sizeof(int64_t) * (size_t)(H.tot_recv + 1)));
  }
  int64_t so = 0, ro = 0;
  for (int p = 0; p < npeers; ++p) {
    // fused: the slices follow the concatenated lists without gaps
    H.sbuf.push_back(H.send_arena + so + (H.fused ? 0 : p));
    H.rbuf.push_back(H.recv_arena + ro + (H.fused ? 0 : p));
    if (H.fused) {
      if (H.nsend[p] > 0) PHX_HIP(hipMemcpyAsync(H.send_cat + so, H.send_idx[p], sizeof(int64_t) * (size_t)H.nsend[p], hipMemcpyDeviceToDevice, st));
      if (H.nrecv[p] > 0) PHX_HIP(hipMemcpyAsync(H.recv_cat + ro, H.recv_idx[p], sizeof(int64_t) * (size_t)H.nrecv[p], hipMemcpyDeviceToDevice, st));
    }
    so += H.nsend[p]; ro += H.nrecv[p];
  }
  return PHX_OK;
}

// pack on the solver stream `st`, send / receive on `on` (st itself, or the communicator's stream behind an event)
static int halo_begin(phx_system *s, phx_comm *c, const HaloSpec &H, const double *vec, bool overlap) {
  hipStream_t st = s->mesh->stream;
  if (H.fused) {
    if (H.tot_send > 0)
      k_halo_pack<<<dim3((unsigned)phx_div_up(H.tot_send, 256)), dim3(256), 0, st>>>(H.tot_send, H.send_cat, vec, H.send_arena);
  } else {
    for (int p = 0; p < H.npeers; ++p)
      if (H.nsend[p] > 0)
        k_halo_pack<<<dim3((unsigned)phx_div_up(H.nsend[p], 256)), dim3(256), 0, st>>>(
            H.nsend[p], H.send_idx[p], vec, H.sbuf[p]);
  }
  PHX_HIP(hipGetLastError());
  hipStream_t on = st;
  if (overlap) {
    PHX_HIP(hipEventRecord(c->ev_packed, st));
    PHX_HIP(hipStreamWaitEvent(c->cs, c->ev_packed, 0));
    on = c->cs;
  }
  PHX_NCCL(g_nccl.GroupStart());
  for (int p = 0; p < H.npeers; ++p) {
    if (H.nsend[p] > 0) PHX_NCCL(g_nccl.Send(H.sbuf[p], (size_t)H.nsend[p], PHX_NCCL_FLOAT64, H.peer[p], c->comm, on));
    if (H.nrecv[p] > 0) PHX_NCCL(g_nccl.Recv(H.rbuf[p], (size_t)H.nrecv[p], PHX_NCCL_FLOAT64, H.peer[p], c->comm, on));
  }
  PHX_NCCL(g_nccl.GroupEnd());
  if (overlap) PHX_HIP(hipEventRecord(c->ev_recvd, c->cs));
  return PHX_OK;
}
// ... and the unpack on the solver stream, once the receives have landed
static int halo_end(phx_system *s, phx_comm *c, const HaloSpec &H, double *vec, bool overlap) {
  hipStream_t st = s->mesh->stream;
  if (overlap) PHX_HIP(hipStreamWaitEvent(st, c->ev_recvd, 0));
  if (H.fused) {
    if (H.tot_recv > 0)
      k_halo_unpack<<<dim3((unsigned)phx_div_up(H.tot_recv, 256)), dim3(256), 0, st>>>(H.tot_recv, H.recv_cat, H.recv_arena, vec);
  } else {
    for (int p = 0; p < H.npeers; ++p)
      if (H.nrecv[p] > 0)
        k_halo_unpack<<<dim3((unsigned)phx_div_up(H.nrecv[p], 256)), dim3(256), 0, st>>>(
            H.nrecv[p], H.recv_idx[p], H.rbuf[p], vec);
  }
  PHX_HIP(hipGetLastError());
  return PHX_OK;
}
static int halo_exchange(phx_system *s, phx_comm *c, const HaloSpec &H, double *vec) {
  PHX_CHECK(halo_begin(s, c, H, vec, false));
  return halo_end(s, c, H, vec, false);
}

// slab-exact preconditioner: the zero-inflow carries of every rank's tridiagonal z recurrences (2 doubles per
// lattice column and rank) between the two halves of an application
static int allgather_carries(phx_system *s, phx_comm *c) {
  phx_box_precond *bp = s->precond;
  const size_t count = (size_t)(2 * bp->g.pitch * bp->g.m[1]);
  PHX_REQUIRE(bp->carry_send && bp->carry_recv, PHX_ERR_VALUE, "carry buffers of the slab-exact preconditioner are not set");
  if (c->nranks == 1) {
    PHX_HIP(hipMemcpyAsync(bp->carry_recv, bp->carry_send, sizeof(double) * count, hipMemcpyDeviceToDevice, s->mesh->stream));
    return PHX_OK;
  }
  PHX_NCCL(g_nccl.AllGather(bp->carry_send, bp->carry_recv, count, PHX_NCCL_FLOAT64, c->comm, s->mesh->stream));
  return PHX_OK;
}

static int allreduce_sum(phx_comm *c, double *buf, size_t count, hipStream_t st) {
  if (c->nranks == 1) return PHX_OK;
  PHX_NCCL(g_nccl.AllReduce(buf, buf, count, PHX_NCCL_FLOAT64, PHX_NCCL_SUM, c->comm, st));
  return PHX_OK;
}
static int allreduce_R(phx_system *s, phx_comm *c, int lo, int hi) {
  return allreduce_sum(c, kr_scal(s) + R_OFF + lo, (size_t)(hi - lo), s->mesh->stream);
}

// Watchdog of the host synchronisations inside the distributed loop: a collective whose partner never arrives would
// otherwise block in hipStreamSynchronize for ever.  PHX_DIST_TIMEOUT_S (default 300; 0 = wait without limit).
static int stream_sync_watchdog(hipStream_t st, const char *what) {
  const double limit = phx_sw_dist_timeout_s();
  if (!(limit > 0.0)) { PHX_HIP(hipStreamSynchronize(st)); return PHX_OK; }
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  for (long spins = 0;; ++spins) {
    const hipError_t e = hipStreamQuery(st);
    if (e == hipSuccess) return PHX_OK;
    if (e != hipErrorNotReady) { phx_set_error("%s: %s", what, hipGetErrorString(e)); return PHX_ERR_HIP; }
    if ((spins & 1023) == 1023) {
      clock_gettime(CLOCK_MONOTONIC, &t1);
      const double dt = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
      if (dt > limit) {
        phx_set_error("%s: the stream did not drain within %g s -- a collective is waiting for a rank that never "
                      "arrived (PHX_DIST_TIMEOUT_S)", what, limit);
        return PHX_ERR_TIMEOUT;
      }
      if (dt > 0.01) { struct timespec nap = {0, 50000}; nanosleep(&nap, nullptr); }
    }
  }
}

// What the BiCGStab driver of phx_solve.hip (kr_drive) needs to run mode 1: nullptr there means the single-rank loop.
struct KrDist {
  phx_comm *c;
  const HaloSpec *H;
  bool overlap;   // halo exchanges overlapped with the rows of the SpMV that read no halo entry
  bool exact;     // slab-exact preconditioner: all-gather of the carries between its two halves
  bool coarse;    // partitioned coarse correction: all-reduce of the coarse vector
  bool pc_all;    // every rank kept the box preconditioner (check schedule, stats[7])
};
static int kr_drive(phx_system *s, const KrDist *d, double rtol, int64_t max_iter, double *x_out, int loc,
                    double *stats);

// peers[npeers], counts[2*npeers] = {nsend, nrecv} per peer, idx[2*npeers] device pointers
// {send_idx, recv_idx} (int64 solver positions), work/scal/own as phx_krylov_attach (already
// attached).  stats[8] as phx_solve: relres / converged refer to the TRUE residual b - A x (verified with one more
// halo exchange + SpMV + all-reduce when the recurrences announce convergence, restart from it when it misses rtol);
// stats[7]: 1 = every rank kept the box preconditioner.
// PHX_DIST_OVERLAP=0: halo exchanges in series on the solver stream (default: overlapped with the rows of the SpMV
// that read no halo entry, on the communicator's own stream -- on a communicator whose phx_halo_selftest has seen the
// overlapped exchange deliver the same entries as the exchange in series; without a self-test: in series).
extern "C" int phx_solve_distributed(phx_system *s, phx_comm *c, int npeers, const int *peers,
                                     const int64_t *counts, const int64_t *const *idx, double rtol,
                                     int64_t max_iter, double *x_out, int loc, double *stats) {
  phx_mesh *m = s->mesh;
  PHX_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  HaloSpec H;
  {
    const int rc = halo_setup(H, c, npeers, peers, counts, idx, st);
    if (rc != PHX_OK) { (void)hipStreamSynchronize(st); halo_free(H); return rc; }
  }
  static const bool overlap_env = phx_sw_dist_overlap();   // latched by the first distributed solve
  // a local matter: sends and receives pair up whatever stream each side issues them on
  const bool overlap = overlap_env && c->overlap_ok && c->nranks > 1 && npeers > 0 && c->cs != nullptr;
  auto body = [&]() -> int {
    if (overlap) PHX_CHECK(phx_spmv_flag_rows(s, npeers, H.recv_idx.data(), H.nrecv.data()));   // all receive lists
    PHX_CHECK(prof_reset(s));
    PHX_CHECK(phx_begin_timing(m));
    PHX_CHECK(kr_phase(s, KR_BEGIN, 1, 0));
    PHX_CHECK(allreduce_R(s, c, R_RHO, R_RR + 1));  // (b, b) and the preconditioner vetoes
    PHX_CHECK(kr_phase(s, KR_BEGIN2, 1, 0));
    PHX_HIP(hipMemcpyAsync(s->scal_h, kr_scal(s), sizeof(double) * 16, hipMemcpyDeviceToHost, st));
    PHX_CHECK(stream_sync_watchdog(st, "start of the distributed solve"));
    // the preconditioner is a COLLECTIVE choice: one veto and every rank iterates with Jacobi, so that all
    // ranks exchange the same vectors and test convergence at the same iterations
    const bool pc_all = s->scal_h[R_OFF + R_RR] == 0.0;
    if (!pc_all) PHX_CHECK(phx_krylov_precond_disable(s));
    // interface elasticity: the coarse correction on top of the vertex blocks, built collectively (phx_coarse.inc.hip);
    // a rank without rows of its own still joins the reductions
    if (s->el_nblk > 0 && m->precond != 0 && !s->cc && !s->cc_tried) {
      s->cc_tried = true;
      const CcReduce red = [&](double *buf, size_t count) -> int { return allreduce_sum(c, buf, count, st); };
      PHX_CHECK(coarse_build(s, s->el_nblk, &s->cc, &red));
    }
    // after the vote: the same on every rank (set up from all-reduced numbers)
    const KrDist d{c, &H, overlap, kr_slab_exact(s), s->cc != nullptr && s->cc->dist, pc_all};
    return kr_drive(s, &d, rtol, max_iter, x_out, loc, stats);
  };
  const int rc = body();
  if (rc != PHX_ERR_TIMEOUT) {   // a wedged stream would block here for ever
    (void)hipStreamSynchronize(st);
    if (c->cs) (void)hipStreamSynchronize(c->cs);
    halo_free(H);
  }
  return rc;
}

// Wiring self-test: every rank sends each peer `tags` gathered at its send positions and receives
// into its recv positions; used by the host to prove both sides enumerate the same DoFs through
// the SAME code path the solver uses (ncclSend/ncclRecv + pack/unpack kernels).
extern "C" int phx_halo_selftest(phx_system *s, phx_comm *c, int npeers, const int *peers,
                                 const int64_t *counts, const int64_t *const *idx, double *vec) {
  PHX_HIP(hipSetDevice(s->mesh->device));
  HaloSpec H;
  int rc = halo_setup(H, c, npeers, peers, counts, idx, s->mesh->stream);
  if (rc != PHX_OK) { (void)hipStreamSynchronize(s->mesh->stream); halo_free(H); return rc; }
  rc = halo_exchange(s, c, H, vec);
  if (rc == PHX_OK) rc = stream_sync_watchdog(s->mesh->stream, "halo self-test");
  // ... and once more through the OVERLAPPED path: the received entries are cleared, exchanged again on the
  // communicator's stream behind the two events, and must come back bit for bit.  Every rank makes both exchanges (they
  // pair up), each decides for itself (`overlap_ok`: a local matter, see phx_solve_distributed).
  if (rc == PHX_OK && c->nranks > 1 && npeers > 0 && c->cs != nullptr) {
    hipStream_t st = s->mesh->stream;
    std::vector<double *> snap((size_t)npeers, nullptr);
    unsigned long long *bad = nullptr;
    bool ok = phx_malloc(&bad, sizeof(unsigned long long)) == hipSuccess;
    for (int p = 0; p < npeers && ok; ++p) ok = phx_malloc(&snap[p], sizeof(double) * (size_t)(H.nrecv[p] > 0 ? H.nrecv[p] : 1)) == hipSuccess;
    if (ok) {
      (void)hipMemsetAsync(bad, 0, sizeof(unsigned long long), st);
      for (int p = 0; p < npeers; ++p)
        if (H.nrecv[p] > 0) {
          const dim3 g((unsigned)phx_div_up(H.nrecv[p], 256)), b(256);
          k_halo_pack<<<g, b, 0, st>>>(H.nrecv[p], H.recv_idx[p], vec, snap[p]);
          (void)hipMemsetAsync(H.rbuf[p], 0xff, sizeof(double) * (size_t)H.nrecv[p], st);   // NaNs: a stale buffer shows
          k_halo_unpack<<<g, b, 0, st>>>(H.nrecv[p], H.recv_idx[p], H.rbuf[p], vec);
        }
      rc = halo_begin(s, c, H, vec, true);
      if (rc == PHX_OK) rc = halo_end(s, c, H, vec, true);
      for (int p = 0; p < npeers && rc == PHX_OK; ++p)
        if (H.nrecv[p] > 0)
          k_halo_compare<<<dim3((unsigned)phx_div_up(H.nrecv[p], 256)), dim3(256), 0, st>>>(H.nrecv[p], H.recv_idx[p], vec, snap[p], bad);
      unsigned long long hbad = 1;
      if (rc == PHX_OK) rc = hipMemcpyAsync(&hbad, bad, sizeof(hbad), hipMemcpyDeviceToHost, st) == hipSuccess ? PHX_OK : PHX_ERR_HIP;
      if (rc == PHX_OK) rc = stream_sync_watchdog(st, "halo self-test (overlapped exchange)");
      if (rc == PHX_OK && c->cs) rc = stream_sync_watchdog(c->cs, "halo self-test (communication stream)");
      c->overlap_ok = rc == PHX_OK && hbad == 0;
      if (rc == PHX_OK && hbad != 0) {
        // the caller checks the entries of the exchange in series: put them back
        for (int p = 0; p < npeers; ++p)
          if (H.nrecv[p] > 0)
            k_halo_unpack<<<dim3((unsigned)phx_div_up(H.nrecv[p], 256)), dim3(256), 0, st>>>(H.nrecv[p], H.recv_idx[p], snap[p], vec);
        (void)hipStreamSynchronize(st);
      }
      if (rc == PHX_OK && hbad != 0)
        fprintf(stderr, "phifem_hip: rank %d: the overlapped halo exchange delivered %llu entries that differ from the exchange in "
                        "series -- halo exchanges stay on the solver stream\n", c->rank, hbad);
    }
    (void)phx_free(bad);
    for (int p = 0; p < npeers; ++p) (void)phx_free(snap[p]);
  }
  (void)hipStreamSynchronize(s->mesh->stream);
  halo_free(H);
  return rc;
}
