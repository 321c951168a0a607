// Every environment variable libphifem_hip.so reads, one function each.  No other file of the library calls getenv.
// The table in DESIGN.md section 8 lists the same names (tests/test_switches.py compares the two).
// "once per process": the first call latches the value; "every call": the environment is looked at again each time.
#pragma once
#include <stdlib.h>

// PHX_KR_IDENTITY (default 1; once per process).  0: the native single-rank BiCGStab keeps the standard loop where it
// would run the identity loop (reference path of tests/test_hip_kr_identity.py).
static inline bool phx_sw_kr_identity() {
  static const int env = getenv("PHX_KR_IDENTITY") ? atoi(getenv("PHX_KR_IDENTITY")) : 1;
  return env != 0;
}

// PHX_KR_REDUCED (default 1; once per process).  0: the identity loop stays on full-length vectors instead of the
// compact stored-row vectors of the reduced loop (reference path of tests/test_hip_kr_reduced.py).
static inline bool phx_sw_kr_reduced() {
  static const int env = getenv("PHX_KR_REDUCED") ? atoi(getenv("PHX_KR_REDUCED")) : 1;
  return env != 0;
}

// PHX_BOX_SLOTS (default 1; every call, i.e. per assembly).  0: the stored rows of a structured P1 system are assembled
// into hashed slots instead of direct-addressed box slots (reference path of tests/test_box_slots.py).
static inline bool phx_sw_box_slots() {
  const char *e = getenv("PHX_BOX_SLOTS");
  return !(e && atoi(e) == 0);
}

// PHX_INNER_BOX (default 1; once per process).  0: a caller-supplied mesh that is a Kuhn box is served by the generic
// path instead of the generated box attached to it.
static inline bool phx_sw_inner_box() {
  static const bool no_inner = getenv("PHX_INNER_BOX") && atoi(getenv("PHX_INNER_BOX")) == 0;
  return !no_inner;
}

// PHX_POOL_LIMIT_GB (default: unset = 60 % of the device memory; read by the caller once per process).  Bytes the
// caching allocator may keep; *set = false when the variable is absent.
static inline double phx_sw_pool_limit_gb(bool *set) {
  const char *e = getenv("PHX_POOL_LIMIT_GB");
  *set = e != nullptr;
  return e ? atof(e) : 0.0;
}

// PHX_DET_LIMIT_GB (default: unset = 20 % of the device memory; read by the caller once per process).  Budget of the
// second accumulators of PHX_OPT_DETERMINISTIC; *set = false when the variable is absent.
static inline double phx_sw_det_limit_gb(bool *set) {
  const char *e = getenv("PHX_DET_LIMIT_GB");
  *set = e != nullptr;
  return e ? atof(e) : 0.0;
}

// PHX_DIST_OVERLAP (default 1; every call -- phx_comm_overlap asks each time, the distributed solve latches its first
// answer).  0: the halo exchange is not overlapped with the SpMV.
static inline bool phx_sw_dist_overlap() {
  return !(getenv("PHX_DIST_OVERLAP") && atoi(getenv("PHX_DIST_OVERLAP")) == 0);
}

// PHX_DIST_FUSED_PACK (default 1; once per process).  0: one pack / unpack launch per peer instead of one for all.
static inline bool phx_sw_dist_fused_pack() {
  static const bool fused = !(getenv("PHX_DIST_FUSED_PACK") && atoi(getenv("PHX_DIST_FUSED_PACK")) == 0);
  return fused;
}

// PHX_DIST_TIMEOUT_S (default 300; once per process).  Seconds a host synchronisation of the distributed loop waits
// for its collective, 0 = without limit (the Python side reads the same variable: dist_solver.dist_timeout_s).
static inline double phx_sw_dist_timeout_s() {
  static const double t = getenv("PHX_DIST_TIMEOUT_S") ? atof(getenv("PHX_DIST_TIMEOUT_S")) : 300.0;
  return t;
}

// PHX_RCCL_LIB (default: unset; every call -- the binding itself happens once).  Path of the collective library to
// load ahead of librccl; nullptr when absent.
static inline const char *phx_sw_rccl_lib() { return getenv("PHX_RCCL_LIB"); }
