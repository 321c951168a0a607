// Ordered stream compaction of entity indices: list = [i in 0..n-1 : pred(i)], ascending.
// The entity arrays here have 1e8..1e9 items of which a thin layer (cut cells, ghost-penalty facets)
// is kept, and the predicates read one tag byte per item: a wavefront walks a contiguous chunk in
// rounds of 64 consecutive items (one 64-byte request per round), ranks the kept ones with a ballot,
// and the per-chunk counts are scanned in between -- two streaming passes over the tag bytes instead
// of a generic look-back select (measured on 2e8 facets: 2.0 ms -> see DESIGN.md).
#pragma once
#include "phx_prim.h"
#include <utility>
#include <vector>

#include "phx_common.h"

#define PHX_SEL_ROUNDS 32
#define PHX_SEL_CHUNK (64 * PHX_SEL_ROUNDS)

// Predicates over ONE tag byte per item may say so: `const int8_t *bytes() const` (the byte array, 4-byte aligned as
// every device allocation is) and `bool test(int tag, int32_t i) const`.  A lane then takes four consecutive items
// from one 32-bit load (a quarter of the load instructions: the byte streams ran at 0.8 TB/s, instruction bound).
template <typename Pred, typename = void> struct sel_has_bytes { static constexpr bool value = false; };
template <typename Pred> struct sel_has_bytes<Pred, decltype((void)std::declval<const Pred &>().bytes())> { static constexpr bool value = true; };

// The selections whose per-chunk counts the tagging kernels leave behind (phx_tag.hip: sel_counts_cut, sel_counts[0 / 1]).
// Cut cells:
struct SelCut {
  const int8_t *t;
  __host__ __device__ bool operator()(const int32_t &c) const { return (t[c] & PHX_TAG_MASK) == 2; }
  __host__ __device__ const int8_t *bytes() const { return t; }           // byte fast path of phx_select.h
  __host__ __device__ bool test(int tag, int32_t) const { return (tag & PHX_TAG_MASK) == 2; }
};
struct SelGhostFacet {
  const int8_t *ft; const int32_t *f2c;
  __host__ __device__ bool operator()(const int32_t &f) const {
    const int t = ft[f];
    return (t == 2 || t == 3) && f2c[2 * (int64_t)f + 1] >= 0;  // dS: interior facets only
  }
  __host__ __device__ const int8_t *bytes() const { return ft; }
  // without a branch around the load (the four loads of a lane go out together): the other tags read facet 0
  __host__ __device__ bool test(int t, int32_t f) const {
    const bool c = t == 2 || t == 3;
    return (f2c[2 * (int64_t)(c ? f : 0) + 1] >= 0) & c;
  }
};
// facets tagged 3 or 4 (the one-sided measures, phx_collect_entities):
struct SelTag34 {
  const int8_t *ft;
  __host__ __device__ bool operator()(const int32_t &f) const { return ft[f] == 3 || ft[f] == 4; }
  __host__ __device__ const int8_t *bytes() const { return ft; }
  __host__ __device__ bool test(int t, int32_t) const { return t == 3 || t == 4; }
};

template <typename Pred, bool FILL>
__global__ void __launch_bounds__(256)
k_select_chunks(int64_t n, Pred pred, int32_t *__restrict__ chunk_counts,
                const int32_t *__restrict__ chunk_offsets, int32_t *__restrict__ list) {
  const int lane = threadIdx.x & 63;
  const int64_t chunk = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t base = chunk * PHX_SEL_CHUNK;
  if (base >= n) return;
  int64_t pos = 0;
  if constexpr (FILL) {
    // The kept items lie in a thin layer: many chunks keep nothing, and the scanned counts say so before the first load
    // (wave-uniform test).  chunk_offsets has nchunks + 1 entries and is the scan of EXACT per-chunk counts of `pred`.
    const int64_t uc = blockIdx.x * (int64_t)(blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int32_t lo = chunk_offsets[uc], hi = chunk_offsets[uc + 1];   // uc == chunk, as a scalar: two scalar loads
    if (hi == lo) return;
    pos = lo;
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  if constexpr (sel_has_bytes<Pred>::value) {
    // items base + 256 r + 4 lane + j, j = 0..3: ascending order = lane-major, j-minor
    const uint32_t *words = reinterpret_cast<const uint32_t *>(pred.bytes());
    // all words of the chunk first: the rounds below store to `list`, which keeps the compiler from moving a later
    // round's load ahead of them (a chunk was eight dependent round trips)
    uint32_t ww[PHX_SEL_ROUNDS / 4];
#pragma unroll
    for (int r = 0; r < PHX_SEL_ROUNDS / 4; ++r) {
      const int64_t i0 = base + r * 256 + lane * 4;
      uint32_t w = 0u;
      if (i0 + 3 < n) w = words[i0 >> 2];          // base and 256 r are multiples of 4
      else for (int j = 0; j < 4; ++j) if (i0 + j < n) w |= (uint32_t)(uint8_t)pred.bytes()[i0 + j] << (8 * j);
      ww[r] = w;
    }
#pragma unroll
    for (int r = 0; r < PHX_SEL_ROUNDS / 4; ++r) {
      const int64_t i0 = base + r * 256 + lane * 4;
      const uint32_t w = ww[r];
      bool keep[4];
      unsigned long long mask[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {   // an item past n has tag 0 and is tested as item 0: test() runs without a branch
        const bool in = i0 + j < n;
        keep[j] = pred.test((int)(int8_t)((w >> (8 * j)) & 255u), (int32_t)(in ? i0 + j : 0)) & in;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) mask[j] = __ballot(keep[j]);
      int before = 0, all = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { before += __popcll(mask[j] & below); all += __popcll(mask[j]); }
      if (FILL) {
        int k = before;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (keep[j]) { list[pos + k] = (int32_t)(i0 + j); ++k; }
      }
      pos += all;
    }
  } else {
    for (int r = 0; r < PHX_SEL_ROUNDS; ++r) {
      const int64_t i = base + r * 64 + lane;
      const bool keep = i < n && pred((int32_t)i);
      const unsigned long long mask = __ballot(keep);
      if (FILL && keep) list[pos + __popcll(mask & below)] = (int32_t)i;
      pos += __popcll(mask);
    }
  }
  if (!FILL && lane == 0) chunk_counts[chunk] = (int32_t)pos;
}

// Allocates *list with exactly the kept count (at least one entry) and returns the count.
// later (nullable): the caller synchronises `stream` before it frees what is pushed here -- the fill pass is then only
// enqueued (one host round trip per selection instead of two).
// known_counts (nullable): the per-chunk counts [nchunks + 1, last entry 0] are already on the device (the kernel that
// wrote the tags counted) -- the counting pass over the items is skipped.  They must be the EXACT counts of `pred` per
// chunk, not upper bounds: the fill pass skips the chunks they call empty.  -DPHX_SELECT_VERIFY counts again and compares.
template <typename Pred>
// known_total >= 0 (with known_counts): the kept count is known on the host as well -- no host round trip at all.
static int phx_select_indices(hipStream_t stream, int64_t n, Pred pred, int32_t **list, int64_t *count,
                              std::vector<void *> *later = nullptr, const int32_t *known_counts = nullptr,
                              int64_t known_total = -1) {
  *list = nullptr;
  *count = 0;
  const int64_t nchunks = phx_div_up(n > 0 ? n : 1, (int64_t)PHX_SEL_CHUNK);
  int32_t *cnt = nullptr, *off = nullptr;
  PHX_HIP(phx_malloc(&off, sizeof(int32_t) * (size_t)(nchunks + 1)));
  const dim3 block(256), grid((unsigned)phx_div_up(nchunks, 4));
  if (!known_counts) {
    PHX_HIP(phx_malloc(&cnt, sizeof(int32_t) * (size_t)(nchunks + 1)));
    PHX_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)(nchunks + 1), stream));
    if (n > 0) k_select_chunks<Pred, false><<<grid, block, 0, stream>>>(n, pred, cnt, nullptr, nullptr);
    known_counts = cnt;
  }
#ifdef PHX_SELECT_VERIFY
  if (!cnt && n > 0) {
    int32_t *chk = nullptr;
    PHX_HIP(phx_malloc(&chk, sizeof(int32_t) * (size_t)nchunks));
    k_select_chunks<Pred, false><<<grid, block, 0, stream>>>(n, pred, chk, nullptr, nullptr);
    std::vector<int32_t> a((size_t)nchunks), b((size_t)nchunks);
    PHX_HIP(hipMemcpyAsync(a.data(), chk, sizeof(int32_t) * (size_t)nchunks, hipMemcpyDeviceToHost, stream));
    PHX_HIP(hipMemcpyAsync(b.data(), known_counts, sizeof(int32_t) * (size_t)nchunks, hipMemcpyDeviceToHost, stream));
    PHX_HIP(hipStreamSynchronize(stream));
    PHX_HIP(phx_free(chk));
    PHX_REQUIRE(a == b, PHX_ERR_VALUE, "phx_select_indices: the known per-chunk counts are not the counts of the predicate");
  }
#endif
  size_t bytes = 0;
  PHX_HIP(phx_exclusive_sum(nullptr, bytes, known_counts, off, (size_t)(nchunks + 1), stream));
  void *tmp = nullptr;
  PHX_HIP(phx_malloc(&tmp, bytes ? bytes : 16));
  PHX_HIP(phx_exclusive_sum(tmp, bytes, known_counts, off, (size_t)(nchunks + 1), stream));
  int32_t total = 0;
  if (known_total >= 0 && later) {
    total = (int32_t)known_total;
  } else {
    PHX_HIP(hipMemcpyAsync(&total, off + nchunks, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    PHX_HIP(hipStreamSynchronize(stream));
  }
  PHX_HIP(phx_malloc(list, sizeof(int32_t) * (size_t)(total > 0 ? total : 1)));
  if (total > 0) k_select_chunks<Pred, true><<<grid, block, 0, stream>>>(n, pred, nullptr, off, *list);
  PHX_HIP(hipGetLastError());
  if (later) {
    later->push_back(tmp); later->push_back(off);
    if (cnt) later->push_back(cnt);
  } else {
    PHX_HIP(hipStreamSynchronize(stream));
    PHX_HIP(phx_free(tmp)); PHX_HIP(phx_free(cnt)); PHX_HIP(phx_free(off));
  }
  *count = total;
  return PHX_OK;
}
