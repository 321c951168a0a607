// Stored-row product of the reduced BiCGStab loop (included by phx_solve.hip): y_B = (A x)_B over the SELL-16 slices of
// a structured system on one rank, y and the dot-product operands compact vectors indexed by SELL slot.
//
// The arithmetic is that of the stored-row branch of k_spmv_sell<DOTS, true>, term for term: four lanes per row, entry
// k of row r of a slice at base + 16 k + r, rounds of four trips, the tail, two shuffles; 256-thread blocks of four
// slices with the same block -> slice map, so y is the same bits and the per-block dot partials have the same
// composition.  What differs is what a wavefront waits for and what it holds:
//   * nothing of the stencil and value-indexed branches of k_spmv_sell (their registers and the dictionary LDS capped
//     that kernel at 6 waves per SIMD): this one fits 8;
//   * the slice bounds are one wave-uniform scalar load (the slice index goes through readfirstlane), not a per-lane
//     8-byte vector load in front of the stream;
//   * rows[ci], d0[ci] and d1[ci] are requested before the entry loop, so the epilogue has its operands when the last
//     gather returns;
//   * slices are sorted by length, trips is wave-uniform: where a slice has eight trips or more, eight column / value
//     loads are in flight before the first gather (same sums in the same order as two rounds of four), never a clamped
//     duplicate.
// The second launch bound asks for 8 waves per SIMD, i.e. at most 64 VGPRs: without it the round of eight takes 66 / 68.
template <int DOTS>
__global__ void __launch_bounds__(256, 8)
k_spmv_red(int64_t nslices, const int64_t *__restrict__ slice_ptr, const int32_t *__restrict__ scol,
           const double *__restrict__ sval, const double *__restrict__ x, double *__restrict__ y,
           const int32_t *__restrict__ rows, const double *__restrict__ d0, const double *__restrict__ d1,
           double *__restrict__ out0, double *__restrict__ out1, double *__restrict__ out2, int xcd_group,
           int64_t nb_sell, DotPart part) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  int64_t bid = blockIdx.x;
  if (xcd_group > 0) {   // PHX_OPT_SPMV_XCD_GROUP, as k_spmv_sell
    const int64_t super = 8 * (int64_t)xcd_group, sg = bid / super;
    if ((sg + 1) * super <= nb_sell) {
      const int64_t rem = bid - sg * super;
      bid = sg * super + (rem & 7) * xcd_group + (rem >> 3);
    }
  }
  const int64_t s = bid * 4 + wave;   // wave-uniform
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;   // this lane's share of (y, d0), (y, y) and (y, d1)
  if (s < nslices) {
    const int64_t base = slice_ptr[s];
    const int trips = (int)((slice_ptr[s + 1] - base) >> 6);   // width / 4
    const int64_t ci = s * 16 + (lane & 15);
    // the epilogue's operands, requested ahead of the stream.  Every lane asks (the four lanes of a row for the same
    // entry): under `lane < 16` the join of the branch waited for rows[ci] before the first matrix load was issued
    const int32_t rr = rows[ci];
    const double e0 = DOTS > 0 ? d0[ci] : 0.0, e1 = DOTS > 2 ? d1[ci] : 0.0;
    const int32_t *c = scol + base + lane;
    const double *v = sval + base + lane;
    double acc = 0.0;
    int j = 0;
    for (; j + 8 <= trips; j += 8) {
      int32_t cc[8];
      double vv[8], xs[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) { cc[q] = NT_LOAD(&c[(j + q) * 64]); vv[q] = NT_LOAD(&v[(j + q) * 64]); }
#pragma unroll
      for (int q = 0; q < 8; ++q) xs[q] = x[cc[q]];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc = __builtin_fma(vv[q], xs[q], acc);
    }
    for (; j + 4 <= trips; j += 4) {
      int32_t cc[4];
      double vv[4], xs[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { cc[q] = NT_LOAD(&c[(j + q) * 64]); vv[q] = NT_LOAD(&v[(j + q) * 64]); }
#pragma unroll
      for (int q = 0; q < 4; ++q) xs[q] = x[cc[q]];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = __builtin_fma(vv[q], xs[q], acc);
    }
    for (; j < trips; ++j) acc = __builtin_fma(NT_LOAD(&v[j * 64]), x[NT_LOAD(&c[j * 64])], acc);
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    if (lane < 16 && rr >= 0) {   // rr = -1: padding of the last slice
      y[ci] = acc;
      if (DOTS > 0) p0 = __builtin_fma(acc, e0, p0);
      if (DOTS > 1) p1 = __builtin_fma(acc, acc, p1);
      if (DOTS > 2) p2 = __builtin_fma(acc, e1, p2);
    }
  }
  if (DOTS > 0) {
    // DOTS == 1: out0 += (y, d0);  DOTS == 3: also out1 += (y, y), out2 += (y, d1)
    __shared__ double red[DOTS > 0 ? DOTS : 1][4];
    p0 = wave_sum(p0);
    if (DOTS > 1) p1 = wave_sum(p1);
    if (DOTS > 2) p2 = wave_sum(p2);
    if (lane == 0) {
      red[0][wave] = p0;
      if (DOTS > 1) red[1][wave] = p1;
      if (DOTS > 2) red[2][wave] = p2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const double s0 = red[0][0] + red[0][1] + red[0][2] + red[0][3];
      const double s1 = DOTS > 1 ? red[1][0] + red[1][1] + red[1][2] + red[1][3] : 0.0;
      const double s2 = DOTS > 2 ? red[2][0] + red[2][1] + red[2][2] + red[2][3] : 0.0;
      if (part.p0) {   // PHX_OPT_DETERMINISTIC: one entry per block, summed in a fixed order by k_fold_partials
        part.p0[blockIdx.x] = s0;
        if (DOTS > 1) part.p1[blockIdx.x] = s1;
        if (DOTS > 2) part.p2[blockIdx.x] = s2;
      } else {
        const int slot = (blockIdx.x & (NSLOT - 1)) * SLOT_STRIDE;
        unsafeAtomicAdd(out0 + slot, s0);
        if (DOTS > 1) unsafeAtomicAdd(out1 + slot, s1);
        if (DOTS > 2) unsafeAtomicAdd(out2 + slot, s2);
      }
    }
  }
}
