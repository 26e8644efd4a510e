// Median high-pass on the device (prom_highpass_set_median): the exposures' models with a running median along each
// order's pixels subtracted or divided out, M' = M - B or M / B, in the place of k_highpass in every chain that runs
// the resident high-pass.  Definitions in prom_hip.h ("median high-pass on the device").
//
// k_median: the ownership, the tiles, the staging and the ring of ORIGINAL values are k_highpass's (prom_highpass.hip,
// highpass_index.h): a workgroup of kHpBlock threads owns one (exposure, trial, segment) and filters it in place, it
// reads ahead before it writes the tile behind.  The window function is a selection (median_index.h): per tile the
// staged stretch (at most kHpTile + 2 h positions) is sorted by (key, position) with a bitonic network over 16-bit
// stretch indices in LDS, which gives every position a rank; a lane then finds, for each of its kHpOut consecutive
// outputs, the rank that has the wanted count of its window's ranks below it, by bisection over the rank's bits, and
// reads the value back.  A wave whose windows lie inside the segment and hold no NaN (k_highpass's vote) knows the
// count, 2 h + 1, and needs one bisection.  The result is a value of the window or the rounded mean of two, so the bits
// depend on nothing but the definition.
#include "prom_internal.h"
#include "median_index.h"

namespace prom {

template <int MODE>
__global__ void __launch_bounds__(kHpBlock) k_median(double* __restrict__ model, const int32_t* __restrict__ seg_first,
                                                      const int32_t* __restrict__ perm, int32_t h, int32_t n_seg,
                                                      int32_t n_pix) {
  __shared__ double ring[kHpRingPad];
  __shared__ __attribute__((aligned(8))) uint16_t idx[kMdStretch], rk[kMdStretch];
  const int32_t tid = threadIdx.x;
  const int32_t s = hp_wg_segment(blockIdx.x, n_seg);
  double* M = model + hp_row_first(hp_wg_row(blockIdx.x, n_seg), n_pix);
  const int32_t first = seg_first[s], n = seg_first[s + 1] - first;
  const int32_t n_tiles = hp_tiles(n);
  for (int32_t tile = 0; tile < n_tiles; ++tile) {
    const int32_t stage_end = hp_stage_end(tile, h);
    for (int32_t i = hp_stage_first(tile, h) + tid; i < stage_end; i += kHpBlock) {
      double m = __builtin_nan("");
      if (i >= 0 && i < n) m = M[perm[hp_perm_at(first, i)]];
      ring[hp_slot(i)] = m;
    }
    // the stretch's indices in order, and no rank beyond them
    const int32_t base = md_base(tile, h), len = md_len(tile, n, h);
    const int32_t p = md_pow2(len), bits = md_bits(p);
    for (int32_t q = tid; q < kMdStretch; q += kHpBlock) {
      if (q < p)
        idx[q] = (uint16_t)q;
      else
        rk[q] = (uint16_t)kMdNoRank;
    }
    __syncthreads();
    for (int32_t k = 2; k <= p; k <<= 1)
      for (int32_t j = k >> 1; j > 0; j >>= 1) {
        for (int32_t t = tid; t < (p >> 1); t += kHpBlock) md_sort_pair(ring, idx, base, len, t, j, k);
        __syncthreads();
      }
    for (int32_t r = tid; r < p; r += kHpBlock) md_rank_write(ring, idx, rk, base, len, r);
    __syncthreads();
    const int32_t o = hp_out_first(tile, tid);
    // (every lane of the wave takes part in the vote, also one without an output)
    const bool clean = !__any(hp_lane_sees_nan(ring, hp_out_first(tile, tid & ~63), tid & 63, h));
    if (o < n) {
      double B[kHpOut];
      if (clean)
        md_median<kHpOut, true>(ring, idx, rk, base, md_q_first(tid), h, bits, B);
      else
        md_median<kHpOut, false>(ring, idx, rk, base, md_q_first(tid), h, bits, B);
#pragma unroll
      for (int v = 0; v < kHpOut; ++v)
        if (o + v < n) M[perm[hp_perm_at(first, o + v)]] = hp_apply<MODE>(ring[hp_slot(o + v)], B[v]);
    }
    __syncthreads();   // the next tile's staging takes the slots of positions this tile has just read
  }
}

void launch_median(hipStream_t s, double* model, const int32_t* seg_first, const int32_t* perm, int32_t half_width,
                   int32_t mode, int64_t n_rows, int32_t n_seg, int32_t n_pix, hipEvent_t ev0, hipEvent_t ev1) {
  if (n_pix <= 0 || n_rows <= 0 || n_seg <= 0) return;
  if (half_width < 0 || half_width > kHpMaxHalf) throw Error(PROM_E_ARG, "k_median: half_width outside [0, 512]");
  const int64_t wgs = hp_workgroups(n_rows, n_seg);
  if (wgs > (((int64_t)1 << 31) - 1))
    throw Error(PROM_E_ARG, "k_median: n_exp n_trial n_seg too large for one launch");
  const dim3 grid((uint32_t)wgs);
  if (ev0) PROM_HIP(hipEventRecord(ev0, s));
  if (mode == 0)
    hipLaunchKernelGGL((k_median<0>), grid, dim3(kHpBlock), 0, s, model, seg_first, perm, half_width, n_seg, n_pix);
  else
    hipLaunchKernelGGL((k_median<1>), grid, dim3(kHpBlock), 0, s, model, seg_first, perm, half_width, n_seg, n_pix);
  PROM_HIP(hipGetLastError());
  if (ev1) PROM_HIP(hipEventRecord(ev1, s));
}

}  // namespace prom
