// High-pass filtered exposures on the device (prom_highpass_set / prom_transit_expose_highpass /
// prom_spectrum_expose_highpass): the exposures' models with a running weighted mean along each order's pixels
// subtracted or divided out, M' = M - B or M / B, then (on request) the resident SYSREM filter, then the seven moments
// against the data.  Definitions in prom_hip.h.
//
//   k_expose          (prom_expose.hip, unchanged) model[e][j][p] = M, the unfiltered model of the whole table
//   k_highpass        model[e][j][p] = M' in place
//   k_detrend         (prom_detrend.hip, unchanged, on request) the SYSREM filter of M' in place, flag[j][p]
//   k_model_moments   (prom_detrend.hip, unchanged) the partial records of the moments
//   k_vmap_reduce     (prom_vmap.hip, unchanged) the chunks' records in chunk order
//
// k_highpass: a workgroup of kHpBlock threads owns one (exposure, trial, segment): nobody else reads or writes that
// stretch of the model, so the filter needs no second buffer.  The segment's positions reach the model through perm
// (the pixels lie sorted by wavelength, the orders interleaved where they overlap).  The workgroup walks the segment
// in ascending tiles of kHpTile outputs with a rolling window in LDS that holds the original values of
// [tile_first - h, tile_end + h): it reads ahead from memory, gathered through perm, before it writes the tile
// behind, and keeps the last h originals in the ring, so an overwritten value is never read again (highpass_index.h
// has the invariants, the host harness walks them).  A position outside the segment and a NaN model value are both
// NaN in the ring; the definition skips either.
//
// A lane owns kHpOut consecutive outputs and walks the ring once for all of them (hp_window): per tap one ds_read_b64
// feeds kHpOut multiplies and adds.  The ring skips a double after every 32, so that lanes kHpOut doubles apart do not
// meet in a bank.  g[d] is uniform over the workgroup: scalar loads.  A wave whose windows all lie inside the segment
// and hold no NaN (each lane looks at a share of the wave's stretch of the ring, then a vote) takes the path without
// validity tests and den sums; the bits are the same.  There is no cross-lane arithmetic, so the bits do not depend on
// the layout.
#include "prom_internal.h"
#include "highpass_index.h"

namespace prom {

template <int MODE>
__global__ void __launch_bounds__(kHpBlock) k_highpass(double* __restrict__ model, const int32_t* __restrict__ seg_first,
                                                        const int32_t* __restrict__ perm, const double* __restrict__ g,
                                                        int32_t h, double den_full, int32_t n_seg, int32_t n_pix) {
  __shared__ double ring[kHpRingPad];
  const int32_t tid = threadIdx.x;
  const int32_t s = hp_wg_segment(blockIdx.x, n_seg);
  double* M = model + hp_row_first(hp_wg_row(blockIdx.x, n_seg), n_pix);
  const int32_t first = seg_first[s], n = seg_first[s + 1] - first;
  const int32_t n_tiles = hp_tiles(n);
  for (int32_t tile = 0; tile < n_tiles; ++tile) {
    // read ahead: the originals this tile's window still lacks (all of them lie at or above the tile's first output)
    const int32_t stage_end = hp_stage_end(tile, h);
    for (int32_t i = hp_stage_first(tile, h) + tid; i < stage_end; i += kHpBlock) {
      double m = __builtin_nan("");
      if (i >= 0 && i < n) m = M[perm[hp_perm_at(first, i)]];
      ring[hp_slot(i)] = m;
    }
    __syncthreads();
    const int32_t o = hp_out_first(tile, tid);
    // (every lane of the wave takes part in the vote, also one without an output)
    const bool clean = !__any(hp_lane_sees_nan(ring, hp_out_first(tile, tid & ~63), tid & 63, h));
    if (o < n) {
      double B[kHpOut];
      if (clean)
        hp_window<kHpOut, true>(ring, o, h, g, den_full, B);
      else
        hp_window<kHpOut, false>(ring, o, h, g, den_full, B);
#pragma unroll
      for (int v = 0; v < kHpOut; ++v)
        if (o + v < n) M[perm[hp_perm_at(first, o + v)]] = hp_apply<MODE>(ring[hp_slot(o + v)], B[v]);
    }
    __syncthreads();   // the next tile's staging takes the slots of positions this tile has just read
  }
}

void launch_highpass(hipStream_t s, double* model, const int32_t* seg_first, const int32_t* perm, const double* g,
                     int32_t half_width, double den_full, int32_t mode, int64_t n_rows, int32_t n_seg, int32_t n_pix,
                     hipEvent_t ev0, hipEvent_t ev1) {
  if (n_pix <= 0 || n_rows <= 0 || n_seg <= 0) return;
  if (half_width < 0 || half_width > kHpMaxHalf) throw Error(PROM_E_ARG, "k_highpass: half_width outside [0, 512]");
  const int64_t wgs = hp_workgroups(n_rows, n_seg);
  if (wgs > (((int64_t)1 << 31) - 1))
    throw Error(PROM_E_ARG, "k_highpass: n_exp n_trial n_seg too large for one launch");
  const dim3 grid((uint32_t)wgs);
  if (ev0) PROM_HIP(hipEventRecord(ev0, s));
  if (mode == 0)
    hipLaunchKernelGGL((k_highpass<0>), grid, dim3(kHpBlock), 0, s, model, seg_first, perm, g, half_width, den_full,
                       n_seg, n_pix);
  else
    hipLaunchKernelGGL((k_highpass<1>), grid, dim3(kHpBlock), 0, s, model, seg_first, perm, g, half_width, den_full,
                       n_seg, n_pix);
  PROM_HIP(hipGetLastError());
  if (ev1) PROM_HIP(hipEventRecord(ev1, s));
}

}  // namespace prom
