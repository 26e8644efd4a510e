// Detrended exposures on the device (prom_detrend_set / prom_transit_expose_detrended /
// prom_spectrum_expose_detrended): the exposures' models with a systematics basis projected out per pixel column,
// M' = M - U (W_p M), and the seven moments of M' against the data.  Definitions in prom_hip.h.
//
//   k_expose          (prom_expose.hip, unchanged) model[e][j][p] = M_e, the unfiltered model of the whole table
//   k_detrend         model[e][j][p] = M'_e in place; flag[j][p] = the column is filterable
//   k_model_moments   part[e][j][chunk] = {m0 .. m6, n_used} of a model that lies in memory
//   k_vmap_reduce     (prom_vmap.hip, with the exposure in the phase's place) the chunks' records in chunk order
//
// k_detrend: a thread owns one column (trial j, pixel p) of the model; a workgroup takes kDtTile consecutive pixels
// of kDtTrials consecutive trials, so a wave reads and writes along p.  Pass 1 walks the exposures and keeps the
// n_comp coefficients in registers (the kernel is compiled once per n_comp: no indexed register array, no scratch);
// pass 2 walks them again and writes M' over M.  Only the column's thread touches the column, so the pass needs no
// barrier and no second buffer.  The out-of-place form (OUT, the recovery grids) reads the column from `src`, another
// buffer of the same shape that stays untouched, and writes it to `model`: the same thread, the same values in the same
// order, so the bits are the in-place form's, whose instantiation is what it was.  The trials of a workgroup read the same W[k][e][p0 .. p0 + 63] lines at the same
// step: they share them through the compute unit's L1 (and the workgroups of other trial groups through L2), not
// through LDS.  U[e][k] is uniform over the workgroup: scalar loads.  There is no cross-lane arithmetic, so the
// bits do not depend on the layout.
//
// k_model_moments is k_vmap's step 4 alone with k_expose's shape: a workgroup takes one exposure, kVmChunk consecutive
// tiles of kVmTile pixels and kVmTrials consecutive trials; thread r * kVmTile + t belongs to (trial r, pixel t) of
// the current tile.  The terms, the butterfly, the tile order and the record are k_expose's text, so for a model
// without NaN and U = 0 the eight numbers are prom_spectrum_expose's bit for bit.  No atomics.
#include "prom_internal.h"
#include "detrend_index.h"
#include "order_sysrem_index.h"

namespace prom {

static_assert(kDtBlock == 256 && kDtTile == 64, "a wave of k_detrend reads 64 consecutive pixels of one trial");
static_assert(kVmTile == 32 && kVmTile * kVmTrials == kVmBlock, "one thread per (pixel, trial) of a tile");

template <int NC, bool OUT>
__global__ void __launch_bounds__(kDtBlock) k_detrend(double* __restrict__ model, const double* __restrict__ src,
                                                       const double* __restrict__ U, const double* __restrict__ W,
                                                       uint8_t* __restrict__ flag, int32_t n_exp, int32_t n_trial,
                                                       int32_t n_pix, int32_t n_tiles) {
  const int32_t tid = threadIdx.x;
  const int32_t p = dt_pixel(dt_wg_tile(blockIdx.x, n_tiles), tid);
  const int32_t j = dt_trial(dt_wg_group(blockIdx.x, n_tiles), tid);
  if (p >= n_pix || j >= n_trial) return;
  double* M = model + ex_model(0, j, p, n_trial, n_pix);
  const double* S = OUT ? src + ex_model(0, j, p, n_trial, n_pix) : M;   // (in place: src is not looked at)
  const int64_t m_stride = (int64_t)n_trial * n_pix;
  double c[NC];
  const bool ok = dt_coefficients<NC>(S, m_stride, W + dt_w(0, 0, p, n_exp, n_pix), n_pix, n_exp, c);
  dt_apply<NC>(S, M, m_stride, U, n_exp, c, ok);
  flag[dt_flag(j, p, n_pix)] = ok ? 1 : 0;
}

// The per-order instantiation (a per-order filter resident, prom_detrend_set_orders / prom_detrend_build_orders):
// k_detrend's text with the U pointer moved per lane by seg_of[p] n_exp NC, the basis of p's own order; W is per pixel
// already.  U becomes a vector load.  A kernel of its own, so that k_detrend's instantiations are what they were.
template <int NC, bool OUT>
__global__ void __launch_bounds__(kDtBlock) k_detrend_orders(double* __restrict__ model, const double* __restrict__ src,
                                                              const double* __restrict__ U,
                                                              const double* __restrict__ W,
                                                              const int32_t* __restrict__ seg_of,
                                                              uint8_t* __restrict__ flag, int32_t n_exp,
                                                              int32_t n_trial, int32_t n_pix, int32_t n_tiles) {
  const int32_t tid = threadIdx.x;
  const int32_t p = dt_pixel(dt_wg_tile(blockIdx.x, n_tiles), tid);
  const int32_t j = dt_trial(dt_wg_group(blockIdx.x, n_tiles), tid);
  if (p >= n_pix || j >= n_trial) return;
  double* M = model + ex_model(0, j, p, n_trial, n_pix);
  const double* S = OUT ? src + ex_model(0, j, p, n_trial, n_pix) : M;   // (in place: src is not looked at)
  const int64_t m_stride = (int64_t)n_trial * n_pix;
  double c[NC];
  const bool ok = dt_coefficients<NC>(S, m_stride, W + dt_w(0, 0, p, n_exp, n_pix), n_pix, n_exp, c);
  dt_apply<NC>(S, M, m_stride, U + fo_u(seg_of[p], n_exp, NC), n_exp, c, ok);
  flag[dt_flag(j, p, n_pix)] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(kVmBlock) k_model_moments(const double* __restrict__ model,
                                                             const uint8_t* __restrict__ flag,
                                                             const double* __restrict__ data,
                                                             const double* __restrict__ ivar, int32_t n_pix,
                                                             int32_t n_trial, int32_t j_first, int32_t nb,
                                                             int32_t n_chunks, double* __restrict__ part) {
  const int32_t tid = threadIdx.x;
  const int32_t e = blockIdx.y;
  const int32_t chunk = vm_wg_chunk(blockIdx.x, n_chunks), gb = vm_wg_group(blockIdx.x, n_chunks);
  const int32_t jb0 = vm_group_first(gb);                    // first trial of the group inside the batch
  const int32_t nt = nb - jb0 < kVmTrials ? nb - jb0 : kVmTrials;
  const int32_t r = vm_entry_trial(tid), t = vm_entry_pixel(tid);
  double acc[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) acc[i] = 0.0;
  int64_t cnt = 0;
  const int32_t tile0 = vm_chunk_first(chunk), ntile = vm_chunk_count(chunk, n_pix);
  for (int32_t ti = 0; ti < ntile; ++ti) {
    const int32_t p0 = vm_tile_first(tile0 + ti), np = vm_tile_count(tile0 + ti, n_pix);
    const bool live = r < nt && t < np;
    // the terms of this thread's pixel, added over the tile's pixels in a fixed shape
    double tm[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) tm[i] = 0.0;
    int32_t c = 0;
    if (live) {
      const int32_t j = j_first + jb0 + r;
      const int64_t at = ex_data(e, p0 + t, n_pix);
      const double iv = ivar[at], d = data[at];
      const double M = model[ex_model(e, j, p0 + t, n_trial, n_pix)];
      const bool ok = flag[dt_flag(j, p0 + t, n_pix)] != 0;
      if (iv > 0.0 && iv < __builtin_inf() && __builtin_fabs(d) < __builtin_inf() && ok && M == M) {
        const double ivM = iv * M, ivd = iv * d, df = M - d;
        tm[0] = iv;
        tm[1] = ivM;
        tm[2] = ivd;
        tm[3] = ivM * M;
        tm[4] = ivM * d;
        tm[5] = ivd * d;
        tm[6] = iv * (df * df);
        c = 1;
      }
    }
#pragma unroll
    for (int m = 1; m < kVmTile; m <<= 1) {
#pragma unroll
      for (int i = 0; i < 7; ++i) tm[i] += __shfl_xor(tm[i], m, 64);
      c += __shfl_xor(c, m, 64);
    }
    if (t == 0) {
#pragma unroll
      for (int i = 0; i < 7; ++i) acc[i] += tm[i];
      cnt += c;
    }
  }
  if (t == 0 && r < nt) {
    const int64_t slot = vm_part_slot(e, jb0 + r, chunk, nb, n_chunks);
#pragma unroll
    for (int i = 0; i < 7; ++i) part[slot + i] = acc[i];
    reinterpret_cast<int64_t*>(part)[slot + 7] = cnt;
  }
}

void launch_detrend(hipStream_t s, double* model, const double* U, const double* W, uint8_t* flag, int32_t n_exp,
                    int32_t n_comp, int32_t n_trial, int32_t n_pix, hipEvent_t ev0, hipEvent_t ev1, const double* src,
                    const int32_t* seg_of) {
  if (n_pix <= 0 || n_exp <= 0 || n_trial <= 0) return;
  if (n_comp < 1 || n_comp > kDtMaxComp) throw Error(PROM_E_ARG, "k_detrend: n_comp outside [1, 16]");
  const int64_t wgs = dt_workgroups(n_trial, n_pix);
  if (wgs > (((int64_t)1 << 31) - 1)) throw Error(PROM_E_ARG, "k_detrend: n_trial n_pix too large for one launch");
  const dim3 grid((uint32_t)wgs);
  const int32_t n_tiles = dt_tiles(n_pix);
  if (ev0) PROM_HIP(hipEventRecord(ev0, s));
  switch (n_comp) {
#define PROM_DT_CASE(NC)                                                                                        \
  case NC:                                                                                                      \
    if (seg_of && src && src != model)                                                                          \
      hipLaunchKernelGGL((k_detrend_orders<NC, true>), grid, dim3(kDtBlock), 0, s, model, src, U, W, seg_of,    \
                         flag, n_exp, n_trial, n_pix, n_tiles);                                                 \
    else if (seg_of)                                                                                            \
      hipLaunchKernelGGL((k_detrend_orders<NC, false>), grid, dim3(kDtBlock), 0, s, model, nullptr, U, W,       \
                         seg_of, flag, n_exp, n_trial, n_pix, n_tiles);                                         \
    else if (src && src != model)                                                                               \
      hipLaunchKernelGGL((k_detrend<NC, true>), grid, dim3(kDtBlock), 0, s, model, src, U, W, flag, n_exp,      \
                         n_trial, n_pix, n_tiles);                                                              \
    else                                                                                                        \
      hipLaunchKernelGGL((k_detrend<NC, false>), grid, dim3(kDtBlock), 0, s, model, nullptr, U, W, flag, n_exp, \
                         n_trial, n_pix, n_tiles);                                                              \
    break;
    PROM_DT_CASE(1) PROM_DT_CASE(2) PROM_DT_CASE(3) PROM_DT_CASE(4) PROM_DT_CASE(5) PROM_DT_CASE(6) PROM_DT_CASE(7)
    PROM_DT_CASE(8) PROM_DT_CASE(9) PROM_DT_CASE(10) PROM_DT_CASE(11) PROM_DT_CASE(12) PROM_DT_CASE(13)
    PROM_DT_CASE(14) PROM_DT_CASE(15) PROM_DT_CASE(16)
#undef PROM_DT_CASE
  }
  PROM_HIP(hipGetLastError());
  if (ev1) PROM_HIP(hipEventRecord(ev1, s));
}

void launch_model_moments(hipStream_t s, const double* model, const uint8_t* flag, const double* data,
                          const double* ivar, int32_t n_pix, int32_t n_exp, int32_t n_trial, int32_t j_first,
                          int32_t nb, double* part, hipEvent_t ev0, hipEvent_t ev1) {
  if (n_pix <= 0 || n_exp <= 0 || nb <= 0) return;
  const int32_t n_chunks = vm_chunks(n_pix);
  const dim3 grid((uint32_t)(vm_groups(nb) * n_chunks), (uint32_t)n_exp);
  if (ev0) PROM_HIP(hipEventRecord(ev0, s));
  hipLaunchKernelGGL(k_model_moments, grid, dim3(kVmBlock), 0, s, model, flag, data, ivar, n_pix, n_trial, j_first, nb,
                     n_chunks, part);
  PROM_HIP(hipGetLastError());
  if (ev1) PROM_HIP(hipEventRecord(ev1, s));
}

}  // namespace prom
