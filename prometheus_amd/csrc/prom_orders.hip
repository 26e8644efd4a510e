// Per-order moments on the device (prom_orders_set / prom_transit_expose_orders / prom_spectrum_expose_orders): the
// seven moments and n_used of the exposures' final model per (exposure, trial, echelle order), and per (exposure, trial)
// the totals of the Brogi & Line likelihood, chi-square and scaled chi-square over the kept orders.  Definitions in
// prom_hip.h.
//
//   k_expose          (prom_expose.hip, unchanged) model[e][j][p] = M, the unfiltered model of the whole table
//   k_highpass        (prom_highpass.hip, unchanged, on request) the high-pass in place
//   k_detrend         (prom_detrend.hip, unchanged, on request) the SYSREM filter in place, flag[j][p]
//   k_model_moments   (prom_detrend.hip, unchanged, on request) the lumped moments, with k_vmap_reduce
//   k_order_moments   orec[e][j][s] = {m0 .. m6, n_used} of the final model over order s
//   k_order_totals    tot[e][j] = {sum loglike_s, sum m6_s, sum chi2_scaled_s, sum n_used_s} over the entering orders
//
// k_order_moments: a workgroup of kOdBlock threads owns one (exposure, group of kOdTrials consecutive trials, order);
// thread r * kOdTile + t belongs to (trial r, position t of the current tile).  It walks the order's tiles in ascending
// order; a position reaches the model, the data, ivar and the flag through perm (the pixels lie sorted by wavelength,
// the orders interleaved where they overlap; a real order is a few contiguous runs, so a wave's reads stay coalesced
// per run).  The terms, the used rule and the butterfly are k_model_moments' text; lane t = 0 adds the tiles' sums in
// tile order and writes the record itself.  There is no chunk level, no partial buffer, no second kernel for the
// moments, no atomics and no LDS: one workgroup per order is deliberate (an order of 4,096 pixels is 128 serial tiles;
// the workgroups are n_exp x trial groups x orders, thousands with one trial).  The two trials of a wave read the same
// data, ivar and perm entries, which L1 serves.  The butterfly is the only cross-lane arithmetic and it stays inside
// the kOdTile lanes of one trial, so a record depends on its own (e, j, s) alone.
//
// k_order_totals: one thread per (exposure, trial of the batch) walks the orders' records in ascending s.
#include "prom_internal.h"
#include "order_index.h"

namespace prom {

static_assert(kOdTile == 32 && kOdBlock == 256, "one thread per (position, trial) of a tile, two trials per wave");
static_assert(kOdTile == kVmTile && kOdTrials == kVmTrials, "the tile and the trial group are k_model_moments'");

__global__ void __launch_bounds__(kOdBlock) k_order_moments(const double* __restrict__ model,
                                                             const uint8_t* __restrict__ flag,
                                                             const double* __restrict__ data,
                                                             const double* __restrict__ ivar,
                                                             const int32_t* __restrict__ seg_first,
                                                             const int32_t* __restrict__ perm, int32_t n_pix,
                                                             int32_t n_trial, int32_t j_first, int32_t nb,
                                                             int32_t n_groups, int32_t n_seg,
                                                             double* __restrict__ orec) {
  const int32_t tid = threadIdx.x;
  const int32_t s = od_wg_segment(blockIdx.x, n_seg), gb = od_wg_group(blockIdx.x, n_groups, n_seg);
  const int32_t e = od_wg_exposure(blockIdx.x, n_groups, n_seg);
  const int32_t jb0 = od_group_first(gb);                    // first trial of the group inside the batch
  const int32_t nt = nb - jb0 < kOdTrials ? nb - jb0 : kOdTrials;
  const int32_t r = od_thread_trial(tid), t = od_thread_pos(tid);
  const int32_t first = seg_first[s], n = seg_first[s + 1] - first;
  double acc[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) acc[i] = 0.0;
  int64_t cnt = 0;
  const int32_t ntile = od_tiles(n);
  for (int32_t tile = 0; tile < ntile; ++tile) {
    const bool live = r < nt && t < od_tile_count(tile, n);
    // the terms of this thread's position, added over the tile's positions in a fixed shape
    double tm[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) tm[i] = 0.0;
    int32_t c = 0;
    if (live) {
      const int32_t j = j_first + jb0 + r;
      const int32_t p = perm[od_perm_at(first, od_tile_first(tile) + t)];
      const int64_t at = ex_data(e, p, n_pix);
      const double iv = ivar[at], d = data[at];
      const double M = model[ex_model(e, j, p, n_trial, n_pix)];
      const bool ok = flag[dt_flag(j, p, n_pix)] != 0;
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
    for (int m = 1; m < kOdTile; m <<= 1) {
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
    const int64_t slot = od_record(e, jb0 + r, s, nb, n_seg);
#pragma unroll
    for (int i = 0; i < 7; ++i) orec[slot + i] = acc[i];
    reinterpret_cast<int64_t*>(orec)[slot + 7] = cnt;
  }
}

__global__ void __launch_bounds__(kOdBlock) k_order_totals(const double* __restrict__ orec,
                                                            const uint8_t* __restrict__ keep, int32_t n_exp,
                                                            int32_t n_trial, int32_t j_first, int32_t nb, int32_t n_seg,
                                                            double* __restrict__ tot) {
  const int64_t i = (int64_t)blockIdx.x * kOdBlock + threadIdx.x;
  if (i >= (int64_t)n_exp * nb) return;
  const int32_t e = (int32_t)(i / nb), jb = (int32_t)(i % nb);
  double ll = 0.0, chi2 = 0.0, scaled = 0.0, count = 0.0;
  for (int32_t s = 0; s < n_seg; ++s) {
    const double* m = orec + od_record(e, jb, s, nb, n_seg);
    const int64_t nu = reinterpret_cast<const int64_t*>(m)[7];
    if (!od_enters(keep[s], nu)) continue;
    ll = dt_add(ll, od_loglike(nu, log(od_log_argument(m))));
    chi2 = dt_add(chi2, m[6]);
    scaled = dt_add(scaled, od_chi2_scaled(m));
    count = dt_add(count, (double)nu);
  }
  double* out = tot + od_total(e, j_first + jb, n_trial);
  out[0] = ll;
  out[1] = chi2;
  out[2] = scaled;
  out[3] = count;
}

void launch_order_moments(hipStream_t s, const double* model, const uint8_t* flag, const double* data,
                          const double* ivar, const int32_t* seg_first, const int32_t* perm, int32_t n_pix,
                          int32_t n_exp, int32_t n_trial, int32_t j_first, int32_t nb, int32_t n_seg, double* orec,
                          hipEvent_t ev0, hipEvent_t ev1) {
  if (n_pix <= 0 || n_exp <= 0 || nb <= 0 || n_seg <= 0) return;
  const int32_t n_groups = od_groups(nb);
  const int64_t wgs = od_workgroups(n_exp, n_groups, n_seg);
  if (wgs > (((int64_t)1 << 31) - 1))
    throw Error(PROM_E_ARG, "k_order_moments: n_exp, the batch's trial groups and n_seg too large for one launch");
  if (ev0) PROM_HIP(hipEventRecord(ev0, s));
  hipLaunchKernelGGL(k_order_moments, dim3((uint32_t)wgs), dim3(kOdBlock), 0, s, model, flag, data, ivar, seg_first, perm,
                     n_pix, n_trial, j_first, nb, n_groups, n_seg, orec);
  PROM_HIP(hipGetLastError());
  if (ev1) PROM_HIP(hipEventRecord(ev1, s));
}

void launch_order_totals(hipStream_t s, const double* orec, const uint8_t* keep, int32_t n_exp, int32_t n_trial,
                         int32_t j_first, int32_t nb, int32_t n_seg, double* tot, hipEvent_t ev0, hipEvent_t ev1) {
  if (n_exp <= 0 || nb <= 0 || n_seg <= 0) return;
  const int64_t blocks = ((int64_t)n_exp * nb + kOdBlock - 1) / kOdBlock;
  if (ev0) PROM_HIP(hipEventRecord(ev0, s));
  hipLaunchKernelGGL(k_order_totals, dim3((uint32_t)blocks), dim3(kOdBlock), 0, s, orec, keep, n_exp, n_trial, j_first,
                     nb, n_seg, tot);
  PROM_HIP(hipGetLastError());
  if (ev1) PROM_HIP(hipEventRecord(ev1, s));
}

}  // namespace prom
