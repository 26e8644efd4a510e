// Index arithmetic and the totals' formulas of the per-order moments (prom_orders.hip): the (exposure, trial group,
// order) a workgroup of k_order_moments owns, the tiles it walks, the entry of perm a position reads, the slot of a
// record, the batches under the scratch cap, and the statistics k_order_totals forms from a record (the definition in
// prom_hip.h, "per-order moments on the device").  A model value's slot is expose_index.h's ex_model, the data's
// ex_data, a flag's detrend_index.h's dt_flag; the group of trials is vmap_index.h's.
//
// Plain inline functions shared by the kernels and by the host harness (tests/helpers/order_host.cpp,
// tests/test_order_moments_cpu.py), which walks every (exposure, trial group, order, tile, thread) with the same text.
//
// The invariants: every entry of perm a workgroup reads lies inside its order's stretch of perm[n_pix]; every model,
// data and flag value inside its array; a record lies inside the batch's orec[n_exp][nb][n_seg][kOdRecord] and is
// written exactly once; a total's slot inside tot[n_exp][n_trial][kOdTotals].
//
// The constants can be overridden at compile time (PROM_OD_*): the host harness is also built with small ones.  The
// kernels are built with the defaults only.
//
// Rounding: every product, quotient, sum and difference of the totals' formulas is rounded on its own (__dmul_rn /
// __ddiv_rn / __dadd_rn on the device, plain operators in a translation unit built with -ffp-contract=off on the host).
#pragma once

#include "detrend_index.h"

#ifndef PROM_OD_TILE
#define PROM_OD_TILE ::prom::kVmTile
#endif
#ifndef PROM_OD_TRIALS
#define PROM_OD_TRIALS ::prom::kVmTrials
#endif

namespace prom {

constexpr int kOdTile = PROM_OD_TILE;           // consecutive positions of a tile: the butterfly's width (k_model_moments')
constexpr int kOdTrials = PROM_OD_TRIALS;       // consecutive trials of a workgroup
constexpr int kOdBlock = kOdTile * kOdTrials;   // threads of a workgroup: one per (trial, position) of a tile
constexpr int kOdRecord = 8;                    // doubles of a record: m0 .. m6 and n_used (int64 bits)
constexpr int kOdTotals = 4;                    // doubles of (e, j)'s totals: loglike, chi2, chi2_scaled, n_used
static_assert((kOdTile & (kOdTile - 1)) == 0 && kOdTile >= 1 && kOdTile <= 64, "the butterfly stays inside a wave");

// ---- the workgroup's share: blockIdx.x = (e * n_groups + group_in_batch) * n_seg + order ---------------------------
PROM_OBS_HD int32_t od_groups(int32_t n_trial) { return (n_trial + kOdTrials - 1) / kOdTrials; }
PROM_OBS_HD int32_t od_group_first(int32_t group) { return group * kOdTrials; }
PROM_OBS_HD int64_t od_workgroups(int32_t n_exp, int32_t n_groups, int32_t n_seg) {
  return (int64_t)n_exp * n_groups * n_seg;
}
PROM_OBS_HD int32_t od_wg_segment(int32_t bx, int32_t n_seg) { return bx % n_seg; }
PROM_OBS_HD int32_t od_wg_group(int32_t bx, int32_t n_groups, int32_t n_seg) { return (bx / n_seg) % n_groups; }
PROM_OBS_HD int32_t od_wg_exposure(int32_t bx, int32_t n_groups, int32_t n_seg) { return (bx / n_seg) / n_groups; }
// thread tid = r * kOdTile + t belongs to (trial r of the group, position t of the current tile)
PROM_OBS_HD int32_t od_thread_trial(int32_t tid) { return tid / kOdTile; }
PROM_OBS_HD int32_t od_thread_pos(int32_t tid) { return tid % kOdTile; }

// ---- tiles of an order of n positions --------------------------------------------------------------------------------
PROM_OBS_HD int32_t od_tiles(int32_t n) { return (n + kOdTile - 1) / kOdTile; }
PROM_OBS_HD int32_t od_tile_first(int32_t tile) { return tile * kOdTile; }
PROM_OBS_HD int32_t od_tile_count(int32_t tile, int32_t n) {
  const int32_t r = n - tile * kOdTile;
  return r < kOdTile ? r : kOdTile;
}
// the entry of perm that holds the device pixel of position i in the order that starts at entry `first`
PROM_OBS_HD int32_t od_perm_at(int32_t first, int32_t i) { return first + i; }

// ---- records, totals and batches -------------------------------------------------------------------------------------
// orec[e][jb][s][kOdRecord] of a batch of nb trials (jb = j - first trial of the batch): the record's first double
PROM_OBS_HD int64_t od_record(int32_t e, int32_t jb, int32_t s, int32_t nb, int32_t n_seg) {
  return (((int64_t)e * nb + jb) * n_seg + s) * kOdRecord;
}
PROM_OBS_HD int64_t od_record_doubles(int32_t n_exp, int32_t nb, int32_t n_seg) {
  return (int64_t)n_exp * nb * n_seg * kOdRecord;
}
// tot[e][j][kOdTotals] of the whole table
PROM_OBS_HD int64_t od_total(int32_t e, int32_t j, int32_t n_trial) { return ((int64_t)e * n_trial + j) * kOdTotals; }
// trial groups a batch may hold under a scratch cap in bytes (one at least), the grid below 2^31
PROM_OBS_HD int32_t od_batch_groups(int64_t cap_bytes, int32_t n_exp, int32_t n_seg, int32_t n_groups) {
  const int64_t per_group = od_record_doubles(n_exp, kOdTrials, n_seg) * 8;
  int64_t g = per_group > 0 ? cap_bytes / per_group : n_groups;
  if (g < 1) g = 1;
  const int64_t per_grid = od_workgroups(n_exp, 1, n_seg);
  const int64_t gmax = (((int64_t)1 << 31) - 1) / (per_grid > 0 ? per_grid : 1);
  if (g > gmax) g = gmax;   // (the launcher has refused a table whose single group is too large already)
  if (g < 1) g = 1;
  return g < n_groups ? (int32_t)g : n_groups;
}

// ---- separately rounded arithmetic (the products and sums are detrend_index.h's dt_mul / dt_add) ---------------------
PROM_OBS_HD double od_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}
// observation._ratio: a / b, NaN where b == 0
PROM_OBS_HD double od_ratio(double a, double b) { return b == 0.0 ? __builtin_nan("") : od_div(a, b); }

// ---- the statistics of one record, in the order observation.VelocityMap evaluates them -------------------------------
// chi2_scaled = m5 - m4 m4 / m3
PROM_OBS_HD double od_chi2_scaled(const double* m) { return dt_add(m[5], -od_ratio(dt_mul(m[4], m[4]), m[3])); }
// the argument of loglike's logarithm: s_f^2 - 2 C + s_g^2
PROM_OBS_HD double od_log_argument(const double* m) {
  const double sf = od_ratio(dt_add(m[5], -od_ratio(dt_mul(m[2], m[2]), m[0])), m[0]);
  const double sg = od_ratio(dt_add(m[3], -od_ratio(dt_mul(m[1], m[1]), m[0])), m[0]);
  const double ccf = dt_add(m[4], -od_ratio(dt_mul(m[1], m[2]), m[0]));
  const double c = od_ratio(ccf, m[0]);
  return dt_add(dt_add(sf, -dt_mul(2.0, c)), sg);
}
// loglike = (-0.5 n_used) ln(argument); `lg` is the logarithm of od_log_argument
PROM_OBS_HD double od_loglike(int64_t n_used, double lg) { return dt_mul(dt_mul(-0.5, (double)n_used), lg); }
// an order enters the totals when it is kept and has two used positions at least
PROM_OBS_HD bool od_enters(uint8_t keep, int64_t n_used) { return keep != 0 && n_used >= 2; }

}  // namespace prom
