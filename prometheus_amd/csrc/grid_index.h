// Index arithmetic of the injection grids (prom_*_inject_grid / prom_*_recover_grid, prom_hip.h "injection grids on
// the device"): where injection b of a sub-batch keeps its slice of every per-injection buffer, the threads of the two
// kernels the grid adds (k_gather_grid, k_inject_grid), and the planner that cuts a list of injections into
// sub-batches under a byte cap.
//
// Plain inline functions shared by the kernels (prom_sysrem.hip, prom_filter.hip), the C-ABI layer
// (prom_api_inject.hip) and the host harness (tests/helpers/grid_host.cpp, tests/test_inject_grid_cpu.py), which walks
// every thread of every batched kernel with this text.  The arithmetic of an entry is not here: it stays sy_* of
// sysrem_index.h, fw_* of filter_index.h and dt_* of detrend_index.h, so the bits of injection b are the single call's.
//
// The layout: a per-injection buffer of the single call with n entries becomes [B][n], injection b's slice first to
// last, so every kernel of the single call runs on b's slice with its own index functions after one offset, and the
// single call is the batch of one (offset 0): the C-ABI layer runs it as a list of one.  The injection is blockIdx.y of every batched launch.  The two buffers
// k_expose writes and reads keep its layout with the injection in the trial's place: Fj[e][b][tap] and model[e][b][p].
// The flags are [B][kGrFlags]: a component that ends sets flag `col` of its own row and nothing else.
#pragma once

#include "filter_index.h"
#include "sysrem_index.h"

namespace prom {

constexpr int kGrFlags = kSyMaxComp + 1;     // `ended` flags of one injection (one per column of U; the row's length)
constexpr int kGrMaxBatch = 65535;           // injections of a sub-batch at most: blockIdx.y of one launch

// ---- injection b's slice of a per-injection buffer ------------------------------------------------------------------
// D, out (cleaned): [B][n_exp][n_pix]
PROM_OBS_HD int64_t gr_data(int32_t b, int32_t n_exp, int32_t n_pix) { return (int64_t)b * n_exp * n_pix; }
// r, w: [B][n_exp][pitch]
PROM_OBS_HD int64_t gr_work(int32_t b, int32_t n_exp, int64_t pitch) { return (int64_t)b * n_exp * pitch; }
// a: [B][n_exp]
PROM_OBS_HD int64_t gr_a(int32_t b, int32_t n_exp) { return (int64_t)b * n_exp; }
// part: [B][n_exp][n_tiles] pairs
PROM_OBS_HD int64_t gr_part(int32_t b, int32_t n_exp, int32_t n_tiles) { return (int64_t)b * n_exp * n_tiles; }
// U: [B][n_exp][n_cols]
PROM_OBS_HD int64_t gr_u(int32_t b, int32_t n_exp, int32_t n_cols) { return (int64_t)b * n_exp * n_cols; }
// W: [B][n_cols][n_exp][n_pix]
PROM_OBS_HD int64_t gr_w(int32_t b, int32_t n_cols, int32_t n_exp, int32_t n_pix) {
  return (int64_t)b * n_cols * n_exp * n_pix;
}
// ended: flag `col` of injection b
PROM_OBS_HD int64_t gr_flag(int32_t b, int32_t col) { return (int64_t)b * kGrFlags + col; }

// ---- k_gather_grid: thread i of blockIdx.x owns (e, tap); Fj[e][b][tap] = F[e][trial[b]][tap] ----------------------
PROM_OBS_HD int64_t gr_gather_from(int32_t e, int32_t trial, int32_t tap, int32_t n_trial, int32_t n_tap) {
  return ex_factor(e, trial, tap, n_trial, n_tap);
}
PROM_OBS_HD int64_t gr_gather_to(int32_t e, int32_t b, int32_t tap, int32_t n_inj, int32_t n_tap) {
  return ex_factor(e, b, tap, n_inj, n_tap);
}
// ---- k_inject_grid: thread i of blockIdx.x owns (e, p); D[b][e][p] of raw[e][p] and model[e][b][p] ------------------
PROM_OBS_HD int64_t gr_inject_model(int32_t e, int32_t b, int32_t p, int32_t n_inj, int32_t n_pix) {
  return ex_model(e, b, p, n_inj, n_pix);
}
PROM_OBS_HD int64_t gr_inject_to(int32_t b, int32_t e, int32_t p, int32_t n_exp, int32_t n_pix) {
  return gr_data(b, n_exp, n_pix) + ex_data(e, p, n_pix);
}

// ---- the sub-batches ----------------------------------------------------------------------------------------------------
// bytes of the work buffers one injection adds to a sub-batch: D, out, the injected model, r, w, a, part, U, Fj, the
// flags and, for a recovery, W
PROM_OBS_HD int64_t gr_injection_bytes(int32_t n_exp, int32_t n_pix, int32_t n_cols, int32_t n_tap, bool recover) {
  const int64_t n = (int64_t)n_exp * n_pix, work = (int64_t)n_exp * sy_pitch(n_pix);
  int64_t d = 3 * n + 2 * work + n_exp + 2 * (int64_t)n_exp * sy_tiles(n_pix) + (int64_t)n_exp * n_cols +
              (int64_t)n_exp * n_tap;
  if (recover) d += (int64_t)n_cols * n;
  return 8 * d + 4 * kGrFlags;
}
// injections of a sub-batch under `cap` bytes: one at least, kGrMaxBatch and the list at most
PROM_OBS_HD int32_t gr_sub_batch(int64_t cap, int64_t per_injection, int32_t n_inj) {
  int64_t nb = per_injection > 0 ? cap / per_injection : kGrMaxBatch;
  if (nb < 1) nb = 1;
  if (nb > kGrMaxBatch) nb = kGrMaxBatch;
  if (nb > n_inj) nb = n_inj;
  return (int32_t)nb;
}
// sub-batch s holds the injections [gr_sub_first(s, nb), ... + gr_sub_count(s, nb, n_inj))
PROM_OBS_HD int32_t gr_sub_batches(int32_t n_inj, int32_t nb) { return nb > 0 ? (n_inj + nb - 1) / nb : 0; }
PROM_OBS_HD int32_t gr_sub_first(int32_t s, int32_t nb) { return s * nb; }
PROM_OBS_HD int32_t gr_sub_count(int32_t s, int32_t nb, int32_t n_inj) {
  const int32_t left = n_inj - s * nb;
  return left < nb ? left : nb;
}

}  // namespace prom
