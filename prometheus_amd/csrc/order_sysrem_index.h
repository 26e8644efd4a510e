// Index arithmetic of SYSREM per echelle order on the device (prom_sysrem_clean_orders, prom_*_inject_orders,
// prom_*_inject_grid_orders; prom_hip.h "SYSREM per order on the device"): an order is one more batch item of the
// SYSREM kernels.  Batch item y = b n_seg + s of the pitched work buffers, of a, of the partials, of U and of the flags
// is order s of injection b; every item has the common width n_max = max n_s, so k_sysrem_fill, k_sysrem_step and
// k_sysrem_rows run unchanged with n_inj n_seg items and n_pix = n_max.  Two kernels are the orders' own:
//   k_sysrem_prep_orders    item y, exposure e, position i < pitch: w and r from D[b][e][perm[first_s + i]] and
//                           ivar[e][perm[first_s + i]] for i < n_s, w = 0 and r = +0 beyond
//   k_sysrem_finish_orders  item y, exposure e, position i < n_s: out[b][e][perm[first_s + i]]
//
// Plain inline functions shared by the kernels (prom_sysrem.hip), the C-ABI layer (prom_api_inject.hip) and the host
// harness (tests/helpers/order_sysrem_host.cpp, tests/test_sysrem_orders_cpu.py), which walks every thread of the two
// kernels with this text.  The arithmetic of an entry stays sy_* of sysrem_index.h.
//
// The lemma the layout rests on (the harness checks it on values): padding an order from n_s to n_max appends whole
// tiles whose partials are {+0, +0} and, inside the order's last tile, lanes whose sums stay +0.  Every lane and row
// sum starts at +0 and a sum of two values is -0 only when both are -0, so no sum is ever -0; adding +0 to a value
// that is not -0 leaves its bits.  The padded item's row sums are therefore the single call's on n_s pixels: the shape
// of a row sum is a function of n_s alone.
//
// Unequal orders pay for the padding (every item is n_max wide).  Echelle orders have equal pixel counts; no compacted
// layout is built.
#pragma once

#include "grid_index.h"

namespace prom {

// ---- the items ----------------------------------------------------------------------------------------------------------
PROM_OBS_HD int32_t os_item(int32_t b, int32_t s, int32_t n_seg) { return b * n_seg + s; }
PROM_OBS_HD int32_t os_item_injection(int32_t y, int32_t n_seg) { return y / n_seg; }
PROM_OBS_HD int32_t os_item_order(int32_t y, int32_t n_seg) { return y % n_seg; }
// the common width: the longest order (0 without a pixel)
PROM_OBS_HD int32_t os_n_max(int32_t n_seg, const int32_t* seg_first) {
  int32_t m = 0;
  for (int32_t s = 0; s < n_seg; ++s) {
    const int32_t n = seg_first[s + 1] - seg_first[s];
    if (n > m) m = n;
  }
  return m;
}
// the slot of position i of order s in perm
PROM_OBS_HD int32_t os_slot(const int32_t* seg_first, int32_t s, int32_t i) { return seg_first[s] + i; }
// D[b][e][p], out[b][e][p] of the table's pixel p
PROM_OBS_HD int64_t os_data(int32_t b, int32_t e, int32_t p, int32_t n_exp, int32_t n_pix) {
  return gr_data(b, n_exp, n_pix) + ex_data(e, p, n_pix);
}
// r[y][e][i], w[y][e][i] of the pitched work buffers (pitch = sy_pitch(n_max))
PROM_OBS_HD int64_t os_work(int32_t y, int32_t e, int32_t i, int32_t n_exp, int64_t pitch) {
  return gr_work(y, n_exp, pitch) + sy_at(e, i, pitch);
}
// U_out[b][s][e][col] is item y's slice of U: gr_u(y, n_exp, n_cols) + sy_u(e, col, n_cols)

// ---- the per-order filter ---------------------------------------------------------------------------------------------
// U[n_seg][n_exp][K]: the basis of order s; k_filter_weights_orders and k_detrend_orders move U by it per lane
PROM_OBS_HD int64_t fo_u(int32_t s, int32_t n_exp, int32_t n_comp) { return (int64_t)s * n_exp * n_comp; }
// seg_of[p]: the order of the device pixel p, formed on the host from the resident orders
inline void fo_seg_of(int32_t n_seg, const int32_t* seg_first, const int32_t* perm, int32_t* seg_of) {
  for (int32_t s = 0; s < n_seg; ++s)
    for (int32_t i = seg_first[s]; i < seg_first[s + 1]; ++i) seg_of[perm[i]] = s;
}

// ---- the sub-batches --------------------------------------------------------------------------------------------------
// bytes of the work buffers one injection adds to a sub-batch: D, out and the injected model over the table, Fj, and
// per order r, w (pitched to n_max), a, part, U and the flags
PROM_OBS_HD int64_t os_injection_bytes(int32_t n_exp, int32_t n_pix, int32_t n_seg, int32_t n_max, int32_t n_cols,
                                       int32_t n_tap) {
  const int64_t n = (int64_t)n_exp * n_pix, work = (int64_t)n_exp * sy_pitch(n_max);
  const int64_t per_order = 2 * work + n_exp + 2 * (int64_t)n_exp * sy_tiles(n_max) + (int64_t)n_exp * n_cols;
  return 8 * (3 * n + (int64_t)n_exp * n_tap + n_seg * per_order) + 4 * (int64_t)kGrFlags * n_seg;
}
// injections of a sub-batch under `cap` bytes: one at least, the list at most, and n_inj_sub n_seg <= kGrMaxBatch
// (0: n_seg alone is above kGrMaxBatch, no launch can hold one injection)
PROM_OBS_HD int32_t os_sub_batch(int64_t cap, int64_t per_injection, int32_t n_inj, int32_t n_seg) {
  if (n_seg < 1 || n_seg > kGrMaxBatch) return 0;
  int32_t nb = gr_sub_batch(cap, per_injection, n_inj);
  if (nb > kGrMaxBatch / n_seg) nb = kGrMaxBatch / n_seg;
  return nb;
}

}  // namespace prom
