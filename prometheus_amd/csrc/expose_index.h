// Index arithmetic of k_expose (prom_expose.hip) that is its own: the entries of the exposure table a workgroup reads
// (a tap's row and weight, a (trial, tap)'s factor), the row of R a tap reads, the exposure's data and the slot of a
// model value.  Everything else -- the chunk of tiles and the group of trials a workgroup takes, the bracketed
// searches, the stage, a support's points and the slot of a partial record (with the exposure in the phase's place)
// -- is vmap_index.h's, unchanged.
//
// Plain inline functions shared by the kernel and by the host harness (tests/helpers/expose_host.cpp,
// tests/test_expose_cpu.py), which walks every (batch, exposure, chunk, trial group, tile, tap, pixel, trial) with the
// same text and checks every index the kernel would form.
//
// The invariants: a tap's entry lies inside row[n_exp][n_tap] and a[n_exp][n_tap]; a factor's inside
// F[n_exp][n_trial][n_tap]; a live tap's row of R lies inside R[n_orb][n_wav] (prom_expose_set admits rows in
// [0, n_orb) only); a data entry lies inside data[n_exp][n_pix]; a model value lies inside
// model[n_exp][n_trial][n_pix] and is written exactly once.
#pragma once

#include "vmap_index.h"

namespace prom {

// row[e][i] and a[e][i]
PROM_OBS_HD int64_t ex_tap(int32_t e, int32_t i, int32_t n_tap) { return (int64_t)e * n_tap + i; }
// F[e][j][i]
PROM_OBS_HD int64_t ex_factor(int32_t e, int32_t j, int32_t i, int32_t n_trial, int32_t n_tap) {
  return ((int64_t)e * n_trial + j) * n_tap + i;
}
// a tap is live when its weight is > 0 (a dead tap is skipped: nothing of it is read but the weight)
PROM_OBS_HD bool ex_live(double a) { return a > 0.0; }
// the first value of a tap's row of R
PROM_OBS_HD int64_t ex_row_first(int32_t row, int32_t n_wav) { return (int64_t)row * n_wav; }
// data[e][p] and ivar[e][p]
PROM_OBS_HD int64_t ex_data(int32_t e, int32_t p, int32_t n_pix) { return (int64_t)e * n_pix + p; }
// model[e][j][p]
PROM_OBS_HD int64_t ex_model(int32_t e, int32_t j, int32_t p, int32_t n_trial, int32_t n_pix) {
  return ((int64_t)e * n_trial + j) * n_pix + p;
}

}  // namespace prom
