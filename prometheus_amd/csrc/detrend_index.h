// Index arithmetic and the two per-column functions of the detrended exposures (prom_detrend.hip): the column
// (trial j, pixel p) a thread of k_detrend owns, the entries of the filter it reads (U[e][k], W[k][e][p]), the flag
// it writes, and the coefficients / apply steps of the definition in prom_hip.h ("detrended exposures on the
// device").  A model value's slot is expose_index.h's ex_model, the data's ex_data; the chunk of tiles, the group of
// trials and the partial record of k_model_moments are vmap_index.h's, unchanged.
//
// Plain inline functions shared by the kernels and by the host harness (tests/helpers/detrend_host.cpp,
// tests/test_detrend_cpu.py), which walks every thread's indices with the same text and evaluates the two column
// functions against values it is given.
//
// The invariants: a column's thread is the only one that reads or writes model[.][j][p] in k_detrend and writes
// flag[j][p] exactly once; every U entry lies inside U[n_exp][n_comp], every W entry inside W[n_comp][n_exp][n_pix].
//
// Rounding: every product and every sum of the column functions is rounded on its own.  On the device they are
// __dmul_rn / __dadd_rn, which the compiler never fuses; on the host plain operators in a translation unit built
// with -ffp-contract=off.
#pragma once

#include "expose_index.h"

namespace prom {

constexpr int kDtMaxComp = 16;   // components of a filter at most
constexpr int kDtTile = 64;      // consecutive pixels of a k_detrend workgroup: one wave reads along p
constexpr int kDtTrials = 4;     // consecutive trials of a k_detrend workgroup (they read the same W lines)
constexpr int kDtBlock = kDtTile * kDtTrials;

// ---- the workgroup's share: blockIdx.x = group * n_tiles + tile ----------------------------------------------------
PROM_OBS_HD int32_t dt_tiles(int32_t n_pix) { return (n_pix + kDtTile - 1) / kDtTile; }
PROM_OBS_HD int32_t dt_groups(int32_t n_trial) { return (n_trial + kDtTrials - 1) / kDtTrials; }
PROM_OBS_HD int64_t dt_workgroups(int32_t n_trial, int32_t n_pix) { return (int64_t)dt_groups(n_trial) * dt_tiles(n_pix); }
PROM_OBS_HD int32_t dt_wg_tile(int32_t bx, int32_t n_tiles) { return bx % n_tiles; }
PROM_OBS_HD int32_t dt_wg_group(int32_t bx, int32_t n_tiles) { return bx / n_tiles; }
// thread tid's column (it has one when p < n_pix and j < n_trial)
PROM_OBS_HD int32_t dt_pixel(int32_t tile, int32_t tid) { return tile * kDtTile + tid % kDtTile; }
PROM_OBS_HD int32_t dt_trial(int32_t group, int32_t tid) { return group * kDtTrials + tid / kDtTile; }

// ---- the filter and the flags --------------------------------------------------------------------------------------
// U[e][k]
PROM_OBS_HD int64_t dt_u(int32_t e, int32_t k, int32_t n_comp) { return (int64_t)e * n_comp + k; }
// W[k][e][p], p fastest
PROM_OBS_HD int64_t dt_w(int32_t k, int32_t e, int32_t p, int32_t n_exp, int32_t n_pix) {
  return ((int64_t)k * n_exp + e) * n_pix + p;
}
// flag[j][p]: 1 when the column is filterable
PROM_OBS_HD int64_t dt_flag(int32_t j, int32_t p, int32_t n_pix) { return (int64_t)j * n_pix + p; }

// ---- separately rounded arithmetic ---------------------------------------------------------------------------------
PROM_OBS_HD double dt_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}
PROM_OBS_HD double dt_add(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(a, b);
#else
  return a + b;
#endif
}

// ---- the two column functions --------------------------------------------------------------------------------------
// Column (j, p): M points at model[0][j][p] and W at W[0][0][p]; m_stride = n_trial n_pix doubles between exposures,
// w_stride = n_pix between a component's exposures.  NC is the filter's n_comp.
//
// Coefficients: c_k = +0, then in ascending e every term with W[k][e][p] != 0 adds fl(W M).  A term with W == 0 is
// skipped and its M enters nothing.  Returns whether the column is filterable: no exposure with a W != 0 has NaN M.
template <int NC>
PROM_OBS_HD bool dt_coefficients(const double* M, int64_t m_stride, const double* W, int64_t w_stride, int32_t n_exp,
                                 double (&c)[NC]) {
#pragma unroll
  for (int k = 0; k < NC; ++k) c[k] = 0.0;
  bool ok = true;
  for (int32_t e = 0; e < n_exp; ++e) {
    const double m = M[e * m_stride];
    bool any = false;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const double w = W[((int64_t)k * n_exp + e) * w_stride];
      if (w != 0.0) {
        c[k] = dt_add(c[k], dt_mul(w, m));
        any = true;
      }
    }
    ok = ok && !(any && m != m);
  }
  return ok;
}

// Apply: M'_e = M_e, then in ascending k M'_e = fl(M'_e - fl(U[e][k] c_k)), written over M_e; NaN down a column
// that is not filterable.
// The out-of-place form reads the column of S and writes the column of M (the same strides): the same values in the
// same order, so M's bits are the in-place form's whatever S is, M itself included.
template <int NC>
PROM_OBS_HD void dt_apply(const double* S, double* M, int64_t m_stride, const double* U, int32_t n_exp,
                          const double (&c)[NC], bool ok) {
  for (int32_t e = 0; e < n_exp; ++e) {
    double m = S[e * m_stride];
#pragma unroll
    for (int k = 0; k < NC; ++k) m = dt_add(m, -dt_mul(U[dt_u(e, k, NC)], c[k]));
    M[e * m_stride] = ok ? m : __builtin_nan("");
  }
}
template <int NC>
PROM_OBS_HD void dt_apply(double* M, int64_t m_stride, const double* U, int32_t n_exp, const double (&c)[NC], bool ok) {
  dt_apply<NC>(M, M, m_stride, U, n_exp, c, ok);
}

}  // namespace prom
