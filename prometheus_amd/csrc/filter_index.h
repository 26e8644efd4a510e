// Index arithmetic and the per-pixel function of the filter's weights on the device (prom_filter.hip): the pixel a
// thread of k_filter_weights owns, the entries it reads (U[e][k], ivar[e][p]) and writes (W[k][e][p]), and the
// definition of prom_hip.h ("the filter's weights on the device") as one function of a pixel's column.  U's and W's
// slots are detrend_index.h's dt_u and dt_w, ivar's is expose_index.h's ex_data.
//
// Plain inline functions shared by the kernel and by the host harness (tests/helpers/filter_host.cpp,
// tests/test_filter_cpu.py), which walks every thread's indices with the same text and evaluates the per-pixel
// function against columns it is given.
//
// The invariants: a pixel's thread is the only one that reads ivar[.][p] or writes W[.][.][p], and it writes every
// W[k][e][p] exactly once; every U entry lies inside U[n_exp][K]; a thread past n_pix touches nothing.
//
// Rounding: every product, sum, difference, quotient and square root is rounded on its own.  On the device they are
// __dmul_rn / __dadd_rn / __ddiv_rn / __dsqrt_rn, which the compiler never fuses; on the host plain operators in a
// translation unit built with -ffp-contract=off.
#pragma once

#include "detrend_index.h"

#if defined(__HIPCC__)
#define PROM_OBS_HD_M __host__ __device__ inline
#else
#define PROM_OBS_HD_M inline
#endif

namespace prom {

constexpr int kFwTile = 64;   // consecutive pixels of a k_filter_weights workgroup: one wave, lane = pixel

// ---- the workgroup's share: blockIdx.x = tile ----------------------------------------------------------------------
PROM_OBS_HD int32_t fw_tiles(int32_t n_pix) { return (n_pix + kFwTile - 1) / kFwTile; }
// thread tid's pixel (it has one when p < n_pix)
PROM_OBS_HD int32_t fw_pixel(int32_t tile, int32_t tid) { return tile * kFwTile + tid; }
// entry (i, j), i >= j, of the lower triangle kept row by row
PROM_OBS_HD constexpr int fw_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// ---- separately rounded arithmetic ---------------------------------------------------------------------------------
PROM_OBS_HD double fw_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}
PROM_OBS_HD double fw_sqrt(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(a);
#else
  return __builtin_sqrt(a);
#endif
}
// fl(a - fl(b c))
PROM_OBS_HD double fw_submul(double a, double b, double c) { return dt_add(a, -dt_mul(b, c)); }
// v_e: the inverse variance when it is finite and > 0, else +0
PROM_OBS_HD double fw_weight(double iv) { return (iv > 0.0 && iv < __builtin_inf()) ? iv : 0.0; }

// ---- the triangle's storage ----------------------------------------------------------------------------------------
// The first NR entries (row by row) are registers, the others lie in memory at mem[(entry - NR) * pitch]: the kernel
// keeps them in LDS as [entry][lane] (pitch = kFwTile, conflict-free) where an instantiation's registers run out;
// the host and the other instantiations keep all of them in the array (NR = fw_entries(K), mem unused).  Every entry
// index is a compile-time constant once the loops are unrolled, so the choice costs nothing at run time.
PROM_OBS_HD constexpr int fw_entries(int K) { return K * (K + 1) / 2; }
template <int NR>
struct FwTri {
  double reg[NR > 0 ? NR : 1];
  double* mem;
  int32_t pitch;
  PROM_OBS_HD_M double get(int at) const { return at < NR ? reg[at < NR ? at : 0] : mem[(at - NR) * pitch]; }
  PROM_OBS_HD_M void set(int at, double v) {
    if (at < NR)
      reg[at < NR ? at : 0] = v;
    else
      mem[(at - NR) * pitch] = v;
  }
};

// ---- the solve of one exposure -------------------------------------------------------------------------------------
// x = N^-1 (v u) through the factor L (row by row, fw_tri); u points at U[e][0].  Returns whether every x is finite.
template <int K, int NR>
PROM_OBS_HD bool fw_solve(const FwTri<NR>& L, const double* u, double v, double (&x)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) {   // forward: y_i, the sum in ascending k
    double s = dt_mul(v, u[i]);
#pragma unroll
    for (int k = 0; k < i; ++k) s = fw_submul(s, L.get(fw_tri(i, k)), x[k]);
    x[i] = fw_div(s, L.get(fw_tri(i, i)));
  }
  bool finite = true;
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {   // backward: x_i over y_i, the sum in descending k
    double s = x[i];
#pragma unroll
    for (int k = K - 1; k > i; --k) s = fw_submul(s, L.get(fw_tri(k, i)), x[k]);
    x[i] = fw_div(s, L.get(fw_tri(i, i)));
    finite = finite && __builtin_fabs(x[i]) < __builtin_inf();
  }
  return finite;
}

// ---- the per-pixel function ----------------------------------------------------------------------------------------
// Pixel p: iv points at ivar[0][p] and W at W[0][0][p]; stride = n_pix doubles between a column's exposures (of ivar
// and of one component of W).  U is U[n_exp][K].  Every W[k][e][p] is stored exactly once, in the last walk.
// The triangle lives in L (its mem and pitch set by the caller); NR is its register share.
template <int K, int NR>
PROM_OBS_HD void fw_weights(FwTri<NR>& L, const double* U, const double* iv, double* W, int64_t stride, int32_t n_exp) {
#pragma unroll
  for (int i = 0; i < fw_entries(K); ++i) L.set(i, 0.0);
  // pass 1: the normal matrix's lower triangle, in ascending e
  int32_t cnt = 0;
  for (int32_t e = 0; e < n_exp; ++e) {
    const double v = fw_weight(iv[e * stride]);
    if (v > 0.0) {
      ++cnt;
      const double* u = U + dt_u(e, 0, K);
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const double t = dt_mul(v, u[i]);
#pragma unroll
        for (int j = 0; j <= i; ++j) L.set(fw_tri(i, j), dt_add(L.get(fw_tri(i, j)), dt_mul(t, u[j])));
      }
    }
  }
  // the tolerance: dmax = N_00, then every larger N_ii in ascending i
  double dmax = L.get(0);
#pragma unroll
  for (int i = 1; i < K; ++i)
    if (L.get(fw_tri(i, i)) > dmax) dmax = L.get(fw_tri(i, i));
  const double tol = dt_mul(dt_mul((double)K, 0x1p-52), dmax);
  // the factorisation in place, column by column; a pivot that is not > tol (NaN included) makes the pixel singular
  bool regular = cnt >= K;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    double s = L.get(fw_tri(j, j));
#pragma unroll
    for (int k = 0; k < j; ++k) s = fw_submul(s, L.get(fw_tri(j, k)), L.get(fw_tri(j, k)));
    regular = regular && s > tol;
    const double d = fw_sqrt(s);
    L.set(fw_tri(j, j), d);
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
      double t = L.get(fw_tri(i, j));
#pragma unroll
      for (int k = 0; k < j; ++k) t = fw_submul(t, L.get(fw_tri(i, k)), L.get(fw_tri(j, k)));
      L.set(fw_tri(i, j), fw_div(t, d));
    }
  }
  double x[K];
  // pass 2: a regular pixel solves every weighted exposure once without storing: one x that is not finite zeroes it
  if (regular)
    for (int32_t e = 0; e < n_exp; ++e) {
      const double v = fw_weight(iv[e * stride]);
      if (v > 0.0) regular = fw_solve<K, NR>(L, U + dt_u(e, 0, K), v, x) && regular;
    }
  // pass 3: solve again and store; +0 for an exposure without weight and throughout a pixel that is not regular
  for (int32_t e = 0; e < n_exp; ++e) {
    const double v = fw_weight(iv[e * stride]);
    const bool on = regular && v > 0.0;
    if (on) fw_solve<K, NR>(L, U + dt_u(e, 0, K), v, x);
#pragma unroll
    for (int k = 0; k < K; ++k) W[((int64_t)k * n_exp + e) * stride] = on ? x[k] : 0.0;
  }
}

}  // namespace prom
