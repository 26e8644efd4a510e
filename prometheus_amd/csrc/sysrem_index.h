// Index arithmetic, the fixed shape of the row sums and the entry functions of SYSREM on the device
// (prom_sysrem.hip): the pixels a lane of k_sysrem_step owns, the entries of the pitched work buffers it reads and
// writes, the slot of a partial, the tiles a lane of k_sysrem_rows adds, and the arithmetic of the definition in
// prom_hip.h ("injection and SYSREM on the device").
//
// Plain inline functions shared by the kernels and by the host harness (tests/helpers/sysrem_host.cpp,
// tests/test_sysrem_cpu.py), which walks every workgroup's and lane's indices with the same text and evaluates the
// column fit and the row shape on values it is given.  tests/helpers/sysrem_ref.py reads the constants below and
// restates the shape in numpy.
//
// The work buffers r and w are pitched: a row holds sy_pitch(n_pix) doubles, a whole number of tiles, and the
// entries past n_pix hold w = 0 and r = +0, so a lane's kSyVec consecutive pixels are one aligned vector and a tile
// needs no tail test: an entry with w = 0 adds nothing anywhere.
//
// The shape of a row sum (num and den of fit_a alike), for one exposure, a function of n_pix alone:
//   lane    a lane owns kSyVec consecutive pixels; its sum starts at +0 and takes the terms of its pixels with w > 0
//           in ascending pixel order
//   tile    the 64 lanes of a tile (kSyTile = 64 kSyVec consecutive pixels) hold t[0 .. 63]; for m = 1, 2, 4, 8, 16, 32
//           in turn every t[l] becomes fl(t[l] + t[l ^ m]) (all l at once); t[0] is the tile's partial
//   row     lane l of a wave of k_sysrem_rows starts at +0 and adds the partials of the tiles l, l + 64, l + 128, ...
//           in ascending order (a lane without a tile keeps +0); the same butterfly over the 64 lanes gives the sum
//
// The invariants: a lane's vector lies inside a row of the pitched buffers; r[e][p] is read by the lane that owns p
// and written by it alone; part[e][tile] is written exactly once per step and read exactly once by k_sysrem_rows;
// a[e] and U[e][col] are written exactly once per k_sysrem_rows.
//
// Rounding: every product, sum, quotient and square root is rounded on its own.  On the device they are __dmul_rn /
// __dadd_rn / __ddiv_rn / __dsqrt_rn, which the compiler never fuses; on the host plain operators in a translation
// unit built with -ffp-contract=off.
#pragma once

#include <cmath>

#include "expose_index.h"

#ifndef PROM_SY_VEC
#define PROM_SY_VEC 2   // (build macro for A/B builds of the pixels a lane owns: 1, 2 or 4)
#endif

namespace prom {

constexpr int kSyVec = PROM_SY_VEC;          // consecutive pixels of a lane of k_sysrem_step: one aligned vector load
constexpr int kSyBlock = 64;                 // threads of a k_sysrem_step workgroup: one wave, no LDS, no barrier
constexpr int kSyTile = kSyBlock * kSyVec;   // consecutive pixels of a k_sysrem_step workgroup
constexpr int kSyRowsBlock = 1024;           // threads of the one k_sysrem_rows workgroup: a wave per exposure in turn
constexpr int kSyMaxExp = 4096;              // exposures at most (k_sysrem_rows keeps a[e] in LDS)
constexpr int kSyMaxComp = 16;               // columns of U at most (the cap of the filter, kDtMaxComp)
constexpr int kSyFlatBlock = 256;            // threads of the elementwise kernels

static_assert(kSyVec == 1 || kSyVec == 2 || kSyVec == 4, "a lane's pixels are one or two 16-byte loads, or one double");

// ---- the tiles and the pitched buffers -----------------------------------------------------------------------------
PROM_OBS_HD int32_t sy_tiles(int32_t n_pix) { return (n_pix + kSyTile - 1) / kSyTile; }
PROM_OBS_HD int64_t sy_pitch(int32_t n_pix) { return (int64_t)sy_tiles(n_pix) * kSyTile; }
// the first of the kSyVec pixels of a lane (all of them lie below the pitch)
PROM_OBS_HD int32_t sy_pixel(int32_t tile, int32_t lane) { return tile * kSyTile + lane * kSyVec; }
// r[e][p] and w[e][p] of the pitched buffers
PROM_OBS_HD int64_t sy_at(int32_t e, int32_t p, int64_t pitch) { return (int64_t)e * pitch + p; }
// part[e][tile]: a pair {num, den}
PROM_OBS_HD int64_t sy_part(int32_t e, int32_t tile, int32_t n_tiles) { return (int64_t)e * n_tiles + tile; }
// U[e][col]
PROM_OBS_HD int64_t sy_u(int32_t e, int32_t col, int32_t n_cols) { return (int64_t)e * n_cols + col; }
// k_sysrem_rows: the i-th tile of lane l, and how many it has
PROM_OBS_HD int32_t sy_rows_tile(int32_t lane, int32_t i) { return lane + 64 * i; }
PROM_OBS_HD int32_t sy_rows_count(int32_t lane, int32_t n_tiles) { return lane < n_tiles ? (n_tiles - lane + 63) / 64 : 0; }
// the flat kernels: workgroups over n entries
PROM_OBS_HD int64_t sy_flat_workgroups(int64_t n) { return (n + kSyFlatBlock - 1) / kSyFlatBlock; }

// ---- separately rounded arithmetic ---------------------------------------------------------------------------------
PROM_OBS_HD double sy_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}
PROM_OBS_HD double sy_add(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(a, b);
#else
  return a + b;
#endif
}
PROM_OBS_HD double sy_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}
PROM_OBS_HD double sy_sqrt(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(a);
#else
  return std::sqrt(a);
#endif
}

// ---- the entry functions of the definition -------------------------------------------------------------------------
// D of an injection: raw where the model has no value, else fl(raw fl(1 + fl(scale fl(M - 1))))
PROM_OBS_HD double sy_inject(double raw, double M, double scale) {
  if (M != M) return raw;
  return sy_mul(raw, sy_add(1.0, sy_mul(scale, sy_add(M, -1.0))));
}
// w of an entry: ivar when it is finite and > 0 and D is finite, else 0
PROM_OBS_HD double sy_weight(double iv, double d) {
  return (iv > 0.0 && iv < __builtin_inf() && __builtin_fabs(d) < __builtin_inf()) ? iv : 0.0;
}
// one term of fit_c (x = a_e) or of fit_a (x = c_p): skipped altogether when w = 0
PROM_OBS_HD void sy_fit_add(double w, double r, double x, double* num, double* den) {
  if (w > 0.0) {
    *num = sy_add(*num, sy_mul(sy_mul(w, r), x));
    *den = sy_add(*den, sy_mul(w, sy_mul(x, x)));
  }
}
// c_p or a_e of its sums
PROM_OBS_HD double sy_ratio(double num, double den) { return den > 0.0 ? sy_div(num, den) : 0.0; }
// the residual after a component: fl(r - fl(a c)) where w > 0
PROM_OBS_HD double sy_residual(double w, double r, double a, double c) {
  return w > 0.0 ? sy_add(r, -sy_mul(a, c)) : r;
}
// the first a of a component
PROM_OBS_HD double sy_first_a(int32_t n_exp) { return sy_div(1.0, sy_sqrt((double)n_exp)); }

// ---- the shape on the host (the kernels use __shfl_xor for the same exchanges) -------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
// the butterfly over t[0 .. 63]: afterwards every t[l] holds the sum
static inline void sy_butterfly_host(double* t) {
  for (int m = 1; m < 64; m <<= 1) {
    double u[64];
    for (int l = 0; l < 64; ++l) u[l] = sy_add(t[l], t[l ^ m]);
    for (int l = 0; l < 64; ++l) t[l] = u[l];
  }
}
#endif

}  // namespace prom
