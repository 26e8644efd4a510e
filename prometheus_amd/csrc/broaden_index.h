// Index arithmetic and the evaluation text of the broadened spectra (prom_broaden.hip): the tile of outputs a workgroup
// of k_broaden takes, the membership test of the definition in prom_hip.h ("broadened spectra on the device"), the
// ends of an output's support, the union a tile stages in LDS and the walk over a support that forms num[o] and den.
//
// Plain inline functions shared by the kernel and by the host harness (tests/helpers/broaden_host.cpp,
// tests/test_broaden_cpu.py), which walks every tile and lane with the same text and evaluates every output with it.
//
// The invariants.  For one output w the scaled offset t(w') = fl(fl(fl(fl(wav[w'] - wav[w]) r) - b0) s) is
// non-decreasing in w': wav ascends, r > 0 and s > 0, and rounding is monotone; r is finite (the entries require it),
// so t is never NaN.  Both membership predicates (t >= 0, t > n_k - 1) are therefore monotone in w', a binary search
// over [0, n_wav] finds the first index at which each holds, and the support is [a, b) with 0 <= a <= b <= n_wav.
// Nothing is assumed about how a and b move with w.  A tile first tries the window [lower end of its first output,
// upper end of its last output), two searches in the grid: when it holds at most kBrStage points it is staged, every
// lane searches its ends inside the stage, and br_end_certain proves each of them against the grid; on a grid where
// the ends do move monotonically with w every lane's ends lie inside the window and are proven.  If one lane's are not
// (or the window does not fit), every lane searches the grid itself and the tile's union is the minimum of a and the
// maximum of b over its lanes with a support, staged only when it holds at most kBrStage points.  Either way every
// lane's [a, b) is exactly the membership's and lies inside what is staged.  A tile that is not staged reads the global
// arrays at the same indices in the same order.
//
// Rounding: every product, sum and difference is rounded on its own (__dmul_rn / __dadd_rn on the device, plain
// operators in a translation unit built with -ffp-contract=off on the host), the divisions are IEEE.
#pragma once

#include "obs_index.h"

namespace prom {

constexpr int kBrBlock = 256;     // threads of a workgroup = outputs of a tile (lane = output)
constexpr int kBrPhases = 8;      // rows of R a workgroup carries: g = kern q is formed once for all of them
constexpr int kBrStage = 576;     // grid points staged per tile at most: wav, q and kBrPhases rows of R are 46,080 B,
                                  // with the 1,025 kernel records of 16 B at most 62,480 B, inside the 64 KB a
                                  // launch may ask for; with 33 records three workgroups share a CU's 160 KB
constexpr int kBrMaxNodes = 1025; // nodes of a kernel at most

// a kernel node's record: K[i] and D[i] = fl(K[i + 1] - K[i]) (the last node's D is 0 and never read)
struct BrRec {
  double K, D;
};
// the resident kernel as the evaluation sees it
struct BrKern {
  double b0, s;
  int32_t n_k;
};

// ---- separately rounded arithmetic ---------------------------------------------------------------------------------
PROM_OBS_HD double br_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}
PROM_OBS_HD double br_add(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(a, b);
#else
  return a + b;
#endif
}
PROM_OBS_HD double br_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}

// ---- the definition's scalars ----------------------------------------------------------------------------------------
// r of an output at wavelength x
PROM_OBS_HD double br_r(double x) { return br_div(1.0, x); }
// t of the candidate at x1 for the output at x: fl(fl(fl(fl(x1 - x) r) - b0) s)   (fl(a - b) is fl(a + (-b)))
PROM_OBS_HD double br_t(double x1, double x, double r, const BrKern& k) {
  return br_mul(br_add(br_mul(br_add(x1, -x), r), -k.b0), k.s);
}
PROM_OBS_HD bool br_member(double t, const BrKern& k) { return t >= 0.0 && t <= (double)(k.n_k - 1); }
// kern of a member's t: i = min(floor(t), n_k - 2), a = t - i (exact), fl(K[i] + fl(a D[i]))
PROM_OBS_HD double br_kern(double t, const BrKern& k, const BrRec* rec) {
  int32_t i = (int32_t)t;
  if (i > k.n_k - 2) i = k.n_k - 2;
  const BrRec c = rec[i];
  return br_add(c.K, br_mul(t - (double)i, c.D));
}

// ---- the ends of a support -------------------------------------------------------------------------------------------
// The first index in [lo, hi] at which the predicate holds (lower end: t >= 0, upper end: t > n_k - 1); hi: nowhere in
// [lo, hi).  W is indexed by w' - base (the grid itself: base = 0; the stage: base = its first point).  One loop for
// both ends; at most ceil(log2(hi - lo + 1)) steps.
PROM_OBS_HD bool br_pred(double x1, double x, double r, const BrKern& k, bool upper) {
  const double t = br_t(x1, x, r, k);
  return upper ? t > (double)(k.n_k - 1) : t >= 0.0;
}
PROM_OBS_HD int32_t br_end_in(const double* W, int32_t base, int32_t lo, int32_t hi, double x, double r,
                              const BrKern& k, bool upper) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (br_pred(W[mid - base], x, r, k, upper)) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// ... over the whole grid
PROM_OBS_HD int32_t br_end(const double* wav, int32_t n, double x, double r, const BrKern& k, bool upper) {
  return br_end_in(wav, 0, 0, n, x, r, k, upper);
}
// An end e found inside the window [lo, hi] is the grid's end when the predicate fails just below e and holds at e.
// The search itself proves both for lo < e < hi; at the window's own ends the grid decides (one load each).
PROM_OBS_HD bool br_end_certain(const double* wav, int32_t n, int32_t lo, int32_t hi, int32_t e, double x, double r,
                                const BrKern& k, bool upper) {
  const bool below = e > lo || e == 0 || !br_pred(wav[e - 1], x, r, k, upper);
  const bool at = e < hi || e == n || br_pred(wav[e], x, r, k, upper);
  return below && at;
}

// ---- tiles and the stage -----------------------------------------------------------------------------------------------
PROM_OBS_HD int32_t br_tiles(int32_t n_wav) { return (n_wav + kBrBlock - 1) / kBrBlock; }
PROM_OBS_HD int32_t br_groups(int32_t n_orb) { return (n_orb + kBrPhases - 1) / kBrPhases; }
// the last output of a tile
PROM_OBS_HD int32_t br_tile_last(int32_t tile, int32_t n_wav) {
  const int32_t e = (tile + 1) * kBrBlock;
  return (e < n_wav ? e : n_wav) - 1;
}
// the output of thread tid in a tile (it has one only when this is < n_wav)
PROM_OBS_HD int32_t br_output(int32_t tile, int32_t tid) { return tile * kBrBlock + tid; }
// a window or union [lo, hi) is staged when it is not empty and holds at most kBrStage points (the union: lo is the
// minimum of a, hi the maximum of b over the lanes with b > a; without such a lane lo > hi)
PROM_OBS_HD bool br_staged(int32_t lo, int32_t hi) { return hi > lo && hi - lo <= kBrStage; }
// bytes of LDS a launch asks for: the stage and the kernel's records
PROM_OBS_HD int32_t br_lds_bytes(int32_t n_k) {
  return (int32_t)sizeof(double) * (2 + kBrPhases) * kBrStage + (int32_t)sizeof(BrRec) * n_k;
}

// ---- the walk ----------------------------------------------------------------------------------------------------------
// num[g] and den of the output at x over its support [a, b): W and Q hold wav and q and Rr the first of ng <= kBrPhases
// rows `stride` doubles apart, all indexed by w' - base (the stage: base = its first point; global memory: base = 0).
// The terms enter in ascending w'.  The membership test inside the loop decides nothing for a support found by
// br_end; it keeps the record index in range whatever the caller passes.
PROM_OBS_HD void br_walk(const double* W, const double* Q, const double* Rr, int64_t stride, int32_t base, int32_t ng,
                         int32_t a, int32_t b, double x, double r, const BrKern& k, const BrRec* rec,
                         double (&num)[kBrPhases], double& den) {
#pragma unroll
  for (int g = 0; g < kBrPhases; ++g) num[g] = 0.0;
  den = 0.0;
  for (int32_t w1 = a; w1 < b; ++w1) {
    const int32_t i = w1 - base;
    const double t = br_t(W[i], x, r, k);
    if (!br_member(t, k)) continue;
    const double gq = br_mul(br_kern(t, k, rec), Q[i]);
    den = br_add(den, gq);
#pragma unroll
    for (int g = 0; g < kBrPhases; ++g)
      if (g < ng) num[g] = br_add(num[g], br_mul(gq, Rr[(int64_t)g * stride + i]));
  }
}
// R_b of a row from its sums: num / den (IEEE), NaN when den == 0
PROM_OBS_HD double br_result(double num, double den) { return den == 0.0 ? __builtin_nan("") : br_div(num, den); }

}  // namespace prom
