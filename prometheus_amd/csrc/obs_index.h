// Index arithmetic of k_observe (prom_observe.hip): a pixel in the model frame, its support in the wavelength grid,
// the tile of pixels a workgroup takes, the wavelength range the tile stages in LDS and the points a lane reads.
//
// Plain inline functions shared by the kernel and by the host harness (tests/helpers/observe_host.cpp,
// tests/test_observe_cpu.py), which walks every (tile, pixel, iteration, lane) with the same text and checks every
// index the kernel would form.
//
// The invariants: a support [a, b) lies inside [0, n_wav); the stage [s0, s1) lies inside [0, n_wav) and holds at
// most kObsStage points; a pixel reads the stage only when its whole support lies inside it (offsets w - s0 in
// [0, s1 - s0)), otherwise it reads the global arrays at w in [a, b).
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PROM_OBS_HD __host__ __device__ inline
#else
#define PROM_OBS_HD static inline
#endif

namespace prom {

constexpr int kObsBlock = 256;    // threads of a k_observe workgroup (4 waves)
constexpr int kObsTile = 32;      // consecutive pixels per workgroup
constexpr int kObsStage = 496;    // wavelengths staged per workgroup at most (wav, q and kObsPhases rows of R: 39 KB,
                                  // four workgroups in a CU's 160 KB)
constexpr int kObsPhases = 8;     // phases per workgroup when all phases share the frame factor

// pixel p of phase o in the model frame: L = fl(lam f), S = fl(sig f), c = fl(k S)
struct ObsPix {
  double L, S, c;
};
PROM_OBS_HD ObsPix obs_pixel(double lam, double sig, double k, double f) {
  ObsPix x;
  x.L = lam * f;
  x.S = sig * f;
  x.c = k * x.S;
  return x;
}

// membership of a grid point: |wav - L| <= c, both ends inclusive (the difference in float64)
PROM_OBS_HD bool obs_member(double wav, double L, double c) { return __builtin_fabs(wav - L) <= c; }

// one end of a support's candidates: the first index in [0, n] whose wavelength is >= x (upper: > x); n: none.
// One loop for both ends, so that lanes searching a lower and an upper end side by side do not diverge
PROM_OBS_HD int32_t obs_bound(const double* wav, int32_t n, double x, bool upper) {
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    const double v = wav[mid];
    if (upper ? v <= x : v < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the target of a pixel's end: fl(L - c) or fl(L + c).  Where the difference wav - L is exact (c well below L, every
// spectrograph width) rounding is monotone and no member lies outside the candidates; obs_trim does not rely on it
PROM_OBS_HD double obs_target(const ObsPix& x, bool upper) { return upper ? x.L + x.c : x.L - x.c; }

// the support [a, b) from the candidates [a, b): membership is decided by the test alone.  The ends move inwards
// past candidates that are no members and outwards over members the rounded targets left out (c not small against
// L: the rounded difference can admit a point just beyond fl(L +- c)); the rounded difference is monotone in wav,
// so the members are contiguous
PROM_OBS_HD void obs_trim(const double* wav, int32_t n, double L, double c, int32_t* a_io, int32_t* b_io) {
  int32_t a = *a_io, b = *b_io;
  if (b < a) b = a;
  while (a < b && !obs_member(wav[a], L, c)) ++a;
  while (b > a && !obs_member(wav[b - 1], L, c)) --b;
  if (a == b) {
    // no member among the candidates: one may still sit next to them
    if (a < n && obs_member(wav[a], L, c)) b = a + 1;
    else if (a > 0 && obs_member(wav[a - 1], L, c)) --a;
  }
  if (a < b) {
    while (a > 0 && obs_member(wav[a - 1], L, c)) --a;
    while (b < n && obs_member(wav[b], L, c)) ++b;
  }
  *a_io = a;
  *b_io = b;
}

PROM_OBS_HD int32_t obs_tiles(int32_t n_pix) { return (n_pix + kObsTile - 1) / kObsTile; }
PROM_OBS_HD int32_t obs_tile_first(int32_t tile) { return tile * kObsTile; }
PROM_OBS_HD int32_t obs_tile_count(int32_t tile, int32_t n_pix) {
  const int32_t r = n_pix - tile * kObsTile;
  return r < kObsTile ? r : kObsTile;
}

// a pixel whose support is not empty and fits the stage takes part in choosing the staged range
PROM_OBS_HD bool obs_votes(int32_t a, int32_t b, int32_t cap) { return b > a && b - a <= cap; }

// the staged range of a tile from its pixels' supports: from the lowest voting support on, cap points at most
PROM_OBS_HD void obs_stage(const int32_t* a, const int32_t* b, int32_t n, int32_t cap, int32_t* s0_out,
                           int32_t* s1_out) {
  int32_t s0 = 0, s1 = 0;
  bool any = false;
  for (int32_t j = 0; j < n; ++j) {
    if (!obs_votes(a[j], b[j], cap)) continue;
    if (!any || a[j] < s0) s0 = a[j];
    if (!any || b[j] > s1) s1 = b[j];
    any = true;
  }
  if (s1 - s0 > cap) s1 = s0 + cap;
  *s0_out = s0;
  *s1_out = s1;
}

// the pixel reads the stage (its whole support is inside it); otherwise it reads the global arrays
PROM_OBS_HD bool obs_staged(int32_t a, int32_t b, int32_t s0, int32_t s1) { return a >= s0 && b <= s1; }

// passes of a wave over a support, and the grid point a lane takes in pass `it` (it reads only where this < b)
PROM_OBS_HD int32_t obs_passes(int32_t a, int32_t b) { return (b - a + 63) >> 6; }
PROM_OBS_HD int32_t obs_point(int32_t a, int32_t it, int32_t lane) { return a + 64 * it + lane; }

}  // namespace prom
