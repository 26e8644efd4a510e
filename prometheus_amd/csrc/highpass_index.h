// Index arithmetic and the window function of the high-pass filtered exposures (prom_highpass.hip): the (row, segment)
// a workgroup of k_highpass owns, the tiles it walks, the positions it stages into its rolling window and their ring
// slots, the outputs a lane owns, and the smooth model B of the definition in prom_hip.h ("high-pass filtered
// exposures on the device").  A model value's slot is expose_index.h's ex_model: a row is one (exposure, trial).
//
// Plain inline functions shared by the kernel and by the host harness (tests/helpers/highpass_host.cpp,
// tests/test_highpass_cpu.py), which walks every thread and step with the same text and evaluates the window function
// against rows it is given.
//
// The walk.  A segment of n positions is taken in ascending tiles of kHpTile outputs.  Before tile t computes, the
// ring holds the ORIGINAL values of the positions [t0 - h, t0 + kHpTile + h), t0 = t kHpTile: tile 0 stages all of
// them, a later tile only [t0 + h, t0 + kHpTile + h), because [t0 - h, t0 + h) is still there from the tile before.
// A position outside [0, n) is staged as NaN, which is how the ring marks "invalid": the definition skips a NaN
// value whatever its cause.  Then a barrier, the tile's outputs are formed from the ring and written over the model
// at [t0, t0 + kHpTile), and a second barrier precedes the next staging.  A wave whose windows hold no NaN at all
// (hp_lane_sees_nan) takes the window function's path without validity tests.
//
// The invariants: every position a tile stages is >= t0 (tile 0: every position at all), and everything written
// before lies below t0, so no value is read from memory after it was overwritten; the slots staged for tile t + 1 are
// those of the positions [t0 - kHpRing + kHpTile + h, t0 - kHpRing + 2 kHpTile + h), which end at or below
// t0 + kHpTile - h, the lowest position tile t + 1 reads, because kHpRing >= kHpTile + 2 h; a window of
// kHpTile + 2 h <= kHpRing consecutive positions has distinct slots.
//
// Rounding: every product and every sum of the window function is rounded on its own (__dmul_rn / __dadd_rn on the
// device, plain operators in a translation unit built with -ffp-contract=off on the host), the divisions are IEEE.
#pragma once

#include "expose_index.h"

namespace prom {

constexpr int kHpBlock = 256;                        // threads of a workgroup
#if defined(PROM_HP_OUT)
constexpr int kHpOut = PROM_HP_OUT;                  // (a measurement build: tools/highpass_bench.py's table)
#else
constexpr int kHpOut = 4;                            // consecutive outputs of a lane: a ring value is read once for them
#endif
constexpr int kHpTile = kHpBlock * kHpOut;           // outputs of a tile
constexpr int kHpMaxHalf = 512;                      // half width of the taps at most
constexpr int kHpRing = kHpTile + 2 * kHpMaxHalf <= 2048 ? 2048 : 4096;   // positions of the ring, a power of two
constexpr int kHpRingPad = kHpRing + kHpRing / 32;   // doubles of the ring: one spare double after every 32
static_assert(kHpRing >= kHpTile + 2 * kHpMaxHalf && (kHpRing & (kHpRing - 1)) == 0, "the ring holds a tile's window");
static_assert(kHpOut == 1 || kHpOut == 2 || kHpOut == 4 || kHpOut == 8, "outputs of a lane");

// ---- the workgroup's share: blockIdx.x = row * n_seg + segment, row = e * n_trial + j ------------------------------
PROM_OBS_HD int64_t hp_workgroups(int64_t n_rows, int32_t n_seg) { return n_rows * n_seg; }
PROM_OBS_HD int32_t hp_wg_segment(int32_t bx, int32_t n_seg) { return bx % n_seg; }
PROM_OBS_HD int32_t hp_wg_row(int32_t bx, int32_t n_seg) { return bx / n_seg; }
// the first model value of a row
PROM_OBS_HD int64_t hp_row_first(int32_t row, int32_t n_pix) { return (int64_t)row * n_pix; }
// the entry of perm that holds the device pixel of position i in the segment that starts at entry `first`
PROM_OBS_HD int32_t hp_perm_at(int32_t first, int32_t i) { return first + i; }

// ---- tiles, staging and the ring ---------------------------------------------------------------------------------
PROM_OBS_HD int32_t hp_tiles(int32_t n) { return (n + kHpTile - 1) / kHpTile; }
PROM_OBS_HD int32_t hp_tile_first(int32_t tile) { return tile * kHpTile; }
// tile t stages the positions [hp_stage_first, hp_stage_end), thread tid those at tid, tid + kHpBlock, ... from the first
PROM_OBS_HD int32_t hp_stage_first(int32_t tile, int32_t h) { return tile == 0 ? -h : hp_tile_first(tile) + h; }
PROM_OBS_HD int32_t hp_stage_end(int32_t tile, int32_t h) { return hp_tile_first(tile) + kHpTile + h; }
// the ring slot of position i >= -kHpMaxHalf.  ds_read_b64 serves two groups of 32 lanes, and a double's bank pair is
// its index mod 32: lanes kHpOut doubles apart would share a bank kHpOut ways, so every 32 doubles the ring skips
// one, which moves each group of 32 / kHpOut lanes on by one bank pair.
PROM_OBS_HD int32_t hp_slot(int32_t i) {
  const int32_t r = (i + kHpMaxHalf) & (kHpRing - 1);
  return r + (r >> 5);
}
// the first of the kHpOut consecutive outputs of thread tid in a tile
PROM_OBS_HD int32_t hp_out_first(int32_t tile, int32_t tid) { return hp_tile_first(tile) + tid * kHpOut; }
// The clean test of a wave (64 consecutive threads, so 64 kHpOut consecutive outputs from wave_first on): its
// outputs' windows together are [wave_first - h, wave_first + 64 kHpOut + h), all staged.  Lane `lane` looks at the
// positions wave_first - h + lane, + 64, ... below the end and says whether one holds NaN (a position outside the
// segment, or a NaN model value).  When no lane says so, every window of the wave lies inside the segment and holds no
// NaN.
PROM_OBS_HD bool hp_lane_sees_nan(const double* ring, int32_t wave_first, int32_t lane, int32_t h) {
  bool bad = false;
  for (int32_t i = wave_first - h + lane; i < wave_first + 64 * kHpOut + h; i += 64) {
    const double m = ring[hp_slot(i)];
    bad = bad || m != m;
  }
  return bad;
}

// ---- separately rounded arithmetic ---------------------------------------------------------------------------------
PROM_OBS_HD double hp_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}
PROM_OBS_HD double hp_add(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(a, b);
#else
  return a + b;
#endif
}
PROM_OBS_HD double hp_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}

// ---- the window function -------------------------------------------------------------------------------------------
// den of a window that lies inside its segment and holds no NaN: +0, then g[|d|] for d = -h .. h in ascending order,
// the sequence every such window sees.  The host forms it once per filter.
PROM_OBS_HD double hp_den_full(const double* g, int32_t h) {
  double den = 0.0;
  for (int32_t d = -h; d <= h; ++d) den = hp_add(den, g[d < 0 ? -d : d]);
  return den;
}

// One step of the window walk: the weights slide on by one, and the ring value m at offset k from the lane's first
// output enters output v with the weight w[v] = g[|k - v|] when |k - v| <= h.  ALL: every v is in range (the caller
// knows), so nothing is tested.
template <int V, bool CLEAN, bool ALL>
PROM_OBS_HD void hp_step(double m, int32_t k, int32_t h, const double* g, double (&w)[V], double (&num)[V],
                         double (&den)[V]) {
#pragma unroll
  for (int v = V - 1; v > 0; --v) w[v] = w[v - 1];
  w[0] = g[k < 0 ? -k : (k <= h ? k : 0)];              // (beyond h no output reads w[0] any more)
  const bool ok = CLEAN || m == m;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int32_t d = k - v;
    if ((ALL || (d >= -h && d <= h)) && ok) {
      num[v] = hp_add(num[v], hp_mul(w[v], m));
      if (!CLEAN) den[v] = hp_add(den[v], w[v]);
    }
  }
}

// B of the V consecutive outputs o .. o + V - 1 (o a multiple of V) from the ring, which holds the originals of
// [o - h, o + V - 1 + h] (NaN where invalid).  The ring is walked once in ascending position; each output therefore
// takes its own terms in ascending i', as the definition asks.  The weights slide through w: w[v] at step k is w[0]
// of step k - v.  The steps [-h + V - 1, h], at which every output is in range, run without a test; where k is a
// multiple of V the positions o + k .. o + k + V - 1 lie in one run of 32 ring doubles (o, kHpMaxHalf and 32 are
// multiples of V), so their slots are consecutive and one slot is computed for V steps.
// CLEAN: the ring holds no NaN there and every window lies inside the segment, so no value is tested and den is
// den_full.
template <int V, bool CLEAN>
PROM_OBS_HD void hp_window(const double* ring, int32_t o, int32_t h, const double* g, double den_full, double (&B)[V]) {
  static_assert(kHpMaxHalf % V == 0 && 32 % V == 0, "V consecutive slots");
  double num[V], den[V], w[V];
#pragma unroll
  for (int v = 0; v < V; ++v) num[v] = den[v] = w[v] = 0.0;
  int32_t k = -h;
  if (-h + V - 1 <= h) {
    for (; k < -h + V - 1; ++k) hp_step<V, CLEAN, false>(ring[hp_slot(o + k)], k, h, g, w, num, den);
    for (; k <= h && (k & (V - 1)) != 0; ++k) hp_step<V, CLEAN, true>(ring[hp_slot(o + k)], k, h, g, w, num, den);
    for (; k + V - 1 <= h; k += V) {
      const double* at = ring + hp_slot(o + k);
      double m[V];
#pragma unroll
      for (int i = 0; i < V; ++i) m[i] = at[i];
#pragma unroll
      for (int i = 0; i < V; ++i) hp_step<V, CLEAN, true>(m[i], k + i, h, g, w, num, den);
    }
    for (; k <= h; ++k) hp_step<V, CLEAN, true>(ring[hp_slot(o + k)], k, h, g, w, num, den);
  }
  for (; k <= h + V - 1; ++k) hp_step<V, CLEAN, false>(ring[hp_slot(o + k)], k, h, g, w, num, den);
#pragma unroll
  for (int v = 0; v < V; ++v) B[v] = hp_div(num[v], CLEAN ? den_full : den[v]);
}

// M' of a model value m and its smooth model B: mode 0 subtracts, mode 1 divides.  A NaN m gives NaN either way.
template <int MODE>
PROM_OBS_HD double hp_apply(double m, double B) {
  return MODE == 0 ? hp_add(m, -B) : hp_div(m, B);
}

}  // namespace prom
