// Index arithmetic and the selection function of the median high-pass (prom_median.hip): the running median B of the
// definition in prom_hip.h ("median high-pass on the device").  The (row, segment) a workgroup owns, its tiles, what
// it stages and the ring of originals are highpass_index.h's, unchanged; only the window function differs: a
// selection instead of two sums.
//
// Plain inline functions shared by the kernel and by the host harness (tests/helpers/median_host.cpp,
// tests/test_median_cpu.py), which walks every thread and step with the same text.
//
// Per tile, after the staging barrier:
//   the stretch   the positions [base, base + len), base = t0 - h, len = min(kHpTile, n - t0) + 2 h <= kMdStretch: all
//                 a window of the tile's outputs can hold.  q = position - base is a stretch index.
//   the sort      idx[0 .. P), P the power of two >= len, starts as 0 .. P - 1 and is sorted ascending by
//                 (key, q) with a bitonic network (md_sort_pair; a barrier after every stage).  The key of a value is
//                 the order-preserving integer of its bits (md_key: -0 below +0, the infinities ordinary values); a NaN,
//                 a position outside the segment (staged as NaN) and q >= len have the key kMdNoKey, above every value's.
//   the ranks     rk[q] = r where idx[r] = q holds a value, 0xffff where it holds none (md_rank_write).  Ranks are
//                 distinct, so the order among equal values is fixed (by position), and a window's k-th value is the
//                 one whose rank has exactly k of the window's ranks below it.
//   the selection md_median: a lane owns kHpOut consecutive outputs, whose windows are rk[q0 + v .. q0 + v + 2 h].  It
//                 counts a window's values (ranks below 0x8000), then finds the rank with k ranks below it by
//                 bisection over the rank's bits, highest first: log2 P rounds of one walk over the 2 h + kHpOut ranks,
//                 each rank read once for the lane's outputs.  An even count takes a second bisection for the upper
//                 middle.  The value is read back through idx from the ring.  CLEAN (the wave's vote,
//                 hp_lane_sees_nan): every window holds 2 h + 1 values, so k = h and nothing is counted first.
//
// The bits are those of the definition whatever the method: B is one of the window's values, or fl(fl(lo + hi) 0.5).
#pragma once

#include "highpass_index.h"

namespace prom {

constexpr int kMdStretch = kHpTile + 2 * kHpMaxHalf;   // positions of a tile's stretch at most
constexpr uint64_t kMdNoKey = ~(uint64_t)0;            // above the key of every value (+inf: 0xfff0...)
constexpr uint32_t kMdNoRank = 0xffffu;                // the rank of a position without a value
static_assert(kMdStretch <= kHpRing, "a stretch's positions have distinct ring slots");
static_assert((kMdStretch & (kMdStretch - 1)) == 0 && kMdStretch <= 0x8000, "ranks fit 15 bits");
static_assert(kHpOut == 4, "the selection reads four ranks at a time from a lane's first window on");

// ---- the stretch of a tile ---------------------------------------------------------------------------------------------
PROM_OBS_HD int32_t md_base(int32_t tile, int32_t h) { return hp_tile_first(tile) - h; }
PROM_OBS_HD int32_t md_len(int32_t tile, int32_t n, int32_t h) {
  const int32_t left = n - hp_tile_first(tile);
  return (left < kHpTile ? left : kHpTile) + 2 * h;
}
// the power of two >= len (len >= 1) and its logarithm
PROM_OBS_HD int32_t md_pow2(int32_t len) {
  int32_t p = 1;
  while (p < len) p <<= 1;
  return p;
}
PROM_OBS_HD int32_t md_bits(int32_t p) {
  int32_t b = 0;
  while ((1 << b) < p) ++b;
  return b;
}
// the stretch index of the first output of thread tid (its window starts there: q = o - h - base)
PROM_OBS_HD int32_t md_q_first(int32_t tid) { return tid * kHpOut; }

// ---- the order of the values ---------------------------------------------------------------------------------------------
PROM_OBS_HD uint64_t md_key(double x) {
  uint64_t b;
  __builtin_memcpy(&b, &x, sizeof b);
  return (b >> 63) ? ~b : (b | ((uint64_t)1 << 63));
}
// the key of stretch index q
PROM_OBS_HD uint64_t md_key_at(const double* ring, int32_t base, int32_t len, int32_t q) {
  if (q >= len) return kMdNoKey;
  const double m = ring[hp_slot(base + q)];
  return m != m ? kMdNoKey : md_key(m);
}

// ---- the sort --------------------------------------------------------------------------------------------------------------
// the stages of the network over p entries: (k, j) for k = 2, 4, .. p and j = k / 2, k / 4, .. 1; in each the pairs
// t = 0 .. p / 2 - 1.  Pair t of stage (k, j) compares the entries lo (bit j clear) and lo + j and leaves them
// ascending where lo's bit k is clear, descending where it is set.
PROM_OBS_HD int32_t md_pair_lo(int32_t t, int32_t j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }
PROM_OBS_HD void md_sort_pair(const double* ring, uint16_t* idx, int32_t base, int32_t len, int32_t t, int32_t j,
                              int32_t k) {
  const int32_t lo = md_pair_lo(t, j), hi = lo + j;
  const int32_t qa = idx[lo], qb = idx[hi];
  const uint64_t ka = md_key_at(ring, base, len, qa), kb = md_key_at(ring, base, len, qb);
  const bool a_after_b = ka > kb || (ka == kb && qa > qb);
  if (a_after_b == ((lo & k) == 0)) {
    idx[lo] = (uint16_t)qb;
    idx[hi] = (uint16_t)qa;
  }
}
// after the sort: the rank of the position idx[r]
PROM_OBS_HD void md_rank_write(const double* ring, const uint16_t* idx, uint16_t* rk, int32_t base, int32_t len,
                               int32_t r) {
  const int32_t q = idx[r];
  rk[q] = (uint16_t)(md_key_at(ring, base, len, q) == kMdNoKey ? kMdNoRank : (uint32_t)r);
}

// ---- the selection -----------------------------------------------------------------------------------------------------------
// One step of the walk over the ranks: the rank r at offset d from the lane's first window's start lies in the window of
// output v when 0 <= d - v <= w2 = 2 h, and counts for it when it is below cand[v].  ALL: it lies in every window.
template <int V, bool ALL>
PROM_OBS_HD void md_count_step(uint32_t r, int32_t d, int32_t w2, const uint32_t (&cand)[V], int32_t (&cnt)[V]) {
#pragma unroll
  for (int v = 0; v < V; ++v)
    if (ALL || (d - v >= 0 && d - v <= w2)) cnt[v] += r < cand[v] ? 1 : 0;
}
// four consecutive ranks from stretch index q, a multiple of 4: one 64-bit LDS read (rk is 8-byte aligned; rank i is
// bits 16 i .. 16 i + 15 on the little-endian device and hosts)
PROM_OBS_HD uint64_t md_load4(const uint16_t* rk, int32_t q) {
  uint64_t w;
  __builtin_memcpy(&w, __builtin_assume_aligned(rk + q, 8), sizeof w);
  return w;
}
// cnt[v] = how many ranks of window v (rk[q0 + v .. q0 + v + w2]) lie below cand[v].  q0 is a multiple of 4 (V = 4
// outputs a lane), so the walk takes the ranks four at a time, d0 = 0, 4, ..: a group whose offsets d0 .. d0 + 3 lie in
// every window (3 <= d0, d0 + 3 <= w2) runs without a test, and several groups' reads are in flight at once; the first
// group and the last one or two test each rank's window.  The last group may read up to two ranks past the lane's last
// window (offsets w2 + 4, w2 + 5 for odd h): they lie inside rk (q0 + w2 + 5 < kMdStretch then) and in no window.
template <int V>
PROM_OBS_HD void md_count(const uint16_t* rk, int32_t q0, int32_t w2, const uint32_t (&cand)[V], int32_t (&cnt)[V]) {
  static_assert(V == 4, "four ranks to a read, four outputs to a lane");
#pragma unroll
  for (int v = 0; v < V; ++v) cnt[v] = 0;
  int32_t d0 = 0;
  {
    const uint64_t w = md_load4(rk, q0);
#pragma unroll
    for (int i = 0; i < 4; ++i) md_count_step<V, false>((uint32_t)(w >> (16 * i)) & 0xffffu, i, w2, cand, cnt);
    d0 = 4;
  }
#pragma unroll 4
  for (; d0 + 3 <= w2; d0 += 4) {
    const uint64_t w = md_load4(rk, q0 + d0);
#pragma unroll
    for (int i = 0; i < 4; ++i) md_count_step<V, true>((uint32_t)(w >> (16 * i)) & 0xffffu, d0 + i, w2, cand, cnt);
  }
  for (; d0 <= w2 + V - 1; d0 += 4) {
    const uint64_t w = md_load4(rk, q0 + d0);
#pragma unroll
    for (int i = 0; i < 4; ++i) md_count_step<V, false>((uint32_t)(w >> (16 * i)) & 0xffffu, d0 + i, w2, cand, cnt);
  }
}
// ans[v] = the rank in window v with exactly k[v] of the window's ranks below it (k[v] < the window's count of values;
// a window without a value gives a number that is no rank).  bits: ranks are below 1 << bits.
template <int V>
PROM_OBS_HD void md_kth_rank(const uint16_t* rk, int32_t q0, int32_t w2, int32_t bits, const int32_t (&k)[V],
                             uint32_t (&ans)[V]) {
#pragma unroll
  for (int v = 0; v < V; ++v) ans[v] = 0;
  for (int32_t b = bits - 1; b >= 0; --b) {
    uint32_t cand[V];
    int32_t cnt[V];
#pragma unroll
    for (int v = 0; v < V; ++v) cand[v] = ans[v] | ((uint32_t)1 << b);
    md_count<V>(rk, q0, w2, cand, cnt);
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (cnt[v] <= k[v]) ans[v] = cand[v];
  }
}
// the value whose rank is r
PROM_OBS_HD double md_value(const double* ring, const uint16_t* idx, int32_t base, uint32_t r) {
  return ring[hp_slot(base + (int32_t)idx[r])];
}

// B of the V consecutive outputs whose first window starts at stretch index q0.  A window without a value gives NaN
// (its output is NaN whatever B is: its own value is none).
template <int V, bool CLEAN>
PROM_OBS_HD void md_median(const double* ring, const uint16_t* idx, const uint16_t* rk, int32_t base, int32_t q0,
                           int32_t h, int32_t bits, double (&B)[V]) {
  const int32_t w2 = 2 * h;
  int32_t c[V], k[V];
  uint32_t lo[V], hi[V];
  if (CLEAN) {
#pragma unroll
    for (int v = 0; v < V; ++v) c[v] = w2 + 1, k[v] = h;
  } else {
    uint32_t any[V];
#pragma unroll
    for (int v = 0; v < V; ++v) any[v] = 0x8000u;
    md_count<V>(rk, q0, w2, any, c);
#pragma unroll
    for (int v = 0; v < V; ++v) k[v] = c[v] > 0 ? (c[v] - 1) / 2 : 0;
  }
  md_kth_rank<V>(rk, q0, w2, bits, k, lo);
  bool even = false;
#pragma unroll
  for (int v = 0; v < V; ++v) hi[v] = lo[v], even = even || (c[v] > 0 && (c[v] & 1) == 0);
  if (!CLEAN && even) {
#pragma unroll
    for (int v = 0; v < V; ++v) k[v] = c[v] / 2;
    md_kth_rank<V>(rk, q0, w2, bits, k, hi);
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    if (c[v] == 0) {
      B[v] = __builtin_nan("");
    } else if (c[v] & 1) {
      B[v] = md_value(ring, idx, base, lo[v]);
    } else {
      B[v] = hp_mul(hp_add(md_value(ring, idx, base, lo[v]), md_value(ring, idx, base, hi[v])), 0.5);
    }
  }
}

}  // namespace prom
