// Host harness of SYSREM per order (prometheus_amd/csrc/order_sysrem_index.h).  Built by
// tests/test_sysrem_orders_cpu.py as a stand-alone program with its own main (also with -fsanitize=address,undefined).
//
//   audit     walks, for a list of shapes, every thread of k_sysrem_prep_orders and k_sysrem_finish_orders with the
//             header's own functions in the kernels' order, through arrays exactly as long as their shapes say: orders
//             of n_s in {1, T - 1, T, T + 1, 3 T + 5} mixed in one table and interleaved (perm is not monotonic, across
//             the orders and inside every second one), n_exp in {1, 2, 7, 70}, 1 and 3 injections.  Counts every index
//             out of range, every work entry of every item (padding included) not written exactly once, every D entry
//             not read exactly once by the prep kernel and every cleaned entry not written exactly once
//   lemma     evaluates an order's row sums (num and den of fit_a) through sy_* in the kernels' shape at width n_s and
//             at width n_max, on random values with cancelling terms, zeros and entries without weight: the bits must
//             be equal and no sum may be -0
//   planner   os_sub_batch under byte caps and at the 65,535-item cap (n_inj n_seg just below, at and above it)
//
// It prints its counters and returns 1 when anything was off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "order_sysrem_index.h"

using namespace prom;

enum { C_THREADS, C_WORK_OOR, C_DATA_OOR, C_PERM_OOR, C_VISIT_ERR, C_COUNT };
static const char* kNames[C_COUNT] = {"threads", "work_oor", "data_oor", "perm_oor", "visit_err"};

// orders of the given lengths dealt over the pixels in turn (so they interleave), every second one reversed
static void make_orders(const std::vector<int32_t>& len, std::vector<int32_t>* seg_first, std::vector<int32_t>* perm) {
  const int32_t n_seg = (int32_t)len.size();
  std::vector<std::vector<int32_t>> mem((size_t)n_seg);
  int32_t n_pix = 0;
  for (int32_t n : len) n_pix += n;
  int32_t s = 0;
  for (int32_t p = 0; p < n_pix; ++p) {
    while ((int32_t)mem[(size_t)s].size() >= len[(size_t)s]) s = (s + 1) % n_seg;
    mem[(size_t)s].push_back(p);
    s = (s + 1) % n_seg;
  }
  seg_first->assign(1, 0);
  perm->clear();
  for (int32_t k = 0; k < n_seg; ++k) {
    if (k % 2)
      for (size_t i = mem[(size_t)k].size(); i-- > 0;) perm->push_back(mem[(size_t)k][i]);
    else
      for (int32_t p : mem[(size_t)k]) perm->push_back(p);
    seg_first->push_back((int32_t)perm->size());
  }
}

static void audit(int32_t n_exp, int32_t n_inj, const std::vector<int32_t>& seg_first, const std::vector<int32_t>& perm,
                  int64_t* cnt) {
  for (int i = 0; i < C_COUNT; ++i) cnt[i] = 0;
  const int32_t n_seg = (int32_t)seg_first.size() - 1, n_pix = (int32_t)perm.size();
  const int32_t n_max = os_n_max(n_seg, seg_first.data());
  const int64_t pitch = sy_pitch(n_max);
  const int32_t items = n_inj * n_seg;
  const int64_t n_work = (int64_t)items * n_exp * pitch, n_data = (int64_t)n_inj * n_exp * n_pix;
  if (pitch < n_max || pitch % kSyTile != 0 || items > kGrMaxBatch) ++cnt[C_VISIT_ERR];
  bool monotonic = true;
  for (int32_t i = 1; i < n_pix; ++i) monotonic = monotonic && perm[(size_t)i] > perm[(size_t)i - 1];
  if (n_seg > 1 && monotonic) ++cnt[C_VISIT_ERR];   // (the shapes are meant to interleave)
  // ---- k_sysrem_prep_orders: grid (flat over n_exp pitch, items)
  {
    std::vector<int32_t> wr((size_t)n_work, 0), rd((size_t)n_data, 0);
    const int64_t wgs = sy_flat_workgroups((int64_t)n_exp * pitch);
    for (int32_t y = 0; y < items; ++y)
      for (int64_t bx = 0; bx < wgs; ++bx)
        for (int32_t tid = 0; tid < kSyFlatBlock; ++tid) {
          const int64_t t = bx * kSyFlatBlock + tid;
          if (t >= (int64_t)n_exp * pitch) continue;
          ++cnt[C_THREADS];
          const int32_t b = os_item_injection(y, n_seg), s = os_item_order(y, n_seg);
          if (b < 0 || b >= n_inj || s < 0 || s >= n_seg || os_item(b, s, n_seg) != y) ++cnt[C_VISIT_ERR];
          const int32_t e = (int32_t)(t / pitch), i = (int32_t)(t % pitch);
          const int32_t n_s = seg_first[(size_t)s + 1] - seg_first[(size_t)s];
          if (i < n_s) {
            const int32_t slot = os_slot(seg_first.data(), s, i);
            if (slot < 0 || slot >= n_pix) {
              ++cnt[C_PERM_OOR];
              continue;
            }
            const int32_t p = perm[(size_t)slot];
            const int64_t da = os_data(b, e, p, n_exp, n_pix), iv = ex_data(e, p, n_pix);
            if (da < 0 || da >= n_data || iv < 0 || iv >= (int64_t)n_exp * n_pix)
              ++cnt[C_DATA_OOR];
            else
              ++rd[(size_t)da];
          }
          const int64_t at = os_work(y, e, i, n_exp, pitch);
          if (at < 0 || at >= n_work)
            ++cnt[C_WORK_OOR];
          else
            ++wr[(size_t)at];
        }
    for (auto v : wr) cnt[C_VISIT_ERR] += v != 1;
    for (auto v : rd) cnt[C_VISIT_ERR] += v != 1;
  }
  // ---- the step kernels see item y as a table n_max wide: its slice must be the single call's of the batch item y
  for (int32_t y = 0; y < items; ++y)
    if (gr_work(y, n_exp, pitch) != os_work(y, 0, 0, n_exp, pitch) ||
        gr_work(y, n_exp, pitch) + (int64_t)n_exp * pitch > n_work)
      ++cnt[C_WORK_OOR];
  // ---- k_sysrem_finish_orders: grid (flat over n_exp n_max, items)
  {
    std::vector<int32_t> ow((size_t)n_data, 0);
    const int64_t wgs = sy_flat_workgroups((int64_t)n_exp * n_max);
    for (int32_t y = 0; y < items; ++y)
      for (int64_t bx = 0; bx < wgs; ++bx)
        for (int32_t tid = 0; tid < kSyFlatBlock; ++tid) {
          const int64_t t = bx * kSyFlatBlock + tid;
          if (t >= (int64_t)n_exp * n_max) continue;
          ++cnt[C_THREADS];
          const int32_t b = os_item_injection(y, n_seg), s = os_item_order(y, n_seg);
          const int32_t e = (int32_t)(t / n_max), i = (int32_t)(t % n_max);
          if (i >= seg_first[(size_t)s + 1] - seg_first[(size_t)s]) continue;
          const int32_t slot = os_slot(seg_first.data(), s, i);
          if (slot < 0 || slot >= n_pix) {
            ++cnt[C_PERM_OOR];
            continue;
          }
          const int32_t p = perm[(size_t)slot];
          const int64_t at = os_work(y, e, i, n_exp, pitch), da = os_data(b, e, p, n_exp, n_pix);
          if (at < 0 || at >= n_work) ++cnt[C_WORK_OOR];
          if (da < 0 || da >= n_data)
            ++cnt[C_DATA_OOR];
          else
            ++ow[(size_t)da];
        }
    for (auto v : ow) cnt[C_VISIT_ERR] += v != 1;
  }
}

// ---- the lemma ------------------------------------------------------------------------------------------------------
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double rnd() {   // (0, 1), 53 bits
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return ((double)(g_state >> 11) + 0.5) / 9007199254740992.0;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// num and den of one exposure's row over n positions, in the kernels' shape at the given width: k_sysrem_prep_orders'
// padding, k_sysrem_step's lane sums and butterfly per tile, k_sysrem_rows' lanes and butterfly
static void row_sums(const std::vector<double>& w0, const std::vector<double>& r0, const std::vector<double>& c0,
                     int32_t n, int32_t width, double* num, double* den) {
  const int32_t n_tiles = sy_tiles(width);
  const int64_t pitch = sy_pitch(width);
  std::vector<double> w((size_t)pitch, 0.0), r((size_t)pitch, 0.0), c((size_t)pitch, 0.0);   // c of a column without
  for (int32_t i = 0; i < n; ++i) {                                                            // weight: ratio(0, 0)
    w[(size_t)i] = w0[(size_t)i];
    r[(size_t)i] = w0[(size_t)i] > 0.0 ? r0[(size_t)i] : 0.0;
    c[(size_t)i] = c0[(size_t)i];
  }
  std::vector<double> pn((size_t)n_tiles), pd((size_t)n_tiles);
  for (int32_t tile = 0; tile < n_tiles; ++tile) {
    double tn[64], td[64];
    for (int32_t lane = 0; lane < kSyBlock; ++lane) {
      const int32_t p = sy_pixel(tile, lane);
      tn[lane] = td[lane] = 0.0;
      for (int v = 0; v < kSyVec; ++v)
        sy_fit_add(w[(size_t)sy_at(0, p + v, pitch)], r[(size_t)sy_at(0, p + v, pitch)], c[(size_t)(p + v)], &tn[lane],
                   &td[lane]);
    }
    sy_butterfly_host(tn);
    sy_butterfly_host(td);
    pn[(size_t)sy_part(0, tile, n_tiles)] = tn[0];
    pd[(size_t)sy_part(0, tile, n_tiles)] = td[0];
  }
  double tn[64], td[64];
  for (int32_t lane = 0; lane < 64; ++lane) {
    tn[lane] = td[lane] = 0.0;
    for (int32_t i = 0; i < sy_rows_count(lane, n_tiles); ++i) {
      const size_t pa = (size_t)sy_part(0, sy_rows_tile(lane, i), n_tiles);
      tn[lane] = sy_add(tn[lane], pn[pa]);
      td[lane] = sy_add(td[lane], pd[pa]);
    }
  }
  sy_butterfly_host(tn);
  sy_butterfly_host(td);
  *num = tn[0];
  *den = td[0];
}

static int lemma() {
  const int32_t T = kSyTile;
  const int32_t ns[] = {1, 2, T - 1, T, T + 1, 3 * T + 5, 63 * T + 7};
  const int32_t widths[] = {T + 1, 3 * T + 5, 64 * T + 1, 130 * T};   // (the last two: a rows lane with several tiles)
  int bad = 0, cases = 0, exact_zero = 0;
  for (int32_t n : ns)
    for (int kind = 0; kind < 4; ++kind) {
      std::vector<double> w((size_t)n), r((size_t)n), c((size_t)n);
      for (int32_t i = 0; i < n; ++i) {
        w[(size_t)i] = rnd() < 0.1 ? 0.0 : 1e4 * (0.1 + rnd());
        r[(size_t)i] = (rnd() - 0.5) * std::ldexp(1.0, (int)(40 * rnd()) - 20);
        c[(size_t)i] = rnd() < 0.1 ? 0.0 : rnd() - 0.5;
      }
      if (kind == 1)   // cancelling pairs: the numerator is exactly zero
        for (int32_t i = 0; i + 1 < n; i += 2) {
          w[(size_t)i + 1] = w[(size_t)i];
          c[(size_t)i + 1] = c[(size_t)i];
          r[(size_t)i + 1] = -r[(size_t)i];
        }
      if (kind == 2)   // negative terms only, and negative zeros among the products
        for (int32_t i = 0; i < n; ++i) r[(size_t)i] = i % 3 ? -std::fabs(r[(size_t)i]) : -0.0;
      if (kind == 3)   // nothing weighted
        for (int32_t i = 0; i < n; ++i) w[(size_t)i] = 0.0;
      double n0, d0;
      row_sums(w, r, c, n, n, &n0, &d0);
      bad += (n0 == 0.0 && std::signbit(n0)) || (d0 == 0.0 && std::signbit(d0));
      exact_zero += n0 == 0.0;
      for (int32_t width : widths) {
        if (width < n) continue;
        double n1, d1;
        row_sums(w, r, c, n, width, &n1, &d1);
        bad += !same_bits(n0, n1) || !same_bits(d0, d1);
        ++cases;
      }
    }
  std::printf("lemma cases=%d exact_zero_sums=%d mismatches=%d\n", cases, exact_zero, bad);
  return bad != 0 || exact_zero < 7;
}

// ---- the planner ----------------------------------------------------------------------------------------------------
static int planner() {
  int bad = 0;
  const int32_t n_exp = 48, n_pix = 48000, n_seg = 24, n_max = 2000, n_cols = 6, n_tap = 2;
  const int64_t per = os_injection_bytes(n_exp, n_pix, n_seg, n_max, n_cols, n_tap);
  // the byte count, restated: D, out, model [n_exp][n_pix]; Fj; per order r, w, a, part pairs, U; the flags
  const int64_t work = (int64_t)n_exp * sy_pitch(n_max);
  const int64_t want = 8 * (3 * (int64_t)n_exp * n_pix + (int64_t)n_exp * n_tap +
                            n_seg * (2 * work + n_exp + 2 * (int64_t)n_exp * sy_tiles(n_max) + (int64_t)n_exp * n_cols)) +
                       4 * (int64_t)kGrFlags * n_seg;
  bad += per != want;
  bad += os_sub_batch(per - 1, per, 10, n_seg) != 1;          // one at least
  bad += os_sub_batch(3 * per, per, 10, n_seg) != 3;
  bad += os_sub_batch(4 * per - 1, per, 10, n_seg) != 3;
  bad += os_sub_batch(100 * per, per, 10, n_seg) != 10;       // the list at most
  bad += os_sub_batch((int64_t)1 << 62, per, 1 << 20, n_seg) != kGrMaxBatch / n_seg;
  // one order and one injection's bytes: the grids' own planner
  bad += os_sub_batch(5 * per, per, 9, 1) != gr_sub_batch(5 * per, per, 9);
  // the item cap: n_inj n_seg just below, at and above 65,535
  const int64_t big = (int64_t)1 << 62;
  bad += os_sub_batch(big, 1, 13107, 5) != 13107;             // 65,535 items
  bad += os_sub_batch(big, 1, 13106, 5) != 13106;             // 65,530
  bad += os_sub_batch(big, 1, 13108, 5) != 13107;             // 65,540 asked, 65,535 given
  bad += os_sub_batch(big, 1, 3, kGrMaxBatch) != 1;           // an injection fills a launch
  bad += os_sub_batch(big, 1, 3, kGrMaxBatch + 1) != 0;       // no launch holds one injection
  bad += os_sub_batch(big, 1, 3, kGrMaxBatch - 1) != 1;
  bad += os_sub_batch(big, 1, 0, 5) != 0;                     // an empty list
  for (int32_t n_inj : {1, 7, 13107, 13108, 40000})
    for (int32_t segs : {1, 5, 24, 80, 65535}) {
      const int32_t nb = os_sub_batch(big, 1, n_inj, segs);
      bad += nb < 1 || nb > n_inj || (int64_t)nb * segs > kGrMaxBatch;
      int64_t covered = 0;
      for (int32_t s = 0; s < gr_sub_batches(n_inj, nb); ++s) covered += gr_sub_count(s, nb, n_inj);
      bad += covered != n_inj;
    }
  std::printf("planner per_injection=%lld errors=%d\n", (long long)per, bad);
  return bad != 0;
}

int main() {
  const int32_t T = kSyTile;
  const std::vector<std::vector<int32_t>> tables = {
      {1, T - 1, T, T + 1, 3 * T + 5},   // every length of the list mixed in one table
      {3 * T + 5, 1, T + 1},
      {T, T, T},                         // equal orders: no padding but the tile's
      {T + 1},                           // one order
      {1, 2, 1}};                        // hardly a pixel
  const int32_t exps[] = {1, 2, 7, 70};
  const int32_t injs[] = {1, 3};
  int rc = 0, n_shapes = 0;
  for (const auto& len : tables) {
    std::vector<int32_t> seg_first, perm;
    make_orders(len, &seg_first, &perm);
    for (int32_t n_exp : exps)
      for (int32_t n_inj : injs) {
        ++n_shapes;
        int64_t cnt[C_COUNT];
        audit(n_exp, n_inj, seg_first, perm, cnt);
        std::printf("n_seg=%d n_pix=%d n_max=%d n_exp=%d n_inj=%d:", (int)len.size(), (int)perm.size(),
                    os_n_max((int32_t)len.size(), seg_first.data()), n_exp, n_inj);
        for (int i = 0; i < C_COUNT; ++i) std::printf(" %s=%lld", kNames[i], (long long)cnt[i]);
        std::printf("\n");
        for (int i = C_WORK_OOR; i < C_COUNT; ++i) rc |= cnt[i] != 0;
      }
  }
  std::printf("shapes=%d tile=%d\n", n_shapes, T);
  rc |= lemma();
  rc |= planner();
  return rc;
}
