// Host harness of the injection grids' index arithmetic (prometheus_amd/csrc/grid_index.h) over the batched kernels of
// prom_sysrem.hip, prom_filter.hip and prom_detrend.hip.  Built by tests/test_inject_grid_cpu.py as a stand-alone
// program with its own main (also with -fsanitize=address,undefined).
//
//   grid_host           walks, for n_inj in {1, 2, 5} x n_pix in {1, T - 1, T, T + 1, 3 T + 5} x n_exp in {1, 2, 7}, every
//                       thread of every batched launch (k_gather_grid, k_inject_grid, k_sysrem_prep, _fill, _step, _rows,
//                       _finish, k_filter_weights and the out-of-place k_detrend) with the headers' own functions in the
//                       kernels' order, blockIdx.y = the injection, through arrays exactly as long as the C-ABI layer
//                       makes them; counts every index outside its buffer (oor), every access of injection b outside
//                       b's own slice, the `ended` flags included (foreign), every entry of a per-injection buffer not
//                       written exactly once (visit_err), and every sub-batch plan that does not cover the list exactly
//                       once or exceeds its cap with more than one injection (plan_err), for caps that give 1, 2 and
//                       n_inj sub-batches
//   grid_host <file>    evaluates a batch in the kernels' order, launch by launch with the flags as the launches see
//                       them, on a case it is given: n_inj, n_exp, n_pix, n_comp, n_iter, ones, n_trial and then, as
//                       hexadecimal floats, raw[n_exp][n_pix], ivar[n_exp][n_pix], model[n_exp][n_inj][n_pix],
//                       scale[n_inj], the table's model T[n_exp][n_trial][n_pix], and per injection the expected
//                       U[n_exp][n_cols], cleaned[n_exp][n_pix], W[n_cols][n_exp][n_pix] and the filtered
//                       T'[n_exp][n_trial][n_pix]; the results must agree bit for bit (NaN with NaN, signs of zero), and
//                       T must come out untouched
//
// It prints its counters and returns 1 when anything was off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "grid_index.h"

using namespace prom;

enum { C_WORKGROUPS, C_THREADS, C_OOR, C_FOREIGN, C_VISIT_ERR, C_PLAN_ERR, C_COUNT };
static const char* kNames[C_COUNT] = {"workgroups", "threads", "oor", "foreign", "visit_err", "plan_err"};

// a buffer of B slices, injection b's first to last (or, `inner` > 0, [x][B][inner] as k_expose lays out a table of B
// trials): every access names its injection
struct Sliced {
  int64_t slice, inner;
  int32_t B;
  std::vector<int32_t> wr;
  Sliced(int64_t slice_, int32_t B_, int64_t inner_ = 0) : slice(slice_), inner(inner_), B(B_), wr((size_t)(slice_ * B_), 0) {}
  bool at(int64_t i, int32_t b, int64_t* cnt) const {
    if (i < 0 || i >= slice * B) {
      ++cnt[C_OOR];
      return false;
    }
    const int32_t owner = inner > 0 ? (int32_t)((i / inner) % B) : (int32_t)(i / slice);
    if (owner != b) ++cnt[C_FOREIGN];
    return true;
  }
  void read(int64_t i, int32_t b, int64_t* cnt) const { at(i, b, cnt); }
  void write(int64_t i, int32_t b, int64_t* cnt) {
    if (at(i, b, cnt)) ++wr[(size_t)i];
  }
  void once(int64_t* cnt) {
    for (auto& v : wr) {
      cnt[C_VISIT_ERR] += v != 1;
      v = 0;
    }
  }
};

static void shared_read(int64_t i, int64_t n, int64_t* cnt) { cnt[C_OOR] += i < 0 || i >= n; }

static void plan_audit(int32_t n_exp, int32_t n_pix, int32_t n_cols, int32_t n_tap, int32_t n_inj, int64_t* cnt) {
  for (int recover = 0; recover < 2; ++recover) {
    const int64_t per = gr_injection_bytes(n_exp, n_pix, n_cols, n_tap, recover != 0);
    if (per <= 0) ++cnt[C_PLAN_ERR];
    const int32_t half = (n_inj + 1) / 2;
    const int64_t caps[] = {per * n_inj, per * n_inj + per - 1, per * half, per, per - 1, 1, per * 100000};
    const int32_t want[] = {1, 1, n_inj > 1 ? 2 : 1, n_inj, n_inj, n_inj, 1};
    for (int i = 0; i < 7; ++i) {
      const int32_t nb = gr_sub_batch(caps[i], per, n_inj), n_sub = gr_sub_batches(n_inj, nb);
      if (nb < 1 || nb > kGrMaxBatch || nb > n_inj || n_sub != want[i]) ++cnt[C_PLAN_ERR];
      if (nb > 1 && nb * per > caps[i]) ++cnt[C_PLAN_ERR];
      std::vector<int32_t> seen((size_t)n_inj, 0);
      for (int32_t s = 0; s < n_sub; ++s) {
        const int32_t b0 = gr_sub_first(s, nb), c = gr_sub_count(s, nb, n_inj);
        if (c < 1 || c > nb) ++cnt[C_PLAN_ERR];
        for (int32_t b = b0; b < b0 + c; ++b) {
          if (b < 0 || b >= n_inj)
            ++cnt[C_PLAN_ERR];
          else
            ++seen[(size_t)b];
        }
      }
      for (auto v : seen) cnt[C_PLAN_ERR] += v != 1;
    }
  }
  if (gr_sub_batch((int64_t)1 << 62, 1, 1 << 30) != kGrMaxBatch) ++cnt[C_PLAN_ERR];
}

static void grid_audit(int32_t B, int32_t n_exp, int32_t n_pix, int32_t n_cols, int64_t* cnt) {
  for (int i = 0; i < C_COUNT; ++i) cnt[i] = 0;
  const int32_t n_tap = 2, n_trial = 3, n_tiles = sy_tiles(n_pix);
  const int64_t pitch = sy_pitch(n_pix), n = (int64_t)n_exp * n_pix;
  std::vector<int32_t> trial((size_t)B);
  for (int32_t b = 0; b < B; ++b) trial[(size_t)b] = (2 * b + 1) % n_trial;
  Sliced Fj((int64_t)n_exp * n_tap, B, n_tap), model(n, B, n_pix), D(n, B), out(n, B), r(n_exp * pitch, B),
      w(n_exp * pitch, B), a(n_exp, B), part((int64_t)n_exp * n_tiles, B), U((int64_t)n_exp * n_cols, B),
      ended(kGrFlags, B), W((int64_t)n_cols * n, B);
  plan_audit(n_exp, n_pix, n_cols, n_tap, B, cnt);
  // ---- k_gather_grid
  for (int32_t b = 0; b < B; ++b)
    for (int64_t bx = 0; bx < sy_flat_workgroups((int64_t)n_exp * n_tap); ++bx) {
      ++cnt[C_WORKGROUPS];
      for (int32_t tid = 0; tid < kSyFlatBlock; ++tid) {
        const int64_t i = bx * kSyFlatBlock + tid;
        if (i >= (int64_t)n_exp * n_tap) continue;
        ++cnt[C_THREADS];
        const int32_t e = (int32_t)(i / n_tap), tap = (int32_t)(i % n_tap);
        shared_read(gr_gather_from(e, trial[(size_t)b], tap, n_trial, n_tap), (int64_t)n_exp * n_trial * n_tap, cnt);
        Fj.write(gr_gather_to(e, b, tap, B, n_tap), b, cnt);
      }
    }
  Fj.once(cnt);
  // ---- k_inject_grid (the model of k_expose over the table of B trials is written by k_expose itself)
  for (int32_t b = 0; b < B; ++b)
    for (int64_t bx = 0; bx < sy_flat_workgroups(n); ++bx) {
      ++cnt[C_WORKGROUPS];
      for (int32_t tid = 0; tid < kSyFlatBlock; ++tid) {
        const int64_t i = bx * kSyFlatBlock + tid;
        if (i >= n) continue;
        ++cnt[C_THREADS];
        const int32_t e = (int32_t)(i / n_pix), p = (int32_t)(i % n_pix);
        shared_read(ex_data(e, p, n_pix), n, cnt);
        model.read(gr_inject_model(e, b, p, B, n_pix), b, cnt);
        D.write(gr_inject_to(b, e, p, n_exp, n_pix), b, cnt);
      }
    }
  D.once(cnt);
  // ---- k_sysrem_prep
  for (int32_t b = 0; b < B; ++b)
    for (int64_t bx = 0; bx < sy_flat_workgroups(n_exp * pitch); ++bx) {
      ++cnt[C_WORKGROUPS];
      for (int32_t tid = 0; tid < kSyFlatBlock; ++tid) {
        const int64_t i = bx * kSyFlatBlock + tid;
        if (i >= n_exp * pitch) continue;
        ++cnt[C_THREADS];
        const int32_t e = (int32_t)(i / pitch), p = (int32_t)(i % pitch);
        if (p < n_pix) {
          D.read(gr_data(b, n_exp, n_pix) + ex_data(e, p, n_pix), b, cnt);
          shared_read(ex_data(e, p, n_pix), n, cnt);   // ivar
        }
        w.write(gr_work(b, n_exp, pitch) + sy_at(e, p, pitch), b, cnt);
        r.write(gr_work(b, n_exp, pitch) + sy_at(e, p, pitch), b, cnt);
      }
    }
  w.once(cnt);
  r.once(cnt);
  for (int32_t col = 0; col < n_cols; ++col) {
    // ---- k_sysrem_fill
    for (int32_t b = 0; b < B; ++b)
      for (int64_t bx = 0; bx < sy_flat_workgroups(n_exp); ++bx) {
        ++cnt[C_WORKGROUPS];
        for (int32_t tid = 0; tid < kSyFlatBlock; ++tid) {
          const int32_t e = (int32_t)bx * kSyFlatBlock + tid;
          if (e >= n_exp) continue;
          ++cnt[C_THREADS];
          a.write(gr_a(b, n_exp) + e, b, cnt);
          U.write(gr_u(b, n_exp, n_cols) + sy_u(e, col, n_cols), b, cnt);
        }
      }
    a.once(cnt);
    // ---- k_sysrem_step: the launcher passes ended + col; a wave per (tile, injection); both walks
    for (int32_t b = 0; b < B; ++b)
      for (int32_t tile = 0; tile < n_tiles; ++tile) {
        ++cnt[C_WORKGROUPS];
        for (int32_t lane = 0; lane < kSyBlock; ++lane) {
          ++cnt[C_THREADS];
          ended.read(col + gr_flag(b, 0), b, cnt);
          const int32_t p = sy_pixel(tile, lane);
          for (int32_t e = 0; e < n_exp; ++e) {
            a.read(gr_a(b, n_exp) + e, b, cnt);
            const int64_t at = gr_work(b, n_exp, pitch) + sy_at(e, p, pitch);
            if ((at * 8) % (kSyVec * 8) != 0) ++cnt[C_OOR];   // (one aligned vector)
            for (int v = 0; v < kSyVec; ++v) {
              w.read(at + v, b, cnt);
              r.write(at + v, b, cnt);   // (read in both walks, written back by the last step)
            }
            if (lane == 0) part.write(gr_part(b, n_exp, n_tiles) + sy_part(e, tile, n_tiles), b, cnt);
          }
        }
      }
    r.once(cnt);
    part.once(cnt);
    // ---- k_sysrem_rows: one workgroup per injection, blockIdx.x
    for (int32_t b = 0; b < B; ++b) {
      ++cnt[C_WORKGROUPS];
      ended.write(col + gr_flag(b, 0), b, cnt);   // (read by every thread, set by thread 0)
      for (int32_t wave = 0; wave < kSyRowsBlock / 64; ++wave)
        for (int32_t e = wave; e < n_exp; e += kSyRowsBlock / 64)
          for (int32_t lane = 0; lane < 64; ++lane)
            for (int32_t i = 0; i < sy_rows_count(lane, n_tiles); ++i)
              part.write(gr_part(b, n_exp, n_tiles) + sy_part(e, sy_rows_tile(lane, i), n_tiles), b, cnt);   // (a read)
      for (int32_t tid = 0; tid < kSyRowsBlock; ++tid)
        for (int32_t e = tid; e < n_exp; e += kSyRowsBlock) {
          ++cnt[C_THREADS];
          a.write(gr_a(b, n_exp) + e, b, cnt);
          U.write(gr_u(b, n_exp, n_cols) + sy_u(e, col, n_cols), b, cnt);
        }
    }
    part.once(cnt);
    a.once(cnt);
  }
  // U: once by k_sysrem_fill and once by k_sysrem_rows per column; every flag of a column in use once
  for (auto& v : U.wr) {
    cnt[C_VISIT_ERR] += v != 2;
    v = 0;
  }
  for (int32_t b = 0; b < B; ++b)
    for (int32_t col = 0; col < kGrFlags; ++col)
      cnt[C_VISIT_ERR] += ended.wr[(size_t)gr_flag(b, col)] != (col < n_cols ? 1 : 0);
  // ---- k_sysrem_finish
  for (int32_t b = 0; b < B; ++b)
    for (int64_t bx = 0; bx < sy_flat_workgroups(n); ++bx) {
      ++cnt[C_WORKGROUPS];
      for (int32_t tid = 0; tid < kSyFlatBlock; ++tid) {
        const int64_t i = bx * kSyFlatBlock + tid;
        if (i >= n) continue;
        ++cnt[C_THREADS];
        const int32_t e = (int32_t)(i / n_pix), p = (int32_t)(i % n_pix);
        r.read(gr_work(b, n_exp, pitch) + sy_at(e, p, pitch), b, cnt);
        w.read(gr_work(b, n_exp, pitch) + sy_at(e, p, pitch), b, cnt);
        D.read(gr_data(b, n_exp, n_pix) + ex_data(e, p, n_pix), b, cnt);
        out.write(gr_data(b, n_exp, n_pix) + ex_data(e, p, n_pix), b, cnt);
      }
    }
  out.once(cnt);
  // ---- k_filter_weights: a thread per (pixel, injection); fw_weights reads U + dt_u(e, 0, K) and iv[e stride], and
  // writes W[(k n_exp + e) stride]
  for (int32_t b = 0; b < B; ++b)
    for (int32_t tile = 0; tile < fw_tiles(n_pix); ++tile) {
      ++cnt[C_WORKGROUPS];
      for (int32_t tid = 0; tid < kFwTile; ++tid) {
        const int32_t p = fw_pixel(tile, tid);
        if (p >= n_pix) continue;
        ++cnt[C_THREADS];
        for (int32_t e = 0; e < n_exp; ++e) {
          shared_read(ex_data(0, p, n_pix) + (int64_t)e * n_pix, n, cnt);
          for (int32_t k = 0; k < n_cols; ++k) {
            U.read(gr_u(b, n_exp, n_cols) + dt_u(e, 0, n_cols) + k, b, cnt);
            W.write(gr_w(b, n_cols, n_exp, n_pix) + dt_w(0, 0, p, n_exp, n_pix) + ((int64_t)k * n_exp + e) * n_pix, b, cnt);
          }
        }
      }
    }
  W.once(cnt);
  // ---- k_detrend out of place, one launch per injection: the column of src read, the same column of dst written
  const int64_t n_model = n * n_trial;
  for (int32_t b = 0; b < B; ++b) {
    std::vector<int32_t> dst((size_t)n_model, 0), flag((size_t)n_trial * n_pix, 0);
    const int32_t dt_t = dt_tiles(n_pix);
    for (int64_t bx = 0; bx < dt_workgroups(n_trial, n_pix); ++bx) {
      ++cnt[C_WORKGROUPS];
      for (int32_t tid = 0; tid < kDtBlock; ++tid) {
        const int32_t p = dt_pixel(dt_wg_tile((int32_t)bx, dt_t), tid), j = dt_trial(dt_wg_group((int32_t)bx, dt_t), tid);
        if (p >= n_pix || j >= n_trial) continue;
        ++cnt[C_THREADS];
        const int64_t m0 = ex_model(0, j, p, n_trial, n_pix), m_stride = (int64_t)n_trial * n_pix;
        for (int32_t e = 0; e < n_exp; ++e) {
          const int64_t at = m0 + e * m_stride;
          if (at < 0 || at >= n_model) {
            ++cnt[C_OOR];
            continue;
          }
          ++dst[(size_t)at];
          for (int32_t k = 0; k < n_cols; ++k) {
            W.read(gr_w(b, n_cols, n_exp, n_pix) + dt_w(0, 0, p, n_exp, n_pix) + ((int64_t)k * n_exp + e) * n_pix, b, cnt);
            U.read(gr_u(b, n_exp, n_cols) + dt_u(e, k, n_cols), b, cnt);
          }
        }
        const int64_t fa = dt_flag(j, p, n_pix);
        if (fa < 0 || fa >= (int64_t)n_trial * n_pix)
          ++cnt[C_OOR];
        else
          ++flag[(size_t)fa];
      }
    }
    for (auto v : dst) cnt[C_VISIT_ERR] += v != 1;
    for (auto v : flag) cnt[C_VISIT_ERR] += v != 1;
  }
}

// ---- the evaluation ---------------------------------------------------------------------------------------------------
static bool same_bits(double x, double y) {
  if (x != x && y != y) return true;
  return std::memcmp(&x, &y, sizeof x) == 0;
}

template <int K>
static void weights_pixel(const double* U, const double* iv, double* W, int64_t stride, int32_t n_exp) {
  FwTri<fw_entries(K)> L;
  L.mem = nullptr;
  L.pitch = 0;
  fw_weights<K, fw_entries(K)>(L, U, iv, W, stride, n_exp);
}

template <int K>
static bool detrend_column(const double* S, double* M, int64_t m_stride, const double* U, const double* W, int64_t w_stride,
                           int32_t n_exp) {
  double c[K];
  const bool ok = dt_coefficients<K>(S, m_stride, W, w_stride, n_exp, c);
  dt_apply<K>(S, M, m_stride, U, n_exp, c, ok);
  return ok;
}

#define GRID_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

struct Batch {
  int32_t B, n_exp, n_pix, n_cols, n_tiles;
  int64_t pitch;
  std::vector<double> D, out, r, w, a, part, U, W;
  std::vector<int32_t> ended;
};

// k_sysrem_step of injection b (the launcher's ended + col), every tile
static void step(Batch& s, int32_t b, int32_t col, bool last) {
  if (s.ended[(size_t)(col + gr_flag(b, 0))]) return;
  double* r = s.r.data() + gr_work(b, s.n_exp, s.pitch);
  const double* w = s.w.data() + gr_work(b, s.n_exp, s.pitch);
  const double* a = s.a.data() + gr_a(b, s.n_exp);
  double* part = s.part.data() + 2 * gr_part(b, s.n_exp, s.n_tiles);
  std::vector<double> c((size_t)s.pitch, 0.0);
  for (int32_t tile = 0; tile < s.n_tiles; ++tile) {
    for (int32_t lane = 0; lane < kSyBlock; ++lane) {
      const int32_t p = sy_pixel(tile, lane);
      for (int v = 0; v < kSyVec; ++v) {
        double num = 0.0, den = 0.0;
        for (int32_t e = 0; e < s.n_exp; ++e)
          sy_fit_add(w[sy_at(e, p + v, s.pitch)], r[sy_at(e, p + v, s.pitch)], a[e], &num, &den);
        c[(size_t)(p + v)] = sy_ratio(num, den);
      }
    }
    for (int32_t e = 0; e < s.n_exp; ++e) {
      if (last) {
        for (int32_t lane = 0; lane < kSyBlock; ++lane)
          for (int v = 0; v < kSyVec; ++v) {
            const int64_t at = sy_at(e, sy_pixel(tile, lane) + v, s.pitch);
            r[at] = sy_residual(w[at], r[at], a[e], c[(size_t)(sy_pixel(tile, lane) + v)]);
          }
        continue;
      }
      double tn[64], td[64];
      for (int32_t lane = 0; lane < kSyBlock; ++lane) {
        const int32_t p = sy_pixel(tile, lane);
        tn[lane] = td[lane] = 0.0;
        for (int v = 0; v < kSyVec; ++v)
          sy_fit_add(w[sy_at(e, p + v, s.pitch)], r[sy_at(e, p + v, s.pitch)], c[(size_t)(p + v)], &tn[lane], &td[lane]);
      }
      sy_butterfly_host(tn);
      sy_butterfly_host(td);
      part[2 * sy_part(e, tile, s.n_tiles)] = tn[0];
      part[2 * sy_part(e, tile, s.n_tiles) + 1] = td[0];
    }
  }
}

// k_sysrem_rows of injection b
static void rows(Batch& s, int32_t b, int32_t col) {
  int32_t* ended = s.ended.data() + col + gr_flag(b, 0);
  if (*ended) return;
  const double* part = s.part.data() + 2 * gr_part(b, s.n_exp, s.n_tiles);
  double* a = s.a.data() + gr_a(b, s.n_exp);
  double* U = s.U.data() + gr_u(b, s.n_exp, s.n_cols);
  std::vector<double> sA((size_t)s.n_exp);
  for (int32_t e = 0; e < s.n_exp; ++e) {
    double tn[64], td[64];
    for (int32_t lane = 0; lane < 64; ++lane) {
      tn[lane] = td[lane] = 0.0;
      for (int32_t i = 0; i < sy_rows_count(lane, s.n_tiles); ++i) {
        const int64_t pa = sy_part(e, sy_rows_tile(lane, i), s.n_tiles);
        tn[lane] = sy_add(tn[lane], part[2 * pa]);
        td[lane] = sy_add(td[lane], part[2 * pa + 1]);
      }
    }
    sy_butterfly_host(tn);
    sy_butterfly_host(td);
    sA[(size_t)e] = sy_ratio(tn[0], td[0]);
  }
  double sum = 0.0;
  for (int32_t e = 0; e < s.n_exp; ++e) sum = sy_add(sum, sy_mul(sA[(size_t)e], sA[(size_t)e]));
  const double norm = sy_sqrt(sum);
  const bool ok = norm > 0.0;
  for (int32_t e = 0; e < s.n_exp; ++e) {
    const double v = ok ? sy_div(sA[(size_t)e], norm) : 0.0;
    a[e] = v;
    U[sy_u(e, col, s.n_cols)] = v;
  }
  if (!ok) *ended = 1;
}

static void fill(Batch& s, int32_t b, int32_t col, double value) {
  for (int32_t e = 0; e < s.n_exp; ++e) {
    s.a[(size_t)(gr_a(b, s.n_exp) + e)] = value;
    s.U[(size_t)(gr_u(b, s.n_exp, s.n_cols) + sy_u(e, col, s.n_cols))] = value;
  }
}

static int batch_case(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 1;
  int B = 0, n_exp = 0, n_pix = 0, n_comp = 0, n_iter = 0, ones = 0, n_trial = 0;
  if (std::fscanf(f, "%d %d %d %d %d %d %d", &B, &n_exp, &n_pix, &n_comp, &n_iter, &ones, &n_trial) != 7) return 1;
  const int32_t n_cols = n_comp + ones;
  if (B < 1 || n_exp < 1 || n_exp > kSyMaxExp || n_pix < 1 || n_cols < 1 || n_cols > kSyMaxComp || n_trial < 1) return 1;
  auto read = [&](std::vector<double>& v, size_t n) {
    v.resize(n);
    char buf[64];
    for (size_t i = 0; i < n; ++i) {
      if (std::fscanf(f, "%63s", buf) != 1) return false;
      v[i] = std::strtod(buf, nullptr);   // hexadecimal floats, "nan" and "inf"
    }
    return true;
  };
  const size_t n = (size_t)n_exp * n_pix, nt = n * n_trial;
  std::vector<double> raw, ivar, model, scale, T, want_U, want_out, want_W, want_T;
  if (!read(raw, n) || !read(ivar, n) || !read(model, n * B) || !read(scale, (size_t)B) || !read(T, nt) ||
      !read(want_U, (size_t)B * n_exp * n_cols) || !read(want_out, n * B) || !read(want_W, n * B * n_cols) ||
      !read(want_T, nt * B))
    return 1;
  std::fclose(f);
  Batch s;
  s.B = B, s.n_exp = n_exp, s.n_pix = n_pix, s.n_cols = n_cols, s.n_tiles = sy_tiles(n_pix), s.pitch = sy_pitch(n_pix);
  const size_t work = (size_t)(n_exp * s.pitch);
  s.D.assign(n * B, -7.0), s.out.assign(n * B, -7.0), s.r.assign(work * B, -7.0), s.w.assign(work * B, -7.0);
  s.a.assign((size_t)n_exp * B, -7.0), s.part.assign(2 * (size_t)n_exp * s.n_tiles * B, -7.0);
  s.U.assign((size_t)n_exp * n_cols * B, -7.0), s.W.assign(n * n_cols * B, -7.0);
  s.ended.assign((size_t)kGrFlags * B, 0);
  // k_inject_grid, k_sysrem_prep
  for (int32_t b = 0; b < B; ++b)
    for (int32_t e = 0; e < n_exp; ++e)
      for (int32_t p = 0; p < n_pix; ++p)
        s.D[(size_t)gr_inject_to(b, e, p, n_exp, n_pix)] = sy_inject(
            raw[(size_t)ex_data(e, p, n_pix)], model[(size_t)gr_inject_model(e, b, p, B, n_pix)], scale[(size_t)b]);
  for (int32_t b = 0; b < B; ++b)
    for (int32_t e = 0; e < n_exp; ++e)
      for (int32_t p = 0; p < (int32_t)s.pitch; ++p) {
        double wv = 0.0, rv = 0.0;
        if (p < n_pix) {
          const double d = s.D[(size_t)(gr_data(b, n_exp, n_pix) + ex_data(e, p, n_pix))];
          wv = sy_weight(ivar[(size_t)ex_data(e, p, n_pix)], d);
          if (wv > 0.0) rv = d;
        }
        s.w[(size_t)(gr_work(b, n_exp, s.pitch) + sy_at(e, p, s.pitch))] = wv;
        s.r[(size_t)(gr_work(b, n_exp, s.pitch) + sy_at(e, p, s.pitch))] = rv;
      }
  // the launches of launch_sysrem, each over every injection before the next
  int32_t col = 0;
  if (ones) {
    for (int32_t b = 0; b < B; ++b) fill(s, b, col, 1.0);
    for (int32_t b = 0; b < B; ++b) step(s, b, col, true);
    ++col;
  }
  for (int32_t k = 0; k < n_comp; ++k, ++col) {
    for (int32_t b = 0; b < B; ++b) fill(s, b, col, sy_first_a(n_exp));
    for (int32_t it = 0; it < n_iter; ++it) {
      for (int32_t b = 0; b < B; ++b) step(s, b, col, false);
      for (int32_t b = 0; b < B; ++b) rows(s, b, col);
    }
    for (int32_t b = 0; b < B; ++b) step(s, b, col, true);
  }
  // k_sysrem_finish
  for (int32_t b = 0; b < B; ++b)
    for (int32_t e = 0; e < n_exp; ++e)
      for (int32_t p = 0; p < n_pix; ++p) {
        const size_t at = (size_t)(gr_work(b, n_exp, s.pitch) + sy_at(e, p, s.pitch));
        const size_t da = (size_t)(gr_data(b, n_exp, n_pix) + ex_data(e, p, n_pix));
        s.out[da] = s.w[at] > 0.0 ? s.r[at] : s.D[da];
      }
  // k_filter_weights, then the out-of-place k_detrend of every injection from the one model T
  std::vector<double> Tf(nt * B, -7.0);
  const std::vector<double> T0 = T;
  int ended_cols = 0;
  for (int32_t b = 0; b < B; ++b) {
    const double* U = s.U.data() + gr_u(b, n_exp, n_cols);
    double* W = s.W.data() + gr_w(b, n_cols, n_exp, n_pix);
    for (int32_t p = 0; p < n_pix; ++p) switch (n_cols) {
#define X(K)                                                                                                       \
  case K:                                                                                                          \
    weights_pixel<K>(U, ivar.data() + ex_data(0, p, n_pix), W + dt_w(0, 0, p, n_exp, n_pix), n_pix, n_exp);       \
    break;
        GRID_CASES(X)
#undef X
      }
    for (int32_t j = 0; j < n_trial; ++j)
      for (int32_t p = 0; p < n_pix; ++p) {
        const int64_t m0 = ex_model(0, j, p, n_trial, n_pix), m_stride = (int64_t)n_trial * n_pix;
        switch (n_cols) {
#define X(K)                                                                                                       \
  case K:                                                                                                          \
    detrend_column<K>(T.data() + m0, Tf.data() + nt * b + m0, m_stride, U, W + dt_w(0, 0, p, n_exp, n_pix), n_pix, \
                      n_exp);                                                                                      \
    break;
          GRID_CASES(X)
#undef X
        }
      }
    for (int32_t c = 0; c < n_cols; ++c) ended_cols += s.ended[(size_t)gr_flag(b, c)];
  }
  int bad = 0;
  for (size_t i = 0; i < s.U.size(); ++i) bad += !same_bits(s.U[i], want_U[i]);
  for (size_t i = 0; i < s.out.size(); ++i) bad += !same_bits(s.out[i], want_out[i]);
  for (size_t i = 0; i < s.W.size(); ++i) bad += !same_bits(s.W[i], want_W[i]);
  for (size_t i = 0; i < Tf.size(); ++i) bad += !same_bits(Tf[i], want_T[i]);
  for (size_t i = 0; i < T.size(); ++i) bad += !same_bits(T[i], T0[i]);
  std::printf("batch n_inj=%d n_exp=%d n_pix=%d n_cols=%d ended=%d mismatches=%d\n", B, n_exp, n_pix, n_cols, ended_cols,
              bad);
  return bad != 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return batch_case(argv[1]);
  const int32_t T = kSyTile;
  const int32_t injs[] = {1, 2, 5}, pix[] = {1, T - 1, T, T + 1, 3 * T + 5}, exps[] = {1, 2, 7}, cols[] = {1, 3, 16};
  int rc = 0, n_shapes = 0;
  for (int32_t B : injs)
    for (int32_t n_pix : pix)
      for (int32_t n_exp : exps) {
        const int32_t n_cols = cols[n_shapes % 3];
        ++n_shapes;
        int64_t cnt[C_COUNT];
        grid_audit(B, n_exp, n_pix, n_cols, cnt);
        std::printf("n_inj=%d n_exp=%d n_pix=%d n_cols=%d:", B, n_exp, n_pix, n_cols);
        for (int i = 0; i < C_COUNT; ++i) std::printf(" %s=%lld", kNames[i], (long long)cnt[i]);
        std::printf(" bytes=%lld/%lld\n", (long long)gr_injection_bytes(n_exp, n_pix, n_cols, 2, false),
                    (long long)gr_injection_bytes(n_exp, n_pix, n_cols, 2, true));
        for (int i = C_OOR; i < C_COUNT; ++i) rc |= cnt[i] != 0;
      }
  std::printf("shapes=%d tile=%d flags=%d\n", n_shapes, T, kGrFlags);
  return rc;
}
