// Host harness of the target-window planner, for CPU tests only (tests/test_window_plan_cpu.py).
//
// Linked with prometheus_amd/csrc/prom_window.hip compiled as C++ (pure host code): tw_plan runs
// build_target_windows and hands back the raw plan; the tw_* exports are tw_index.h's functions, the very text
// k_sigma_tw compiles; tw_audit walks a plan the way the kernel does (every window, wave, dispatched row or pair,
// chunk and lane of the first pass, every item of the second) with those functions and counts every index that
// would leave its array, and how often each (row, wavelength) is stored.
//
// old_rule (a test-only argument): the pair dispatch as it was before empty rows counted as absent -- a row without
// wavelengths in the window still ran beside a live partner -- so the test can show that the audit sees the
// out-of-range reads that rule produced.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "prom_internal.h"
#include "tw_index.h"

namespace {

struct Plan {
  std::vector<prom::SigSeg> seg;
  std::vector<int32_t> row, lam;
  int32_t n_win = 0;
};

enum {
  A_LANES = 0,        // lanes that read a wavelength (computed or prefetched)
  A_GLOBAL_OOR,       // global wavelength index outside [0, n_wav)
  A_STAGED_OOR,       // staged offset outside [0, (lw1 - lw0) + 64)
  A_PADDING,          // staged offset inside the 64 entries of padding (never stored from)
  A_GUESS_OOR,        // guess outside [0, m - 2]
  A_STEP_OOR,         // one-node correction outside the staged x's
  A_BRACKET_BAD,      // a storing lane whose corrected guess is not numpy's bracket (kind 1)
  A_WIN_FIRST,        // first-pass windows
  A_WIN_SECOND,       // second-pass windows
  A_PAIR_EMPTY_LOW,   // first-pass windows with an empty row beside a live partner, the empty row at w1 == 0
  A_PAIR_EMPTY_HIGH,  // ... at w0 == n_wav
  A_PAIR_EMPTY_MID,   // ... in the interior
  A_PAIR_EMPTY_WIN,   // first-pass windows with any such pair
  A_WIN_GLOBAL_OOR,   // windows with a global index out of range
  A_WIN_STAGED_OOR,   // windows with a staged offset out of range
  A_N
};

struct Audit {
  const double* wav;
  int64_t n_wav;
  const double* shift;
  int32_t n_rows, ns;
  const double* const* X;
  const int64_t* nx;
  const uint8_t* rare;
  uint8_t* stored;
  int64_t* cnt;
  // the window
  const prom::SigSeg* sg;
  const int32_t *wa, *wz;
  int32_t lw0, nlam;
  bool g_oor, s_oor;

  // one lane's read: the wavelength index it forms and, when that is in range, the lookups of the wavelength read
  void lane_read(int32_t o, int32_t w0, int32_t w1, int32_t k, int32_t lane, bool computed) {
    cnt[A_LANES] += 1;
    double lamv;
    if (nlam > 0) {
      const int32_t off = prom::tw_lam_staged(w0, w1, k, lane, lw0);
      if (off < 0 || off >= nlam + 64) {
        cnt[A_STAGED_OOR] += 1;
        s_oor = true;
        return;
      }
      if (off >= nlam) {   // (padding: no defined wavelength; the lane is past its row's end)
        cnt[A_PADDING] += 1;
        if (computed && prom::tw_chunk_first(w0, k) + lane < w1) cnt[A_STAGED_OOR] += 1;   // (a storing lane never)
        return;
      }
      lamv = wav[lw0 + off];
    } else {
      const int32_t w = prom::tw_lam_global(w0, w1, k, lane);
      if (w < 0 || w >= n_wav) {
        cnt[A_GLOBAL_OOR] += 1;
        g_oor = true;
        return;
      }
      lamv = wav[w];
    }
    if (!computed) return;
    const int32_t c0 = prom::tw_chunk_first(w0, k);
    const bool stores = c0 + lane < w1;
    const double t = shift[o] * lamv;
    for (int s = 0; s < ns; ++s) {
      const prom::SigSeg& e = sg[s];
      const int32_t g = prom::tw_guess(t, e.inv, e.xs, e.m);
      if (g < 0 || g > e.m - 2) {
        cnt[A_GUESS_OOR] += 1;
        continue;
      }
      if ((e.kind & 3) != 1) continue;   // (kind 3: bisection over the staged slice)
      const double* x = X[s] + e.lo;     // x[0 .. m - 1] staged, x[m] the last upper node
      const bool lo = t < x[g], hi = t >= x[g + 1];
      int32_t kf = g;
      if (lo | hi) {
        kf = lo ? g - 1 : g + 1;
        if (kf < 0 || kf > e.m - 1) {
          cnt[A_STEP_OOR] += 1;
          continue;
        }
      }
      if (stores && !(kf <= e.m - 2 && x[kf] <= t && t < x[kf + 1])) cnt[A_BRACKET_BAD] += 1;
    }
    if (stores) stored[(int64_t)o * n_wav + c0 + lane] += 1;
  }

  // k_sigma_tw's rows(): the NP rows' chunks k = k0, k0 + G, ...
  void rows(const int32_t* os, int np, int32_t k0, int32_t G) {
    int32_t nch = 0;
    for (int p = 0; p < np; ++p) nch = std::max(nch, prom::tw_chunks(wa[os[p]], wz[os[p]]));
    if (nlam > 0) {
      for (int32_t k = k0; k < nch; k += G)
        for (int p = 0; p < np; ++p)
          for (int32_t lane = 0; lane < 64; ++lane) lane_read(os[p], wa[os[p]], wz[os[p]], k, lane, true);
    } else {
      const int B = 4 / np;   // (chunks loaded at a time before any is computed)
      for (int32_t k = k0; k < nch; k += B * G)
        for (int j = 0; j < B; ++j)
          for (int p = 0; p < np; ++p)
            for (int32_t lane = 0; lane < 64; ++lane)
              lane_read(os[p], wa[os[p]], wz[os[p]], k + j * G, lane, k + j * G < nch);
    }
  }

  bool rare_row(int32_t o) const { return rare && rare[o]; }

  void first_pass(int rp, bool old_rule) {
    for (int32_t wv = 0; wv < 4; ++wv) {
      if (rp == 1) {
        const int32_t G = prom::tw_waves_per_unit(n_rows);
        for (int32_t o = wv / G; o < n_rows; o += 4 / G) {
          if (rare_row(o)) continue;
          rows(&o, 1, wv % G, G);
        }
      } else {
        const int32_t P = (n_rows + 1) >> 1;
        const int32_t G = prom::tw_waves_per_unit(P);
        for (int32_t q = wv / G; q < P; q += 4 / G) {
          const int32_t oa = 2 * q, ob = 2 * q + 1;
          bool ra, rb;
          if (old_rule) {
            ra = rare_row(oa);
            rb = ob >= n_rows || rare_row(ob);
          } else {
            ra = prom::tw_row_absent(rare_row(oa), wa[oa], wz[oa]);
            rb = ob >= n_rows || prom::tw_row_absent(rare_row(ob), wa[ob], wz[ob]);
          }
          const int32_t pr = prom::tw_pair_rows(ra, rb);
          if (pr == 3) {
            const int32_t os[2] = {oa, ob};
            rows(os, 2, wv % G, G);
          } else if (pr != 0) {
            const int32_t o = pr == 1 ? oa : ob;
            rows(&o, 1, wv % G, G);
          }
        }
      }
    }
  }

  // k_sigma_tw's second pass: items (row, chunk) of the rows it takes, to the waves round robin
  void second_pass(bool wrare) {
    for (int32_t wv = 0; wv < 4; ++wv) {
      int32_t o = 0, c = wv;
      for (;;) {
        int32_t w0 = 0, w1 = 0;
        while (o < n_rows) {
          if (wrare || rare_row(o)) {
            w0 = wa[o];
            w1 = wz[o];
            const int32_t nch = (w1 - w0 + 63) >> 6;
            if (c < nch) break;
            c -= nch;
          }
          ++o;
        }
        if (o >= n_rows) break;
        for (int32_t lane = 0; lane < 64; ++lane) {
          const int32_t w = w0 + c * 64 + lane;
          const bool live = w < w1;
          const int32_t r = live ? w : w1 - 1;
          cnt[A_LANES] += 1;
          if (r < 0 || r >= n_wav) {
            cnt[A_GLOBAL_OOR] += 1;
            g_oor = true;
          }
          if (live) stored[(int64_t)o * n_wav + w] += 1;
        }
        c += 4;
      }
    }
  }
};

}  // namespace

extern "C" {

// the plan of build_target_windows; null when the planner declines the inputs
void* tw_plan(const double* wav, int64_t n_wav, const double* shift, int32_t n_rows, int32_t ns,
              const double* const* X, const int64_t* nx, int32_t lds, int32_t lamcap, int32_t rowcap, int64_t pmax,
              int32_t* n_win) {
  std::vector<std::vector<double>> tabs(ns);
  std::vector<const std::vector<double>*> tp(ns);
  for (int s = 0; s < ns; ++s) {
    tabs[s].assign(X[s], X[s] + nx[s]);
    tp[s] = &tabs[s];
  }
  Plan* p = new Plan;
  if (!prom::build_target_windows(wav, n_wav, shift, n_rows, tp, lds, lamcap, rowcap, pmax, p->seg, p->row, p->lam,
                                  p->n_win)) {
    delete p;
    *n_win = 0;
    return nullptr;
  }
  *n_win = p->n_win;
  return p;
}

// seg: n_win x ns SigSeg; row: (n_win + 1) x n_rows starts (the last the terminal row); lam: n_win x {lw0, lw1}
void tw_plan_copy(const void* h, void* seg, int32_t* row, int32_t* lam) {
  const Plan* p = static_cast<const Plan*>(h);
  std::memcpy(seg, p->seg.data(), p->seg.size() * sizeof(prom::SigSeg));
  std::memcpy(row, p->row.data(), p->row.size() * sizeof(int32_t));
  std::memcpy(lam, p->lam.data(), p->lam.size() * sizeof(int32_t));
}

void tw_plan_free(void* h) { delete static_cast<Plan*>(h); }

int32_t tw_sizeof_seg() { return (int32_t)sizeof(prom::SigSeg); }

// tw_index.h, elementwise
void tw_guess_n(int64_t n, const double* t, const double* inv, const double* xs, const int32_t* m, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = prom::tw_guess(t[i], inv[i], xs[i], m[i]);
}
int32_t tw_waves_per_unit(int32_t n) { return prom::tw_waves_per_unit(n); }
int32_t tw_pair_rows(int32_t absent_a, int32_t absent_b) { return prom::tw_pair_rows(absent_a != 0, absent_b != 0); }
int32_t tw_row_absent(int32_t past_or_rare, int32_t w0, int32_t w1) {
  return prom::tw_row_absent(past_or_rare != 0, w0, w1) ? 1 : 0;
}
int32_t tw_chunks(int32_t w0, int32_t w1) { return prom::tw_chunks(w0, w1); }
int32_t tw_chunk_read(int32_t w0, int32_t w1, int32_t k) { return prom::tw_chunk_read(w0, w1, k); }
int32_t tw_lam_staged(int32_t w0, int32_t w1, int32_t k, int32_t lane, int32_t lw0) {
  return prom::tw_lam_staged(w0, w1, k, lane, lw0);
}
int32_t tw_lam_global(int32_t w0, int32_t w1, int32_t k, int32_t lane) {
  return prom::tw_lam_global(w0, w1, k, lane);
}

// walk the plan as k_sigma_tw<.., RP = rp> does; stored[n_rows x n_wav] counts the stores of every (row, wavelength)
// (zeroed by the caller), cnt[A_N] the counters above; rare[n_rows] (or null): rows the second pass takes
int32_t tw_audit_counters() { return A_N; }
void tw_audit(const double* wav, int64_t n_wav, const double* shift, int32_t n_rows, int32_t ns,
              const double* const* X, const int64_t* nx, const void* seg, const int32_t* row, const int32_t* lam,
              int32_t n_win, int32_t rp, int32_t old_rule, const uint8_t* rare, uint8_t* stored, int64_t* cnt) {
  Audit a;
  a.wav = wav; a.n_wav = n_wav; a.shift = shift; a.n_rows = n_rows; a.ns = ns; a.X = X; a.nx = nx;
  a.rare = rare; a.stored = stored; a.cnt = cnt;
  for (int i = 0; i < A_N; ++i) cnt[i] = 0;
  for (int32_t b = 0; b < n_win; ++b) {
    a.sg = static_cast<const prom::SigSeg*>(seg) + (int64_t)b * ns;
    a.wa = row + (int64_t)b * n_rows;
    a.wz = a.wa + n_rows;
    a.lw0 = lam[2 * b];
    a.nlam = lam[2 * b + 1] - a.lw0;
    a.g_oor = a.s_oor = false;
    bool wrare = false;
    for (int s = 0; s < ns; ++s) wrare = wrare || ((a.sg[s].kind & 3) != 1 && (a.sg[s].kind & 3) != 3);
    if (!wrare) {
      cnt[A_WIN_FIRST] += 1;
      // (a property of the plan, whatever the rule: pairs of rows neither in the second pass, one empty, one live)
      bool any = false;
      for (int32_t q = 0; 2 * q + 1 < n_rows; ++q) {
        const int32_t oa = 2 * q, ob = 2 * q + 1;
        if (a.rare_row(oa) || a.rare_row(ob)) continue;
        const bool ea = a.wa[oa] >= a.wz[oa], eb = a.wa[ob] >= a.wz[ob];
        if (ea == eb) continue;
        const int32_t oe = ea ? oa : ob;
        any = true;
        if (a.wz[oe] == 0) cnt[A_PAIR_EMPTY_LOW] += 1;
        else if (a.wa[oe] == n_wav) cnt[A_PAIR_EMPTY_HIGH] += 1;
        else cnt[A_PAIR_EMPTY_MID] += 1;
      }
      if (any) cnt[A_PAIR_EMPTY_WIN] += 1;
      a.first_pass(rp, old_rule != 0);
    } else {
      cnt[A_WIN_SECOND] += 1;
    }
    a.second_pass(wrare);
    if (a.g_oor) cnt[A_WIN_GLOBAL_OOR] += 1;
    if (a.s_oor) cnt[A_WIN_STAGED_OOR] += 1;
  }
}

}  // extern "C"

#ifdef WINDOW_HOST_MAIN
// stand-alone run (sanitizer builds): plans and audits the problems of a file written by the test module's
// dump_inputs(): int64 {n_wav, n_rows, ns, lds, lamcap, rowcap, pmax, nx[ns]}, then wav, shift and the tables
int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    FILE* f = std::fopen(argv[i], "rb");
    if (!f) return 2;
    int64_t h[7];
    if (std::fread(h, sizeof(int64_t), 7, f) != 7) return 2;
    const int64_t n_wav = h[0];
    const int32_t n_rows = (int32_t)h[1], ns = (int32_t)h[2];
    std::vector<int64_t> nx(ns);
    if (std::fread(nx.data(), sizeof(int64_t), ns, f) != (size_t)ns) return 2;
    std::vector<double> wav(n_wav), shift(n_rows);
    if (std::fread(wav.data(), 8, n_wav, f) != (size_t)n_wav) return 2;
    if (std::fread(shift.data(), 8, n_rows, f) != (size_t)n_rows) return 2;
    std::vector<std::vector<double>> X(ns);
    std::vector<const double*> Xp(ns);
    for (int s = 0; s < ns; ++s) {
      X[s].resize(nx[s]);
      if (std::fread(X[s].data(), 8, nx[s], f) != (size_t)nx[s]) return 2;
      Xp[s] = X[s].data();
    }
    std::fclose(f);
    int32_t nw = 0;
    void* p = tw_plan(wav.data(), n_wav, shift.data(), n_rows, ns, Xp.data(), nx.data(), (int32_t)h[3], (int32_t)h[4],
                      (int32_t)h[5], h[6], &nw);
    if (!p) return 3;
    const Plan* pl = static_cast<const Plan*>(p);
    for (int rp = 1; rp <= 2; ++rp) {
      std::vector<uint8_t> stored((size_t)n_rows * n_wav, 0);
      int64_t cnt[A_N];
      tw_audit(wav.data(), n_wav, shift.data(), n_rows, ns, Xp.data(), nx.data(), pl->seg.data(), pl->row.data(),
               pl->lam.data(), nw, rp, 0, nullptr, stored.data(), cnt);
      int64_t bad = 0;
      for (uint8_t v : stored) bad += v != 1;
      std::printf("%s: %d windows, RP %d, lanes %lld, out of range %lld global %lld staged, guess %lld, step %lld, "
                  "bracket %lld, points not stored once %lld\n", argv[i], nw, rp, (long long)cnt[A_LANES],
                  (long long)cnt[A_GLOBAL_OOR], (long long)cnt[A_STAGED_OOR], (long long)cnt[A_GUESS_OOR],
                  (long long)cnt[A_STEP_OOR], (long long)cnt[A_BRACKET_BAD], (long long)bad);
    }
    tw_plan_free(p);
  }
  return 0;
}
#endif
