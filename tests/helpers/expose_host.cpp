// Host harness of k_expose's index arithmetic (prometheus_amd/csrc/expose_index.h over vmap_index.h and
// obs_index.h): walks every batch, exposure, chunk, trial group, tile, tap, thread, pass and lane of an expose call
// with the headers' own functions, in the kernel's order, and counts every index that would fall outside the
// exposure table, R, the stage, the data, the model or the scratch.  Built by tests/test_expose_cpu.py as a
// stand-alone program with its own main (also with -fsanitize=address,undefined); with small constants
// (-DPROM_VM_TILE=.. -DPROM_VM_STAGE=.. -DPROM_VM_CHUNK=.. -DPROM_VM_TRIALS=..) the same walk crosses every edge
// on a small set.  It prints its counters and returns 1 when an index was out of range or a case was not met.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "expose_index.h"

using namespace prom;

enum { C_WORKGROUPS, C_BATCHES, C_LIVE_TAPS, C_DEAD_TAPS, C_POINTS, C_STAGED, C_FALLBACK, C_EMPTY, C_TABLE_OOR,
       C_R_OOR, C_STAGE_OOR, C_DATA_OOR, C_MODEL_OOR, C_PART_OOR, C_VISIT_ERR, C_COUNT };
static const char* kNames[C_COUNT] = {"workgroups", "batches", "live_taps", "dead_taps", "points", "staged",
                                      "fallback", "empty", "table_oor", "r_oor", "stage_oor", "data_oor",
                                      "model_oor", "part_oor", "visit_err"};

// rows and weights [n_exp][n_tap], F [n_exp][n_trial][n_tap]; cap_bytes: the scratch cap (the launcher's batching).
// The arrays are exactly as long as their shapes say, so a sanitizer sees an index past them.
static void ex_audit(const std::vector<double>& wav, const std::vector<double>& lam, const std::vector<double>& sig,
                     double k, int32_t n_orb, int32_t n_exp, int32_t n_trial, int32_t n_tap,
                     const std::vector<int32_t>& row, const std::vector<double>& wgt, const std::vector<double>& F,
                     int64_t cap_bytes, int64_t* cnt) {
  for (int i = 0; i < C_COUNT; ++i) cnt[i] = 0;
  const int32_t n_wav = (int32_t)wav.size(), n_pix = (int32_t)lam.size();
  const int64_t n_R = (int64_t)n_orb * n_wav, n_data = (int64_t)n_exp * n_pix;
  const int64_t n_model = (int64_t)n_exp * n_trial * n_pix, n_taps = (int64_t)n_exp * n_tap;
  const int64_t n_F = n_taps * n_trial;
  if ((int64_t)row.size() != n_taps || (int64_t)wgt.size() != n_taps || (int64_t)F.size() != n_F) ++cnt[C_TABLE_OOR];
  const int32_t n_chunks = vm_chunks(n_pix), n_groups = vm_groups(n_trial);
  const int32_t bg = vm_batch_groups(cap_bytes, n_exp, n_chunks, n_groups);
  if (bg < 1) ++cnt[C_PART_OOR];
  const int32_t nb_max = bg * kVmTrials < n_trial ? bg * kVmTrials : n_trial;
  const int64_t part_cap = vm_part_doubles(n_exp, nb_max, n_chunks);
  std::vector<int32_t> model_writes((size_t)n_model, 0);
  std::vector<char> written;
  for (int32_t g0 = 0; g0 < n_groups; g0 += bg) {
    ++cnt[C_BATCHES];
    const int32_t j_first = vm_group_first(g0);
    const int32_t nb = nb_max < n_trial - j_first ? nb_max : n_trial - j_first;
    if (nb < 1 || j_first + nb > n_trial) ++cnt[C_PART_OOR];
    written.assign((size_t)part_cap, 0);
    const int32_t grid_x = vm_groups(nb) * n_chunks;
    for (int32_t e = 0; e < n_exp; ++e)
      for (int32_t bx = 0; bx < grid_x; ++bx) {
        ++cnt[C_WORKGROUPS];
        const int32_t chunk = vm_wg_chunk(bx, n_chunks), gb = vm_wg_group(bx, n_chunks);
        const int32_t jb0 = vm_group_first(gb);
        const int32_t nt = nb - jb0 < kVmTrials ? nb - jb0 : kVmTrials;
        if (chunk < 0 || chunk >= n_chunks || nt < 1 || j_first + jb0 + nt > n_trial) ++cnt[C_PART_OOR];
        const int32_t tile0 = vm_chunk_first(chunk), ntile = vm_chunk_count(chunk, n_pix);
        if (ntile < 1) ++cnt[C_VISIT_ERR];
        for (int32_t ti = 0; ti < ntile; ++ti) {
          const int32_t p0 = vm_tile_first(tile0 + ti), np = vm_tile_count(tile0 + ti, n_pix);
          if (p0 < 0 || np < 1 || p0 + np > n_pix) ++cnt[C_VISIT_ERR];
          for (int32_t tap = 0; tap < n_tap; ++tap) {
            const int64_t at = ex_tap(e, tap, n_tap);
            if (at < 0 || at >= n_taps) {
              ++cnt[C_TABLE_OOR];
              continue;
            }
            if (!ex_live(wgt[(size_t)at])) {
              ++cnt[C_DEAD_TAPS];
              continue;   // nothing else of a dead tap is read: its row may be anything
            }
            ++cnt[C_LIVE_TAPS];
            const int32_t rw = row[(size_t)at];
            const int64_t r0 = ex_row_first(rw, n_wav);
            if (rw < 0 || rw >= n_orb || r0 < 0 || r0 + n_wav > n_R) {
              ++cnt[C_R_OOR];
              continue;
            }
            double sF[kVmTrials];
            for (int32_t r = 0; r < kVmTrials; ++r) {
              sF[r] = 1.0;
              if (r < nt) {
                const int64_t fa = ex_factor(e, j_first + jb0 + r, tap, n_trial, n_tap);
                if (fa < 0 || fa >= n_F) ++cnt[C_TABLE_OOR]; else sF[r] = F[(size_t)fa];
              }
            }
            int32_t rmin, rmax;
            vm_extremes(sF, nt, &rmin, &rmax);
            if (rmin < 0 || rmin >= nt || rmax < 0 || rmax >= nt) ++cnt[C_TABLE_OOR];
            double sX[4][kVmTile];
            int32_t sI[4][kVmTile];
            for (int32_t which = 0; which < 4; ++which)
              for (int32_t tt = 0; tt < kVmTile; ++tt) {
                sX[which][tt] = 0.0;
                sI[which][tt] = 0;
                if (tt < np) {
                  const ObsPix px = obs_pixel(lam[p0 + tt], sig[p0 + tt], k, sF[which < 2 ? rmin : rmax]);
                  sX[which][tt] = obs_target(px, which & 1);
                  sI[which][tt] = obs_bound(wav.data(), n_wav, sX[which][tt], which & 1);
                }
              }
            int32_t sA[kVmTile * kVmTrials], sB[kVmTile * kVmTrials];
            bool any = false;
            int32_t a_min = INT32_MAX, b_max = 0;
            for (int32_t tid = 0; tid < kVmTile * kVmTrials; ++tid) {
              const int32_t r = vm_entry_trial(tid), t = vm_entry_pixel(tid);
              int32_t a = 0, b = 0;
              if (r < nt && t < np) {
                const ObsPix px = obs_pixel(lam[p0 + t], sig[p0 + t], k, sF[r]);
                a = vm_bound(wav.data(), n_wav, obs_target(px, false), false, sX[0][t], sX[2][t], sI[0][t], sI[2][t]);
                b = vm_bound(wav.data(), n_wav, obs_target(px, true), true, sX[1][t], sX[3][t], sI[1][t], sI[3][t]);
                obs_trim(wav.data(), n_wav, px.L, px.c, &a, &b);
                if (a < 0 || b < a || b > n_wav) ++cnt[C_R_OOR];
              }
              sA[tid] = a;
              sB[tid] = b;
              const int32_t va = vm_vote_a(a, b, kVmStage), vb = vm_vote_b(a, b, kVmStage);
              if (va != INT32_MAX) any = true;
              a_min = va < a_min ? va : a_min;
              b_max = vb > b_max ? vb : b_max;
            }
            int32_t s0, s1;
            vm_stage(any, a_min, b_max, kVmStage, &s0, &s1);
            const int32_t ns = s1 - s0;
            if (ns < 0 || ns > kVmStage || s0 < 0 || s1 > n_wav) ++cnt[C_STAGE_OOR];
            for (int32_t i = 0; i < ns; ++i)   // wav, q and the tap's row of R at s0 + i
              if (s0 + i < 0 || s0 + i >= n_wav || r0 + s0 + i < 0 || r0 + s0 + i >= n_R) ++cnt[C_STAGE_OOR];
            for (int32_t en = 0; en < nt * kVmTile; ++en) {
              const int32_t a = sA[en], b = sB[en];
              const bool staged = obs_staged(a, b, s0, s1);
              if (vm_entry_pixel(en) < np) {
                if (a == b) ++cnt[C_EMPTY]; else if (staged) ++cnt[C_STAGED]; else ++cnt[C_FALLBACK];
              } else if (a != b) {
                ++cnt[C_VISIT_ERR];
              }
              int64_t pts = 0;
              for (int32_t it = 0; it < vm_passes(a, b); ++it)
                for (int32_t l = 0; l < kVmLanes; ++l) {
                  const int32_t w = vm_point(a, it, l);
                  if (w >= b) continue;
                  ++pts;
                  if (staged) {
                    const int32_t i = w - s0;
                    if (i < 0 || i >= ns || i >= kVmStage) ++cnt[C_STAGE_OOR];
                  } else if (w < 0 || w >= n_wav || r0 + w < 0 || r0 + w >= n_R) {
                    ++cnt[C_R_OOR];
                  }
                }
              if (pts != b - a) ++cnt[C_R_OOR];   // every point of the support exactly once
              cnt[C_POINTS] += pts;
            }
          }
          // step 4: the exposure's data, and the model value of every live (trial, pixel)
          for (int32_t tid = 0; tid < kVmTile * kVmTrials; ++tid) {
            const int32_t r = vm_entry_trial(tid), t = vm_entry_pixel(tid);
            if (!(r < nt && t < np)) continue;
            const int64_t da = ex_data(e, p0 + t, n_pix);
            if (da < 0 || da >= n_data) ++cnt[C_DATA_OOR];
            const int64_t ma = ex_model(e, j_first + jb0 + r, p0 + t, n_trial, n_pix);
            if (ma < 0 || ma >= n_model) ++cnt[C_MODEL_OOR]; else ++model_writes[(size_t)ma];
          }
        }
        for (int32_t r = 0; r < nt; ++r) {
          const int64_t slot = vm_part_slot(e, jb0 + r, chunk, nb, n_chunks);
          if (slot < 0 || slot + kVmRecord > part_cap || slot + kVmRecord > vm_part_doubles(n_exp, nb, n_chunks) ||
              written[(size_t)slot])
            ++cnt[C_PART_OOR];
          else
            written[(size_t)slot] = 1;
        }
      }
    // the reduction (k_vmap_reduce with n_exp for n_orb) reads every record of the batch: each must have been written
    for (int32_t e = 0; e < n_exp; ++e)
      for (int32_t jb = 0; jb < nb; ++jb)
        for (int32_t ch = 0; ch < n_chunks; ++ch) {
          const int64_t slot = vm_part_slot(e, jb, ch, nb, n_chunks);
          if (slot < 0 || slot + kVmRecord > part_cap || !written[(size_t)slot]) ++cnt[C_PART_OOR];
        }
  }
  for (int32_t v : model_writes)
    if (v != 1) ++cnt[C_VISIT_ERR];   // every (exposure, trial, pixel) exactly once
}

// a coarse / fine grid with duplicates, pixels beyond both ends, a tiny and a huge width; 5 exposures over 3 rows with
// 6 taps (some dead, at the head, inside and at the tail; one exposure all dead; a dead tap whose row is out of
// range, which nothing may read), trial groups a few km/s wide with a +-300 km/s tap; the whole table at once and
// in batches of one group
int main() {
  std::vector<double> wav;
  double x = 5880e-8;
  for (int i = 0; i < 4000; ++i) {
    wav.push_back(x);
    x += (i % 29 == 0) ? 0.0 : ((i / 700) % 2 ? 1e-11 : 2e-10);
  }
  const int32_t n_pix = kVmChunk * kVmTile + kVmTile + 1, n_orb = 3, n_exp = 5, n_trial = 2 * kVmTrials + 3, n_tap = 6;
  std::vector<double> lam(n_pix), sig(n_pix), wgt((size_t)n_exp * n_tap), F((size_t)n_exp * n_trial * n_tap);
  std::vector<int32_t> row((size_t)n_exp * n_tap);
  for (int32_t p = 0; p < n_pix; ++p) {
    lam[p] = wav.front() - 1e-8 + (wav.back() - wav.front() + 2e-8) * p / (n_pix - 1);
    sig[p] = p % 97 == 5 ? 1e-3 : (p % 89 == 7 ? 1e-13 : lam[p] / (140000.0 * 2.3548200450309493));
  }
  for (int32_t e = 0; e < n_exp; ++e)
    for (int32_t i = 0; i < n_tap; ++i) {
      const bool dead = e == 3 || (e == 0 && i < 2) || (e == 1 && i % 2) || (e == 2 && i >= 4);
      wgt[(size_t)e * n_tap + i] = dead ? 0.0 : 1.0 / n_tap;
      row[(size_t)e * n_tap + i] = dead && i == 1 ? 1 << 30 : (e + i) % n_orb;
      for (int32_t j = 0; j < n_trial; ++j) {
        double v = (j - 9) * 2.0e5 + (i - 2) * 1.0e5 + (e - 2) * 8.0e5;   // cm/s
        if (j % kVmTrials == 5 && i == 3) v = (j & kVmTrials) ? 3.0e7 : -3.0e7;
        F[((size_t)e * n_trial + j) * n_tap + i] = std::sqrt((1.0 - v / 2.99792458e10) / (1.0 + v / 2.99792458e10));
      }
    }
  int64_t cnt[C_COUNT];
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    ex_audit(wav, lam, sig, 5.0, n_orb, n_exp, n_trial, n_tap, row, wgt, F, pass ? 1 : (int64_t)256 << 20, cnt);
    std::printf("pass %d:", pass);
    for (int i = 0; i < C_COUNT; ++i) std::printf(" %s=%lld", kNames[i], (long long)cnt[i]);
    std::printf("\n");
    for (int i = C_TABLE_OOR; i < C_COUNT; ++i) bad += cnt[i] != 0;
    bad += !(cnt[C_STAGED] && cnt[C_FALLBACK] && cnt[C_EMPTY] && cnt[C_LIVE_TAPS] && cnt[C_DEAD_TAPS]);
    bad += cnt[C_BATCHES] != (pass ? 3 : 1);
  }
  return bad ? 1 : 0;
}
