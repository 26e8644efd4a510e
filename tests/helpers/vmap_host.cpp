// Host harness of k_vmap's index arithmetic (prometheus_amd/csrc/vmap_index.h over obs_index.h): walks every batch,
// phase, chunk, tile, trial group, pixel, trial, pass and lane of a map with the headers' own functions, in the
// kernel's order, and counts every index that would fall outside the stage, the arrays or the scratch.  Built by
// tests/helpers/vmap_plan.py as a shared library (ctypes), with the real constants or with small ones
// (-DPROM_VM_TILE=.. -DPROM_VM_STAGE=.. -DPROM_VM_CHUNK=.. -DPROM_VM_TRIALS=..), or with -DVMAP_HOST_MAIN as a
// stand-alone program (for a run under -fsanitize=address,undefined).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vmap_index.h"

using namespace prom;

enum { C_LANES, C_POINTS, C_STAGED, C_FALLBACK, C_EMPTY, C_STAGED_OOR, C_GLOBAL_OOR, C_STAGE_LOAD_OOR, C_PART_OOR,
       C_VISIT_ERR, C_STAGE_MAX, C_WORKGROUPS, C_BATCHES, C_STAGE_VALUES, C_FALLBACK_VALUES, C_FULL_SEARCHES,
       C_BRACKET_SEARCHES, C_BRACKET_WIDTH, C_COUNT };

extern "C" {

int32_t vm_audit_counters() { return C_COUNT; }
int32_t vm_const(int32_t which) {
  return which == 0 ? kVmTile : which == 1 ? kVmStage : which == 2 ? kVmChunk : which == 3 ? kVmTrials : kVmLanes;
}

// F[n_orb][n_trial]; cap_bytes: the scratch cap (the launcher's batching); supp_out (may be null):
// [n_orb][n_trial][n_pix][2] the supports the walk found
void vm_audit(const double* wav, int32_t n_wav, const double* lam, const double* sig, double k, const double* F,
              int32_t n_pix, int32_t n_orb, int32_t n_trial, int64_t cap_bytes, int64_t* cnt, int32_t* supp_out) {
  for (int i = 0; i < C_COUNT; ++i) cnt[i] = 0;
  if (n_pix <= 0) return;
  const int32_t n_chunks = vm_chunks(n_pix), n_groups = vm_groups(n_trial);
  const int32_t bg = vm_batch_groups(cap_bytes, n_orb, n_chunks, n_groups);
  if (bg < 1) ++cnt[C_PART_OOR];
  const int32_t nb_max = bg * kVmTrials < n_trial ? bg * kVmTrials : n_trial;
  const int64_t part_cap = vm_part_doubles(n_orb, nb_max, n_chunks);
  std::vector<int32_t> visits((size_t)n_orb * n_trial * n_pix, 0);
  std::vector<char> written;
  for (int32_t g0 = 0; g0 < n_groups; g0 += bg) {
    ++cnt[C_BATCHES];
    const int32_t j_first = vm_group_first(g0);
    const int32_t nb = nb_max < n_trial - j_first ? nb_max : n_trial - j_first;
    if (nb < 1 || j_first + nb > n_trial) ++cnt[C_PART_OOR];
    written.assign((size_t)part_cap, 0);
    const int32_t grid_x = vm_groups(nb) * n_chunks;
    for (int32_t o = 0; o < n_orb; ++o)
      for (int32_t bx = 0; bx < grid_x; ++bx) {
        ++cnt[C_WORKGROUPS];
        const int32_t chunk = vm_wg_chunk(bx, n_chunks), gb = vm_wg_group(bx, n_chunks);
        const int32_t jb0 = vm_group_first(gb);
        const int32_t nt = nb - jb0 < kVmTrials ? nb - jb0 : kVmTrials;
        if (chunk < 0 || chunk >= n_chunks || nt < 1 || j_first + jb0 + nt > n_trial) ++cnt[C_PART_OOR];
        double sF[kVmTrials];
        for (int32_t r = 0; r < kVmTrials; ++r) sF[r] = r < nt ? F[(int64_t)o * n_trial + j_first + jb0 + r] : 1.0;
        int32_t rmin, rmax;
        vm_extremes(sF, nt, &rmin, &rmax);
        if (rmin < 0 || rmin >= nt || rmax < 0 || rmax >= nt) ++cnt[C_PART_OOR];
        const int32_t tile0 = vm_chunk_first(chunk), ntile = vm_chunk_count(chunk, n_pix);
        if (ntile < 1) ++cnt[C_VISIT_ERR];
        for (int32_t ti = 0; ti < ntile; ++ti) {
          const int32_t p0 = vm_tile_first(tile0 + ti), np = vm_tile_count(tile0 + ti, n_pix);
          if (p0 < 0 || np < 1 || p0 + np > n_pix) ++cnt[C_VISIT_ERR];
          double sX[4][kVmTile];
          int32_t sI[4][kVmTile];
          for (int32_t which = 0; which < 4; ++which)
            for (int32_t tt = 0; tt < kVmTile; ++tt) {
              sX[which][tt] = 0.0;
              sI[which][tt] = 0;
              if (tt < np) {
                const ObsPix px = obs_pixel(lam[p0 + tt], sig[p0 + tt], k, sF[which < 2 ? rmin : rmax]);
                sX[which][tt] = obs_target(px, which & 1);
                sI[which][tt] = obs_bound(wav, n_wav, sX[which][tt], which & 1);
              }
            }
          int32_t sA[kVmTile * kVmTrials], sB[kVmTile * kVmTrials];
          bool any = false;
          int32_t a_min = INT32_MAX, b_max = 0;
          for (int32_t r = 0; r < kVmTrials; ++r)
            for (int32_t t = 0; t < kVmTile; ++t) {
              const int32_t e = vm_entry(r, t);
              if (vm_entry_trial(e) != r || vm_entry_pixel(e) != t) ++cnt[C_VISIT_ERR];
              int32_t a = 0, b = 0;
              if (r < nt && t < np) {
                const ObsPix px = obs_pixel(lam[p0 + t], sig[p0 + t], k, sF[r]);
                for (int end = 0; end < 2; ++end) {
                  const double x = obs_target(px, end);
                  const double x_lo = sX[end][t], x_hi = sX[2 + end][t];
                  const int32_t i_lo = sI[end][t], i_hi = sI[2 + end][t];
                  const bool inside = x_lo <= x && x <= x_hi && 0 <= i_lo && i_lo <= i_hi && i_hi <= n_wav;
                  if (inside) {
                    ++cnt[C_BRACKET_SEARCHES];
                    cnt[C_BRACKET_WIDTH] += i_hi - i_lo;
                  } else {
                    ++cnt[C_FULL_SEARCHES];
                  }
                  const int32_t v = vm_bound(wav, n_wav, x, end, x_lo, x_hi, i_lo, i_hi);
                  if (v != obs_bound(wav, n_wav, x, end)) ++cnt[C_GLOBAL_OOR];   // the bracket changes no answer
                  (end ? b : a) = v;
                }
                obs_trim(wav, n_wav, px.L, px.c, &a, &b);
                if (a < 0 || b < a || b > n_wav) ++cnt[C_GLOBAL_OOR];
                if (supp_out) {
                  const int64_t at = (((int64_t)o * n_trial + j_first + jb0 + r) * n_pix + p0 + t) * 2;
                  supp_out[at] = a;
                  supp_out[at + 1] = b;
                }
              }
              sA[e] = a;
              sB[e] = b;
              const int32_t va = vm_vote_a(a, b, kVmStage), vb = vm_vote_b(a, b, kVmStage);
              if (va != INT32_MAX) any = true;
              a_min = va < a_min ? va : a_min;
              b_max = vb > b_max ? vb : b_max;
            }
          int32_t s0, s1;
          vm_stage(any, a_min, b_max, kVmStage, &s0, &s1);
          const int32_t ns = s1 - s0;
          if (ns < 0 || ns > kVmStage || s0 < 0 || s1 > n_wav) ++cnt[C_STAGE_LOAD_OOR];
          if (ns > cnt[C_STAGE_MAX]) cnt[C_STAGE_MAX] = ns;
          cnt[C_STAGE_VALUES] += 3 * (int64_t)ns;   // wav, q and one row of R, once for all trials of the group
          for (int32_t tid = 0; tid < kVmBlock; ++tid)
            for (int32_t i = tid; i < ns; i += kVmBlock)
              if (i < 0 || i >= kVmStage || s0 + i < 0 || s0 + i >= n_wav) ++cnt[C_STAGE_LOAD_OOR];
          for (int32_t e = 0; e < nt * kVmTile; ++e) {
            const int32_t r = vm_entry_trial(e), t = vm_entry_pixel(e);
            const int32_t a = sA[e], b = sB[e];
            const bool staged = obs_staged(a, b, s0, s1);
            if (t < np) {
              if (a == b) ++cnt[C_EMPTY]; else if (staged) ++cnt[C_STAGED]; else ++cnt[C_FALLBACK];
              const int64_t at = ((int64_t)o * n_trial + j_first + jb0 + r) * n_pix + p0 + t;
              if (at < 0 || at >= (int64_t)visits.size()) ++cnt[C_VISIT_ERR]; else ++visits[(size_t)at];
            } else if (a != b) {
              ++cnt[C_VISIT_ERR];
            }
            int64_t pts = 0;
            for (int32_t it = 0; it < vm_passes(a, b); ++it)
              for (int32_t l = 0; l < kVmLanes; ++l) {
                ++cnt[C_LANES];
                const int32_t w = vm_point(a, it, l);
                if (w >= b) continue;
                ++pts;
                if (staged) {
                  const int32_t i = w - s0;
                  if (i < 0 || i >= ns || i >= kVmStage) ++cnt[C_STAGED_OOR];
                } else {
                  cnt[C_FALLBACK_VALUES] += 3;
                }
                if (w < a || w >= b || w < 0 || w >= n_wav) ++cnt[C_GLOBAL_OOR];
              }
            if (pts != b - a) ++cnt[C_GLOBAL_OOR];   // every point of the support exactly once
            cnt[C_POINTS] += pts;
          }
        }
        for (int32_t r = 0; r < nt; ++r) {
          const int64_t slot = vm_part_slot(o, jb0 + r, chunk, nb, n_chunks);
          if (slot < 0 || slot + kVmRecord > part_cap || slot + kVmRecord > vm_part_doubles(n_orb, nb, n_chunks) ||
              written[(size_t)slot])
            ++cnt[C_PART_OOR];
          else
            written[(size_t)slot] = 1;
        }
      }
    // the reduction reads every record of the batch: each must have been written
    for (int32_t o = 0; o < n_orb; ++o)
      for (int32_t jb = 0; jb < nb; ++jb)
        for (int32_t ch = 0; ch < n_chunks; ++ch) {
          const int64_t slot = vm_part_slot(o, jb, ch, nb, n_chunks);
          if (slot < 0 || slot + kVmRecord > part_cap || !written[(size_t)slot]) ++cnt[C_PART_OOR];
        }
  }
  for (int32_t v : visits)
    if (v != 1) ++cnt[C_VISIT_ERR];   // every (phase, trial, pixel) exactly once
}

}  // extern "C"

#ifdef VMAP_HOST_MAIN
// a coarse / fine grid with duplicates, pixels beyond both ends, a tiny and a huge width, trial groups a few km/s and
// +-300 km/s wide, the whole table at once and in batches of one group
int main() {
  std::vector<double> wav;
  double x = 5880e-8;
  for (int i = 0; i < 4000; ++i) {
    wav.push_back(x);
    x += (i % 29 == 0) ? 0.0 : ((i / 700) % 2 ? 1e-11 : 2e-10);
  }
  const int32_t n_wav = (int32_t)wav.size(), n_pix = 16 * 32 + 33, n_orb = 3, n_trial = 2 * 8 + 3;
  std::vector<double> lam(n_pix), sig(n_pix), F((size_t)n_orb * n_trial);
  for (int32_t p = 0; p < n_pix; ++p) {
    lam[p] = wav.front() - 1e-8 + (wav.back() - wav.front() + 2e-8) * p / (n_pix - 1);
    sig[p] = p % 97 == 5 ? 1e-3 : (p % 89 == 7 ? 1e-13 : lam[p] / (140000.0 * 2.3548200450309493));
  }
  for (int32_t o = 0; o < n_orb; ++o)
    for (int32_t j = 0; j < n_trial; ++j) {
      double v = (j - 9) * 2.0e5 + (o - 1) * 8.0e5;   // cm/s
      if (j % 8 == 5) v = (j & 8) ? 3.0e7 : -3.0e7;
      F[(size_t)o * n_trial + j] = std::sqrt((1.0 - v / 2.99792458e10) / (1.0 + v / 2.99792458e10));
    }
  int64_t cnt[C_COUNT];
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    vm_audit(wav.data(), n_wav, lam.data(), sig.data(), 5.0, F.data(), n_pix, n_orb, n_trial,
             pass ? 1 : (int64_t)256 << 20, cnt, nullptr);
    std::printf("pass %d:", pass);
    for (int i = 0; i < C_COUNT; ++i) std::printf(" %lld", (long long)cnt[i]);
    std::printf("\n");
    bad += cnt[C_STAGED_OOR] || cnt[C_GLOBAL_OOR] || cnt[C_STAGE_LOAD_OOR] || cnt[C_PART_OOR] || cnt[C_VISIT_ERR];
    bad += !(cnt[C_STAGED] && cnt[C_FALLBACK] && cnt[C_EMPTY]);
    bad += cnt[C_BATCHES] != (pass ? 3 : 1);
  }
  return bad ? 1 : 0;
}
#endif
