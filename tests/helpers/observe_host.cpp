// Host harness of k_observe's index arithmetic (prometheus_amd/csrc/obs_index.h): walks every workgroup, pixel,
// pass and lane of a launch with the header's own functions, in the kernel's order, and counts every index that
// would fall outside the stage or the arrays.  Built by tests/test_observe_cpu.py as a shared library (ctypes), or
// with -DOBSERVE_HOST_MAIN as a stand-alone program (for a run under -fsanitize=address,undefined).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "obs_index.h"

using namespace prom;

enum { C_LANES, C_POINTS, C_STAGED_PIX, C_FALLBACK_PIX, C_EMPTY_PIX, C_STAGED_OOR, C_GLOBAL_OOR, C_STAGE_LOAD_OOR,
       C_OUT_OOR, C_STAGE_MAX, C_WORKGROUPS, C_STAGE_POINTS, C_FALLBACK_POINTS, C_STAGE_VALUES, C_FALLBACK_VALUES, C_COUNT };

extern "C" {

int32_t obs_audit_counters() { return C_COUNT; }
int32_t obs_const(int32_t which) { return which == 0 ? kObsTile : which == 1 ? kObsStage : which == 2 ? kObsPhases : kObsBlock; }

// supp_out (may be null): [groups][n_pix][2] the supports the walk found
void obs_audit(const double* wav, int32_t n_wav, const double* lam, const double* sig, double k, const double* f,
               int32_t n_pix, int32_t n_orb, int64_t* cnt, int32_t* supp_out) {
  for (int i = 0; i < C_COUNT; ++i) cnt[i] = 0;
  const int32_t group = f ? 1 : kObsPhases;
  const int32_t n_groups = (n_orb + group - 1) / group;
  std::vector<char> touched((size_t)n_orb * (size_t)n_pix, 0);
  for (int32_t by = 0; by < n_groups; ++by)
    for (int32_t tile = 0; tile < obs_tiles(n_pix); ++tile) {
      ++cnt[C_WORKGROUPS];
      const int32_t o0 = by * group;
      const int32_t ng = n_orb - o0 < group ? n_orb - o0 : group;
      const int32_t p0 = obs_tile_first(tile), np = obs_tile_count(tile, n_pix);
      if (o0 < 0 || o0 >= n_orb || p0 < 0 || np < 1 || p0 + np > n_pix) ++cnt[C_OUT_OOR];
      const double fo = f ? f[o0] : 1.0;
      int32_t sA[kObsTile], sB[kObsTile];
      for (int32_t t = 0; t < kObsTile; ++t) {
        sA[t] = sB[t] = 0;
        if (t < np) {
          const ObsPix x = obs_pixel(lam[p0 + t], sig[p0 + t], k, fo);
          sA[t] = obs_bound(wav, n_wav, obs_target(x, false), false);
          sB[t] = obs_bound(wav, n_wav, obs_target(x, true), true);
          obs_trim(wav, n_wav, x.L, x.c, &sA[t], &sB[t]);
          if (sA[t] < 0 || sB[t] < sA[t] || sB[t] > n_wav) ++cnt[C_GLOBAL_OOR];
          if (supp_out) {
            supp_out[2 * ((int64_t)by * n_pix + p0 + t)] = sA[t];
            supp_out[2 * ((int64_t)by * n_pix + p0 + t) + 1] = sB[t];
          }
        }
      }
      int32_t s0, s1;
      obs_stage(sA, sB, np, kObsStage, &s0, &s1);
      const int32_t ns = s1 - s0;
      if (ns < 0 || ns > kObsStage || s0 < 0 || s1 > n_wav) ++cnt[C_STAGE_LOAD_OOR];
      if (ns > cnt[C_STAGE_MAX]) cnt[C_STAGE_MAX] = ns;
      cnt[C_STAGE_POINTS] += ns;
      cnt[C_STAGE_VALUES] += (int64_t)ns * (2 + ng);   // doubles the workgroup stages: wav, q and ng rows of R
      for (int32_t tid = 0; tid < kObsBlock; ++tid)
        for (int32_t i = tid; i < ns; i += kObsBlock)
          if (i < 0 || i >= kObsStage || s0 + i < 0 || s0 + i >= n_wav) ++cnt[C_STAGE_LOAD_OOR];
      for (int32_t wave = 0; wave < kObsBlock / 64; ++wave)
        for (int32_t j = wave; j < np; j += kObsBlock / 64) {
          const int32_t a = sA[j], b = sB[j];
          const bool staged = obs_staged(a, b, s0, s1);
          if (a == b) ++cnt[C_EMPTY_PIX]; else if (staged) ++cnt[C_STAGED_PIX]; else ++cnt[C_FALLBACK_PIX];
          int64_t pts = 0;
          for (int32_t it = 0; it < obs_passes(a, b); ++it)
            for (int32_t lane = 0; lane < 64; ++lane) {
              ++cnt[C_LANES];
              const int32_t w = obs_point(a, it, lane);
              if (w >= b) continue;
              ++pts;
              if (staged) {
                const int32_t i = w - s0;
                if (i < 0 || i >= ns || i >= kObsStage) ++cnt[C_STAGED_OOR];
              } else {
                ++cnt[C_FALLBACK_POINTS];
                cnt[C_FALLBACK_VALUES] += 2 + ng;   // ... and reads from global memory instead
              }
              if (w < 0 || w >= n_wav) ++cnt[C_GLOBAL_OOR];
            }
          if (pts != b - a) ++cnt[C_GLOBAL_OOR];   // every point of the support exactly once
          cnt[C_POINTS] += pts;
          for (int32_t g = 0; g < ng; ++g) {
            const int64_t at = (int64_t)(o0 + g) * n_pix + p0 + j;
            if (at < 0 || at >= (int64_t)n_orb * n_pix || touched[(size_t)at]) ++cnt[C_OUT_OOR]; else touched[(size_t)at] = 1;
          }
        }
    }
  for (char t : touched)
    if (!t) ++cnt[C_OUT_OOR];   // every output written exactly once
}

}  // extern "C"

#ifdef OBSERVE_HOST_MAIN
// a coarse / fine grid with duplicates, pixels beyond both ends, a tiny and a huge width, shared and per-phase frames
int main() {
  std::vector<double> wav;
  double x = 5880e-8;
  for (int i = 0; i < 4000; ++i) {
    wav.push_back(x);
    x += (i % 29 == 0) ? 0.0 : ((i / 700) % 2 ? 1e-11 : 2e-10);
  }
  const int32_t n_wav = (int32_t)wav.size(), n_pix = 1000 + 33, n_orb = 17;
  std::vector<double> lam(n_pix), sig(n_pix), f(n_orb);
  for (int32_t p = 0; p < n_pix; ++p) {
    lam[p] = wav.front() - 1e-8 + (wav.back() - wav.front() + 2e-8) * p / (n_pix - 1);
    sig[p] = p % 97 == 5 ? 1e-3 : (p % 89 == 7 ? 1e-13 : lam[p] / (140000.0 * 2.3548200450309493));
  }
  for (int32_t o = 0; o < n_orb; ++o) f[o] = 1.0 + 1e-4 * (o - 8) / 8.0;
  int64_t cnt[C_COUNT];
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    obs_audit(wav.data(), n_wav, lam.data(), sig.data(), 5.0, pass ? f.data() : nullptr, n_pix, n_orb, cnt, nullptr);
    std::printf("pass %d:", pass);
    for (int i = 0; i < C_COUNT; ++i) std::printf(" %lld", (long long)cnt[i]);
    std::printf("\n");
    bad += cnt[C_STAGED_OOR] || cnt[C_GLOBAL_OOR] || cnt[C_STAGE_LOAD_OOR] || cnt[C_OUT_OOR];
    bad += !(cnt[C_STAGED_PIX] && cnt[C_FALLBACK_PIX] && cnt[C_EMPTY_PIX]);
  }
  return bad ? 1 : 0;
}
#endif
