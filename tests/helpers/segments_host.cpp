// Host harness of prom_transit_set's pure planners, for CPU tests only (tests/test_segments_cpu.py).
//
// Linked with prometheus_amd/csrc/prom_segments.hip compiled as C++ (pure host code): sg_build runs
// build_sigma_segments and hands back the raw arrays, sg_guess_n is the device's seg_guess (prom_device.h) restated
// for the host -- fma, truncation, then the clamp to [0, m - 2] -- and the other exports are the planners themselves.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "prom_internal.h"

extern "C" {

int32_t sg_sizeof_seg() { return (int32_t)sizeof(prom::SigSeg); }
// kSigBlockW, kSigSeg, tc_slice_cap(arg), kRmStarMax
int32_t sg_const(int32_t which, int32_t arg) {
  const int32_t v[4] = {prom::kSigBlockW, prom::kSigSeg, prom::tc_slice_cap(arg), prom::kRmStarMax};
  return v[which];
}

// shift: [n_atoms][n_orb]; sizes: {seg, seg4, sdir, fb, fb_tc, n_dir, noguess}; null when no segments can be built
void* sg_build(const double* wav, int64_t n_wav, int32_t n_atoms, const double* const* X, const int64_t* nx,
               const double* shift, int64_t n_orb, int32_t use_dir, int32_t no_guess, int64_t* sizes) {
  std::vector<std::vector<double>> tabs(n_atoms);
  std::vector<const std::vector<double>*> tp(n_atoms);
  std::vector<const double*> sp(n_atoms);
  for (int a = 0; a < n_atoms; ++a) {
    tabs[a].assign(X[a], X[a] + nx[a]);
    tp[a] = &tabs[a];
    sp[a] = shift + (int64_t)a * n_orb;
  }
  prom::SigmaSegments* g = new prom::SigmaSegments;
  if (!prom::build_sigma_segments(wav, n_wav, tp, sp, n_orb, use_dir != 0, no_guess != 0, *g)) {
    delete g;
    return nullptr;
  }
  const int64_t sz[7] = {(int64_t)g->seg.size(), (int64_t)g->seg4.size(), (int64_t)g->sdir.size(), (int64_t)g->fb.size(),
                         (int64_t)g->fb_tc.size(), g->n_dir, g->noguess};
  std::memcpy(sizes, sz, sizeof(sz));
  return g;
}

void sg_copy(const void* h, void* seg, void* seg4, int32_t* sdir, int32_t* fb, int32_t* fb_tc) {
  const prom::SigmaSegments* g = static_cast<const prom::SigmaSegments*>(h);
  std::memcpy(seg, g->seg.data(), g->seg.size() * sizeof(prom::SigSeg));
  std::memcpy(seg4, g->seg4.data(), g->seg4.size() * sizeof(prom::SigSeg));
  std::memcpy(sdir, g->sdir.data(), g->sdir.size() * sizeof(int32_t));
  std::memcpy(fb, g->fb.data(), g->fb.size() * sizeof(int32_t));
  std::memcpy(fb_tc, g->fb_tc.data(), g->fb_tc.size() * sizeof(int32_t));
}

void sg_free(void* h) { delete static_cast<prom::SigmaSegments*>(h); }

void sg_guess_n(int64_t n, const double* t, const double* xs, const double* inv, const int32_t* m, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) {
    const int32_t g = (int32_t)std::fma(t[i], inv[i], xs[i]);
    out[i] = std::max(std::min(g, m[i] - 2), 0);
  }
}

int64_t sg_pair_mirrors(const double* cy, const double* cz, int64_t n_pr, int32_t* mirror) {
  std::vector<int32_t> m;
  const int64_t n = prom::pair_mirrors(cy, cz, n_pr, m);
  std::memcpy(mirror, m.data(), m.size() * sizeof(int32_t));
  return n;
}

// sl: [tiles of 256 wavelengths][3]
void sg_star_slices(const double* wav, int64_t n_wav, const double* X, int64_t nx, double s_min, double s_max,
                    int32_t* sl) {
  const std::vector<int32_t> v = prom::star_slices(wav, n_wav, std::vector<double>(X, X + nx), s_min, s_max);
  std::memcpy(sl, v.data(), v.size() * sizeof(int32_t));
}

int32_t sg_factor_range(const double* v, int64_t n, double* smin, double* smax) {
  return prom::factor_range(v, n, *smin, *smax) ? 1 : 0;
}

int32_t sg_poly_degree(const double* amax, int32_t n, int32_t enabled) {
  return prom::sigma_poly_degree(amax, n, enabled != 0);
}

int32_t sg_density_bounded(int32_t kind, const double* p) { return prom::density_bounded(kind, p) ? 1 : 0; }

}  // extern "C"

#ifdef SEGMENTS_HOST_MAIN
// stand-alone run (sanitizer builds): builds the segments of the problems of files written by the test module's
// dump_inputs(): int64 {n_wav, n_atoms, n_orb, nx[n_atoms]}, then wav, shift[n_atoms][n_orb] and the tables; then
// pairs chords made of the file's wavelengths and slices its first table as a star table
int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    FILE* f = std::fopen(argv[i], "rb");
    if (!f) return 2;
    int64_t h[3];
    if (std::fread(h, sizeof(int64_t), 3, f) != 3) return 2;
    const int64_t n_wav = h[0], n_orb = h[2];
    const int32_t na = (int32_t)h[1];
    std::vector<int64_t> nx(na);
    if (std::fread(nx.data(), sizeof(int64_t), na, f) != (size_t)na) return 2;
    std::vector<double> wav(n_wav), shift(na * n_orb);
    if (std::fread(wav.data(), 8, n_wav, f) != (size_t)n_wav) return 2;
    if (std::fread(shift.data(), 8, shift.size(), f) != shift.size()) return 2;
    std::vector<std::vector<double>> X(na);
    std::vector<const double*> Xp(na);
    for (int a = 0; a < na; ++a) {
      X[a].resize(nx[a]);
      if (std::fread(X[a].data(), 8, nx[a], f) != (size_t)nx[a]) return 2;
      Xp[a] = X[a].data();
    }
    std::fclose(f);
    for (int mode = 0; mode < 3; ++mode) {   // default, no directories, no guesses
      int64_t sz[7];
      void* g = sg_build(wav.data(), n_wav, na, Xp.data(), nx.data(), shift.data(), n_orb, mode != 1, mode == 2, sz);
      if (!g) return 3;
      std::printf("%s mode %d: %lld segments, %lld directories with %lld buckets, oversize blocks %lld / %lld, "
                  "unguessed %lld\n", argv[i], mode, (long long)sz[0], (long long)sz[5], (long long)sz[2],
                  (long long)sz[3], (long long)sz[4], (long long)sz[6]);
      sg_free(g);
    }
    std::vector<int32_t> mir(n_wav), sl(3 * ((n_wav + 255) / 256));
    std::vector<double> cy(n_wav), cz(n_wav);
    for (int64_t w = 0; w < n_wav; ++w) {
      cy[w] = wav[w >> 1];
      cz[w] = (w & 1) ? 1.0 : -1.0;
    }
    const int64_t np = sg_pair_mirrors(cy.data(), cz.data(), n_wav, mir.data());
    sg_star_slices(wav.data(), n_wav, Xp[0], nx[0], shift[0], shift[0], sl.data());
    std::printf("%s: %lld mirror pairs, first star slice {%d, %d, %d}\n", argv[i], (long long)np, sl[0], sl[1], sl[2]);
  }
  return 0;
}
#endif
