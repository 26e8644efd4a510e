// Host harness of the high-pass filtered exposures' index arithmetic and window function
// (prometheus_amd/csrc/highpass_index.h).  Built by tests/test_highpass_cpu.py as a stand-alone program with its own
// main (also with -fsanitize=address,undefined).
//
//   highpass_host                walks, for every half width of a list, a model row whose segments have the lengths of
//                                a list and are interleaved through perm: every workgroup, tile, thread and step of
//                                k_highpass in the kernel's order (stage, barrier, compute and write, barrier), with the
//                                header's own functions, through a ring and arrays exactly as long as their shapes say.
//                                It counts every ring slot, perm entry and model value out of range, every ring slot
//                                read that does not hold the original of the position intended, every model value read
//                                after it was overwritten or not written exactly once, and every result whose bits
//                                differ from the definition evaluated directly on the untouched row
//   highpass_host <file>         filters one row it is given as one segment: the file holds n, h and mode and then, as
//                                hexadecimal floats, g[h + 1], M[n] and the expected M'[n]; the results must agree bit
//                                for bit (NaN with NaN)
//
// It prints its counters and returns 1 when anything was off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "highpass_index.h"

using namespace prom;

enum { C_WORKGROUPS, C_TILES, C_CLEAN_WAVES, C_OUTPUTS, C_RING_OOR, C_PERM_OOR, C_MODEL_OOR, C_SLOT_ERR, C_STALE_READ,
       C_VISIT_ERR, C_MISMATCH, C_COUNT };
static const char* kNames[C_COUNT] = {"workgroups", "tiles", "clean_waves", "outputs", "ring_oor", "perm_oor",
                                      "model_oor", "slot_err", "stale_read", "visit_err", "mismatch"};

static bool same_bits(double a, double b) {
  if (a != a && b != b) return true;
  return std::memcmp(&a, &b, sizeof a) == 0;
}

// the definition, evaluated directly: position i of a segment whose originals are x[0 .. n)
static double define(const std::vector<double>& x, int32_t i, int32_t h, const std::vector<double>& g, int mode) {
  const int32_t n = (int32_t)x.size();
  double num = 0.0, den = 0.0;
  for (int32_t ip = (i - h > 0 ? i - h : 0); ip <= (i + h < n - 1 ? i + h : n - 1); ++ip) {
    if (x[(size_t)ip] != x[(size_t)ip]) continue;
    const double w = g[(size_t)(ip > i ? ip - i : i - ip)];
    num = num + w * x[(size_t)ip];
    den = den + w;
  }
  const double B = num / den;
  return mode == 0 ? x[(size_t)i] - B : x[(size_t)i] / B;
}

// one workgroup of k_highpass: the segment of n positions whose perm entries start at `first`, in row `model`
template <int MODE>
static void workgroup(std::vector<double>& model, std::vector<int32_t>& written, const std::vector<int32_t>& perm,
                      int32_t first, int32_t n, const std::vector<double>& g, int32_t h, double den_full,
                      const std::vector<double>* want, int64_t* cnt) {
  const int32_t n_pix = (int32_t)model.size();
  std::vector<double> ring((size_t)kHpRingPad, 0.0);
  std::vector<int64_t> held((size_t)kHpRingPad, INT64_MIN);   // the position whose original a slot holds
  std::vector<double> x((size_t)n);                           // the untouched originals, for the direct evaluation
  for (int32_t i = 0; i < n; ++i) x[(size_t)i] = model[(size_t)perm[(size_t)(first + i)]];
  ++cnt[C_WORKGROUPS];
  const int32_t n_tiles = hp_tiles(n);
  for (int32_t tile = 0; tile < n_tiles; ++tile) {
    ++cnt[C_TILES];
    const int32_t stage_end = hp_stage_end(tile, h);
    for (int32_t tid = 0; tid < kHpBlock; ++tid)
      for (int32_t i = hp_stage_first(tile, h) + tid; i < stage_end; i += kHpBlock) {
        double m = std::nan("");
        if (i >= 0 && i < n) {
          const int32_t pa = hp_perm_at(first, i);
          if (pa < 0 || pa >= (int32_t)perm.size()) {
            ++cnt[C_PERM_OOR];
            continue;
          }
          const int32_t p = perm[(size_t)pa];
          if (p < 0 || p >= n_pix) {
            ++cnt[C_MODEL_OOR];
            continue;
          }
          if (written[(size_t)p]) ++cnt[C_STALE_READ];
          m = model[(size_t)p];
        }
        const int32_t slot = hp_slot(i);
        if (i < -kHpMaxHalf || slot < 0 || slot >= kHpRingPad) {
          ++cnt[C_RING_OOR];
          continue;
        }
        ring[(size_t)slot] = m;
        held[(size_t)slot] = i;
      }
    // ---- barrier
    bool clean = false;
    for (int32_t tid = 0; tid < kHpBlock; ++tid) {
      if ((tid & 63) == 0) {   // the wave's vote; every slot a lane looks at holds the position intended
        const int32_t wave_first = hp_out_first(tile, tid);
        clean = true;
        for (int32_t lane = 0; lane < 64; ++lane) {
          for (int32_t i = wave_first - h + lane; i < wave_first + 64 * kHpOut + h; i += 64) {
            const int32_t slot = hp_slot(i);
            if (slot < 0 || slot >= kHpRingPad)
              ++cnt[C_RING_OOR];
            else if (held[(size_t)slot] != i)
              ++cnt[C_SLOT_ERR];
          }
          if (hp_lane_sees_nan(ring.data(), wave_first, lane, h)) clean = false;
        }
        if (clean) {
          ++cnt[C_CLEAN_WAVES];   // the claim behind the fast path: every window lies inside and holds no NaN
          for (int32_t q = wave_first - h; q < wave_first + 64 * kHpOut + h; ++q)
            if (q < 0 || q >= n || x[(size_t)q] != x[(size_t)q]) ++cnt[C_SLOT_ERR];
        }
      }
      const int32_t o = hp_out_first(tile, tid);
      if (!(o < n)) continue;
      if (o % kHpOut != 0) ++cnt[C_SLOT_ERR];
      // every slot hp_window reads: position o + k for k in [-h, h + kHpOut - 1], and the runs of kHpOut slots
      for (int32_t k = -h; k <= h + kHpOut - 1; ++k) {
        const int32_t slot = hp_slot(o + k);
        if (slot < 0 || slot >= kHpRingPad)
          ++cnt[C_RING_OOR];
        else if (held[(size_t)slot] != o + k)
          ++cnt[C_SLOT_ERR];
        if ((k & (kHpOut - 1)) == 0)
          for (int i = 0; i < kHpOut; ++i)
            if (hp_slot(o + k) + i != hp_slot(o + k + i)) ++cnt[C_SLOT_ERR];
      }
      double B[kHpOut];
      if (clean)
        hp_window<kHpOut, true>(ring.data(), o, h, g.data(), den_full, B);
      else
        hp_window<kHpOut, false>(ring.data(), o, h, g.data(), den_full, B);
      for (int v = 0; v < kHpOut; ++v) {
        if (!(o + v < n)) continue;
        ++cnt[C_OUTPUTS];
        const int32_t p = perm[(size_t)hp_perm_at(first, o + v)];
        if (p < 0 || p >= n_pix) {
          ++cnt[C_MODEL_OOR];
          continue;
        }
        if (held[(size_t)hp_slot(o + v)] != o + v) ++cnt[C_SLOT_ERR];
        const double r = hp_apply<MODE>(ring[(size_t)hp_slot(o + v)], B[v]);
        model[(size_t)p] = r;
        ++written[(size_t)p];
        if (!same_bits(r, define(x, o + v, h, g, MODE))) ++cnt[C_MISMATCH];
        if (want && !same_bits(r, (*want)[(size_t)(o + v)])) ++cnt[C_MISMATCH];
      }
    }
    // ---- barrier
  }
}

static void run(std::vector<double>& model, std::vector<int32_t>& written, const std::vector<int32_t>& perm,
                int32_t first, int32_t n, const std::vector<double>& g, int32_t h, int mode,
                const std::vector<double>* want, int64_t* cnt) {
  const double den_full = hp_den_full(g.data(), h);
  if (mode == 0)
    workgroup<0>(model, written, perm, first, n, g, h, den_full, want, cnt);
  else
    workgroup<1>(model, written, perm, first, n, g, h, den_full, want, cnt);
}

static int report(const char* what, const int64_t* cnt) {
  std::printf("%s:", what);
  for (int i = 0; i < C_COUNT; ++i) std::printf(" %s=%lld", kNames[i], (long long)cnt[i]);
  std::printf("\n");
  int rc = 0;
  for (int i = C_RING_OOR; i < C_COUNT; ++i) rc |= cnt[i] != 0;
  return rc;
}

static int row_case(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 1;
  int n = 0, h = 0, mode = 0;
  if (std::fscanf(f, "%d %d %d", &n, &h, &mode) != 3 || n < 1 || h < 0 || h > kHpMaxHalf || mode < 0 || mode > 1) return 1;
  auto read = [&](std::vector<double>& v, size_t count) {
    v.resize(count);
    char buf[64];
    for (size_t i = 0; i < count; ++i) {
      if (std::fscanf(f, "%63s", buf) != 1) return false;
      v[i] = std::strtod(buf, nullptr);   // hexadecimal floats, "nan" and "inf"
    }
    return true;
  };
  std::vector<double> g, M, want;
  if (!read(g, (size_t)h + 1) || !read(M, (size_t)n) || !read(want, (size_t)n)) return 1;
  std::fclose(f);
  std::vector<int32_t> perm((size_t)n), written((size_t)n, 0);
  for (int32_t i = 0; i < n; ++i) perm[(size_t)i] = i;
  int64_t cnt[C_COUNT] = {0};
  run(M, written, perm, 0, n, g, h, mode, &want, cnt);
  for (int32_t i = 0; i < n; ++i)
    if (written[(size_t)i] != 1) ++cnt[C_VISIT_ERR];
  char what[64];
  std::snprintf(what, sizeof what, "row n=%d h=%d mode=%d", n, h, mode);
  return report(what, cnt);
}

int main(int argc, char** argv) {
  if (argc > 1) return row_case(argv[1]);
  // the lengths about a wave, a workgroup's threads and the tile (one tile, a tile and one more, four tiles)
  const int32_t lengths[] = {1, 2, 255, 256, 257, 515, kHpTile - 1, kHpTile, kHpTile + 1, 3 * kHpTile + 452};
  const int32_t halves[] = {0, 3, 255, 256, 300, 512};
  const int n_seg = (int)(sizeof lengths / sizeof lengths[0]);
  int32_t n_pix = 0;
  std::vector<int32_t> seg_first(1, 0);
  for (int32_t n : lengths) seg_first.push_back(n_pix += n);
  // an interleaved perm: the pixels are dealt to the segments that still lack some, in turn; every second segment
  // takes its positions in descending pixel order
  std::vector<int32_t> perm((size_t)n_pix), filled((size_t)n_seg, 0);
  for (int32_t p = 0, s = 0; p < n_pix; ++p) {
    while (filled[(size_t)s] == lengths[s]) s = (s + 1) % n_seg;
    const int32_t i = s % 2 ? lengths[s] - 1 - filled[(size_t)s] : filled[(size_t)s];
    perm[(size_t)(seg_first[(size_t)s] + i)] = p;
    ++filled[(size_t)s];
    s = (s + 1) % n_seg;
  }
  int rc = 0;
  for (int32_t h : halves)
    for (int mode = 0; mode < 2; ++mode) {
      std::vector<double> g((size_t)h + 1);
      for (int32_t d = 0; d <= h; ++d) g[(size_t)d] = std::exp(-0.5 * (d / 40.0) * (d / 40.0)) * (d % 7 == 3 ? 0.0 : 1.0);
      // a row about 1 with a few NaN (one in 97; in the long segment a run of 700, none from position 1600 on, so
      // that its third tile is clean while h <= 452) and a zero
      std::vector<double> model((size_t)n_pix);
      uint64_t z = 88172645463325252ull + (uint64_t)h * 2 + (uint64_t)mode;
      for (int32_t p = 0; p < n_pix; ++p) {
        z ^= z << 13, z ^= z >> 7, z ^= z << 17;
        model[(size_t)p] = 1.0 - 0.05 * (double)(z >> 11) / 9007199254740992.0;
        if (z % 97 == 0) model[(size_t)p] = std::nan("");
      }
      const int32_t long_first = seg_first[(size_t)n_seg - 1];
      for (int32_t i = 900; i < 1600; ++i) model[(size_t)perm[(size_t)(long_first + i)]] = std::nan("");
      for (int32_t i = 1600; i < lengths[n_seg - 1]; ++i) {
        double& m = model[(size_t)perm[(size_t)(long_first + i)]];
        if (m != m) m = 0.97;
      }
      model[(size_t)perm[(size_t)(long_first + 2000)]] = 0.0;
      std::vector<int32_t> written((size_t)n_pix, 0);
      int64_t cnt[C_COUNT] = {0};
      for (int s = 0; s < n_seg; ++s)
        run(model, written, perm, seg_first[(size_t)s], lengths[s], g, h, mode, nullptr, cnt);
      for (int32_t p = 0; p < n_pix; ++p)
        if (written[(size_t)p] != 1) ++cnt[C_VISIT_ERR];
      if (cnt[C_OUTPUTS] != n_pix || hp_workgroups(1, n_seg) != n_seg) ++cnt[C_VISIT_ERR];
      char what[64];
      std::snprintf(what, sizeof what, "h=%d mode=%d n_pix=%d", h, mode, n_pix);
      rc |= report(what, cnt);
    }
  return rc;
}
