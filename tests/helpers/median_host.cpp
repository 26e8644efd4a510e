// Host harness of the median high-pass' index arithmetic and selection function (prometheus_amd/csrc/median_index.h
// over highpass_index.h).  Built by tests/test_median_cpu.py as a stand-alone program with its own main (also with
// -fsanitize=address,undefined).
//
//   median_host                  walks, for every half width of a list, a model row whose segments have the lengths of a
//                                list and are interleaved through perm: every workgroup, tile, thread and step of
//                                k_median in the kernel's order (stage, barrier, the sort's stages with a barrier each,
//                                the ranks, barrier, select and write, barrier), with the headers' own functions,
//                                through a ring, index and rank arrays exactly as long as their shapes say.  It counts
//                                every ring slot, index or rank entry, perm entry and model value out of range, every
//                                ring slot read that does not hold the original of the position intended, a sort that
//                                does not end ascending in (key, position), every model value read after it was
//                                overwritten or not written exactly once, and every result whose bits differ from the
//                                definition evaluated directly on the untouched row
//   median_host <file>           filters one row it is given as one segment: the file holds n, h and mode and then, as
//                                hexadecimal floats, M[n] and the expected M'[n]; the results must agree bit for bit
//                                (NaN with NaN)
//
// It prints its counters and returns 1 when anything was off.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "median_index.h"

using namespace prom;

enum { C_WORKGROUPS, C_TILES, C_CLEAN_WAVES, C_EVEN, C_OUTPUTS, C_RING_OOR, C_LDS_OOR, C_PERM_OOR, C_MODEL_OOR,
       C_SLOT_ERR, C_SORT_ERR, C_STALE_READ, C_VISIT_ERR, C_MISMATCH, C_COUNT };
static const char* kNames[C_COUNT] = {"workgroups", "tiles", "clean_waves", "even_counts", "outputs", "ring_oor",
                                      "lds_oor", "perm_oor", "model_oor", "slot_err", "sort_err", "stale_read",
                                      "visit_err", "mismatch"};

static bool same_bits(double a, double b) {
  if (a != a && b != b) return true;
  return std::memcmp(&a, &b, sizeof a) == 0;
}

static uint64_t key_of(double x) {
  uint64_t b;
  std::memcpy(&b, &x, sizeof b);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the definition, evaluated directly: position i of a segment whose originals are x[0 .. n)
static double define(const std::vector<double>& x, int32_t i, int32_t h, int mode, int64_t* cnt) {
  const int32_t n = (int32_t)x.size();
  std::vector<std::pair<uint64_t, double>> w;
  for (int32_t ip = (i - h > 0 ? i - h : 0); ip <= (i + h < n - 1 ? i + h : n - 1); ++ip)
    if (x[(size_t)ip] == x[(size_t)ip]) w.push_back({key_of(x[(size_t)ip]), x[(size_t)ip]});
  std::sort(w.begin(), w.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  const size_t c = w.size();
  double B = std::nan("");
  if (c % 2 == 1) B = w[(c - 1) / 2].second;
  if (c > 0 && c % 2 == 0) {
    const double sum = w[c / 2 - 1].second + w[c / 2].second;
    B = sum * 0.5;
    if (x[(size_t)i] == x[(size_t)i]) ++cnt[C_EVEN];
  }
  return mode == 0 ? x[(size_t)i] - B : x[(size_t)i] / B;
}

// one workgroup of k_median: the segment of n positions whose perm entries start at `first`, in row `model`
template <int MODE>
static void workgroup(std::vector<double>& model, std::vector<int32_t>& written, const std::vector<int32_t>& perm,
                      int32_t first, int32_t n, int32_t h, const std::vector<double>* want, int64_t* cnt) {
  const int32_t n_pix = (int32_t)model.size();
  std::vector<double> ring((size_t)kHpRingPad, 0.0);
  std::vector<int64_t> held((size_t)kHpRingPad, INT64_MIN);   // the position whose original a slot holds
  std::vector<uint16_t> idx((size_t)kMdStretch, 0xdead), rk((size_t)kMdStretch, 0xdead);
  std::vector<double> x((size_t)n);                           // the untouched originals, for the direct evaluation
  for (int32_t i = 0; i < n; ++i) x[(size_t)i] = model[(size_t)perm[(size_t)(first + i)]];
  ++cnt[C_WORKGROUPS];
  const int32_t n_tiles = hp_tiles(n);
  for (int32_t tile = 0; tile < n_tiles; ++tile) {
    ++cnt[C_TILES];
    const int32_t stage_end = hp_stage_end(tile, h);
    const int32_t base = md_base(tile, h), len = md_len(tile, n, h);
    const int32_t p = md_pow2(len), bits = md_bits(p);
    if (len < 1 || len > kMdStretch || p < len || p > kMdStretch || (1 << bits) != p || base < -kHpMaxHalf)
      ++cnt[C_LDS_OOR];
    for (int32_t tid = 0; tid < kHpBlock; ++tid) {
      for (int32_t i = hp_stage_first(tile, h) + tid; i < stage_end; i += kHpBlock) {
        double m = std::nan("");
        if (i >= 0 && i < n) {
          const int32_t pa = hp_perm_at(first, i);
          if (pa < 0 || pa >= (int32_t)perm.size()) {
            ++cnt[C_PERM_OOR];
            continue;
          }
          const int32_t pp = perm[(size_t)pa];
          if (pp < 0 || pp >= n_pix) {
            ++cnt[C_MODEL_OOR];
            continue;
          }
          if (written[(size_t)pp]) ++cnt[C_STALE_READ];
          m = model[(size_t)pp];
        }
        const int32_t slot = hp_slot(i);
        if (i < -kHpMaxHalf || slot < 0 || slot >= kHpRingPad) {
          ++cnt[C_RING_OOR];
          continue;
        }
        ring[(size_t)slot] = m;
        held[(size_t)slot] = i;
      }
      for (int32_t q = tid; q < kMdStretch; q += kHpBlock) {
        if (q < p)
          idx[(size_t)q] = (uint16_t)q;
        else
          rk[(size_t)q] = (uint16_t)kMdNoRank;
      }
    }
    // ---- barrier.  Every position of the stretch sits in the slot the key function reads
    for (int32_t q = 0; q < len; ++q) {
      const int32_t slot = hp_slot(base + q);
      if (slot < 0 || slot >= kHpRingPad)
        ++cnt[C_RING_OOR];
      else if (held[(size_t)slot] != base + q)
        ++cnt[C_SLOT_ERR];
    }
    for (int32_t k = 2; k <= p; k <<= 1)
      for (int32_t j = k >> 1; j > 0; j >>= 1) {
        std::vector<int32_t> touched((size_t)p, 0);
        for (int32_t tid = 0; tid < kHpBlock; ++tid)
          for (int32_t t = tid; t < (p >> 1); t += kHpBlock) {
            const int32_t lo = md_pair_lo(t, j), hi = lo + j;
            if (lo < 0 || hi >= p || idx[(size_t)lo] >= p || idx[(size_t)hi] >= p) {
              ++cnt[C_LDS_OOR];
              continue;
            }
            ++touched[(size_t)lo], ++touched[(size_t)hi];
            md_sort_pair(ring.data(), idx.data(), base, len, t, j, k);
          }
        for (int32_t q = 0; q < p; ++q)
          if (touched[(size_t)q] != 1) ++cnt[C_SORT_ERR];   // a stage's pairs are disjoint and cover the entries
        // ---- barrier
      }
    for (int32_t r = 0; r + 1 < p; ++r) {   // ascending in (key, position), every index once
      const int32_t qa = idx[(size_t)r], qb = idx[(size_t)r + 1];
      const uint64_t ka = md_key_at(ring.data(), base, len, qa), kb = md_key_at(ring.data(), base, len, qb);
      if (!(ka < kb || (ka == kb && qa < qb))) ++cnt[C_SORT_ERR];
    }
    for (int32_t tid = 0; tid < kHpBlock; ++tid)
      for (int32_t r = tid; r < p; r += kHpBlock) {
        if (idx[(size_t)r] >= p) {
          ++cnt[C_LDS_OOR];
          continue;
        }
        md_rank_write(ring.data(), idx.data(), rk.data(), base, len, r);
      }
    for (int32_t q = 0; q < kMdStretch; ++q) {   // every rank entry is defined: a rank below p or none
      const bool has = q < len && x.size() && base + q >= 0 && base + q < n && x[(size_t)(base + q)] == x[(size_t)(base + q)];
      if (has ? !(rk[(size_t)q] < p && idx[rk[(size_t)q]] == q) : rk[(size_t)q] != kMdNoRank) ++cnt[C_SORT_ERR];
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
      const int32_t q0 = md_q_first(tid);
      // the lane's first window starts at its first output's position less h, and the walk stays inside the ranks
      if (base + q0 != o - h || q0 < 0 || q0 + 2 * h + kHpOut - 1 >= kMdStretch) ++cnt[C_LDS_OOR];
      double B[kHpOut];
      if (clean)
        md_median<kHpOut, true>(ring.data(), idx.data(), rk.data(), base, q0, h, bits, B);
      else
        md_median<kHpOut, false>(ring.data(), idx.data(), rk.data(), base, q0, h, bits, B);
      for (int v = 0; v < kHpOut; ++v) {
        if (!(o + v < n)) continue;
        ++cnt[C_OUTPUTS];
        const int32_t pp = perm[(size_t)hp_perm_at(first, o + v)];
        if (pp < 0 || pp >= n_pix) {
          ++cnt[C_MODEL_OOR];
          continue;
        }
        if (held[(size_t)hp_slot(o + v)] != o + v) ++cnt[C_SLOT_ERR];
        const double r = hp_apply<MODE>(ring[(size_t)hp_slot(o + v)], B[v]);
        model[(size_t)pp] = r;
        ++written[(size_t)pp];
        if (!same_bits(r, define(x, o + v, h, MODE, cnt))) ++cnt[C_MISMATCH];
        if (want && !same_bits(r, (*want)[(size_t)(o + v)])) ++cnt[C_MISMATCH];
      }
    }
    // ---- barrier
  }
}

static void run(std::vector<double>& model, std::vector<int32_t>& written, const std::vector<int32_t>& perm,
                int32_t first, int32_t n, int32_t h, int mode, const std::vector<double>* want, int64_t* cnt) {
  if (mode == 0)
    workgroup<0>(model, written, perm, first, n, h, want, cnt);
  else
    workgroup<1>(model, written, perm, first, n, h, want, cnt);
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
  std::vector<double> M, want;
  if (!read(M, (size_t)n) || !read(want, (size_t)n)) return 1;
  std::fclose(f);
  std::vector<int32_t> perm((size_t)n), written((size_t)n, 0);
  for (int32_t i = 0; i < n; ++i) perm[(size_t)i] = i;
  int64_t cnt[C_COUNT] = {0};
  run(M, written, perm, 0, n, h, mode, &want, cnt);
  for (int32_t i = 0; i < n; ++i)
    if (written[(size_t)i] != 1) ++cnt[C_VISIT_ERR];
  char what[64];
  std::snprintf(what, sizeof what, "row n=%d h=%d mode=%d", n, h, mode);
  return report(what, cnt);
}

int main(int argc, char** argv) {
  if (argc > 1) return row_case(argv[1]);
  const int32_t lengths[] = {1, 2, 3, kHpTile - 1, kHpTile, kHpTile + 1, 2 * kHpTile + 5};
  const int32_t halves[] = {0, 1, 3, 255, 256, 512};
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
      // a row about 1, quantised to 1/64 in every third value so that ties are common, with a few NaN (one in 53),
      // signed zeros and infinities; the segment of exactly one tile holds no NaN, so its inner waves are clean
      std::vector<double> model((size_t)n_pix);
      uint64_t z = 88172645463325252ull + (uint64_t)h * 2 + (uint64_t)mode;
      for (int32_t p = 0; p < n_pix; ++p) {
        z ^= z << 13, z ^= z >> 7, z ^= z << 17;
        double m = 1.0 - 0.05 * (double)(z >> 11) / 9007199254740992.0;
        if (p % 3 == 0) m = std::floor(m * 64.0) / 64.0;
        if (z % 53 == 0) m = std::nan("");
        if (z % 211 == 1) m = 0.0;
        if (z % 211 == 2) m = -0.0;
        if (z % 499 == 3) m = INFINITY;
        if (z % 499 == 4) m = -INFINITY;
        model[(size_t)p] = m;
      }
      const int32_t tile_first = seg_first[4];
      for (int32_t i = 0; i < kHpTile; ++i) {
        double& m = model[(size_t)perm[(size_t)(tile_first + i)]];
        if (m != m) m = 0.97;
      }
      const int32_t long_first = seg_first[6];   // ... and the longest one none in [500, 1800): a clean wave at h = 512
      for (int32_t i = 500; i < 1800; ++i) {
        double& m = model[(size_t)perm[(size_t)(long_first + i)]];
        if (m != m) m = 0.96;
      }
      std::vector<int32_t> written((size_t)n_pix, 0);
      int64_t cnt[C_COUNT] = {0};
      for (int s = 0; s < n_seg; ++s) run(model, written, perm, seg_first[(size_t)s], lengths[s], h, mode, nullptr, cnt);
      for (int32_t p = 0; p < n_pix; ++p)
        if (written[(size_t)p] != 1) ++cnt[C_VISIT_ERR];
      if (cnt[C_OUTPUTS] != n_pix || hp_workgroups(1, n_seg) != n_seg) ++cnt[C_VISIT_ERR];
      char what[64];
      std::snprintf(what, sizeof what, "h=%d mode=%d n_pix=%d", h, mode, n_pix);
      rc |= report(what, cnt);
    }
  return rc;
}
