// Host harness of k_broaden's index arithmetic and evaluation text (prometheus_amd/csrc/broaden_index.h), compiled
// with -ffp-contract=off like the library.  It reads one design from a file,
//
//   n_wav n_orb n_k b0 s / wav[n_wav] / R[n_orb][n_wav] / K[n_k] / want[n_orb][n_wav]      (hex floats)
//
// and walks every (tile, group, lane) exactly as the kernel does: the window of the tile's first and last output, the
// lanes' ends inside it with their proof (or, failing that, every lane's ends by br_end and the union by minimum and
// maximum), the stage filled when br_staged says so, the walk from the stage or from the global arrays.  It checks that
//   every output is owned exactly once per row                                              (owner_err)
//   each lane's [a, b) is exactly the set of members of the definition's test                (end_err)
//   a staged tile's union holds at most kBrStage points and every lane's reads lie inside it (stage_err)
//   the record index of every term lies in [0, n_k - 2]                                     (rec_err)
//   the result equals `want` bit for bit, NaN for NaN                                       (mismatch)
//   a staged tile's result equals the same walk over the global arrays                       (path_err)
// and prints the counts with the tiles staged and not, the tiles that kept their window and those whose lanes searched
// the grid, and the supports' minimum, mean and maximum.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "broaden_index.h"

using namespace prom;

static bool same_bits(double a, double b) {
  if (a != a || b != b) return (a != a) == (b != b);
  return std::memcmp(&a, &b, sizeof(double)) == 0;
}

static bool read_doubles(FILE* f, std::vector<double>& v, size_t n) {
  v.resize(n);
  char tok[64];
  for (size_t i = 0; i < n; ++i) {
    if (std::fscanf(f, "%63s", tok) != 1) return false;
    v[i] = std::strtod(tok, nullptr);
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: broaden_host design.txt\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_wav = 0, n_orb = 0, n_k = 0;
  char tb[64], ts[64];
  if (std::fscanf(f, "%d %d %d %63s %63s", &n_wav, &n_orb, &n_k, tb, ts) != 5) return 2;
  const BrKern kern{std::strtod(tb, nullptr), std::strtod(ts, nullptr), n_k};
  std::vector<double> wav, R, K, want;
  if (!read_doubles(f, wav, n_wav) || !read_doubles(f, R, (size_t)n_orb * n_wav) || !read_doubles(f, K, n_k) ||
      !read_doubles(f, want, (size_t)n_orb * n_wav))
    return 2;
  std::fclose(f);
  if (n_k < 2 || n_k > kBrMaxNodes || n_wav < 1 || n_orb < 1) return 2;

  // what the host side of the library forms: the records and (k_observe_q's text) the trapezoid weights
  std::vector<BrRec> rec(n_k);
  for (int i = 0; i < n_k; ++i) rec[i] = BrRec{K[i], i + 1 < n_k ? K[i + 1] - K[i] : 0.0};
  std::vector<double> q(n_wav);
  for (int w = 0; w < n_wav; ++w) {
    const double lo = w > 0 ? wav[w - 1] : wav[0], hi = w + 1 < n_wav ? wav[w + 1] : wav[n_wav - 1];
    q[w] = (hi - lo) / 2.0;
  }

  long owner_err = 0, end_err = 0, stage_err = 0, rec_err = 0, mismatch = 0, path_err = 0;
  long staged_tiles = 0, global_tiles = 0, fast_tiles = 0, slow_tiles = 0, sup_min = -1, sup_max = 0;
  double sup_sum = 0.0;
  std::vector<int> owned((size_t)n_orb * n_wav, 0);
  std::vector<double> sW(kBrStage), sQ(kBrStage), sR((size_t)kBrPhases * kBrStage);
  std::vector<int32_t> A(kBrBlock), B(kBrBlock);
  const int tiles = br_tiles(n_wav), groups = br_groups(n_orb);
  if (br_lds_bytes(n_k) > 65536) ++stage_err;
  for (int tile = 0; tile < tiles; ++tile) {
    // the window of the tile's first and last output; when it is staged every lane searches inside it and proves its
    // ends against the grid, otherwise (or when one lane's are not proven) every lane searches the grid and the union
    // is taken: exactly the kernel's steps (the same for every group of rows)
    const double xf = wav[br_output(tile, 0)], xl = wav[br_tile_last(tile, n_wav)];
    int32_t lo = br_end(wav.data(), n_wav, xf, br_r(xf), kern, false);
    int32_t hi = br_end(wav.data(), n_wav, xl, br_r(xl), kern, true);
    bool fast = br_staged(lo, hi);
    if (fast) {
      for (auto& v : sW) v = std::nan("");
      for (int32_t i = 0; i < hi - lo; ++i) sW[i] = wav[lo + i];
      for (int tid = 0; tid < kBrBlock && fast; ++tid) {
        const int32_t w = br_output(tile, tid);
        A[tid] = B[tid] = 0;
        if (w >= n_wav) continue;
        const double x = wav[w], r = br_r(x);
        A[tid] = br_end_in(sW.data(), lo, lo, hi, x, r, kern, false);
        B[tid] = br_end_in(sW.data(), lo, lo, hi, x, r, kern, true);
        fast = br_end_certain(wav.data(), n_wav, lo, hi, A[tid], x, r, kern, false) &&
               br_end_certain(wav.data(), n_wav, lo, hi, B[tid], x, r, kern, true);
      }
    }
    fast ? ++fast_tiles : ++slow_tiles;
    if (!fast) {
      lo = 0x7fffffff;
      hi = 0;
    }
    for (int tid = 0; tid < kBrBlock; ++tid) {
      const int32_t w = br_output(tile, tid);
      if (w >= n_wav) {
        A[tid] = B[tid] = 0;
        continue;
      }
      const double x = wav[w], r = br_r(x);
      if (!fast) {
        A[tid] = br_end(wav.data(), n_wav, x, r, kern, false);
        B[tid] = br_end(wav.data(), n_wav, x, r, kern, true);
      }
      const int32_t a = A[tid], b = B[tid];
      if (a < 0 || b > n_wav || b < a) ++end_err;
      for (int w1 = 0; w1 < n_wav; ++w1) {          // the members are exactly [a, b)
        const double t = br_t(wav[w1], x, r, kern);
        if (br_member(t, kern) != (w1 >= a && w1 < b)) ++end_err;
        if (br_member(t, kern)) {
          int32_t i = (int32_t)t;
          if (i > n_k - 2) i = n_k - 2;
          if (i < 0 || i > n_k - 2) ++rec_err;
        }
      }
      if (!fast && b > a) {
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
      }
      const long n = b - a;
      sup_sum += (double)n;
      if (sup_min < 0 || n < sup_min) sup_min = n;
      if (n > sup_max) sup_max = n;
    }
    const bool staged = br_staged(lo, hi);
    staged ? ++staged_tiles : ++global_tiles;
    if (staged && (hi - lo > kBrStage || lo < 0 || hi > n_wav)) ++stage_err;
    for (int grp = 0; grp < groups; ++grp) {
      const int32_t o0 = grp * kBrPhases;
      const int32_t ng = n_orb - o0 < kBrPhases ? n_orb - o0 : kBrPhases;
      const double* Rg = R.data() + (size_t)o0 * n_wav;
      if (staged) {
        // poison what the tile does not stage, so that a read outside the union shows
        for (auto& v : sW) v = std::nan("");
        for (auto& v : sQ) v = std::nan("");
        for (auto& v : sR) v = std::nan("");
        for (int32_t i = 0; i < hi - lo; ++i) {
          sW[i] = wav[lo + i];
          sQ[i] = q[lo + i];
          for (int g = 0; g < ng; ++g) sR[(size_t)g * kBrStage + i] = Rg[(size_t)g * n_wav + lo + i];
        }
      }
      for (int tid = 0; tid < kBrBlock; ++tid) {
        const int32_t w = br_output(tile, tid);
        if (w >= n_wav) continue;
        const double x = wav[w], r = br_r(x);
        const int32_t a = A[tid], b = B[tid];
        if (staged && b > a && (a < lo || b > hi)) ++stage_err;
        double num[kBrPhases], den, num2[kBrPhases], den2;
        br_walk(wav.data(), q.data(), Rg, n_wav, 0, ng, a, b, x, r, kern, rec.data(), num2, den2);
        if (staged)
          br_walk(sW.data(), sQ.data(), sR.data(), kBrStage, lo, ng, a, b, x, r, kern, rec.data(), num, den);
        else
          br_walk(wav.data(), q.data(), Rg, n_wav, 0, ng, a, b, x, r, kern, rec.data(), num, den);
        for (int g = 0; g < ng; ++g) {
          const size_t at = (size_t)(o0 + g) * n_wav + w;
          const double v = br_result(num[g], den);
          ++owned[at];
          if (!same_bits(v, want[at])) ++mismatch;
          if (!same_bits(v, br_result(num2[g], den2))) ++path_err;
        }
      }
    }
  }
  for (int c : owned)
    if (c != 1) ++owner_err;
  std::printf("tiles=%d groups=%d staged=%ld global=%ld owner_err=%ld end_err=%ld stage_err=%ld rec_err=%ld "
              "mismatch=%ld path_err=%ld support_min=%ld support_mean=%.2f support_max=%ld lds=%d window=%ld searched=%ld\n",
              tiles, groups, staged_tiles, global_tiles, owner_err, end_err, stage_err, rec_err, mismatch, path_err,
              sup_min, sup_sum / n_wav, sup_max, br_lds_bytes(n_k), fast_tiles, slow_tiles);
  return (owner_err || end_err || stage_err || rec_err || mismatch || path_err) ? 1 : 0;
}
