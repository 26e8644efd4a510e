// Host harness of SYSREM's index arithmetic, row shape and entry functions (prometheus_amd/csrc/sysrem_index.h).
// Built by tests/test_sysrem_cpu.py as a stand-alone program with its own main (also with
// -fsanitize=address,undefined).
//
//   sysrem_host                  walks, for a list of shapes, every workgroup and lane of k_sysrem_prep, of
//                                k_sysrem_step (both walks, the partials and the subtraction), of k_sysrem_rows and of
//                                k_sysrem_finish with the header's own functions in the kernels' order, through arrays
//                                exactly as long as their shapes say; counts every index out of range, every entry of
//                                the work buffers not written exactly once by k_sysrem_prep, every r entry not read and
//                                written exactly once per walk, every partial not written exactly once per step and not
//                                read exactly once by k_sysrem_rows, every a, U and cleaned entry not written exactly once
//   sysrem_host <file>           evaluates one step and one k_sysrem_rows on a case it is given, in the kernels' order
//                                (a lane's pixels, the butterfly over the tile, the tiles dealt to 64 sums, the
//                                butterfly): the file holds n_exp, n_pix and then, as hexadecimal floats, D[n_exp][n_pix],
//                                ivar[n_exp][n_pix], a[n_exp], the expected c[n_pix] = fit_c(a), the expected
//                                a'[n_exp] = fit_a(c), the expected norm, and the expected r after subtracting a c; the
//                                results must agree bit for bit (NaN with NaN)
//
// It prints its counters and returns 1 when anything was off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sysrem_index.h"

using namespace prom;

enum { C_WORKGROUPS, C_LANES, C_WORK_OOR, C_DATA_OOR, C_PART_OOR, C_A_OOR, C_U_OOR, C_VISIT_ERR, C_COUNT };
static const char* kNames[C_COUNT] = {"workgroups", "lanes", "work_oor", "data_oor", "part_oor", "a_oor", "u_oor",
                                      "visit_err"};

static void sy_audit(int32_t n_exp, int32_t n_pix, int32_t n_cols, int64_t* cnt) {
  for (int i = 0; i < C_COUNT; ++i) cnt[i] = 0;
  const int32_t n_tiles = sy_tiles(n_pix);
  const int64_t pitch = sy_pitch(n_pix);
  const int64_t n_work = (int64_t)n_exp * pitch, n_data = (int64_t)n_exp * n_pix, n_part = (int64_t)n_exp * n_tiles;
  if (n_tiles < 1 || pitch < n_pix || pitch % kSyTile != 0 || pitch - n_pix >= kSyTile) ++cnt[C_VISIT_ERR];
  // ---- k_sysrem_prep: one thread per entry of the pitched buffers
  {
    std::vector<int32_t> wr((size_t)n_work, 0), rd((size_t)n_data, 0);
    const int64_t wgs = sy_flat_workgroups(n_work);
    for (int64_t bx = 0; bx < wgs; ++bx) {
      ++cnt[C_WORKGROUPS];
      for (int32_t tid = 0; tid < kSyFlatBlock; ++tid) {
        const int64_t i = bx * kSyFlatBlock + tid;
        if (i >= n_work) continue;
        const int32_t e = (int32_t)(i / pitch), p = (int32_t)(i % pitch);
        if (p < n_pix) {
          const int64_t da = ex_data(e, p, n_pix);
          if (da < 0 || da >= n_data)
            ++cnt[C_DATA_OOR];
          else
            ++rd[(size_t)da];
        }
        const int64_t at = sy_at(e, p, pitch);
        if (at < 0 || at >= n_work)
          ++cnt[C_WORK_OOR];
        else
          ++wr[(size_t)at];
      }
    }
    for (auto v : wr) cnt[C_VISIT_ERR] += v != 1;
    for (auto v : rd) cnt[C_VISIT_ERR] += v != 1;
  }
  // ---- k_sysrem_step: a wave per tile; walk 1 reads, walk 2 reads (and writes r in the last step, part otherwise)
  {
    std::vector<int32_t> rd1((size_t)n_work, 0), rd2((size_t)n_work, 0), pw((size_t)n_part, 0);
    for (int32_t tile = 0; tile < n_tiles; ++tile) {
      ++cnt[C_WORKGROUPS];
      for (int32_t lane = 0; lane < kSyBlock; ++lane) {
        ++cnt[C_LANES];
        const int32_t p = sy_pixel(tile, lane);
        if (p < 0 || p % kSyVec != 0 || p + kSyVec > pitch) ++cnt[C_VISIT_ERR];
        for (int32_t e = 0; e < n_exp; ++e) {
          if (e < 0 || e >= n_exp) ++cnt[C_A_OOR];   // a[e]
          const int64_t at = sy_at(e, p, pitch);
          if (at < 0 || at + kSyVec > n_work || (at * 8) % (kSyVec * 8) != 0) {   // (one aligned vector)
            ++cnt[C_WORK_OOR];
            continue;
          }
          for (int v = 0; v < kSyVec; ++v) {
            ++rd1[(size_t)(at + v)];
            ++rd2[(size_t)(at + v)];   // (the last step writes the same entries back)
          }
          if (lane == 0) {
            const int64_t pa = sy_part(e, tile, n_tiles);
            if (pa < 0 || pa >= n_part)
              ++cnt[C_PART_OOR];
            else
              ++pw[(size_t)pa];
          }
        }
      }
    }
    for (auto v : rd1) cnt[C_VISIT_ERR] += v != 1;
    for (auto v : rd2) cnt[C_VISIT_ERR] += v != 1;
    for (auto v : pw) cnt[C_VISIT_ERR] += v != 1;
  }
  // ---- k_sysrem_rows: one workgroup, a wave per exposure in turn, then a[e] and U[e][col]
  for (int32_t col = 0; col < n_cols; ++col) {
    std::vector<int32_t> pr((size_t)n_part, 0), aw((size_t)n_exp, 0), uw((size_t)n_exp * n_cols, 0);
    if (n_exp > kSyMaxExp) ++cnt[C_A_OOR];
    for (int32_t wave = 0; wave < kSyRowsBlock / 64; ++wave)
      for (int32_t e = wave; e < n_exp; e += kSyRowsBlock / 64)
        for (int32_t lane = 0; lane < 64; ++lane) {
          const int32_t n = sy_rows_count(lane, n_tiles);
          for (int32_t i = 0; i < n; ++i) {
            const int32_t t = sy_rows_tile(lane, i);
            const int64_t pa = sy_part(e, t, n_tiles);
            if (t < 0 || t >= n_tiles || pa < 0 || pa >= n_part)
              ++cnt[C_PART_OOR];
            else
              ++pr[(size_t)pa];
          }
        }
    for (int32_t tid = 0; tid < kSyRowsBlock; ++tid)
      for (int32_t e = tid; e < n_exp; e += kSyRowsBlock) {
        ++aw[(size_t)e];
        const int64_t ua = sy_u(e, col, n_cols);
        if (ua < 0 || ua >= (int64_t)n_exp * n_cols)
          ++cnt[C_U_OOR];
        else
          ++uw[(size_t)ua];
      }
    for (auto v : pr) cnt[C_VISIT_ERR] += v != 1;
    for (auto v : aw) cnt[C_VISIT_ERR] += v != 1;
    for (int32_t e = 0; e < n_exp; ++e) cnt[C_VISIT_ERR] += uw[(size_t)sy_u(e, col, n_cols)] != 1;
  }
  // ---- k_sysrem_finish: one thread per entry of the cleaned data
  {
    std::vector<int32_t> ow((size_t)n_data, 0);
    const int64_t wgs = sy_flat_workgroups(n_data);
    for (int64_t bx = 0; bx < wgs; ++bx) {
      ++cnt[C_WORKGROUPS];
      for (int32_t tid = 0; tid < kSyFlatBlock; ++tid) {
        const int64_t i = bx * kSyFlatBlock + tid;
        if (i >= n_data) continue;
        const int32_t e = (int32_t)(i / n_pix), p = (int32_t)(i % n_pix);
        const int64_t at = sy_at(e, p, pitch), da = ex_data(e, p, n_pix);
        if (at < 0 || at >= n_work) ++cnt[C_WORK_OOR];
        if (da < 0 || da >= n_data)
          ++cnt[C_DATA_OOR];
        else
          ++ow[(size_t)da];
      }
    }
    for (auto v : ow) cnt[C_VISIT_ERR] += v != 1;
  }
}

static bool same_bits(double a, double b) {
  if (a != a && b != b) return true;
  return std::memcmp(&a, &b, sizeof a) == 0;
}

static int step_case(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 1;
  int n_exp = 0, n_pix = 0;
  if (std::fscanf(f, "%d %d", &n_exp, &n_pix) != 2 || n_exp < 1 || n_exp > kSyMaxExp || n_pix < 1) return 1;
  auto read = [&](std::vector<double>& v, size_t n) {
    v.resize(n);
    char buf[64];
    for (size_t i = 0; i < n; ++i) {
      if (std::fscanf(f, "%63s", buf) != 1) return false;
      v[i] = std::strtod(buf, nullptr);   // hexadecimal floats, "nan" and "inf"
    }
    return true;
  };
  const size_t n = (size_t)n_exp * n_pix;
  std::vector<double> D, iv, a, want_c, want_a, want_norm, want_r;
  if (!read(D, n) || !read(iv, n) || !read(a, (size_t)n_exp) || !read(want_c, (size_t)n_pix) ||
      !read(want_a, (size_t)n_exp) || !read(want_norm, 1) || !read(want_r, n))
    return 1;
  std::fclose(f);
  const int32_t n_tiles = sy_tiles(n_pix);
  const int64_t pitch = sy_pitch(n_pix);
  // k_sysrem_prep
  std::vector<double> w((size_t)(n_exp * pitch), 0.0), r((size_t)(n_exp * pitch), 0.0);
  for (int32_t e = 0; e < n_exp; ++e)
    for (int32_t p = 0; p < n_pix; ++p) {
      const double d = D[(size_t)ex_data(e, p, n_pix)];
      const double wv = sy_weight(iv[(size_t)ex_data(e, p, n_pix)], d);
      w[(size_t)sy_at(e, p, pitch)] = wv;
      if (wv > 0.0) r[(size_t)sy_at(e, p, pitch)] = d;
    }
  // k_sysrem_step<false>: per tile and lane the column fit, then per exposure the lane sums and the butterfly
  std::vector<double> c((size_t)pitch, 0.0), part((size_t)n_exp * n_tiles * 2, 0.0);
  for (int32_t tile = 0; tile < n_tiles; ++tile) {
    for (int32_t lane = 0; lane < kSyBlock; ++lane) {
      const int32_t p = sy_pixel(tile, lane);
      for (int v = 0; v < kSyVec; ++v) {
        double num = 0.0, den = 0.0;
        for (int32_t e = 0; e < n_exp; ++e)
          sy_fit_add(w[(size_t)sy_at(e, p + v, pitch)], r[(size_t)sy_at(e, p + v, pitch)], a[(size_t)e], &num, &den);
        c[(size_t)(p + v)] = sy_ratio(num, den);
      }
    }
    for (int32_t e = 0; e < n_exp; ++e) {
      double tn[64], td[64];
      for (int32_t lane = 0; lane < kSyBlock; ++lane) {
        const int32_t p = sy_pixel(tile, lane);
        tn[lane] = td[lane] = 0.0;
        for (int v = 0; v < kSyVec; ++v)
          sy_fit_add(w[(size_t)sy_at(e, p + v, pitch)], r[(size_t)sy_at(e, p + v, pitch)], c[(size_t)(p + v)], &tn[lane],
                     &td[lane]);
      }
      sy_butterfly_host(tn);
      sy_butterfly_host(td);
      part[2 * (size_t)sy_part(e, tile, n_tiles)] = tn[0];
      part[2 * (size_t)sy_part(e, tile, n_tiles) + 1] = td[0];
    }
  }
  // k_sysrem_rows
  std::vector<double> a2((size_t)n_exp, 0.0);
  for (int32_t e = 0; e < n_exp; ++e) {
    double tn[64], td[64];
    for (int32_t lane = 0; lane < 64; ++lane) {
      tn[lane] = td[lane] = 0.0;
      for (int32_t i = 0; i < sy_rows_count(lane, n_tiles); ++i) {
        const size_t pa = (size_t)sy_part(e, sy_rows_tile(lane, i), n_tiles);
        tn[lane] = sy_add(tn[lane], part[2 * pa]);
        td[lane] = sy_add(td[lane], part[2 * pa + 1]);
      }
    }
    sy_butterfly_host(tn);
    sy_butterfly_host(td);
    a2[(size_t)e] = sy_ratio(tn[0], td[0]);
  }
  double s = 0.0;
  for (int32_t e = 0; e < n_exp; ++e) s = sy_add(s, sy_mul(a2[(size_t)e], a2[(size_t)e]));
  const double norm = sy_sqrt(s);
  // k_sysrem_step<true>'s second walk with the case's a and c
  int bad = 0;
  for (int32_t p = 0; p < n_pix; ++p) bad += !same_bits(c[(size_t)p], want_c[(size_t)p]);
  for (int32_t e = 0; e < n_exp; ++e) bad += !same_bits(a2[(size_t)e], want_a[(size_t)e]);
  bad += !same_bits(norm, want_norm[0]);
  for (int32_t e = 0; e < n_exp; ++e)
    for (int32_t p = 0; p < n_pix; ++p) {
      const size_t at = (size_t)sy_at(e, p, pitch);
      bad += !same_bits(sy_residual(w[at], r[at], a[(size_t)e], c[(size_t)p]), want_r[(size_t)ex_data(e, p, n_pix)]);
    }
  std::printf("step n_exp=%d n_pix=%d mismatches=%d\n", n_exp, n_pix, bad);
  return bad != 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return step_case(argv[1]);
  const int32_t T = kSyTile;
  const int32_t pix[] = {1, T - 1, T, T + 1, 3 * T + 5, 64 * T + 1};   // (the last: a lane of k_sysrem_rows with two tiles)
  const int32_t exps[] = {1, 2, 7, 70};
  const int32_t cols[] = {1, 3, 16};
  int rc = 0, n_shapes = 0;
  for (int32_t n_pix : pix)
    for (int32_t n_exp : exps) {
      const int32_t n_cols = cols[n_shapes % 3];
      ++n_shapes;
      int64_t cnt[C_COUNT];
      sy_audit(n_exp, n_pix, n_cols, cnt);
      std::printf("n_exp=%d n_pix=%d n_cols=%d:", n_exp, n_pix, n_cols);
      for (int i = 0; i < C_COUNT; ++i) std::printf(" %s=%lld", kNames[i], (long long)cnt[i]);
      std::printf("\n");
      for (int i = C_WORK_OOR; i < C_COUNT; ++i) rc |= cnt[i] != 0;
      if (cnt[C_LANES] != (int64_t)sy_tiles(n_pix) * kSyBlock) rc = 1;
    }
  std::printf("shapes=%d tile=%d\n", n_shapes, T);
  return rc;
}
