// Host harness of the filter's weights (prometheus_amd/csrc/filter_index.h).  Built by tests/test_filter_cpu.py as a
// stand-alone program with its own main (also with -fsanitize=address,undefined).
//
//   filter_host                  walks, for n_pix in {1, 63, 64, 65, 130} x n_exp in {1, 2, 7, 70} x K in
//                                {1, 2, 6, 11, 16}, every workgroup and thread of k_filter_weights with the header's own
//                                functions in the kernel's order: the ivar entries of the three walks, the U entries and
//                                the W entries of the last walk, through arrays exactly as long as their shapes say;
//                                counts every index out of range, every W entry not written exactly once, every ivar or
//                                U entry never read and every thread past n_pix that has a pixel.  Then it runs
//                                fw_weights itself for every thread on heap arrays of exactly those lengths (the
//                                sanitized build sees any access outside them) and counts the W entries it left
//                                untouched
//   filter_host <file>           evaluates fw_weights on columns it is given: the file holds n_exp, K, n_pix and then,
//                                as hexadecimal floats, U[n_exp][K], ivar[n_exp][n_pix] and the expected
//                                W[K][n_exp][n_pix]; the results must agree bit for bit, signs of zero included
//
// It prints its counters and returns 1 when anything was off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "filter_index.h"

using namespace prom;

enum { C_WORKGROUPS, C_PIXELS, C_IVAR_OOR, C_U_OOR, C_W_OOR, C_VISIT_ERR, C_UNTOUCHED, C_COUNT };
static const char* kNames[C_COUNT] = {"workgroups", "pixels", "ivar_oor", "u_oor", "w_oor", "visit_err", "untouched"};

template <int K>
static void run_pixel(const double* U, const double* iv, double* W, int64_t stride, int32_t n_exp) {
  FwTri<fw_entries(K)> L;
  L.mem = nullptr;
  L.pitch = 0;
  fw_weights<K, fw_entries(K)>(L, U, iv, W, stride, n_exp);
}

static bool run_any(int K, const double* U, const double* iv, double* W, int64_t stride, int32_t n_exp) {
  switch (K) {
#define CASE(NC) case NC: run_pixel<NC>(U, iv, W, stride, n_exp); return true;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13)
    CASE(14) CASE(15) CASE(16)
#undef CASE
  }
  return false;
}

static void fw_audit(int32_t n_exp, int32_t K, int32_t n_pix, int64_t* cnt) {
  for (int i = 0; i < C_COUNT; ++i) cnt[i] = 0;
  const int64_t n_u = (int64_t)n_exp * K, n_iv = (int64_t)n_exp * n_pix, n_w = n_u * n_pix;
  std::vector<int32_t> iv_reads((size_t)n_iv, 0), w_writes((size_t)n_w, 0);
  std::vector<char> u_seen((size_t)n_u, 0);
  const int32_t wgs = fw_tiles(n_pix);
  if (wgs < 1) ++cnt[C_VISIT_ERR];
  // the values of the run: a well-conditioned basis and positive weights; W starts as a pattern no solve produces
  std::vector<double> U((size_t)n_u), iv((size_t)n_iv), W((size_t)n_w);
  for (int64_t i = 0; i < n_u; ++i) U[(size_t)i] = ((i / K) % K == i % K ? 1.0 : 0.0) + 0.01 * (double)((i * 7919) % 13);
  for (int64_t i = 0; i < n_iv; ++i) iv[(size_t)i] = 0.5 + (double)((i * 104729) % 17) / 16.0;
  const double mark = -12345.678;
  for (int64_t i = 0; i < n_w; ++i) W[(size_t)i] = mark;
  for (int32_t bx = 0; bx < wgs; ++bx) {
    ++cnt[C_WORKGROUPS];
    for (int32_t tid = 0; tid < kFwTile; ++tid) {
      const int32_t p = fw_pixel(bx, tid);
      if (p < 0) ++cnt[C_VISIT_ERR];
      if (p >= n_pix) continue;   // (the kernel returns before it forms a pointer)
      ++cnt[C_PIXELS];
      const int64_t i0 = ex_data(0, p, n_pix), w0 = dt_w(0, 0, p, n_exp, n_pix), stride = n_pix;
      for (int pass = 0; pass < 3; ++pass)
        for (int32_t e = 0; e < n_exp; ++e) {
          const int64_t at = i0 + e * stride;   // (fw_weights' iv[e * stride])
          if (at < 0 || at >= n_iv || at != ex_data(e, p, n_pix))
            ++cnt[C_IVAR_OOR];
          else
            ++iv_reads[(size_t)at];
          for (int32_t k = 0; k < K; ++k) {
            const int64_t ua = dt_u(e, 0, K) + k;   // (fw_weights' u[k] behind U + dt_u(e, 0, K))
            if (ua < 0 || ua >= n_u || ua != dt_u(e, k, K))
              ++cnt[C_U_OOR];
            else
              u_seen[(size_t)ua] = 1;
            if (pass != 2) continue;
            const int64_t wa = w0 + ((int64_t)k * n_exp + e) * stride;   // (fw_weights' W[(k n_exp + e) stride])
            if (wa < 0 || wa >= n_w || wa != dt_w(k, e, p, n_exp, n_pix))
              ++cnt[C_W_OOR];
            else
              ++w_writes[(size_t)wa];
          }
        }
      if (!run_any(K, U.data(), iv.data() + i0, W.data() + w0, stride, n_exp)) ++cnt[C_VISIT_ERR];
    }
  }
  for (int64_t i = 0; i < n_iv; ++i)
    if (iv_reads[(size_t)i] != 3) ++cnt[C_VISIT_ERR];
  for (int64_t i = 0; i < n_w; ++i) {
    if (w_writes[(size_t)i] != 1) ++cnt[C_VISIT_ERR];
    if (W[(size_t)i] == mark) ++cnt[C_UNTOUCHED];
  }
  for (int64_t i = 0; i < n_u; ++i)
    if (!u_seen[(size_t)i]) ++cnt[C_VISIT_ERR];
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static int column_case(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 1;
  int n_exp = 0, K = 0, n_pix = 0;
  if (std::fscanf(f, "%d %d %d", &n_exp, &K, &n_pix) != 3 || n_exp < 1 || K < 1 || K > kDtMaxComp || n_pix < 1) return 1;
  auto read = [&](std::vector<double>& v, size_t n) {
    v.resize(n);
    char buf[64];
    for (size_t i = 0; i < n; ++i) {
      if (std::fscanf(f, "%63s", buf) != 1) return false;
      v[i] = std::strtod(buf, nullptr);   // hexadecimal floats, "nan" and "inf"
    }
    return true;
  };
  std::vector<double> U, iv, want;
  if (!read(U, (size_t)n_exp * K) || !read(iv, (size_t)n_exp * n_pix) || !read(want, (size_t)K * n_exp * n_pix)) return 1;
  std::fclose(f);
  std::vector<double> W(want.size(), -1.0);
  for (int32_t p = 0; p < n_pix; ++p)
    if (!run_any(K, U.data(), iv.data() + ex_data(0, p, n_pix), W.data() + dt_w(0, 0, p, n_exp, n_pix), n_pix, n_exp))
      return 1;
  int bad = 0;
  for (size_t i = 0; i < want.size(); ++i) bad += !same_bits(W[i], want[i]);
  std::printf("columns n_exp=%d K=%d n_pix=%d mismatches=%d\n", n_exp, K, n_pix, bad);
  return bad != 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return column_case(argv[1]);
  const int32_t pix[] = {1, 63, 64, 65, 130}, exps[] = {1, 2, 7, 70}, comps[] = {1, 2, 6, 11, 16};
  int rc = 0;
  for (int32_t n_pix : pix)
    for (int32_t n_exp : exps)
      for (int32_t K : comps) {
        int64_t cnt[C_COUNT];
        fw_audit(n_exp, K, n_pix, cnt);
        std::printf("n_pix=%d n_exp=%d K=%d:", n_pix, n_exp, K);
        for (int i = 0; i < C_COUNT; ++i) std::printf(" %s=%lld", kNames[i], (long long)cnt[i]);
        std::printf("\n");
        for (int i = C_IVAR_OOR; i < C_COUNT; ++i) rc |= cnt[i] != 0;
        if (cnt[C_PIXELS] != n_pix) rc = 1;
      }
  return rc;
}
