// Host harness of the detrended exposures' index arithmetic and column functions (prometheus_amd/csrc/detrend_index.h
// over expose_index.h and vmap_index.h).  Built by tests/test_detrend_cpu.py as a stand-alone program with its own
// main (also with -fsanitize=address,undefined).
//
//   detrend_host                 walks, for a list of shapes, every workgroup and thread of k_detrend (the column's
//                                model values in both passes, its U and W entries, its flag) and of k_model_moments
//                                in the launcher's batches (model, flag, data and the partial record), with the
//                                headers' own functions in the kernels' order, through arrays exactly as long as their
//                                shapes say; counts every index out of range, every model value or flag not written
//                                exactly once and every record not written exactly once per batch
//   detrend_host <file>          evaluates dt_coefficients / dt_apply on a case it is given: the file holds n_exp,
//                                n_comp and then, as hexadecimal floats, M[n_exp], U[n_exp][n_comp], W[n_comp][n_exp]
//                                (one column, so n_pix = 1), the expected filterable flag and the expected M'[n_exp];
//                                the results must agree bit for bit (NaN with NaN)
//
// It prints its counters and returns 1 when anything was off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "detrend_index.h"

using namespace prom;

enum { C_WORKGROUPS, C_COLUMNS, C_BATCHES, C_MODEL_OOR, C_U_OOR, C_W_OOR, C_FLAG_OOR, C_DATA_OOR, C_PART_OOR,
       C_VISIT_ERR, C_COUNT };
static const char* kNames[C_COUNT] = {"workgroups", "columns", "batches", "model_oor", "u_oor", "w_oor", "flag_oor",
                                      "data_oor", "part_oor", "visit_err"};

static void dt_audit(int32_t n_exp, int32_t n_comp, int32_t n_trial, int32_t n_pix, int64_t cap_bytes, int64_t* cnt) {
  for (int i = 0; i < C_COUNT; ++i) cnt[i] = 0;
  const int64_t n_model = (int64_t)n_exp * n_trial * n_pix, n_u = (int64_t)n_exp * n_comp;
  const int64_t n_w = n_u * n_pix, n_flag = (int64_t)n_trial * n_pix, n_data = (int64_t)n_exp * n_pix;
  std::vector<int32_t> reads((size_t)n_model, 0), writes((size_t)n_model, 0), flags((size_t)n_flag, 0);
  std::vector<char> w_seen((size_t)n_w, 0), u_seen((size_t)n_u, 0);
  // ---- k_detrend: the whole table in one launch
  const int32_t n_tiles = dt_tiles(n_pix);
  const int64_t wgs = dt_workgroups(n_trial, n_pix);
  if (wgs < 1 || wgs > (((int64_t)1 << 31) - 1)) ++cnt[C_VISIT_ERR];
  const int64_t m_stride = (int64_t)n_trial * n_pix;
  for (int64_t bx = 0; bx < wgs; ++bx) {
    ++cnt[C_WORKGROUPS];
    const int32_t tile = dt_wg_tile((int32_t)bx, n_tiles), group = dt_wg_group((int32_t)bx, n_tiles);
    for (int32_t tid = 0; tid < kDtBlock; ++tid) {
      const int32_t p = dt_pixel(tile, tid), j = dt_trial(group, tid);
      if (p < 0 || j < 0) ++cnt[C_VISIT_ERR];
      if (p >= n_pix || j >= n_trial) continue;
      ++cnt[C_COLUMNS];
      const int64_t m0 = ex_model(0, j, p, n_trial, n_pix), w0 = dt_w(0, 0, p, n_exp, n_pix);
      for (int32_t e = 0; e < n_exp; ++e) {
        const int64_t at = m0 + e * m_stride;          // (dt_coefficients' and dt_apply's M[e * m_stride])
        if (at < 0 || at >= n_model || at != ex_model(e, j, p, n_trial, n_pix)) {
          ++cnt[C_MODEL_OOR];
          continue;
        }
        ++reads[(size_t)at];
        ++writes[(size_t)at];
        for (int32_t k = 0; k < n_comp; ++k) {
          const int64_t wa = w0 + ((int64_t)k * n_exp + e) * n_pix;   // (dt_coefficients' W[(k n_exp + e) w_stride])
          if (wa < 0 || wa >= n_w || wa != dt_w(k, e, p, n_exp, n_pix))
            ++cnt[C_W_OOR];
          else
            w_seen[(size_t)wa] = 1;
          const int64_t ua = dt_u(e, k, n_comp);
          if (ua < 0 || ua >= n_u)
            ++cnt[C_U_OOR];
          else
            u_seen[(size_t)ua] = 1;
        }
      }
      const int64_t fa = dt_flag(j, p, n_pix);
      if (fa < 0 || fa >= n_flag)
        ++cnt[C_FLAG_OOR];
      else
        ++flags[(size_t)fa];
    }
  }
  for (int64_t i = 0; i < n_model; ++i)
    if (reads[(size_t)i] != 1 || writes[(size_t)i] != 1) ++cnt[C_VISIT_ERR];
  for (int64_t i = 0; i < n_flag; ++i)
    if (flags[(size_t)i] != 1) ++cnt[C_VISIT_ERR];
  for (int64_t i = 0; i < n_w; ++i)
    if (!w_seen[(size_t)i]) ++cnt[C_VISIT_ERR];
  for (int64_t i = 0; i < n_u; ++i)
    if (!u_seen[(size_t)i]) ++cnt[C_VISIT_ERR];
  // ---- k_model_moments: batches of whole trial groups under the scratch cap
  const int32_t n_chunks = vm_chunks(n_pix), n_groups = vm_groups(n_trial);
  const int32_t bg = vm_batch_groups(cap_bytes, n_exp, n_chunks, n_groups);
  if (bg < 1) ++cnt[C_PART_OOR];
  const int32_t nb_max = bg * kVmTrials < n_trial ? bg * kVmTrials : n_trial;
  const int64_t part_cap = vm_part_doubles(n_exp, nb_max, n_chunks);
  std::vector<int32_t> mom_reads((size_t)n_model, 0);
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
        for (int32_t tid = 0; tid < kVmBlock; ++tid) {
          const int32_t r = vm_entry_trial(tid), t = vm_entry_pixel(tid);
          for (int32_t ti = 0; ti < ntile; ++ti) {
            const int32_t p0 = vm_tile_first(tile0 + ti), np = vm_tile_count(tile0 + ti, n_pix);
            if (p0 < 0 || np < 1 || p0 + np > n_pix) ++cnt[C_VISIT_ERR];
            if (!(r < nt && t < np)) continue;
            const int32_t j = j_first + jb0 + r;
            const int64_t da = ex_data(e, p0 + t, n_pix), ma = ex_model(e, j, p0 + t, n_trial, n_pix);
            const int64_t fa = dt_flag(j, p0 + t, n_pix);
            if (da < 0 || da >= n_data) ++cnt[C_DATA_OOR];
            if (fa < 0 || fa >= n_flag) ++cnt[C_FLAG_OOR];
            if (ma < 0 || ma >= n_model)
              ++cnt[C_MODEL_OOR];
            else
              ++mom_reads[(size_t)ma];
          }
          if (t == 0 && r < nt) {
            const int64_t slot = vm_part_slot(e, jb0 + r, chunk, nb, n_chunks);
            if (slot < 0 || slot + kVmRecord > part_cap) {
              ++cnt[C_PART_OOR];
              continue;
            }
            if (written[(size_t)slot]) ++cnt[C_VISIT_ERR];
            written[(size_t)slot] = 1;
          }
        }
      }
    for (int64_t s = 0; s < vm_part_doubles(n_exp, nb, n_chunks); s += kVmRecord)
      if (!written[(size_t)s]) ++cnt[C_VISIT_ERR];
  }
  for (int64_t i = 0; i < n_model; ++i)
    if (mom_reads[(size_t)i] != 1) ++cnt[C_VISIT_ERR];
}

static bool same_bits(double a, double b) {
  if (a != a && b != b) return true;
  return std::memcmp(&a, &b, sizeof a) == 0;
}

template <int NC>
static int column_nc(int32_t n_exp, std::vector<double>& M, const std::vector<double>& Ub, const std::vector<double>& W,
                     bool want_ok, const std::vector<double>& want) {
  double c[NC];
  const bool ok = dt_coefficients<NC>(M.data(), 1, W.data(), 1, n_exp, c);
  dt_apply<NC>(M.data(), 1, Ub.data(), n_exp, c, ok);
  int bad = ok != want_ok;
  for (int32_t e = 0; e < n_exp; ++e) bad += !same_bits(M[(size_t)e], want[(size_t)e]);
  return bad;
}

static int column_case(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 1;
  int n_exp = 0, n_comp = 0, want_ok = 0;
  if (std::fscanf(f, "%d %d", &n_exp, &n_comp) != 2 || n_exp < 1 || n_comp < 1 || n_comp > kDtMaxComp) return 1;
  auto read = [&](std::vector<double>& v, size_t n) {
    v.resize(n);
    char buf[64];
    for (size_t i = 0; i < n; ++i) {
      if (std::fscanf(f, "%63s", buf) != 1) return false;
      v[i] = std::strtod(buf, nullptr);   // hexadecimal floats, "nan" and "inf"
    }
    return true;
  };
  std::vector<double> M, Ub, W, want;
  if (!read(M, (size_t)n_exp) || !read(Ub, (size_t)n_exp * n_comp) || !read(W, (size_t)n_comp * n_exp)) return 1;
  if (std::fscanf(f, "%d", &want_ok) != 1 || !read(want, (size_t)n_exp)) return 1;
  std::fclose(f);
  int bad = 1;
  switch (n_comp) {
#define CASE(NC) case NC: bad = column_nc<NC>(n_exp, M, Ub, W, want_ok != 0, want); break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13)
    CASE(14) CASE(15) CASE(16)
#undef CASE
  }
  std::printf("column n_exp=%d n_comp=%d mismatches=%d\n", n_exp, n_comp, bad);
  return bad != 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return column_case(argv[1]);
  // n_exp, n_comp, n_trial, n_pix, scratch cap in bytes (a small cap: one trial group per batch)
  const int64_t big = (int64_t)256 << 20;
  const int64_t shapes[][5] = {{1, 1, 1, 1, big},   {2, 2, 7, 33, big},  {5, 16, 9, 513, big}, {5, 3, 9, 513, 104},
                               {3, 6, 17, 64, 104}, {3, 6, 4, 65, big},  {2, 1, 5, 127, 104},  {4, 2, 33, 1025, big}};
  int rc = 0;
  for (const auto& s : shapes) {
    int64_t cnt[C_COUNT];
    dt_audit((int32_t)s[0], (int32_t)s[1], (int32_t)s[2], (int32_t)s[3], s[4], cnt);
    std::printf("n_exp=%d n_comp=%d n_trial=%d n_pix=%d cap=%lld:", (int)s[0], (int)s[1], (int)s[2], (int)s[3],
                (long long)s[4]);
    for (int i = 0; i < C_COUNT; ++i) std::printf(" %s=%lld", kNames[i], (long long)cnt[i]);
    std::printf("\n");
    for (int i = C_MODEL_OOR; i < C_COUNT; ++i) rc |= cnt[i] != 0;
    if (cnt[C_COLUMNS] != s[2] * s[3]) rc = 1;
  }
  return rc;
}
