// Host harness of the per-order moments' index arithmetic and formulas (prometheus_amd/csrc/order_index.h over
// detrend_index.h, expose_index.h and vmap_index.h).  Built by tests/test_order_moments_cpu.py as a stand-alone program
// with its own main (also with -fsanitize=address,undefined, and with small PROM_OD_TILE / PROM_OD_TRIALS).
//
//   order_host <case> <out>      the case file holds n_exp n_trial n_pix n_seg cap_bytes, then seg_first[n_seg + 1],
//                                perm[n_pix], keep[n_seg], flag[n_trial][n_pix] as integers and model[n_exp][n_trial]
//                                [n_pix], data[n_exp][n_pix], ivar[n_exp][n_pix] as hexadecimal floats.  The program
//                                walks every batch of the launcher (od_batch_groups under cap_bytes), every workgroup of
//                                k_order_moments (exposure, trial group, order), every tile and every thread with the
//                                header's own functions in the kernel's order, through arrays exactly as long as their
//                                shapes say: the terms, the butterfly over the tile's lanes, lane 0's sum in tile order,
//                                the record; then every thread of k_order_totals.  It counts every index out of range
//                                and every record or total not written exactly once, and writes to <out> per (e, j, s)
//                                the seven moments, n_used and the argument of loglike's logarithm, and per (e, j) the
//                                totals of chi2, chi2_scaled and the count (hexadecimal floats), for the test to compare
//                                with the numpy reference bit for bit.
//
// It prints its counters and returns 1 when anything was off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "order_index.h"

using namespace prom;

enum { C_BATCHES, C_WORKGROUPS, C_TILES, C_PERM_OOR, C_MODEL_OOR, C_DATA_OOR, C_FLAG_OOR, C_REC_OOR, C_TOT_OOR,
       C_VISIT_ERR, C_COUNT };
static const char* kNames[C_COUNT] = {"batches", "workgroups", "tiles", "perm_oor", "model_oor", "data_oor", "flag_oor",
                                      "rec_oor", "tot_oor", "visit_err"};

static bool read_i(FILE* f, int64_t* v) {
  long long x;
  if (std::fscanf(f, "%lld", &x) != 1) return false;
  *v = x;
  return true;
}
static bool read_d(FILE* f, double* v) {
  char buf[64];
  if (std::fscanf(f, "%63s", buf) != 1) return false;
  *v = std::strtod(buf, nullptr);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: order_host <case> <out>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int64_t v[5];
  for (auto& x : v)
    if (!read_i(f, &x)) return 2;
  const int32_t n_exp = (int32_t)v[0], n_trial = (int32_t)v[1], n_pix = (int32_t)v[2], n_seg = (int32_t)v[3];
  const int64_t cap_bytes = v[4];
  const int64_t n_model = (int64_t)n_exp * n_trial * n_pix, n_data = (int64_t)n_exp * n_pix;
  const int64_t n_flag = (int64_t)n_trial * n_pix, n_tot = (int64_t)n_exp * n_trial * kOdTotals;
  std::vector<int32_t> seg((size_t)n_seg + 1), perm((size_t)n_pix);
  std::vector<uint8_t> keep((size_t)n_seg), flag((size_t)n_flag);
  std::vector<double> model((size_t)n_model), data((size_t)n_data), ivar((size_t)n_data);
  int64_t x;
  for (auto& s : seg) { if (!read_i(f, &x)) return 2; s = (int32_t)x; }
  for (auto& p : perm) { if (!read_i(f, &x)) return 2; p = (int32_t)x; }
  for (auto& k : keep) { if (!read_i(f, &x)) return 2; k = (uint8_t)x; }
  for (auto& k : flag) { if (!read_i(f, &x)) return 2; k = (uint8_t)x; }
  for (auto& m : model) if (!read_d(f, &m)) return 2;
  for (auto& m : data) if (!read_d(f, &m)) return 2;
  for (auto& m : ivar) if (!read_d(f, &m)) return 2;
  std::fclose(f);

  int64_t cnt[C_COUNT] = {};
  // the caller's arrays, the launcher's repacking
  const int64_t n_rec = (int64_t)n_exp * n_trial * n_seg;
  std::vector<double> out_mom((size_t)n_rec * 7, 0.0), out_arg((size_t)n_rec, 0.0), tot((size_t)n_tot, 0.0);
  std::vector<int64_t> out_nu((size_t)n_rec, 0);
  std::vector<int32_t> rec_seen((size_t)n_rec, 0), tot_seen((size_t)n_exp * n_trial, 0);

  const int32_t n_groups_all = od_groups(n_trial);
  if (od_workgroups(n_exp, 1, n_seg) > (((int64_t)1 << 31) - 1)) ++cnt[C_VISIT_ERR];
  const int32_t bg = od_batch_groups(cap_bytes, n_exp, n_seg, n_groups_all);
  if (bg < 1) ++cnt[C_VISIT_ERR];
  const int32_t nb_max = bg * kOdTrials < n_trial ? bg * kOdTrials : n_trial;
  std::vector<double> tm((size_t)kOdBlock * 7), nx((size_t)kOdBlock * 7), acc((size_t)kOdBlock * 7);
  std::vector<int32_t> cc((size_t)kOdBlock), cx((size_t)kOdBlock);
  std::vector<int64_t> total((size_t)kOdBlock);
  for (int32_t g = 0; g < n_groups_all; g += bg) {
    ++cnt[C_BATCHES];
    const int32_t j_first = od_group_first(g), nb = nb_max < n_trial - j_first ? nb_max : n_trial - j_first;
    const int64_t n_orec = od_record_doubles(n_exp, nb, n_seg);
    if (n_orec * 8 > cap_bytes && bg > 1) ++cnt[C_VISIT_ERR];   // (one group may exceed the cap, more may not)
    std::vector<double> orec((size_t)n_orec, 0.0);
    std::vector<int32_t> written((size_t)(n_orec / kOdRecord), 0);
    // ---- k_order_moments
    const int32_t n_groups = od_groups(nb);
    const int64_t wgs = od_workgroups(n_exp, n_groups, n_seg);
    if (wgs < 1 || wgs > (((int64_t)1 << 31) - 1)) ++cnt[C_VISIT_ERR];
    for (int64_t bx = 0; bx < wgs; ++bx) {
      ++cnt[C_WORKGROUPS];
      const int32_t s = od_wg_segment((int32_t)bx, n_seg), gb = od_wg_group((int32_t)bx, n_groups, n_seg);
      const int32_t e = od_wg_exposure((int32_t)bx, n_groups, n_seg);
      if (s < 0 || s >= n_seg || gb < 0 || gb >= n_groups || e < 0 || e >= n_exp ||
          ((int64_t)e * n_groups + gb) * n_seg + s != bx) {
        ++cnt[C_VISIT_ERR];
        continue;
      }
      const int32_t jb0 = od_group_first(gb);
      const int32_t nt = nb - jb0 < kOdTrials ? nb - jb0 : kOdTrials;
      if (nt < 1) ++cnt[C_VISIT_ERR];
      const int32_t first = seg[(size_t)s], n = seg[(size_t)s + 1] - first;
      std::fill(acc.begin(), acc.end(), 0.0);
      std::fill(total.begin(), total.end(), (int64_t)0);
      const int32_t ntile = od_tiles(n);
      int64_t covered = 0;
      for (int32_t tile = 0; tile < ntile; ++tile) {
        ++cnt[C_TILES];
        covered += od_tile_count(tile, n);
        for (int32_t tid = 0; tid < kOdBlock; ++tid) {
          const int32_t r = od_thread_trial(tid), t = od_thread_pos(tid);
          const bool live = r < nt && t < od_tile_count(tile, n);
          double* m = &tm[(size_t)tid * 7];
          for (int i = 0; i < 7; ++i) m[i] = 0.0;
          cc[(size_t)tid] = 0;
          if (!live) continue;
          const int32_t j = j_first + jb0 + r;
          const int32_t pa = od_perm_at(first, od_tile_first(tile) + t);
          if (pa < first || pa >= first + n || pa >= n_pix) {
            ++cnt[C_PERM_OOR];
            continue;
          }
          const int32_t p = perm[(size_t)pa];
          const int64_t at = ex_data(e, p, n_pix), am = ex_model(e, j, p, n_trial, n_pix), af = dt_flag(j, p, n_pix);
          if (p < 0 || p >= n_pix || at < 0 || at >= n_data) { ++cnt[C_DATA_OOR]; continue; }
          if (j >= n_trial || am < 0 || am >= n_model) { ++cnt[C_MODEL_OOR]; continue; }
          if (af < 0 || af >= n_flag) { ++cnt[C_FLAG_OOR]; continue; }
          const double iv = ivar[(size_t)at], d = data[(size_t)at], M = model[(size_t)am];
          const bool ok = flag[(size_t)af] != 0;
          if (iv > 0.0 && iv < __builtin_inf() && __builtin_fabs(d) < __builtin_inf() && ok && M == M) {
            const double ivM = iv * M, ivd = iv * d, df = M - d;
            m[0] = iv;
            m[1] = ivM;
            m[2] = ivd;
            m[3] = ivM * M;
            m[4] = ivM * d;
            m[5] = ivd * d;
            m[6] = iv * (df * df);
            cc[(size_t)tid] = 1;
          }
        }
        for (int mm = 1; mm < kOdTile; mm <<= 1) {   // __shfl_xor: every thread adds its partner's value at once
          for (int32_t tid = 0; tid < kOdBlock; ++tid) {
            const int32_t o = tid ^ mm;
            if (o < 0 || o >= kOdBlock || od_thread_trial(o) != od_thread_trial(tid)) {
              ++cnt[C_VISIT_ERR];
              continue;
            }
            for (int i = 0; i < 7; ++i) nx[(size_t)tid * 7 + i] = tm[(size_t)tid * 7 + i] + tm[(size_t)o * 7 + i];
            cx[(size_t)tid] = cc[(size_t)tid] + cc[(size_t)o];
          }
          tm.swap(nx);
          cc.swap(cx);
        }
        for (int32_t tid = 0; tid < kOdBlock; ++tid)
          if (od_thread_pos(tid) == 0) {
            for (int i = 0; i < 7; ++i) acc[(size_t)tid * 7 + i] += tm[(size_t)tid * 7 + i];
            total[(size_t)tid] += cc[(size_t)tid];
          }
      }
      if (covered != n) ++cnt[C_VISIT_ERR];
      for (int32_t tid = 0; tid < kOdBlock; ++tid) {
        const int32_t r = od_thread_trial(tid), t = od_thread_pos(tid);
        if (!(t == 0 && r < nt)) continue;
        const int64_t slot = od_record(e, jb0 + r, s, nb, n_seg);
        if (slot < 0 || slot + kOdRecord > n_orec || slot % kOdRecord != 0) {
          ++cnt[C_REC_OOR];
          continue;
        }
        for (int i = 0; i < 7; ++i) orec[(size_t)slot + i] = acc[(size_t)tid * 7 + i];
        std::memcpy(&orec[(size_t)slot + 7], &total[(size_t)tid], sizeof(int64_t));
        ++written[(size_t)(slot / kOdRecord)];
      }
    }
    for (int32_t w : written)
      if (w != 1) ++cnt[C_VISIT_ERR];
    // ---- k_order_totals
    const int64_t blocks = ((int64_t)n_exp * nb + kOdBlock - 1) / kOdBlock;
    for (int64_t i = 0; i < blocks * kOdBlock; ++i) {
      if (i >= (int64_t)n_exp * nb) continue;
      const int32_t e = (int32_t)(i / nb), jb = (int32_t)(i % nb);
      double ll = 0.0, chi2 = 0.0, scaled = 0.0, count = 0.0;
      for (int32_t s = 0; s < n_seg; ++s) {
        const int64_t slot = od_record(e, jb, s, nb, n_seg);
        if (slot < 0 || slot + kOdRecord > n_orec) {
          ++cnt[C_REC_OOR];
          continue;
        }
        const double* m = &orec[(size_t)slot];
        int64_t nu;
        std::memcpy(&nu, m + 7, sizeof(int64_t));
        // (the launcher's copy to the caller's layout, and the argument for the test)
        const int64_t to = ((int64_t)e * n_trial + j_first + jb) * n_seg + s;
        if (to < 0 || to >= n_rec) {
          ++cnt[C_REC_OOR];
          continue;
        }
        for (int k = 0; k < 7; ++k) out_mom[(size_t)to * 7 + k] = m[k];
        out_nu[(size_t)to] = nu;
        out_arg[(size_t)to] = od_log_argument(m);
        ++rec_seen[(size_t)to];
        if (!od_enters(keep[(size_t)s], nu)) continue;
        ll = dt_add(ll, od_loglike(nu, std::log(od_log_argument(m))));
        chi2 = dt_add(chi2, m[6]);
        scaled = dt_add(scaled, od_chi2_scaled(m));
        count = dt_add(count, (double)nu);
      }
      const int64_t ta = od_total(e, j_first + jb, n_trial);
      if (ta < 0 || ta + kOdTotals > n_tot) {
        ++cnt[C_TOT_OOR];
        continue;
      }
      tot[(size_t)ta] = ll;
      tot[(size_t)ta + 1] = chi2;
      tot[(size_t)ta + 2] = scaled;
      tot[(size_t)ta + 3] = count;
      ++tot_seen[(size_t)(ta / kOdTotals)];
    }
  }
  for (int32_t w : rec_seen)
    if (w != 1) ++cnt[C_VISIT_ERR];
  for (int32_t w : tot_seen)
    if (w != 1) ++cnt[C_VISIT_ERR];

  FILE* o = std::fopen(argv[2], "w");
  if (!o) return 2;
  for (int64_t i = 0; i < n_rec; ++i) {
    for (int k = 0; k < 7; ++k) std::fprintf(o, "%a ", out_mom[(size_t)i * 7 + k]);
    std::fprintf(o, "%lld %a\n", (long long)out_nu[(size_t)i], out_arg[(size_t)i]);
  }
  for (int64_t i = 0; i < (int64_t)n_exp * n_trial; ++i)
    std::fprintf(o, "%a %a %a %a\n", tot[(size_t)i * 4], tot[(size_t)i * 4 + 1], tot[(size_t)i * 4 + 2],
                 tot[(size_t)i * 4 + 3]);
  std::fclose(o);

  std::printf("tile=%d trials=%d", kOdTile, kOdTrials);
  bool bad = false;
  for (int i = 0; i < C_COUNT; ++i) {
    std::printf(" %s=%lld", kNames[i], (long long)cnt[i]);
    if (i >= C_PERM_OOR && cnt[i] != 0) bad = true;
  }
  std::printf("\n");
  return bad ? 1 : 0;
}
