// The host arithmetic of prom_transit_set that the kernels trust without checking (pure host code, per set; declared in
// prom_internal.h, tested on the host by tests/test_segments_cpu.py through tests/helpers/segments_host.cpp): the
// sigma segments of the Doppler rows with their bucket directories and oversize-block lists (k_sigma_rows,
// k_sigma_poly, k_sigma_tc, k_sigma_tw), the mirror pairs of the chords (k_mol_list), the star table's node slices
// per wavelength tile (k_tau_rm), the polynomial degree of the sigma rows and the rule that says which built-in
// densities p[0] bounds.  No context, no device call, no environment: the callers' switches are arguments.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <thread>

#include "prom_internal.h"

namespace prom {

namespace {

// numpy's bracket of v: the largest j <= n - 2 with X[j] <= v (0 below)
int64_t bracket(const std::vector<double>& X, double v) {
  const int64_t n = (int64_t)X.size();
  int64_t j = (int64_t)(std::upper_bound(X.begin(), X.end(), v) - X.begin()) - 1;
  return j < 0 ? 0 : (j > n - 2 ? n - 2 : j);
}

// the slice [lo, hi] of targets in [tlo, thi] and its linear bracket guess, verified at both ends of every node
// interval (g and numpy's bracket are monotone step functions, and the bracket is constant inside an interval):
// kind 1 (LDS-sized) or 2 with a guess, 0 without; false: no slice
bool make_seg(const std::vector<double>& X, int32_t n_atoms, double tlo, double thi, SigSeg& e) {
  const int64_t lo = bracket(X, tlo);
  const int64_t hi = bracket(X, thi) + 1;
  const int64_t m = hi - lo + 1;
  if (m < 2 || m > INT32_MAX / 2) return false;
  e.lo = (int32_t)lo;
  e.m = (int32_t)m;
  const double xs = X[lo], span = X[hi] - X[lo];
  const double inv = span > 0.0 ? (double)(m - 1) / span : 0.0;
  const double b0 = -(xs * inv);
  bool lin = span > 0.0 && std::isfinite(inv) && std::isfinite(b0);
  auto guess = [&](double v) -> int64_t {
    const double f = std::fma(v, inv, b0);   // the device's seg_guess
    return f < 0.0 ? 0 : (f >= (double)(m - 2) ? m - 2 : (int64_t)f);
  };
  for (int64_t i = lo; lin && i < hi; ++i) {
    if (X[i] == X[i + 1]) continue;
    const double a = std::max(X[i], tlo), z = std::nextafter(X[i + 1], -INFINITY);
    if (a > z) continue;
    const int64_t k = i - lo;   // numpy's bracket on [X[i], X[i+1]) (i <= hi - 1 <= n - 2)
    const int64_t ga = guess(a), gz = guess(z);
    if (ga < k - 1 || ga > k + 1 || gz < k - 1 || gz > k + 1) lin = false;
  }
  e.kind = 0;
  if (lin) {
    e.kind = (m <= kSigSeg ? 1 : 2) | (m <= tc_slice_cap(n_atoms) ? 64 : 0);
    e.xs = b0;
    e.inv = inv;
  }
  return true;
}

}  // namespace

bool factor_range(const double* v, int64_t n, double& smin, double& smax) {
  smin = INFINITY;
  smax = -INFINITY;
  bool ok = true;
  for (int64_t i = 0; i < n; ++i) {
    if (!(v[i] > 0.0) || !std::isfinite(v[i])) ok = false;
    smin = std::min(smin, v[i]);
    smax = std::max(smax, v[i]);
  }
  return ok;
}

// Per 256-wavelength block and atomic slot, nodes [lo, hi] with X[lo] <= fl(s_min lambda_first) and
// fl(s_max lambda_last) < X[hi] (numpy's bracket j of a target: the largest j <= n-2 with X[j] <= t), and a linear
// bracket guess verified over the slice.
bool build_sigma_segments(const double* wav, int64_t n_wav, const std::vector<const std::vector<double>*>& tabs,
                          const std::vector<const double*>& shift, int64_t n_orb, bool use_dir, bool no_guess,
                          SigmaSegments& out) {
  const int32_t n_atoms = (int32_t)tabs.size();
  if (n_atoms < 1 || n_atoms > 4) return false;
  const int64_t nb = (n_wav + kSigBlockW - 1) / kSigBlockW;
  std::vector<SigSeg>& seg = out.seg;
  std::vector<SigSeg>& seg4 = out.seg4;   // per wavefront
  seg.assign(nb * n_atoms, SigSeg{0, 0, 0, 0, 0.0, 0.0});
  seg4.assign(nb * n_atoms * 4, SigSeg{0, 0, 0, 0, 0.0, 0.0});
  // bucket directories of blocks without a linear guess (their SigSeg appended to seg4 at the end, the buckets in
  // sdir); use_dir false turns them off, for comparisons
  std::vector<SigSeg> segr;
  std::vector<int32_t>& sdir = out.sdir;
  sdir.clear();
  std::mutex segr_mu;
  for (int32_t ia = 0; ia < n_atoms; ++ia) {
    const std::vector<double>& X = *tabs[ia];   // (the host copy of the table's nodes: its size is the table's n)
    const double* sh = shift[ia];
    const int64_t n = (int64_t)X.size();
    double smin, smax;
    const bool ok = factor_range(sh, n_orb, smin, smax) && n >= 2;
    auto blocks = [&](int64_t b0, int64_t b1) {
      for (int64_t b = b0; ok && b < b1; ++b) {
        double lmin = INFINITY, lmax = -INFINITY;
        bool fin = true;
        for (int64_t w = b * kSigBlockW; w < std::min<int64_t>(n_wav, (b + 1) * kSigBlockW); ++w) {
          const double l = wav[w];
          if (!(l > 0.0) || !std::isfinite(l)) fin = false;
          lmin = std::min(lmin, l);
          lmax = std::max(lmax, l);
        }
        if (!fin) continue;
        const double tlo = smin * lmin, thi = smax * lmax;
        // every target inside [x_0, x_{n-1}): no clamp or end rule
        if (!(tlo >= X[0] && thi < X[n - 1])) continue;
        SigSeg& e = seg[b * n_atoms + ia];
        if (!make_seg(X, n_atoms, tlo, thi, e)) continue;
        if ((e.kind & 3) != 0) continue;
        // no guess over the block: one per wavefront of 64 wavelengths (oversize blocks read global records per
        // wavefront, so each wave may take its own slice and guess); m = 0: none for that wave
        bool any = false;
        for (int q = 0; q < kSigBlockW / 64; ++q) {
          double wl = INFINITY, wh = -INFINITY;
          const int64_t w0 = b * kSigBlockW + 64 * q;
          for (int64_t w = w0; w < std::min<int64_t>(n_wav, w0 + 64); ++w) {
            wl = std::min(wl, wav[w]);
            wh = std::max(wh, wav[w]);
          }
          SigSeg& ew = seg4[(b * n_atoms + ia) * 4 + q];
          if (wl <= wh && make_seg(X, n_atoms, smin * wl, smax * wh, ew) && (ew.kind & 3) != 0) {
            ew.kind = 2;   // (read from the global records; never k_seg_exact's exact mark, never LDS)
            any = true;
          } else {
            ew = SigSeg{0, 0, 0, 0, 0.0, 0.0};
          }
        }
        if (any) e.kind |= 8;
        // a slice whose node spacing varies too much for one linear guess: a bucket directory over the slice (B
        // uniform buckets, bucket j -> numpy's bracket at its start), verified within one node of numpy's bracket at
        // every target of the block; B = 4, 16, ..., 1024 times the slice's nodes (kind & 32; pad = its SigSeg in seg4
        // past the per-wavefront entries, whose pad is the directory's offset in sdir)
        if (!use_dir) continue;
        const int64_t lo = e.lo, m = e.m, hi = lo + m - 1;
        const double x0 = X[lo], span = X[hi] - X[lo];
        if (!(span > 0.0)) continue;
        std::vector<int32_t> dv;
        SigSeg de{(int32_t)lo, 0, 32, 0, 0.0, 0.0};
        bool okd = false;
        for (int64_t mult = 4; !okd && mult <= 1024 && m * mult <= (1 << 22); mult *= 4) {
          const int64_t B = m * mult;
          const double inv = (double)B / span, b0 = -(x0 * inv);
          if (!std::isfinite(inv) || !std::isfinite(b0)) break;
          dv.assign(B, 0);
          // bucket j starts at x0 + j span / B: the bracket there, by one sweep over the slice's nodes
          int64_t k = 0;
          for (int64_t j = 0; j < B; ++j) {
            const double v = x0 + span * ((double)j / (double)B);
            while (k < m - 2 && X[lo + k + 1] <= v) ++k;
            dv[j] = (int32_t)k;
          }
          auto gd = [&](double v) -> int64_t {
            const double f = std::fma(v, inv, b0);   // the device's seg_guess with m = B + 1
            const int64_t j = f < 0.0 ? 0 : (f >= (double)(B - 1) ? B - 1 : (int64_t)f);
            return dv[j];
          };
          // verified at the block's actual targets (every row's factor times every wavelength, the kernel's clamped
          // rows and lanes among them; the same products as the kernel's tt[]), so node intervals no target falls in
          // (near-coincident nodes) do not matter
          okd = true;
          for (int64_t o = 0; okd && o < n_orb; ++o) {
            const double v = sh[o];
            for (int64_t w = b * kSigBlockW; okd && w < (b + 1) * kSigBlockW; ++w) {
              const double tt = v * wav[std::min<int64_t>(w, n_wav - 1)];
              const int64_t kk = bracket(X, tt) - lo, g = gd(tt);
              if (kk < 0 || kk > m - 2 || g < kk - 1 || g > kk + 1) okd = false;
            }
          }
          if (okd) {
            de.m = (int32_t)(B + 1);
            de.xs = b0;
            de.inv = inv;
          }
        }
        if (okd) {
          std::lock_guard<std::mutex> lk(segr_mu);
          if (sdir.size() + dv.size() > ((size_t)1 << 26)) continue;   // (256 MB of directories at most)
          de.pad = (int32_t)sdir.size();
          e.pad = (int32_t)(seg4.size() + segr.size());
          segr.push_back(de);
          sdir.insert(sdir.end(), dv.begin(), dv.end());
          e.kind |= 32;
        }
      }
    };
    // independent blocks: split over host threads (the guess verification visits every slice node)
    const int64_t n_thr = std::max<int64_t>(1, std::min<int64_t>(8, nb / 64));
    std::vector<std::thread> pool;
    for (int64_t t = 1; t < n_thr; ++t) pool.emplace_back(blocks, nb * t / n_thr, nb * (t + 1) / n_thr);
    blocks(0, nb / n_thr);
    for (auto& th : pool) th.join();
  }
  if (no_guess)
    for (auto& e : seg) e.kind = 0;
  // (block, species) pairs left with neither a linear guess nor a directory (k_sigma_tc's front row split)
  out.noguess = 0;
  for (const auto& e : seg) out.noguess += (e.kind & 3) == 0 && !(e.kind & 32);
  out.n_dir = (int64_t)segr.size();
  seg4.insert(seg4.end(), segr.begin(), segr.end());
  out.fb.clear();
  out.fb_tc.clear();
  for (int64_t b = 0; b < nb; ++b) {
    bool lds = true, ldt = true;
    for (int32_t a = 0; a < n_atoms; ++a) {
      lds = lds && (seg[b * n_atoms + a].kind & ~64) == 1;
      ldt = ldt && (seg[b * n_atoms + a].kind & 64) != 0;
    }
    if (!lds) out.fb.push_back((int32_t)b);
    if (!ldt) out.fb_tc.push_back((int32_t)b);
  }
  return true;
}

// Sorted by y, each unpaired chord with z != 0 takes the first later chord within 1e-9 of (y, -z) (relative to its
// radius); k_mol_list verifies the sample lists before merging anything.
int64_t pair_mirrors(const double* cy, const double* cz, int64_t n_pr, std::vector<int32_t>& mirror) {
  mirror.assign((size_t)n_pr, -1);
  int64_t n_pairs = 0;
  std::vector<int32_t> ord((size_t)n_pr);
  for (int32_t i = 0; i < (int32_t)n_pr; ++i) ord[i] = i;
  std::sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return cy[a] < cy[b] || (cy[a] == cy[b] && a < b); });
  for (size_t a = 0; a < ord.size(); ++a) {
    const int32_t i = ord[a];
    if (mirror[i] >= 0 || !(cz[i] != 0.0) || !std::isfinite(cy[i]) || !std::isfinite(cz[i])) continue;
    const double tol = 1e-9 * std::max(std::fabs(cy[i]), std::fabs(cz[i]));
    for (size_t b = a + 1; b < ord.size() && cy[ord[b]] - cy[i] <= tol; ++b) {
      const int32_t j = ord[b];
      if (mirror[j] < 0 && std::fabs(cz[j] + cz[i]) <= tol) {
        mirror[i] = j;
        mirror[j] = i;
        ++n_pairs;
        break;
      }
    }
  }
  return n_pairs;
}

// s in [s_min, s_max] and IEEE division is monotone, so fl(lambda / s) lies in
// [fl(lambda_min / s_max), fl(lambda_max / s_min)]
std::vector<int32_t> star_slices(const double* wav, int64_t n_wav, const std::vector<double>& X, double s_min,
                                 double s_max) {
  const int64_t n_tiles = (n_wav + 255) / 256;
  std::vector<int32_t> sl(3 * n_tiles, 0);
  const int64_t n = (int64_t)X.size();
  const bool ok = n >= 2 && s_min > 0.0 && std::isfinite(s_max);
  for (int64_t tl = 0; ok && tl < n_tiles; ++tl) {
    double lmin = INFINITY, lmax = -INFINITY;
    bool fin = true;
    for (int64_t w = tl * 256; w < std::min<int64_t>(n_wav, (tl + 1) * 256); ++w) {
      const double l = wav[w];
      if (!std::isfinite(l)) fin = false;
      lmin = std::min(lmin, l);
      lmax = std::max(lmax, l);
    }
    if (!fin) continue;
    const double tlo = lmin / s_max, thi = lmax / s_min;
    const int64_t lo = bracket(X, tlo);
    const int64_t hi = thi >= X[n - 1] ? n - 1 : bracket(X, thi) + 1;
    const int64_t m = hi - lo + 1;
    if (m < 2 || m > kRmStarMax) continue;   // global lookups for this tile
    int32_t P = 1;
    while (P < m) P <<= 1;
    sl[3 * tl] = (int32_t)lo;
    sl[3 * tl + 1] = (int32_t)m;
    sl[3 * tl + 2] = P / 2;
  }
  return sl;
}

int32_t sigma_poly_degree(const double* amax, int32_t n_tables, bool enabled) {
  bool fin = enabled;
  double am = 0.0;
  for (int32_t i = 0; i < n_tables; ++i) {
    if (!(amax[i] == amax[i])) fin = false;
    else am = std::max(am, amax[i]);
  }
  am *= 1.0 + 1e-6;
  for (int D = 4; fin && D <= 14; D += 2) {
    // Lagrange remainder relative to e^a: am^(D+1) / (D+1)! e^|a| (a < 0 carries the e^|a| factor)
    double term = std::exp(am);
    for (int i = 1; i <= D + 1; ++i) term *= am / (double)i;
    if (term <= std::ldexp(1.0, -53)) return D;
  }
  return 0;
}

// A growing power law (q < 0), a negative scale height, a hydrostatic J_0 below J(R) or a negative n_0 would make the
// normalised columns exceed 1 and the windows' envelopes under-estimate tau.
bool density_bounded(int32_t kind, const double* p) {
  bool bounded = p[0] >= 0.0 && std::isfinite(p[0]);
  if (kind == PROM_DENSITY_BAROMETRIC) bounded = bounded && p[2] > 0.0;
  if (kind == PROM_DENSITY_POWERLAW) bounded = bounded && p[2] >= 0.0 && p[1] > 0.0;
  if (kind == PROM_DENSITY_HYDROSTATIC)
    bounded = bounded && p[4] >= 0.0 && p[1] > 0.0 && p[3] != 0.0 && p[4] >= p[2] / (p[3] * p[1]) * (1.0 - 1e-12);
  return bounded;
}

}  // namespace prom
