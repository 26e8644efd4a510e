// The observation of a spectrum on the device (prom_observe_set / prom_transit_observe / prom_spectrum_observe):
// R[n_orb][n_wav] convolved with a Gaussian line-spread function of per-pixel width, sampled at the detector's
// pixels (per phase in a frame scaled by f[o]), and the chi-square against data.  Definitions in prom_hip.h.
//
//   k_observe_q     the trapezoid weights q_w of the whole grid (the shard's neighbours come in as edges)
//   k_observe       num[o][p] = sum_w g q R, den[o][p] = sum_w g q over each pixel's support
//   k_observe_chi2  per phase: chi2 = sum_used ivar (num / den - data)^2 and the number of used pixels
//
// k_observe: a workgroup takes kObsTile consecutive pixels and a group of phases (kObsPhases when every phase has the
// same frame, else one).  Two lanes per pixel find the ends of the pixel's support (obs_index.h); the union of the
// supports that fit, kObsStage points at most, is staged once in LDS (wav, q and the group's rows of R, read
// coalesced along w).
// A wave then takes a pixel: its lanes stride over the support's points, g q is computed once per point and used
// for every phase of the group, the per-phase sums stay in registers and are reduced across the wave by a butterfly
// of fixed shape.  A pixel whose support is not wholly inside the stage reads the global arrays at the same
// indices in the same order.  No atomics: a result depends on the inputs only.
#include "prom_internal.h"
#include "obs_index.h"

namespace prom {

__global__ void __launch_bounds__(kObsBlock) k_observe_q(const double* __restrict__ wav, int32_t n_wav, double edge_lo,
                                                         double edge_hi, double* __restrict__ q) {
  for (int32_t w = blockIdx.x * kObsBlock + threadIdx.x; w < n_wav; w += gridDim.x * kObsBlock) {
    double lo = w > 0 ? wav[w - 1] : edge_lo, hi = w + 1 < n_wav ? wav[w + 1] : edge_hi;
    if (lo != lo) lo = wav[0];
    if (hi != hi) hi = wav[n_wav - 1];
    q[w] = (hi - lo) / 2.0;
  }
}

static_assert((kObsTile & (kObsTile - 1)) == 0 && 2 * kObsTile <= 64, "one wave searches both ends of a tile's pixels");

__device__ inline double obs_wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ void __launch_bounds__(kObsBlock) k_observe(const double* __restrict__ wav, const double* __restrict__ q,
                                                       const double* __restrict__ R, int32_t n_wav,
                                                       const double* __restrict__ lam, const double* __restrict__ sig,
                                                       const double* __restrict__ f, double k, int32_t n_pix,
                                                       int32_t n_orb, int32_t group, double* __restrict__ num,
                                                       double* __restrict__ den) {
  __shared__ double sW[kObsStage], sQ[kObsStage], sR[kObsPhases][kObsStage];
  __shared__ double sL[kObsTile], sS[kObsTile], sC[kObsTile];
  __shared__ int32_t sA[kObsTile], sB[kObsTile], sRange[2];
  const int32_t tid = threadIdx.x, tile = blockIdx.x;
  const int32_t o0 = blockIdx.y * group;
  const int32_t ng = n_orb - o0 < group ? n_orb - o0 : group;
  const int32_t p0 = obs_tile_first(tile), np = obs_tile_count(tile, n_pix);
  const double fo = f ? f[o0] : 1.0;
  if (tid < 2 * kObsTile) {
    // lanes 0 .. 31 search the pixels' lower ends, lanes 32 .. 63 the upper ends, side by side
    const int32_t j = tid & (kObsTile - 1);
    const bool upper = tid >= kObsTile;
    int32_t v = 0;
    ObsPix x{0.0, 1.0, 0.0};
    if (j < np) {
      x = obs_pixel(lam[p0 + j], sig[p0 + j], k, fo);
      v = obs_bound(wav, n_wav, obs_target(x, upper), upper);
    }
    if (upper) {
      sB[j] = v;
    } else {
      sA[j] = v;
      sL[j] = x.L;
      sS[j] = x.S;
      sC[j] = x.c;
    }
  }
  __syncthreads();
  if (tid < np) obs_trim(wav, n_wav, sL[tid], sC[tid], &sA[tid], &sB[tid]);
  __syncthreads();
  if (tid == 0) obs_stage(sA, sB, np, kObsStage, &sRange[0], &sRange[1]);
  __syncthreads();
  const int32_t s0 = sRange[0], s1 = sRange[1], ns = s1 - s0;
  for (int32_t i = tid; i < ns; i += kObsBlock) {
    sW[i] = wav[s0 + i];
    sQ[i] = q[s0 + i];
  }
  for (int32_t g = 0; g < ng; ++g) {
    const double* r = R + (int64_t)(o0 + g) * n_wav + s0;
    for (int32_t i = tid; i < ns; i += kObsBlock) sR[g][i] = r[i];
  }
  __syncthreads();
  const int32_t wave = tid >> 6, lane = tid & 63;
  for (int32_t j = wave; j < np; j += kObsBlock / 64) {
    const int32_t a = sA[j], b = sB[j];
    const double L = sL[j], S = sS[j];
    const bool staged = obs_staged(a, b, s0, s1);
    const int32_t passes = obs_passes(a, b);
    double dn = 0.0, nm[kObsPhases];
#pragma unroll
    for (int g = 0; g < kObsPhases; ++g) nm[g] = 0.0;
    for (int32_t it = 0; it < passes; ++it) {
      const int32_t w = obs_point(a, it, lane);
      if (w >= b) continue;
      double x, qq, rr[kObsPhases];
      if (staged) {
        const int32_t i = w - s0;
        x = sW[i];
        qq = sQ[i];
#pragma unroll
        for (int g = 0; g < kObsPhases; ++g) rr[g] = g < ng ? sR[g][i] : 0.0;
      } else {
        x = wav[w];
        qq = q[w];
#pragma unroll
        for (int g = 0; g < kObsPhases; ++g) rr[g] = g < ng ? R[(int64_t)(o0 + g) * n_wav + w] : 0.0;
      }
      const double z = (x - L) / S;
      const double gq = exp(-0.5 * z * z) * qq;
      dn += gq;
#pragma unroll
      for (int g = 0; g < kObsPhases; ++g) nm[g] += gq * rr[g];
    }
    dn = obs_wave_sum(dn);
#pragma unroll
    for (int g = 0; g < kObsPhases; ++g) nm[g] = obs_wave_sum(nm[g]);
    if (lane == 0) {
#pragma unroll
      for (int g = 0; g < kObsPhases; ++g)
        if (g < ng) {
          const int64_t at = (int64_t)(o0 + g) * n_pix + p0 + j;
          num[at] = nm[g];
          den[at] = dn;
        }
    }
  }
}

// One workgroup per phase: strided partial sums, then a fixed-order LDS tree (as k_band_stats)
__global__ void __launch_bounds__(kObsBlock) k_observe_chi2(const double* __restrict__ num,
                                                            const double* __restrict__ den,
                                                            const double* __restrict__ data,
                                                            const double* __restrict__ ivar, int32_t n_pix,
                                                            double* __restrict__ chi2, int64_t* __restrict__ n_used) {
  __shared__ double ss[kObsBlock];
  __shared__ int64_t sc[kObsBlock];
  const int64_t o = blockIdx.x;
  double acc = 0.0;
  int64_t cnt = 0;
  for (int32_t p = threadIdx.x; p < n_pix; p += kObsBlock) {
    const int64_t at = o * n_pix + p;
    const double iv = ivar[at], d = data[at], dn = den[at];
    const bool used = iv > 0.0 && iv < __builtin_inf() && __builtin_fabs(d) < __builtin_inf() && dn > 0.0;
    if (used) {
      const double r = num[at] / dn - d;
      acc += iv * (r * r);
      ++cnt;
    }
  }
  ss[threadIdx.x] = acc;
  sc[threadIdx.x] = cnt;
  __syncthreads();
  for (int h = kObsBlock / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      ss[threadIdx.x] += ss[threadIdx.x + h];
      sc[threadIdx.x] += sc[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    chi2[o] = ss[0];
    n_used[o] = sc[0];
  }
}

void launch_observe_q(hipStream_t s, const double* wav, int32_t n_wav, double edge_lo, double edge_hi, double* q) {
  if (n_wav <= 0) return;
  const int32_t g = (n_wav + kObsBlock - 1) / kObsBlock;
  hipLaunchKernelGGL(k_observe_q, dim3(g < 4096 ? g : 4096), dim3(kObsBlock), 0, s, wav, n_wav, edge_lo, edge_hi, q);
  PROM_HIP(hipGetLastError());
}

void launch_observe(hipStream_t s, const double* wav, const double* q, const double* R, int32_t n_wav,
                    const double* lam, const double* sig, const double* f, double k, int32_t n_pix, int32_t n_orb,
                    double* num, double* den, hipEvent_t ev0, hipEvent_t ev1) {
  if (n_pix <= 0 || n_orb <= 0) return;
  // a frame factor per phase: every phase has its own supports, one phase per workgroup
  const int32_t group = f ? 1 : kObsPhases;
  const dim3 grid(obs_tiles(n_pix), (n_orb + group - 1) / group);
  if (ev0) PROM_HIP(hipEventRecord(ev0, s));
  hipLaunchKernelGGL(k_observe, grid, dim3(kObsBlock), 0, s, wav, q, R, n_wav, lam, sig, f, k, n_pix, n_orb, group,
                     num, den);
  PROM_HIP(hipGetLastError());
  if (ev1) PROM_HIP(hipEventRecord(ev1, s));
}

void launch_observe_chi2(hipStream_t s, const double* num, const double* den, const double* data, const double* ivar,
                         int32_t n_pix, int32_t n_orb, double* chi2, int64_t* n_used) {
  hipLaunchKernelGGL(k_observe_chi2, dim3(n_orb), dim3(kObsBlock), 0, s, num, den, data, ivar, n_pix, chi2, n_used);
  PROM_HIP(hipGetLastError());
}

}  // namespace prom
