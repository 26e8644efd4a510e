// Velocity maps on the device (prom_vmap_set / prom_transit_vmap / prom_spectrum_vmap): the observation's model
// spectrum M in every trial frame F[o][j] and, per (phase, trial), the seven inverse-variance weighted moments of M
// against the data and the number of used pixels.  Definitions in prom_hip.h.
//
//   k_vmap         part[o][j][chunk] = {m0 .. m6, n_used} over the chunk's pixels
//   k_vmap_reduce  mom[o][j][0..6], n_used[o][j] = the chunks' records added in chunk order
//
// k_vmap: a workgroup takes one phase, kVmChunk consecutive tiles of kVmTile pixels and kVmTrials consecutive trials;
// thread r * kVmTile + t belongs to (trial r, pixel t) of the current tile.  Per tile:
//   1. 4 * kVmTile threads search the whole grid for both ends of every pixel at the group's smallest and largest
//      factor; then every thread finds its own (pixel, trial)'s ends inside that bracket (vmap_index.h) and trims
//      them with obs_trim, the arbiter of a support;
//   2. the union of the supports that fit, from the lowest on and kVmStage points at most, is staged once for all
//      trials of the group (wav, q and the phase's row of R, read coalesced along w);
//   3. kVmLanes lanes take a (pixel, trial): they stride over the support's points, g q is computed once per point,
//      num and den are reduced by a butterfly of fixed shape inside the kVmLanes lanes.  A support not wholly inside
//      the stage reads the global arrays at the same indices in the same order, so the sums are the same bit for bit;
//   4. thread (r, t) forms M, the used test and the seven terms of its pixel; a butterfly of fixed shape over the
//      kVmTile lanes of trial r adds them (unused pixels and the tile's tail add +0), and lane t = 0 adds the tile's
//      sums to its registers in tile order.
// A trial's numbers depend on the spectrum, the observation and its factor only: not on its position in the group,
// the other trials (they move the stage and the brackets, which change no value) or the batch.  No atomics.
#include "prom_internal.h"
#include "vmap_index.h"

namespace prom {

static_assert(kVmTile == 32 && kVmTile * kVmTrials == kVmBlock, "one thread per (pixel, trial) of a tile");
static_assert(kVmBlock % 64 == 0 && 64 % kVmTile == 0 && 64 % kVmLanes == 0 && (kVmLanes & (kVmLanes - 1)) == 0,
              "the butterflies stay inside a wave");
static_assert((kVmTile * kVmTrials) % (kVmBlock / kVmLanes) == 0 && kVmTile % (kVmBlock / kVmLanes) == 0,
              "every lane group makes the same number of steps");
static_assert(4 * kVmTile <= kVmBlock, "the bracket searches of a tile fit one pass of the workgroup");

__global__ void __launch_bounds__(kVmBlock) k_vmap(const double* __restrict__ wav, const double* __restrict__ q,
                                                    const double* __restrict__ R, int32_t n_wav,
                                                    const double* __restrict__ lam, const double* __restrict__ sig,
                                                    double k, const double* __restrict__ data,
                                                    const double* __restrict__ ivar, const double* __restrict__ F,
                                                    int32_t n_pix, int32_t n_trial, int32_t j_first, int32_t nb,
                                                    int32_t n_chunks, double* __restrict__ part) {
  __shared__ double sW[kVmStage], sQ[kVmStage], sR[kVmStage];
  __shared__ double sL[kVmBlock], sS[kVmBlock], sM[kVmBlock], sD[kVmBlock];
  __shared__ int32_t sA[kVmBlock], sB[kVmBlock];
  __shared__ double sX[4][kVmTile], sF[kVmTrials];
  __shared__ int32_t sI[4][kVmTile], sVa[kVmBlock / 64], sVb[kVmBlock / 64];
  const int32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t o = blockIdx.y;
  const int32_t chunk = vm_wg_chunk(blockIdx.x, n_chunks), gb = vm_wg_group(blockIdx.x, n_chunks);
  const int32_t jb0 = vm_group_first(gb);                    // first trial of the group inside the batch
  const int32_t nt = nb - jb0 < kVmTrials ? nb - jb0 : kVmTrials;
  if (tid < kVmTrials) sF[tid] = tid < nt ? F[(int64_t)o * n_trial + j_first + jb0 + tid] : 1.0;
  __syncthreads();
  int32_t rmin, rmax;
  vm_extremes(sF, nt, &rmin, &rmax);
  const int32_t r = vm_entry_trial(tid), t = vm_entry_pixel(tid);
  const double Fr = sF[r];
  const double* __restrict__ Rrow = R + (int64_t)o * n_wav;
  double acc[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) acc[i] = 0.0;
  int64_t cnt = 0;
  const int32_t tile0 = vm_chunk_first(chunk), ntile = vm_chunk_count(chunk, n_pix);
  for (int32_t ti = 0; ti < ntile; ++ti) {
    const int32_t p0 = vm_tile_first(tile0 + ti), np = vm_tile_count(tile0 + ti, n_pix);
    // 1a. both ends of every pixel at the group's extreme factors, over the whole grid
    if (tid < 4 * kVmTile) {
      const int32_t tt = tid % kVmTile, which = tid / kVmTile;
      const bool upper = (which & 1) != 0;
      double x = 0.0;
      int32_t v = 0;
      if (tt < np) {
        const ObsPix px = obs_pixel(lam[p0 + tt], sig[p0 + tt], k, sF[which < 2 ? rmin : rmax]);
        x = obs_target(px, upper);
        v = obs_bound(wav, n_wav, x, upper);
      }
      sX[which][tt] = x;
      sI[which][tt] = v;
    }
    __syncthreads();
    // 1b. this thread's (pixel, trial): the ends inside the bracket, then the arbiter
    int32_t a = 0, b = 0;
    ObsPix px{0.0, 1.0, 0.0};
    const bool live = r < nt && t < np;
    if (live) {
      px = obs_pixel(lam[p0 + t], sig[p0 + t], k, Fr);
      a = vm_bound(wav, n_wav, obs_target(px, false), false, sX[0][t], sX[2][t], sI[0][t], sI[2][t]);
      b = vm_bound(wav, n_wav, obs_target(px, true), true, sX[1][t], sX[3][t], sI[1][t], sI[3][t]);
      obs_trim(wav, n_wav, px.L, px.c, &a, &b);
    }
    sA[tid] = a;
    sB[tid] = b;
    sL[tid] = px.L;
    sS[tid] = px.S;
    int32_t va = vm_vote_a(a, b, kVmStage), vb = vm_vote_b(a, b, kVmStage);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const int32_t oa = __shfl_xor(va, m, 64), ob = __shfl_xor(vb, m, 64);
      va = oa < va ? oa : va;
      vb = ob > vb ? ob : vb;
    }
    if (lane == 0) {
      sVa[wave] = va;
      sVb[wave] = vb;
    }
    __syncthreads();
    // 2. the stage, once for all trials of the group
    va = sVa[0];
    vb = sVb[0];
#pragma unroll
    for (int i = 1; i < kVmBlock / 64; ++i) {
      va = sVa[i] < va ? sVa[i] : va;
      vb = sVb[i] > vb ? sVb[i] : vb;
    }
    int32_t s0, s1;
    vm_stage(va != INT32_MAX, va, vb, kVmStage, &s0, &s1);
    const int32_t ns = s1 - s0;
    for (int32_t i = tid; i < ns; i += kVmBlock) {
      sW[i] = wav[s0 + i];
      sQ[i] = q[s0 + i];
      sR[i] = Rrow[s0 + i];
    }
    __syncthreads();
    // 3. num and den of every (pixel, trial): kVmLanes lanes each
    const int32_t grp = tid / kVmLanes, l = tid % kVmLanes;
    for (int32_t e = grp; e < nt * kVmTile; e += kVmBlock / kVmLanes) {
      const int32_t ea = sA[e], eb = sB[e];
      const double L = sL[e], S = sS[e];
      const bool staged = obs_staged(ea, eb, s0, s1);
      const int32_t passes = vm_passes(ea, eb);
      double dn = 0.0, nm = 0.0;
      for (int32_t it = 0; it < passes; ++it) {
        const int32_t w = vm_point(ea, it, l);
        if (w >= eb) continue;
        double x, qq, rr;
        if (staged) {
          const int32_t i = w - s0;
          x = sW[i];
          qq = sQ[i];
          rr = sR[i];
        } else {
          x = wav[w];
          qq = q[w];
          rr = Rrow[w];
        }
        const double z = (x - L) / S;
        const double gq = exp(-0.5 * z * z) * qq;
        dn += gq;
        nm += gq * rr;
      }
#pragma unroll
      for (int m = 1; m < kVmLanes; m <<= 1) {
        dn += __shfl_xor(dn, m, 64);
        nm += __shfl_xor(nm, m, 64);
      }
      if (l == 0) {
        sD[e] = dn;
        sM[e] = nm / dn;   // (den == 0: not used below)
      }
    }
    __syncthreads();
    // 4. the terms of this thread's pixel, added over the tile's pixels in a fixed shape
    double tm[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) tm[i] = 0.0;
    int32_t c = 0;
    if (live) {
      const int64_t at = (int64_t)o * n_pix + p0 + t;
      const double iv = ivar[at], d = data[at], dn = sD[tid];
      if (iv > 0.0 && iv < __builtin_inf() && __builtin_fabs(d) < __builtin_inf() && dn > 0.0) {
        const double M = sM[tid];
        const double ivM = iv * M, ivd = iv * d, df = M - d;
        tm[0] = iv;
        tm[1] = ivM;
        tm[2] = ivd;
        tm[3] = ivM * M;
        tm[4] = ivM * d;
        tm[5] = ivd * d;
        tm[6] = iv * (df * df);
        c = 1;
      }
    }
#pragma unroll
    for (int m = 1; m < kVmTile; m <<= 1) {
#pragma unroll
      for (int i = 0; i < 7; ++i) tm[i] += __shfl_xor(tm[i], m, 64);
      c += __shfl_xor(c, m, 64);
    }
    if (t == 0) {
#pragma unroll
      for (int i = 0; i < 7; ++i) acc[i] += tm[i];
      cnt += c;
    }
  }
  if (t == 0 && r < nt) {
    const int64_t slot = vm_part_slot(o, jb0 + r, chunk, nb, n_chunks);
#pragma unroll
    for (int i = 0; i < 7; ++i) part[slot + i] = acc[i];
    reinterpret_cast<int64_t*>(part)[slot + 7] = cnt;
  }
}

// One thread per (phase, trial of the batch, field): the chunks' records in chunk order
__global__ void __launch_bounds__(kVmBlock) k_vmap_reduce(const double* __restrict__ part, int32_t n_orb, int32_t n_trial,
                                                           int32_t j_first, int32_t nb, int32_t n_chunks,
                                                           double* __restrict__ mom, int64_t* __restrict__ n_used) {
  const int64_t i = (int64_t)blockIdx.x * kVmBlock + threadIdx.x;
  if (i >= (int64_t)n_orb * nb * kVmRecord) return;
  const int32_t m = (int32_t)(i % kVmRecord);
  const int64_t oj = i / kVmRecord;
  const int32_t o = (int32_t)(oj / nb), jb = (int32_t)(oj % nb);
  const int64_t out = (int64_t)o * n_trial + j_first + jb;
  if (m < 7) {
    double s = 0.0;
    for (int32_t ch = 0; ch < n_chunks; ++ch) s += part[vm_part_slot(o, jb, ch, nb, n_chunks) + m];
    mom[out * 7 + m] = s;
  } else {
    int64_t s = 0;
    for (int32_t ch = 0; ch < n_chunks; ++ch)
      s += reinterpret_cast<const int64_t*>(part)[vm_part_slot(o, jb, ch, nb, n_chunks) + 7];
    n_used[out] = s;
  }
}

void launch_vmap(hipStream_t s, const double* wav, const double* q, const double* R, int32_t n_wav, const double* lam,
                 const double* sig, double k, const double* data, const double* ivar, const double* F, int32_t n_pix,
                 int32_t n_orb, int32_t n_trial, int32_t j_first, int32_t nb, double* part, hipEvent_t ev0,
                 hipEvent_t ev1) {
  if (n_pix <= 0 || n_orb <= 0 || nb <= 0) return;
  const int32_t n_chunks = vm_chunks(n_pix);
  const dim3 grid((uint32_t)(vm_groups(nb) * n_chunks), (uint32_t)n_orb);
  if (ev0) PROM_HIP(hipEventRecord(ev0, s));
  hipLaunchKernelGGL(k_vmap, grid, dim3(kVmBlock), 0, s, wav, q, R, n_wav, lam, sig, k, data, ivar, F, n_pix, n_trial,
                     j_first, nb, n_chunks, part);
  PROM_HIP(hipGetLastError());
  if (ev1) PROM_HIP(hipEventRecord(ev1, s));
}

void launch_vmap_reduce(hipStream_t s, const double* part, int32_t n_pix, int32_t n_orb, int32_t n_trial,
                        int32_t j_first, int32_t nb, double* mom, int64_t* n_used) {
  if (n_pix <= 0 || n_orb <= 0 || nb <= 0) return;
  const int64_t n = (int64_t)n_orb * nb * kVmRecord;
  hipLaunchKernelGGL(k_vmap_reduce, dim3((uint32_t)((n + kVmBlock - 1) / kVmBlock)), dim3(kVmBlock), 0, s, part, n_orb,
                     n_trial, j_first, nb, vm_chunks(n_pix), mom, n_used);
  PROM_HIP(hipGetLastError());
}

}  // namespace prom
