// Exposures on the device (prom_expose_set / prom_transit_expose / prom_spectrum_expose): per exposure e and trial j
// the model M_e = sum over the exposure's live taps of fl(a_i M_i), M_i the model spectrum of row row[e][i] of R in
// the frame F[e][j][i], and the seven moments of M_e against the exposure's data.  Definitions in prom_hip.h.
//
//   k_expose        part[e][j][chunk] = {m0 .. m6, n_used} over the chunk's pixels; model[e][j][p] on request
//   k_vmap_reduce   (prom_vmap.hip, with the exposure in the phase's place) the chunks' records added in chunk order
//
// k_expose has k_vmap's shape: a workgroup takes one exposure, kVmChunk consecutive tiles of kVmTile pixels and
// kVmTrials consecutive trials; thread r * kVmTile + t belongs to (trial r, pixel t) of the current tile.  Per tile
// it walks the exposure's taps in ascending order; a dead tap (weight not > 0: a workgroup-uniform test on scalar
// data) is skipped before anything of it is read.  For a live tap it runs k_vmap's steps 1 to 3 with the tap's row
// of R and the group's factors F[e][j][i] (the text below is k_vmap's: the same searches, obs_trim, stage, lane
// groups and butterfly, so M_i is k_vmap's M for the same pixel, row and factor bit for bit); thread (r, t) then adds
// fl(a_i M_i) to its M_e (the first live tap starts the sum) and notes whether den_i > 0.  After the last tap comes
// k_vmap's step 4 with M_e and "every live tap had den > 0" in the place of M and den > 0.
// The numbers of (e, j) depend on the spectrum, the pixels, the exposure's live taps in order and its data only: the
// other trials move the stage and the brackets, which change no value; a dead tap changes no state.  No atomics.
#include "prom_internal.h"
#include "expose_index.h"

namespace prom {

static_assert(kVmTile == 32 && kVmTile * kVmTrials == kVmBlock, "one thread per (pixel, trial) of a tile");
static_assert(kVmBlock % 64 == 0 && 64 % kVmTile == 0 && 64 % kVmLanes == 0 && (kVmLanes & (kVmLanes - 1)) == 0,
              "the butterflies stay inside a wave");
static_assert((kVmTile * kVmTrials) % (kVmBlock / kVmLanes) == 0 && kVmTile % (kVmBlock / kVmLanes) == 0,
              "every lane group makes the same number of steps");
static_assert(4 * kVmTile <= kVmBlock, "the bracket searches of a tile fit one pass of the workgroup");

__global__ void __launch_bounds__(kVmBlock) k_expose(const double* __restrict__ wav, const double* __restrict__ q,
                                                      const double* __restrict__ R, int32_t n_wav,
                                                      const double* __restrict__ lam, const double* __restrict__ sig,
                                                      double k, const int32_t* __restrict__ row,
                                                      const double* __restrict__ wgt, const double* __restrict__ F,
                                                      const double* __restrict__ data, const double* __restrict__ ivar,
                                                      int32_t n_pix, int32_t n_trial, int32_t n_tap, int32_t j_first,
                                                      int32_t nb, int32_t n_chunks, double* __restrict__ part,
                                                      double* __restrict__ model) {
  __shared__ double sW[kVmStage], sQ[kVmStage], sR[kVmStage];
  __shared__ double sL[kVmBlock], sS[kVmBlock], sM[kVmBlock], sD[kVmBlock];
  __shared__ int32_t sA[kVmBlock], sB[kVmBlock];
  __shared__ double sX[4][kVmTile], sF[kVmTrials];
  __shared__ int32_t sI[4][kVmTile], sVa[kVmBlock / 64], sVb[kVmBlock / 64];
  const int32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t e = blockIdx.y;
  const int32_t chunk = vm_wg_chunk(blockIdx.x, n_chunks), gb = vm_wg_group(blockIdx.x, n_chunks);
  const int32_t jb0 = vm_group_first(gb);                    // first trial of the group inside the batch
  const int32_t nt = nb - jb0 < kVmTrials ? nb - jb0 : kVmTrials;
  const int32_t r = vm_entry_trial(tid), t = vm_entry_pixel(tid);
  double acc[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) acc[i] = 0.0;
  int64_t cnt = 0;
  const int32_t tile0 = vm_chunk_first(chunk), ntile = vm_chunk_count(chunk, n_pix);
  for (int32_t ti = 0; ti < ntile; ++ti) {
    const int32_t p0 = vm_tile_first(tile0 + ti), np = vm_tile_count(tile0 + ti, n_pix);
    const bool live = r < nt && t < np;
    double Me = 0.0;        // the exposure's model at this thread's (pixel, trial)
    bool covered = true;    // every live tap so far had den > 0
    bool first = true;      // no live tap yet (workgroup-uniform)
    for (int32_t tap = 0; tap < n_tap; ++tap) {
      const double a_tap = wgt[ex_tap(e, tap, n_tap)];
      if (!ex_live(a_tap)) continue;
      const double* __restrict__ Rrow = R + ex_row_first(row[ex_tap(e, tap, n_tap)], n_wav);
      // 0. the group's factors at this tap (the readers of the last tap's are behind its barriers)
      if (tid < kVmTrials) sF[tid] = tid < nt ? F[ex_factor(e, j_first + jb0 + tid, tap, n_trial, n_tap)] : 1.0;
      __syncthreads();
      int32_t rmin, rmax;
      vm_extremes(sF, nt, &rmin, &rmax);
      const double Fr = sF[r];
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
      for (int32_t en = grp; en < nt * kVmTile; en += kVmBlock / kVmLanes) {
        const int32_t ea = sA[en], eb = sB[en];
        const double L = sL[en], S = sS[en];
        const bool staged = obs_staged(ea, eb, s0, s1);
        const int32_t passes = vm_passes(ea, eb);
        double dn = 0.0, nm = 0.0;
        // (one loop per source: the same points in the same order, so the same sums bit for bit)
        if (staged) {
          for (int32_t it = 0; it < passes; ++it) {
            const int32_t w = vm_point(ea, it, l);
            if (w >= eb) continue;
            const int32_t i = w - s0;
            const double z = (sW[i] - L) / S;
            const double gq = exp(-0.5 * z * z) * sQ[i];
            dn += gq;
            nm += gq * sR[i];
          }
        } else {
          for (int32_t it = 0; it < passes; ++it) {
            const int32_t w = vm_point(ea, it, l);
            if (w >= eb) continue;
            const double z = (wav[w] - L) / S;
            const double gq = exp(-0.5 * z * z) * q[w];
            dn += gq;
            nm += gq * Rrow[w];
          }
        }
#pragma unroll
        for (int m = 1; m < kVmLanes; m <<= 1) {
          dn += __shfl_xor(dn, m, 64);
          nm += __shfl_xor(nm, m, 64);
        }
        if (l == 0) {
          sD[en] = dn;
          sM[en] = nm / dn;   // (den == 0: NaN, and the pixel is not covered)
        }
      }
      __syncthreads();
      // the tap's share of this thread's (pixel, trial)
      if (live) {
        const double am = a_tap * sM[tid];
        Me = first ? am : Me + am;
        covered = covered && sD[tid] > 0.0;
      }
      first = false;
    }
    covered = covered && !first;   // no live tap: no model
    // 4. the terms of this thread's pixel, added over the tile's pixels in a fixed shape
    double tm[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) tm[i] = 0.0;
    int32_t c = 0;
    if (live) {
      const int64_t at = ex_data(e, p0 + t, n_pix);
      const double iv = ivar[at], d = data[at];
      if (model) model[ex_model(e, j_first + jb0 + r, p0 + t, n_trial, n_pix)] = covered ? Me : __builtin_nan("");
      if (iv > 0.0 && iv < __builtin_inf() && __builtin_fabs(d) < __builtin_inf() && covered) {
        const double M = Me;
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
    const int64_t slot = vm_part_slot(e, jb0 + r, chunk, nb, n_chunks);
#pragma unroll
    for (int i = 0; i < 7; ++i) part[slot + i] = acc[i];
    reinterpret_cast<int64_t*>(part)[slot + 7] = cnt;
  }
}

void launch_expose(hipStream_t s, const double* wav, const double* q, const double* R, int32_t n_wav, const double* lam,
                   const double* sig, double k, const int32_t* row, const double* wgt, const double* F,
                   const double* data, const double* ivar, int32_t n_pix, int32_t n_exp, int32_t n_trial, int32_t n_tap,
                   int32_t j_first, int32_t nb, double* part, double* model, hipEvent_t ev0, hipEvent_t ev1) {
  if (n_pix <= 0 || n_exp <= 0 || nb <= 0 || n_tap <= 0) return;
  const int32_t n_chunks = vm_chunks(n_pix);
  const dim3 grid((uint32_t)(vm_groups(nb) * n_chunks), (uint32_t)n_exp);
  if (ev0) PROM_HIP(hipEventRecord(ev0, s));
  hipLaunchKernelGGL(k_expose, grid, dim3(kVmBlock), 0, s, wav, q, R, n_wav, lam, sig, k, row, wgt, F, data, ivar, n_pix,
                     n_trial, n_tap, j_first, nb, n_chunks, part, model);
  PROM_HIP(hipGetLastError());
  if (ev1) PROM_HIP(hipEventRecord(ev1, s));
}

}  // namespace prom
