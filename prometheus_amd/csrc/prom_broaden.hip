// Broadened spectra on the device (prom_broaden_set / prom_spectrum_broaden / prom_transit_broaden): R[n_orb][n_wav]
// convolved with a tabulated velocity kernel on the model's own non-uniform wavelength grid,
// R_b[o][w] = sum_w' kern q R[o][w'] / sum_w' kern q over the output's support.  Definitions in prom_hip.h.
//
//   k_observe_q   (prom_observe.hip, unchanged) the trapezoid weights q of the whole grid
//   k_broaden     R_b
//
// k_broaden: a workgroup of kBrBlock threads takes a tile of kBrBlock consecutive outputs and a group of up to
// kBrPhases rows at a time, one group of rows after the other; lane = output.  Two lanes binary-search the global grid
// with the membership predicates themselves (broaden_index.h: they are monotone in w', so no rounded target needs a
// fix-up) for the first output's lower end and the last output's upper end.  When that window holds at most kBrStage
// points, wav and q over it are staged coalesced in LDS next to the kernel's {K, D} records, every lane searches its own
// ends inside the stage, and each end is proven against the grid (br_end_certain: at most one load per end, at the
// window's own ends only).  Should one lane's ends not be proven, or the window not fit, every lane searches the grid and
// the union of the supports (an integer minimum and maximum over the workgroup) is staged when it fits.  The ends, the
// union and the staged wav and q serve every group of rows; the group's rows of R are staged over the same range.
// Each lane then walks its support in ascending w' with num[kBrPhases] and den in registers: the weight kern q is
// formed once per (w, w') and used for every row.  Neighbouring lanes read neighbouring doubles of the
// stage and nearly the same record.  A tile whose union does not fit reads the global arrays at the same indices in
// the same order: the same bits.  There is no cross-lane arithmetic and no atomic; a result depends on wav, its own row
// and the kernel only.  Every loop runs at most n_wav or log2(n_wav) + 1 times.
#include "prom_internal.h"
#include "broaden_index.h"

namespace prom {

// minimum of lo and maximum of hi over the workgroup (integers: the order does not matter)
__device__ inline void br_block_range(int32_t& lo, int32_t& hi, int32_t* sLo, int32_t* sHi, int32_t tid) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const int32_t l2 = __shfl_xor(lo, m, 64), h2 = __shfl_xor(hi, m, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((tid & 63) == 0) {
    sLo[tid >> 6] = lo;
    sHi[tid >> 6] = hi;
  }
  __syncthreads();
#pragma unroll
  for (int v = 0; v < kBrBlock / 64; ++v) {
    lo = sLo[v] < lo ? sLo[v] : lo;
    hi = sHi[v] > hi ? sHi[v] : hi;
  }
}

__global__ void __launch_bounds__(kBrBlock) k_broaden(const double* __restrict__ wav, const double* __restrict__ q,
                                                      const double* __restrict__ R, int32_t n_wav, int32_t n_orb,
                                                      const BrRec* __restrict__ rec, BrKern kern,
                                                      double* __restrict__ Rb) {
  extern __shared__ double br_lds[];
  double* sW = br_lds;
  double* sQ = sW + kBrStage;
  double* sR = sQ + kBrStage;                                             // [kBrPhases][kBrStage]
  BrRec* sK = reinterpret_cast<BrRec*>(sR + kBrPhases * kBrStage);        // [n_k]
  __shared__ int32_t sLo[kBrBlock / 64], sHi[kBrBlock / 64], sWin[2];
  const int32_t tid = threadIdx.x, tile = blockIdx.x;
  const int32_t w = br_output(tile, tid);
  for (int32_t i = tid; i < kern.n_k; i += kBrBlock) sK[i] = rec[i];
  double x = 1.0, r = 1.0;
  if (w < n_wav) {
    x = wav[w];
    r = br_r(x);
  }
  // the window: the lower end of the first output and the upper end of the last, two lanes side by side in the grid
  if (tid < 2) {
    const bool upper = tid == 1;
    const double xe = wav[upper ? br_tile_last(tile, n_wav) : br_output(tile, 0)];
    sWin[tid] = br_end(wav, n_wav, xe, br_r(xe), kern, upper);
  }
  __syncthreads();
  int32_t lo = sWin[0], hi = sWin[1], a = 0, b = 0;
  bool staged = false;
  if (br_staged(lo, hi)) {
    for (int32_t i = tid; i < hi - lo; i += kBrBlock) {
      sW[i] = wav[lo + i];
      sQ[i] = q[lo + i];
    }
    __syncthreads();
    // every lane's ends inside the stage, each proven against the grid
    bool sure = true;
    if (w < n_wav) {
      a = br_end_in(sW, lo, lo, hi, x, r, kern, false);
      b = br_end_in(sW, lo, lo, hi, x, r, kern, true);
      sure = br_end_certain(wav, n_wav, lo, hi, a, x, r, kern, false) &&
             br_end_certain(wav, n_wav, lo, hi, b, x, r, kern, true);
    }
    staged = !__syncthreads_or(!sure);
  }
  if (!staged) {
    // every lane searches the grid; the union of the supports is staged when it fits
    a = b = 0;
    if (w < n_wav) {
      a = br_end(wav, n_wav, x, r, kern, false);
      b = br_end(wav, n_wav, x, r, kern, true);
    }
    lo = b > a ? a : 0x7fffffff;
    hi = b > a ? b : 0;
    br_block_range(lo, hi, sLo, sHi, tid);
    staged = br_staged(lo, hi);
    if (staged) {
      for (int32_t i = tid; i < hi - lo; i += kBrBlock) {
        sW[i] = wav[lo + i];
        sQ[i] = q[lo + i];
      }
    }
  }
  // the groups of rows in turn: the ends, the union and the staged wav and q serve all of them
  for (int32_t o0 = 0; o0 < n_orb; o0 += kBrPhases) {
    const int32_t ng = n_orb - o0 < kBrPhases ? n_orb - o0 : kBrPhases;
    const double* Rg = R + (int64_t)o0 * n_wav;
    __syncthreads();   // the group before has read its rows (the first time: wav and q are staged)
    if (staged) {
      for (int32_t g = 0; g < ng; ++g) {
        const double* row = Rg + (int64_t)g * n_wav + lo;
        for (int32_t i = tid; i < hi - lo; i += kBrBlock) sR[g * kBrStage + i] = row[i];
      }
      __syncthreads();
    }
    if (w < n_wav) {
      double num[kBrPhases], den;
      if (staged)
        br_walk(sW, sQ, sR, kBrStage, lo, ng, a, b, x, r, kern, sK, num, den);
      else
        br_walk(wav, q, Rg, n_wav, 0, ng, a, b, x, r, kern, sK, num, den);
#pragma unroll
      for (int g = 0; g < kBrPhases; ++g)
        if (g < ng) Rb[(int64_t)(o0 + g) * n_wav + w] = br_result(num[g], den);
    }
  }
}

void launch_broaden(hipStream_t s, const double* wav, const double* q, const double* R, int32_t n_wav, int32_t n_orb,
                    const BrRec* rec, const BrKern& kern, double* Rb, hipEvent_t ev0, hipEvent_t ev1) {
  if (n_wav <= 0 || n_orb <= 0) return;
  if (kern.n_k < 2 || kern.n_k > kBrMaxNodes) throw Error(PROM_E_ARG, "k_broaden: n_k outside [2, 1025]");
  const dim3 grid(br_tiles(n_wav));
  if (ev0) PROM_HIP(hipEventRecord(ev0, s));
  hipLaunchKernelGGL(k_broaden, grid, dim3(kBrBlock), br_lds_bytes(kern.n_k), s, wav, q, R, n_wav, n_orb, rec, kern, Rb);
  PROM_HIP(hipGetLastError());
  if (ev1) PROM_HIP(hipEventRecord(ev1, s));
}

}  // namespace prom
