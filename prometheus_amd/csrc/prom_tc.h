// Transmission-curve evaluation shared by the lookup kernels (prom_tcurve.hip: k_tc_build, k_sigma_tc; prom_tw.hip:
// k_sigma_tw).  See prom_tcurve.hip for the curves: R(o, w) = T_o(Y(o, w)), T_o(Y) = tfrac_o + sum_c F_c exp(-N_c Y),
// the sumOverChords disk sum (gasProperties.py:1241-1258) of one effective absorber.
#pragma once
#include "prom_device.h"

namespace prom {

// (kTcEps, the tail threshold of q, its binary exponent kTcExpEps, kTcSat and tc_octaves: tc_phase.h)

// q = Y N_max's binary exponent (q normal and >= 2^-7)
__device__ __forceinline__ int32_t tc_exponent(double q) {
  return (int32_t)((__builtin_bit_cast(unsigned long long, q) >> 52) & 0x7ff) - 1023;
}

// the octave's Chebyshev series at q (normal, inside the table): v = log2 of q's mantissa in [0, 1), Clenshaw in
// u = 2 v - 1 over the 16 coefficients c.  The coefficients come four at a time: the rare octave branch must not
// set the lookup kernels' register peak (all 16 in flight take 32 VGPRs)
__device__ __forceinline__ double tc_clenshaw(double q, const double* __restrict__ c) {
  const double m = __builtin_bit_cast(double, (__builtin_bit_cast(unsigned long long, q) & 0x000fffffffffffffull) |
                                                  0x3ff0000000000000ull);
  const double u = __builtin_fma(2.0, log2(m), -1.0);
  double b1 = 0.0, b2 = 0.0, c0 = 0.0;
#pragma unroll 1
  for (int k0 = kTcD - 4; k0 >= 0; k0 -= 4) {
    const double2 ca = *reinterpret_cast<const double2*>(c + k0), cb = *reinterpret_cast<const double2*>(c + k0 + 2);
    const double cv[4] = {ca.x, ca.y, cb.x, cb.y};
#pragma unroll
    for (int i = 3; i >= 0; --i) {
      if (k0 + i >= 1) {
        const double b0 = __builtin_fma(2.0 * u, b1, cv[i] - b2);
        b2 = b1;
        b1 = b0;
      } else {
        c0 = cv[0];
      }
    }
  }
  return __builtin_fma(u, b1, c0 - b2);
}

// The exact chord sums in chord order with ocml exp: non-finite columns (nf: the reference's order, the NaN pattern --
// tau is NaN for an infinite column where some chi_s sigma_s is not > 0, zr) or beyond a table truncated at the host's
// octave cap (F_out / F_sum weights).  Not inlined and not optimised: inlined, machine LICM hoists ocml exp's constants
// out of the lookup kernels' loops and their register allocation grows by ~10-20 VGPRs for paths that run only in
// pathological cases (k_sigma_tw; k_sigma_tc keeps them inline: there the call's saved registers cost more); the
// operations and their order are the inlined code's (tc_eval, k_sigma_tc), so the sums are bitwise the same.  Each term
// is added with an explicit fma in all three places: left as a * b + c, the unoptimised function fused it and the
// optimised kernels did not (-ffp-contract=off), and the two lookup kernels differed in the last bits beyond a
// truncated table (tests/test_gpu_tc_sweep.py::test_column_kinds_doppler[two-*])
#ifndef PROM_TC_CS_ATTR   // (inlined instead, -DPROM_TC_CS_ATTR=__forceinline__: no scratch, 77 VGPRs, no faster: r06z)
#define PROM_TC_CS_ATTR __noinline__ __attribute__((optnone))
#endif
__device__ PROM_TC_CS_ATTR double tc_chord_sum(double Y, bool nf, bool zr, double fs,
                                                                    const int32_t* __restrict__ fl,
                                                                    const double* __restrict__ nc,
                                                                    const double* __restrict__ fout, int32_t n_pr) {
  const double inv_fs = 1.0 / fs;
  double a = 0.0;
  for (int32_t ci = 0; ci < n_pr; ++ci) {
    if (fl[ci] != 0) continue;
    const double N = nc[ci];
    double tau = N * Y;
    if (nf && zr && !__builtin_isfinite(N)) tau = __builtin_nan("");
    const double e = exp(-tau);
    a = nf ? fma(fout[ci], e, a) : fma(fout[ci] * inv_fs, e, a);   // (ocml's: the builtin is a libcall when unoptimised)
  }
  return a;
}

// T_o(Y) for a phase whose columns are finite (header h, its table rows tabo)
__device__ __forceinline__ double tc_eval(double Y, const double* __restrict__ h, const double* __restrict__ tabo,
                                          const int32_t* __restrict__ fl, const double* __restrict__ nc,
                                          const double* __restrict__ fout, int32_t n_pr, unsigned long long* evals) {
  const double q = Y * h[kTcHNmax];
  const double tf = h[kTcHTfrac];
  if (q < kTcEps) {
    double p = h[kTcHT0 + 5];
#pragma unroll
    for (int e = 4; e >= 0; --e) p = __builtin_fma(p, q, h[kTcHT0 + e]);
    return tf + p;
  }
  const int32_t nact = (int32_t)h[kTcHNact];
  if (!(q == q)) return nact > 0 ? q : tf;   // NaN cross-section: NaN wherever a chord absorbs
  const int32_t L = (int32_t)h[kTcHL];
  const int32_t j = q <= 1.0e300 ? tc_exponent(q) - kTcExpEps : 0x7fffffff;
  if (j < L) return tf + tc_clenshaw(q, tabo + (int64_t)j * kTcD);
  if ((int32_t)h[kTcHFlags] & 1) return tf;   // every chord opaque (tau >= 40)
  // beyond a truncated table: the exact sum over the phase's active chords, in chord order
  const double inv_fs = 1.0 / h[kTcHFsum];
  double a = 0.0;
#pragma unroll 1
  for (int32_t c = 0; c < n_pr; ++c)
    if (fl[c] == 0) a = __builtin_fma(fout[c] * inv_fs, exp(-(nc[c] * Y)), a);
  if (evals) atomicAdd(&evals[threadIdx.x & 63], (unsigned long long)nact);
  return tf + a;
}

// fma(a, b, c) with c wave-uniform in scalar registers: one v_fma_f64 with an SGPR operand.  (Left to itself the
// compiler copies each scalar coefficient into VGPRs -- two v_mov_b32 -- and uses v_fmac: 15 VALU for the tail
// polynomial instead of 7, per point)
__device__ __forceinline__ double fma_s(double a, double b, double c) {
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
  return r;
}

// A row's curve scalars held for all its chunks (k_sigma_tw's first pass): what the q < eps path reads, loaded once
// per row in one batch of scalar loads -- N_max, tfrac and the tail coefficients t_0 .. t_4 in scalar registers, the
// leading coefficient t_5 in a vector pair (fma_s) -- so that path loads nothing per chunk; the rare branches read
// the header h as tc_eval_full does
struct TcRow {
  const double* h;
  const double* tabo;
  double nmax, tf, t[5];
  double t5v;
};

// the header's flags say second pass (2: non-finite columns, 4: truncated at the octave cap), from the double's
// bits: the flags are the double of an integer 0 .. 7, so (flags & 6) != 0 is flags >= 2.0, a compare of its high
// word -- scalar, where the conversion to an integer is a vector instruction and a round trip through a lane
__device__ __forceinline__ bool tc_flags_second_pass(double flags) {
  return (int32_t)(__builtin_bit_cast(unsigned long long, flags) >> 32) >= 0x40000000;
}

// tc_eval_full on a TcRow (the tail polynomial by fma_s: the same operations in the same order, bitwise its result)
__device__ __forceinline__ double tc_eval_full_r(double Y, const TcRow& r) {
  const double q = Y * r.nmax;
  if (q < kTcEps) {
    double p = fma_s(r.t5v, q, r.t[4]);
#pragma unroll
    for (int e = 3; e >= 0; --e) p = fma_s(p, q, r.t[e]);
    return r.tf + p;
  }
  const int32_t nact = (int32_t)r.h[kTcHNact];
  if (!(q == q)) return nact > 0 ? q : r.tf;
  const int32_t L = (int32_t)r.h[kTcHL];
  const int32_t j = q <= 1.0e300 ? tc_exponent(q) - kTcExpEps : 0x7fffffff;
  if (j >= L) return r.tf;
  return r.tf + tc_clenshaw(q, r.tabo + (int64_t)j * kTcD);
}

// tc_eval for a phase whose table covers every q it can reach (curve header flag 4 clear: not truncated at the
// host's octave cap), so the exact per-point sum beyond the table never runs
__device__ __forceinline__ double tc_eval_full(double Y, const double* __restrict__ h, const double* __restrict__ tabo) {
  const double q = Y * h[kTcHNmax];
  const double tf = h[kTcHTfrac];
  if (q < kTcEps) {
    double p = h[kTcHT0 + 5];
#pragma unroll
    for (int e = 4; e >= 0; --e) p = __builtin_fma(p, q, h[kTcHT0 + e]);
    return tf + p;
  }
  const int32_t nact = (int32_t)h[kTcHNact];
  if (!(q == q)) return nact > 0 ? q : tf;
  const int32_t L = (int32_t)h[kTcHL];
  const int32_t j = q <= 1.0e300 ? tc_exponent(q) - kTcExpEps : 0x7fffffff;
  if (j >= L) return tf;   // (every chord opaque: the table's top is 40 N_max / N_min)
  return tf + tc_clenshaw(q, tabo + (int64_t)j * kTcD);
}

}  // namespace prom
