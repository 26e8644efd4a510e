// Index arithmetic of k_sigma_tw's first pass (prom_tw.hip): which rows a wave runs, a row's chunks of 64
// wavelengths, the wavelength a lane reads for a chunk and the linear guess into a window's slice.
//
// Plain inline functions shared by the kernel and by the host harness of the window planner
// (tests/helpers/window_host.cpp, tests/test_window_plan_cpu.py), which walks every (wave, row, chunk, lane) of a
// plan with the same text and checks every index the kernel would form.
//
// The invariant the dispatch keeps: every chunk that is computed belongs to a row with w0 < w1, so a clamped chunk
// start and the w1 - 1 clamp stay inside the row, the staged offset inside [0, (lw1 - lw0) + 64), and the target
// of every wavelength of the row inside the window's slice (guess >= 0 without a lower clamp).
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PROM_TW_HD __host__ __device__ inline
#else
#define PROM_TW_HD static inline
#endif

namespace prom {

// waves of the workgroup (4) per dispatched unit (a row, or a pair of rows): 4 for one unit, 2 for two or three
PROM_TW_HD int32_t tw_waves_per_unit(int32_t n_units) { return n_units >= 4 ? 1 : (n_units == 1 ? 4 : 2); }

// a row the first pass does not run: past the last row, in the second pass (curve header flags 2 or 4), or without
// wavelengths in the window
PROM_TW_HD bool tw_row_absent(bool past_or_rare, int32_t w0, int32_t w1) { return past_or_rare || w0 >= w1; }

// the rows of a pair that run: 3 both side by side, 1 the first alone, 2 the second alone, 0 neither
PROM_TW_HD int32_t tw_pair_rows(bool absent_a, bool absent_b) { return (absent_a ? 0 : 1) | (absent_b ? 0 : 2); }

// chunks of 64 wavelengths of the row [w0, w1)
PROM_TW_HD int32_t tw_chunks(int32_t w0, int32_t w1) { return (w1 - w0 + 63) >> 6; }

// chunk k's first wavelength (stores only where this + lane < w1)
PROM_TW_HD int32_t tw_chunk_first(int32_t w0, int32_t k) { return w0 + 64 * k; }

// the first wavelength a chunk reads: a chunk past the row's end (the row has fewer chunks than its partner, or a
// prefetched batch runs past the last chunk) is clamped to the row's first chunk; it stores nothing
PROM_TW_HD int32_t tw_chunk_read(int32_t w0, int32_t w1, int32_t k) {
  const int32_t c = tw_chunk_first(w0, k);
  return c < w1 ? c : w0;
}

// staged wavelengths: the lane's offset into the window's stage (wavelengths [lw0, lw1) and 64 entries of padding)
PROM_TW_HD int32_t tw_lam_staged(int32_t w0, int32_t w1, int32_t k, int32_t lane, int32_t lw0) {
  return tw_chunk_read(w0, w1, k) + (lane - lw0);
}

// global wavelengths: the lane's index into the wavelength array (lanes past the row's end read its last one)
PROM_TW_HD int32_t tw_lam_global(int32_t w0, int32_t w1, int32_t k, int32_t lane) {
  const int32_t w = tw_chunk_read(w0, w1, k) + lane;
  return w < w1 ? w : w1 - 1;
}

// the linear guess of a target's bracket in a slice of m nodes, clamped above only: a target at or above the
// slice's first node gives fma(t, inv, xs) > -1, whose integer conversion is >= 0
PROM_TW_HD int32_t tw_guess(double t, double inv, double xs, int32_t m) {
  const int32_t g = (int32_t)__builtin_fma(t, inv, xs);
  return g < m - 2 ? g : m - 2;
}

}  // namespace prom
