// Per-phase quantities of the transmission-curve path that k_tc_build (prom_tcurve.hip) fixes before its node sums:
// the phase partials k_columns8 writes per 32 chords (prom_transit.hip) and the rule that turns a phase's folded
// partials into its curve table's extent.
//
// Plain inline functions shared by the kernel and by the host harness tests/helpers/tc_phase_host.cpp
// (tests/test_tc_phase_cpu.py), the way tw_index.h serves k_sigma_tw.  The rule works on a maximum, a minimum and
// integer counts and yields integers: the host test compares it exactly.
#pragma once

#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PROM_TCP_HD __host__ __device__ inline
#else
#define PROM_TCP_HD static inline
#endif

namespace prom {

// Per 32-chord group of one phase (k_columns8, transmission-curve path): the order-independent phase sums
// k_tc_build needs before its node sums (max / min of the active finite columns, chord counts by class)
struct TcPart {
  double nmax, nmin;
  int32_t nact, ntr, nbl, nnf;
};

constexpr double kTcEps = 0x1p-7;        // tail threshold of q
constexpr int kTcExpEps = -7;            // its binary exponent
constexpr double kTcSat = 40.0;          // tau above which a chord is opaque (e^-40 = 4e-18)

// octaves [0, L) that cover q in [eps, qhi]: 0 when qhi < eps, INT32_MAX when not finite
PROM_TCP_HD int32_t tc_octaves(double qhi) {
  if (!(qhi >= kTcEps)) return 0;
  if (!(qhi <= 1.0e300)) return 0x7fffffff;
  unsigned long long u;
  memcpy(&u, &qhi, sizeof(u));
  return ((int32_t)((u >> 52) & 0x7ff) - 1023) - kTcExpEps + 1;
}

// Table extent of a phase: octaves up to the host's bound of q = Y N_max (ybound = the bound of Y), or up to
// q = 40 N_max / N_min (every chord opaque beyond it), whichever comes first; lg caps it.  A phase with a non-finite
// active column, without active chords or with N_max = 0 has no table (fin = 0, L = 0).
PROM_TCP_HD void tc_phase_extent(double nmax, double nmin, int32_t nact, int32_t nnf, double ybound, int32_t lg,
                                 int32_t* fin, int32_t* L, int32_t* top_opaque, int32_t* trunc) {
  *fin = (nnf == 0 && nmax > 0.0 && nact > 0) ? 1 : 0;
  *L = 0;
  *top_opaque = 0;
  *trunc = 0;
  if (*fin) {
    const int32_t L1 = ybound > 0.0 ? tc_octaves(ybound * nmax * (1.0 + 0x1p-40)) : 0x7fffffff;
    const int32_t L2 = tc_octaves(kTcSat * (nmax / nmin));
    if (L2 <= L1 && L2 <= lg) {
      *L = L2;
      *top_opaque = 1;
    } else {
      *L = L1 < lg ? L1 : lg;
      *trunc = L1 > lg ? 4 : 0;   // (the lookups may need the exact sum beyond the table: header flag 4)
    }
  }
}

}  // namespace prom
