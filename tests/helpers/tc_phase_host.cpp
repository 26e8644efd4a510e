// Host harness of prometheus_amd/csrc/tc_phase.h (tests/test_tc_phase_cpu.py): the octave count and the
// table-extent rule k_tc_build applies to a phase's folded partials, compiled as plain C++ with g++.  Built as a
// shared library for the test; with -DTC_PHASE_MAIN it is a stand-alone program (its own main) that runs the same
// entry points over seeded inputs, for runs under -fsanitize=address,undefined.
#include <stdio.h>

#include "tc_phase.h"

extern "C" {

int32_t tcp_sizeof_part() { return (int32_t)sizeof(prom::TcPart); }
int32_t tcp_octaves(double q) { return prom::tc_octaves(q); }

// out = {fin, L, top_opaque, trunc}
void tcp_extent(double nmax, double nmin, int32_t nact, int32_t nnf, double ybound, int32_t lg, int32_t* out) {
  prom::tc_phase_extent(nmax, nmin, nact, nnf, ybound, lg, &out[0], &out[1], &out[2], &out[3]);
}

}  // extern "C"

#ifdef TC_PHASE_MAIN
int main() {
  unsigned long long s = 12345;
  auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1p-53; };
  long tables = 0, bad = 0;
  for (int it = 0; it < 4000; ++it) {
    const double hi = 1e18 * rnd(), lo = hi * rnd() * rnd();
    int32_t out[4];
    const int32_t lg = 1 + it % 64;
    tcp_extent(it % 11 ? hi : 0.0, lo > 0.0 ? lo : __builtin_inf(), it % 13 ? 1 + it % 2400 : 0, it % 17 ? 0 : 1,
               it % 5 ? 1e-12 * rnd() : 0.0, lg, out);
    tables += out[1] > 0;
    bad += out[1] < 0 || out[1] > lg || (out[0] == 0 && (out[1] | out[2] | out[3]) != 0);
  }
  printf("tc_phase_host: 4000 phases, %ld with a table, %ld outside [0, lg]\n", tables, bad);
  return bad != 0;
}
#endif
