// Host harness of the target windows' stage records, for CPU tests only (tests/test_tw_stage_cpu.py).
//
// Compiled as C++ with g++ against prometheus_amd/csrc/tw_stage.h, the very text prom_api_transit.hip (the upload) and
// k_sigma_tw (the staging prologue) compile: tw_stage_records derives the records of a plan as prom_transit_set does,
// tw_stage_entries walks every pool entry of every window the way the prologue does -- its species from the
// record's boundaries, its table record, the LDS slots of its node x and of its {E, L} -- and tw_stage_bases
// unpacks the first pass' lookup bases.
#include <cstdint>

#include "prom_internal.h"
#include "tw_stage.h"

extern "C" {

int32_t tw_stage_sizeof() { return (int32_t)sizeof(prom::TwStage); }

// seg: n_win x ns SigSeg; lam: n_win x {lw0, lw1}; out: n_win records
void tw_stage_records(const void* seg, const int32_t* lam, int32_t n_win, int32_t ns, void* out) {
  const prom::SigSeg* sg = static_cast<const prom::SigSeg*>(seg);
  prom::TwStage* st = static_cast<prom::TwStage*>(out);
  for (int32_t b = 0; b < n_win; ++b) st[b] = prom::tw_stage_of(sg + (int64_t)b * ns, ns, lam[2 * b], lam[2 * b + 1]);
}

// every pool entry i < tot of every window, concatenated (the caller sizes the outputs by the records' tot): its
// species, its table record i + off[species], the LDS slot (in doubles) of its node x and of its {E, L} pair
void tw_stage_entries(const void* recs, int32_t n_win, int32_t ns, int32_t* species, int32_t* rec, int32_t* x_slot,
                      int32_t* el_slot) {
  const prom::TwStage* st = static_cast<const prom::TwStage*>(recs);
  int64_t n = 0;
  for (int32_t b = 0; b < n_win; ++b)
    for (int32_t i = 0; i < st[b].tot; ++i, ++n) {
      const int32_t sp = prom::tw_stage_species(st[b].bnd, ns, i);
      species[n] = sp;
      rec[n] = i + st[b].off[sp];
      x_slot[n] = prom::tw_lds_x(st[b].tot, i, sp);
      el_slot[n] = 2 * i;
    }
}

// the first pass' lookup bases of every window and species, in doubles: node k of species s at x[b][s] + k, its
// {E, L} pair at el[b][s] + 2 k; lam[b]: the first staged wavelength's slot
void tw_stage_bases(const void* recs, int32_t n_win, int32_t ns, int32_t* x, int32_t* el, int32_t* lam) {
  const prom::TwStage* st = static_cast<const prom::TwStage*>(recs);
  for (int32_t b = 0; b < n_win; ++b) {
    for (int32_t s = 0; s < ns; ++s) {
      x[(int64_t)b * ns + s] = prom::tw_stage_xbase(st[b].base[s]);
      el[(int64_t)b * ns + s] = 2 * prom::tw_stage_elbase(st[b].base[s]);
    }
    lam[b] = prom::tw_lds_lam(st[b].tot, ns);
  }
}

}  // extern "C"
