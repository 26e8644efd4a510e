// The stage record of a target window (k_sigma_tw, prom_tw.hip): what every wave of the window's workgroup needs
// to stage the species' slices and the wavelengths into LDS, derived once per set from the finished plan
// (build_target_windows: the window's SigSeg per species and its staged wavelengths [lw0, lw1)) instead of per wave
// from the slices.  64 bytes: one scalar load.
//
// Plain inline functions shared by the host (prom_api_transit.hip: the upload), the kernel and the host harness of
// tests/test_tw_stage_cpu.py, as tw_index.h's.
//
// The pool: staged species (SigSeg kind & 1: kinds 1 and 3) lie in species order, species s at pool entries
// [pad_s, pad_s + m_s) with pad_s the end of the staged species before it (the planner's offsets).  bnd[s] is the
// pool's end after species 0 .. s -- a species without a slice in the pool owns no entry, bnd[s] = bnd[s - 1] -- so
// pool entry i < tot belongs to species #{s < ns - 1 : bnd[s] <= i}, whichever species in between are unstaged.
#pragma once

#include <stdint.h>

#include "tw_index.h"

namespace prom {

enum : int32_t {
  kTwRare = 1,     // some species without a slice in the pool (kinds 0 and 2): the second pass takes the window
  kTwSearch = 2,   // some staged slice without a guess (kind 3): bisection in LDS
  kTwExact = 4     // every species' guess is numpy's bracket at every target (kind & 4 of every species: k_tw_exact)
};

struct TwStage {
  int32_t tot;       // staged nodes (pool entries)
  int32_t lw0;       // first staged wavelength
  int32_t nlam;      // staged wavelengths (0: the rows read them from global memory)
  int32_t mode;      // kTwRare | kTwSearch | kTwExact
  int32_t bnd[4];    // pool end after species 0 .. s (species >= ns: tot)
  int32_t off[4];    // lo_s - pad_s: pool entry i of species s is record lo_s + (i - pad_s) = i + off[s]
  int32_t base[4];   // the slice's LDS bases in doubles from the pool's start, x_0 at the low half (2 tot + pad_s + s),
                     // {E, L}_0 (as double2: pad_s) at the high half; 0 for a species without a slice in the pool
};

// LDS layout of a window with tot pool entries, in doubles: [0, 2 tot) the records {(chi) E_k, L_k} (entry i at 2 i),
// then tot + ns node x's (entry i of species s at 2 tot + i + s and its upper node in the next slot: the species'
// next entry, which holds the same node, or after its last entry the slice's last upper node), then the wavelengths
PROM_TW_HD int32_t tw_lds_x(int32_t tot, int32_t i, int32_t s) { return 2 * tot + i + s; }
PROM_TW_HD int32_t tw_lds_lam(int32_t tot, int32_t ns) { return 3 * tot + ns; }

PROM_TW_HD int32_t tw_stage_xbase(int32_t base) { return base & 0xffff; }
PROM_TW_HD int32_t tw_stage_elbase(int32_t base) { return (int32_t)((uint32_t)base >> 16); }

// the species of pool entry i < tot among ns species
PROM_TW_HD int32_t tw_stage_species(const int32_t* bnd, int32_t ns, int32_t i) {
  int32_t sp = 0;
  for (int32_t s = 0; s + 1 < ns; ++s) sp = i >= bnd[s] ? s + 1 : sp;   // (bnd ascends: the count of bnd[s] <= i)
  return sp;
}

// the record of a window from its ns slices (Seg: SigSeg's lo, m, kind, pad) and staged wavelengths [lw0, lw1)
template <class Seg>
PROM_TW_HD TwStage tw_stage_of(const Seg* sg, int32_t ns, int32_t lw0, int32_t lw1) {
  TwStage st;
  st.tot = 0;
  st.lw0 = lw0;
  st.nlam = lw1 - lw0;
  st.mode = kTwExact;
  for (int32_t s = 0; s < ns; ++s) {
    const int32_t k = sg[s].kind & 3;
    if (k != 1 && k != 3) st.mode |= kTwRare;
    if (k == 3) st.mode |= kTwSearch;
    if (!(sg[s].kind & 4)) st.mode &= ~kTwExact;
    if (sg[s].kind & 1) st.tot = sg[s].pad + sg[s].m > st.tot ? sg[s].pad + sg[s].m : st.tot;
  }
  int32_t end = 0;
  for (int32_t s = 0; s < 4; ++s) {
    const bool staged = s < ns && (sg[s].kind & 1) != 0;
    if (staged) end = sg[s].pad + sg[s].m;
    st.bnd[s] = s < ns ? end : st.tot;
    st.off[s] = staged ? sg[s].lo - sg[s].pad : 0;
    st.base[s] = staged ? (int32_t)(((uint32_t)sg[s].pad << 16) | (uint32_t)tw_lds_x(st.tot, sg[s].pad, s)) : 0;
  }
  return st;
}

}  // namespace prom
