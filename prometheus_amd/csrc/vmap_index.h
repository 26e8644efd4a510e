// Index arithmetic of k_vmap (prom_vmap.hip): the chunk of pixel tiles and the group of trials a workgroup takes, the
// bracketed searches for a (pixel, trial)'s support, the wavelength range a tile stages in LDS for all trials of the
// group, the points a lane reads and the slot of a partial record.
//
// Plain inline functions shared by the kernel and by the host harness (tests/helpers/vmap_host.cpp,
// tests/test_vmap_cpu.py), which walks every (phase, chunk, tile, trial group, pixel, trial, pass, lane) with the same
// text and checks every index the kernel would form.  A support is obs_index.h's: obs_pixel / obs_target / obs_bound
// give the candidates and obs_trim decides.
//
// The invariants: a support [a, b) lies inside [0, n_wav); the stage [s0, s1) lies inside [0, n_wav) and holds at
// most kVmStage points; a (pixel, trial) reads the stage only when its whole support lies inside it (offsets w - s0
// in [0, s1 - s0)), otherwise it reads the global arrays at w in [a, b); a partial record lies inside the scratch of
// the batch.
//
// The constants can be overridden at compile time (PROM_VM_*): the host harness is also built with small ones.  The
// kernel is built with the defaults only.
#pragma once

#include "obs_index.h"

#ifndef PROM_VM_TILE
#define PROM_VM_TILE ::prom::kObsTile
#endif
#ifndef PROM_VM_STAGE
#define PROM_VM_STAGE 1024
#endif
#ifndef PROM_VM_CHUNK
#define PROM_VM_CHUNK 16
#endif
#ifndef PROM_VM_TRIALS
#define PROM_VM_TRIALS 8
#endif

namespace prom {

constexpr int kVmTile = PROM_VM_TILE;       // pixels per tile (kObsTile)
constexpr int kVmStage = PROM_VM_STAGE;     // wavelengths staged per tile at most (wav, q and one row of R: 24 KB)
constexpr int kVmChunk = PROM_VM_CHUNK;     // consecutive tiles per workgroup
constexpr int kVmTrials = PROM_VM_TRIALS;   // consecutive trials per workgroup
constexpr int kVmBlock = 256;               // threads of a k_vmap workgroup: one per (pixel, trial) of a tile
constexpr int kVmLanes = 16;                // lanes that share a (pixel, trial)'s support
constexpr int kVmRecord = 8;                // doubles of a partial record: m0 .. m6 and n_used (int64 bits)

// ---- the workgroup's share ---------------------------------------------------------------------------------------
PROM_OBS_HD int32_t vm_tiles(int32_t n_pix) { return (n_pix + kVmTile - 1) / kVmTile; }
PROM_OBS_HD int32_t vm_chunks(int32_t n_pix) { return (vm_tiles(n_pix) + kVmChunk - 1) / kVmChunk; }
PROM_OBS_HD int32_t vm_groups(int32_t n_trial) { return (n_trial + kVmTrials - 1) / kVmTrials; }
// blockIdx.x = group_in_batch * n_chunks + chunk
PROM_OBS_HD int32_t vm_wg_chunk(int32_t bx, int32_t n_chunks) { return bx % n_chunks; }
PROM_OBS_HD int32_t vm_wg_group(int32_t bx, int32_t n_chunks) { return bx / n_chunks; }
// tiles of a chunk: [first, first + count)
PROM_OBS_HD int32_t vm_chunk_first(int32_t chunk) { return chunk * kVmChunk; }
PROM_OBS_HD int32_t vm_chunk_count(int32_t chunk, int32_t n_pix) {
  const int32_t r = vm_tiles(n_pix) - chunk * kVmChunk;
  return r < kVmChunk ? r : kVmChunk;
}
PROM_OBS_HD int32_t vm_tile_first(int32_t tile) { return tile * kVmTile; }
PROM_OBS_HD int32_t vm_tile_count(int32_t tile, int32_t n_pix) {
  const int32_t r = n_pix - tile * kVmTile;
  return r < kVmTile ? r : kVmTile;
}
// first trial of a group
PROM_OBS_HD int32_t vm_group_first(int32_t group) { return group * kVmTrials; }
// entry e of a tile's (trial, pixel) table: e = r * kVmTile + t
PROM_OBS_HD int32_t vm_entry(int32_t r, int32_t t) { return r * kVmTile + t; }
PROM_OBS_HD int32_t vm_entry_trial(int32_t e) { return e / kVmTile; }
PROM_OBS_HD int32_t vm_entry_pixel(int32_t e) { return e % kVmTile; }

// ---- bracketed searches ------------------------------------------------------------------------------------------
// The positions of the group's smallest and largest factor (the first of equal ones)
PROM_OBS_HD void vm_extremes(const double* F, int32_t n, int32_t* rmin_out, int32_t* rmax_out) {
  int32_t rmin = 0, rmax = 0;
  for (int32_t r = 1; r < n; ++r) {
    if (F[r] < F[rmin]) rmin = r;
    if (F[r] > F[rmax]) rmax = r;
  }
  *rmin_out = rmin;
  *rmax_out = rmax;
}

// One end of a support's candidates for the target x, given the same end for the targets x_lo and x_hi of the group's
// extreme factors (i_lo = obs_bound(wav, n, x_lo, upper), i_hi likewise).  obs_bound is monotone in its target, so
// for x_lo <= x <= x_hi the answer lies in [i_lo, i_hi] and the search runs there; fl(L -+ c) is monotone in the
// factor for k sig < lam, and where it is not (the test below fails) the search runs over the whole grid.
PROM_OBS_HD int32_t vm_bound(const double* wav, int32_t n, double x, bool upper, double x_lo, double x_hi, int32_t i_lo,
                             int32_t i_hi) {
  if (x_lo <= x && x <= x_hi && 0 <= i_lo && i_lo <= i_hi && i_hi <= n)
    return i_lo + obs_bound(wav + i_lo, i_hi - i_lo, x, upper);
  return obs_bound(wav, n, x, upper);
}

// ---- the stage ---------------------------------------------------------------------------------------------------
// A tile's staged range from the lowest lower end and the highest upper end over the voting supports (obs_votes:
// not empty, no wider than the stage): from the lowest on, cap points at most.  No voter: empty
PROM_OBS_HD void vm_stage(bool any, int32_t a_min, int32_t b_max, int32_t cap, int32_t* s0_out, int32_t* s1_out) {
  int32_t s0 = 0, s1 = 0;
  if (any) {
    s0 = a_min;
    s1 = b_max;
    if (s1 - s0 > cap) s1 = s0 + cap;
  }
  *s0_out = s0;
  *s1_out = s1;
}
// what a support contributes to the two extremes (a non-voter leaves them alone)
PROM_OBS_HD int32_t vm_vote_a(int32_t a, int32_t b, int32_t cap) { return obs_votes(a, b, cap) ? a : INT32_MAX; }
PROM_OBS_HD int32_t vm_vote_b(int32_t a, int32_t b, int32_t cap) { return obs_votes(a, b, cap) ? b : 0; }

// ---- a support's points ------------------------------------------------------------------------------------------
// kVmLanes lanes stride over a support; the point lane l reads in pass `it` (it reads only where this < b)
PROM_OBS_HD int32_t vm_passes(int32_t a, int32_t b) { return (b - a + kVmLanes - 1) / kVmLanes; }
PROM_OBS_HD int32_t vm_point(int32_t a, int32_t it, int32_t l) { return a + kVmLanes * it + l; }

// ---- partial records ---------------------------------------------------------------------------------------------
// part[o][jb][chunk][kVmRecord] of a batch of nb trials (jb = j - first trial of the batch): the record's first double
PROM_OBS_HD int64_t vm_part_slot(int32_t o, int32_t jb, int32_t chunk, int32_t nb, int32_t n_chunks) {
  return (((int64_t)o * nb + jb) * n_chunks + chunk) * kVmRecord;
}
PROM_OBS_HD int64_t vm_part_doubles(int32_t n_orb, int32_t nb, int32_t n_chunks) {
  return (int64_t)n_orb * nb * n_chunks * kVmRecord;
}
// trial groups a batch may hold under a scratch cap in bytes (one at least)
PROM_OBS_HD int32_t vm_batch_groups(int64_t cap_bytes, int32_t n_orb, int32_t n_chunks, int32_t n_groups) {
  const int64_t per_group = vm_part_doubles(n_orb, kVmTrials, n_chunks) * 8;
  int64_t g = per_group > 0 ? cap_bytes / per_group : n_groups;
  if (g < 1) g = 1;
  // blockIdx.x = group * n_chunks + chunk stays below 2^31
  const int64_t gmax = (((int64_t)1 << 31) - 1) / (n_chunks > 0 ? n_chunks : 1);
  if (g > gmax) g = gmax;
  return g < n_groups ? (int32_t)g : n_groups;
}

}  // namespace prom
