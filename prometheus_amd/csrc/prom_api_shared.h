// What the translation units of the C-ABI layer share (prom_api.hip, prom_api_transit.hip, prom_api_observe.hip,
// prom_api_expose.hip, prom_api_inject.hip): the guard of every entry, the copies, the checks of tables and density
// models, the few checks the observation entries make in the same words, and the source of an entry's spectrum as a
// value.  Host code only.
#pragma once

#include <algorithm>
#include <cmath>
#include <exception>
#include <string>

#include "prom_internal.h"
#include "vmap_index.h"

namespace prom {
// whether [p, p + n) lies in a buffer of the pinned host pool that is in use (prom_api.hip: prom_host_alloc)
bool pinned_holds(const void* p, size_t n);
}  // namespace prom

namespace {

using prom::DevBuf;
using prom::Error;

template <class F>
int32_t guarded(prom_ctx* ctx, F&& f) {
  if (!ctx) return PROM_E_ARG;
  try {
    PROM_HIP(hipSetDevice(ctx->device));
    f();
    ctx->err.clear();
    return PROM_OK;
  } catch (const Error& e) {
    ctx->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    ctx->err = e.what();
    return PROM_E_HIP;
  }
}

template <class T>
void upload(DevBuf& b, const T* h, int64_t n, hipStream_t s) {
  b.ensure(sizeof(T) * (size_t)std::max<int64_t>(n, 1));
  if (n > 0) PROM_HIP(hipMemcpyAsync(b.p, h, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, s));
}

template <class T>
void download(T* h, const DevBuf& b, int64_t n, hipStream_t s) {
  if (n > 0) PROM_HIP(hipMemcpyAsync(h, b.p, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, s));
}

prom::DensityDev to_dev(const prom_density_model& m) {
  prom::DensityDev d{};
  d.kind = m.kind;
  for (int i = 0; i < 8; ++i) d.p[i] = m.p[i];
  // power law with a small integral exponent q (the setup files' q_esc, e.g. 6): (R / r)^q by repeated
  // squaring on the device (pad = q + 1) instead of a general pow.  Each squaring doubles the relative error
  // already carried, so the error grows about linearly in q: q <= 8 keeps it within ~8 ulp of pow
  // (test_density_plugins, q = 6); larger exponents take pow
  if (m.kind == PROM_DENSITY_POWERLAW && m.p[2] >= 0.0 && m.p[2] <= 8.0 && m.p[2] == std::floor(m.p[2]))
    d.pad = (int32_t)m.p[2] + 1;
  return d;
}

bool valid_kind(int32_t k) { return k >= PROM_DENSITY_BAROMETRIC && k <= PROM_DENSITY_GRIDDED; }

// GRIDDED: grid sizes from p[0..2] (each >= 2) and the packed length of [gx, gy, gz, values]
bool gridded_dims(const prom_density_model& m, int64_t* nx, int64_t* ny, int64_t* nz, int64_t* len) {
  for (int i = 0; i < 3; ++i)
    if (!(m.p[i] >= 2.0 && m.p[i] <= 1.0e6 && m.p[i] == std::floor(m.p[i]))) return false;
  *nx = (int64_t)m.p[0];
  *ny = (int64_t)m.p[1];
  *nz = (int64_t)m.p[2];
  *len = *nx + *ny + *nz + *nx * *ny * *nz;
  return *nx * *ny * *nz < ((int64_t)1 << 31);
}

template <class T>
bool table_ok(const std::vector<T>& v, int32_t id) {
  return id >= 0 && id < (int32_t)v.size() && v[id].live;
}

// a problem's captured graphs go with its buffers and arguments (a new set, a freed table, the context's end)
void drop_graphs(prom::TransitDev& tr) {
  for (auto& g : tr.gexec)
    if (g) {
      (void)hipGraphExecDestroy(g);
      g = nullptr;
    }
}

bool obs_finite(double v) { return std::isfinite(v); }

// the spectrum the transit observe calls read: the last run's R, or its broadened R_b while that is current
// (prom_transit_broaden)
const double* transit_R(prom_ctx* ctx) {
  const prom::TransitDev& tr = ctx->tr;
  return ctx->br.current ? ctx->br.Rb.as<double>() : tr.slot[tr.last].R.as<double>();
}

// ---- the observation entries' common words ---------------------------------------------------------------------------
// a caller's spectrum: the arrays are there (`arrays`), n_wav lies in [1, 2^30] and wav is finite and ascending
void spectrum_check(const char* who, int64_t n_wav, const double* wav, bool arrays) {
  const std::string w(who);
  PROM_REQUIRE(n_wav >= 1 && n_wav <= ((int64_t)1 << 30) && arrays, w + ": bad spectrum");
  for (int64_t i = 0; i < n_wav; ++i)
    PROM_REQUIRE(obs_finite(wav[i]) && (i == 0 || wav[i] >= wav[i - 1]), w + ": wavelengths must be finite and ascending");
}

// a prom_spectrum_* entry's arguments: n_orb is `whose` ("the observation's"), the spectrum is sound; then drop() forgets
// the last call (the uploads may move the buffers it read) and wav and R go to the family's buffers on the context's
// stream, which is returned
template <class Drop>
hipStream_t spectrum_args(prom_ctx* ctx, const char* who, int32_t n_orb, int32_t want_n_orb, const char* whose,
                          int64_t n_wav, const double* wav, const double* R, DevBuf& dwav, DevBuf& dR, Drop&& drop) {
  PROM_REQUIRE(n_orb == want_n_orb, std::string(who) + ": n_orb differs from " + whose);
  spectrum_check(who, n_wav, wav, wav && R);
  drop();
  upload(dwav, wav, n_wav, ctx->stream);
  upload(dR, R, (int64_t)n_orb * n_wav, ctx->stream);
  return ctx->stream;
}

// a prom_transit_* entry's arguments: a completed run whose n_orb is that of `what` ("the exposure table"); the last
// run's stream orders the call after it
struct TransitArgs {
  hipStream_t st;
  const double *wav, *R;
  int64_t n_wav;
};
TransitArgs transit_args(prom_ctx* ctx, const char* who, int32_t n_orb, const char* what) {
  const prom::TransitDev& tr = ctx->tr;
  if (!tr.ran) throw Error(PROM_E_STATE, std::string(who) + ": no completed run");
  if (n_orb != tr.n_orb) throw Error(PROM_E_STATE, std::string(who) + ": " + what + " has another n_orb");
  return TransitArgs{ctx->streams[tr.last], tr.wav.as<double>(), transit_R(ctx), tr.n_wav};
}

// where an entry's spectrum comes from: none (prom_sysrem_clean), the last run's (a prom_transit_* entry) or the
// caller's (n_orb, n_wav, wav, R) (a prom_spectrum_* entry).  `source` is SyDev's last_source of the call.  A family
// resolves it to TransitArgs with its own buffers (ex_args, sy_args), through the two functions above
struct Spectrum {
  int32_t source;   // 1: none, 2: the last run's, 3: the caller's
  int32_t n_orb;
  int64_t n_wav;
  const double *wav, *R;
};
constexpr Spectrum kNoSpectrum{1, 0, 0, nullptr, nullptr}, kLastRun{2, 0, 0, nullptr, nullptr};
Spectrum callers(int32_t n_orb, int64_t n_wav, const double* wav, const double* R) {
  return Spectrum{3, n_orb, n_wav, wav, R};
}

// ---- the exposure table, as the exposures' and the injections' entries ask for it ------------------------------------
constexpr int64_t kMaxGrid = ((int64_t)1 << 31) - 1;   // workgroups of one launch

bool table_present(const prom_ctx* ctx) { return ctx->ex.set && ctx->obs.set && ctx->obs.n_orb == ctx->ex.n_orb; }

void expose_check(prom_ctx* ctx, const char* who) {
  if (!table_present(ctx))
    throw Error(PROM_E_STATE, std::string(who) + ": no exposure table on the context (prom_expose_set; a later "
                                                 "prom_observe_set or a prom_transit_set with another n_orb drops it)");
}

// the sets' own test: the table they belong to is there
void table_check(const prom_ctx* ctx, const char* who) {
  if (!table_present(ctx))
    throw Error(PROM_E_STATE, std::string(who) + ": no exposure table on the context (prom_expose_set)");
}

// "no pixel: every moment 0" for n (row, trial) pairs
void zero_moments(int64_t n, double* mom_out, int64_t* n_used_out) {
  if (mom_out) std::fill(mom_out, mom_out + 7 * n, 0.0);
  if (n_used_out) std::fill(n_used_out, n_used_out + n, (int64_t)0);
}

// the batches of whole trial groups of k_vmap's partial records under the scratch cap, for a table of n_rows rows
struct VmBatches {
  int32_t n_chunks, n_groups, bg, nb_max;   // chunks of pixel tiles, trial groups, groups and trials of a batch at most
};
VmBatches vm_batches(const prom_ctx* ctx, int32_t n_rows, int32_t n_trial) {
  VmBatches b;
  b.n_chunks = prom::vm_chunks(ctx->obs.n_pix);
  b.n_groups = prom::vm_groups(n_trial);
  b.bg = prom::vm_batch_groups(ctx->vmap_scratch_bytes, n_rows, b.n_chunks, b.n_groups);
  b.nb_max = std::min(b.bg * prom::kVmTrials, n_trial);
  return b;
}
// a *_kernel_ms aid times the first batch: its time scales to the table by trial count
double first_batch_scale(int32_t n_trial, int32_t nb_max) { return (double)n_trial / (double)nb_max; }

// the loop of the *_kernel_ms aids: every stream idle, then n_runs times launch() on st and, once st is through, the
// time between events ev[2 i] and ev[2 i + 1] of the context added to sum[i], for i < n_pairs
template <class Launch>
void time_launches(prom_ctx* ctx, hipStream_t st, int32_t n_runs, int n_pairs, double* sum, Launch&& launch) {
  for (auto s : ctx->streams) PROM_HIP(hipStreamSynchronize(s));
  std::fill(sum, sum + n_pairs, 0.0);
  for (int32_t r = 0; r < n_runs; ++r) {
    launch();
    PROM_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n_pairs; ++i) {
      float ms = 0.0f;
      PROM_HIP(hipEventElapsedTime(&ms, ctx->ev[2 * i], ctx->ev[2 * i + 1]));
      sum[i] += ms;
    }
  }
}

}  // namespace
