// C-ABI layer, the spectrum's side: the observation, velocity maps and broadened spectra (declared in
// include/prom_hip.h).  Host code only: argument checks, copies and kernel launches on the context's streams.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "prom_api_shared.h"
#include "broaden_index.h"

extern "C" {

// ------------------------------------------------------------------------------ observation
int32_t prom_observe_set(prom_ctx* ctx, int32_t n_pix, const double* lam, const double* sig, double k, int32_t n_orb,
                         const double* f, const double* data, const double* ivar) {
  return guarded(ctx, [&] {
    prom::ObsDev& ob = ctx->obs;
    ob.set = false;
    ctx->vm.set = false;   // a trial table belongs to the observation it was set for
    ctx->vm.last_wav = ctx->vm.last_R = nullptr;
    ctx->ex.set = false;   // ... and so does an exposure table (its data are in the observation's pixels)
    ctx->ex.last_wav = ctx->ex.last_R = nullptr;
    PROM_REQUIRE(n_pix >= 0 && n_orb >= 1 && n_orb <= 65535 && (n_pix == 0 || (lam && sig)),
                 "prom_observe_set: bad shape");
    PROM_REQUIRE(k > 0.0 && obs_finite(k), "prom_observe_set: the truncation k must be positive");
    PROM_REQUIRE((data == nullptr) == (ivar == nullptr), "prom_observe_set: data and ivar come together");
    for (int32_t p = 0; p < n_pix; ++p) {
      PROM_REQUIRE(obs_finite(lam[p]) && (p == 0 || lam[p] >= lam[p - 1]),
                   "prom_observe_set: pixel centres must be finite and non-decreasing");
      PROM_REQUIRE(sig[p] > 0.0 && obs_finite(sig[p]), "prom_observe_set: widths must be positive");
    }
    bool ones = true;
    for (int32_t o = 0; f && o < n_orb; ++o) {
      PROM_REQUIRE(f[o] > 0.0 && obs_finite(f[o]), "prom_observe_set: frame factors must be positive");
      ones = ones && f[o] == 1.0;
    }
    const hipStream_t st = ctx->stream;
    const int64_t n = (int64_t)n_orb * n_pix;
    upload(ob.lam, lam, n_pix, st);
    upload(ob.sig, sig, n_pix, st);
    ob.has_f = f && !ones;   // all ones: the shared-frame path, the same sums bit for bit
    if (ob.has_f) upload(ob.f, f, n_orb, st);
    ob.has_data = data != nullptr;
    if (ob.has_data) {
      upload(ob.data, data, n, st);
      upload(ob.ivar, ivar, n, st);
    }
    ob.num.ensure(sizeof(double) * (size_t)std::max<int64_t>(n, 1));
    ob.den.ensure(sizeof(double) * (size_t)std::max<int64_t>(n, 1));
    ob.chi2.ensure(sizeof(double) * n_orb);
    ob.n_used.ensure(sizeof(int64_t) * n_orb);
    PROM_HIP(hipStreamSynchronize(st));   // the host arrays are read during the call only
    ob.n_pix = n_pix;
    ob.n_orb = n_orb;
    ob.k = k;
    ob.last_wav = ob.last_R = nullptr;
    ob.set = true;
  });
}

// k_observe of the whole observation on stream st (ev: events around it)
static void observe_launch(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int32_t n_wav,
                           hipEvent_t ev0, hipEvent_t ev1) {
  prom::ObsDev& ob = ctx->obs;
  prom::launch_observe(st, wav, ob.q.as<double>(), R, n_wav, ob.lam.as<double>(), ob.sig.as<double>(),
                       ob.has_f ? ob.f.as<double>() : nullptr, ob.k, ob.n_pix, ob.n_orb, ob.num.as<double>(),
                       ob.den.as<double>(), ev0, ev1);
}

// the shared tail of the two observe calls: q, the sums, chi-square and the copies back, on stream st
static void observe_on(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int64_t n_wav,
                       double edge_lo, double edge_hi, double* num_out, double* den_out, double* chi2_out,
                       int64_t* n_used_out) {
  prom::ObsDev& ob = ctx->obs;
  const bool want_chi2 = chi2_out || n_used_out;
  const int64_t n = (int64_t)ob.n_orb * ob.n_pix;
  ob.q.ensure(sizeof(double) * (size_t)n_wav);
  prom::launch_observe_q(st, wav, (int32_t)n_wav, edge_lo, edge_hi, ob.q.as<double>());
  observe_launch(ctx, st, wav, R, (int32_t)n_wav, nullptr, nullptr);
  ob.last_wav = wav;
  ob.last_R = R;
  ob.last_n_wav = (int32_t)n_wav;
  if (want_chi2)
    prom::launch_observe_chi2(st, ob.num.as<double>(), ob.den.as<double>(), ob.data.as<double>(),
                              ob.ivar.as<double>(), ob.n_pix, ob.n_orb, ob.chi2.as<double>(),
                              ob.n_used.as<int64_t>());
  if (num_out) download(num_out, ob.num, n, st);
  if (den_out) download(den_out, ob.den, n, st);
  if (chi2_out) download(chi2_out, ob.chi2, ob.n_orb, st);
  if (n_used_out) download(n_used_out, ob.n_used, ob.n_orb, st);
  PROM_HIP(hipStreamSynchronize(st));
}

static void observe_check(const prom::ObsDev& ob, const char* who, double edge_lo, double edge_hi, bool want_chi2) {
  if (!ob.set)
    throw Error(PROM_E_STATE, std::string(who) + ": no observation on the context (prom_observe_set; a "
                                                 "prom_transit_set with another n_orb drops it)");
  PROM_REQUIRE(!want_chi2 || (edge_lo != edge_lo && edge_hi != edge_hi),
               std::string(who) + ": chi-square needs the whole grid (both edges NaN)");
  PROM_REQUIRE(!want_chi2 || ob.has_data, std::string(who) + ": chi-square needs data and ivar (prom_observe_set)");
  PROM_REQUIRE(!std::isinf(edge_lo) && !std::isinf(edge_hi), std::string(who) + ": infinite edge");
}

int32_t prom_transit_observe(prom_ctx* ctx, double edge_lo, double edge_hi, double* num_out, double* den_out,
                             double* chi2_out, int64_t* n_used_out) {
  return guarded(ctx, [&] {
    prom::ObsDev& ob = ctx->obs;
    observe_check(ob, "prom_transit_observe", edge_lo, edge_hi, chi2_out || n_used_out);
    const TransitArgs t = transit_args(ctx, "prom_transit_observe", ob.n_orb, "the observation");
    PROM_REQUIRE(!ctx->br.current || (edge_lo != edge_lo && edge_hi != edge_hi),
                 "prom_transit_observe: the broadened spectrum covers the whole grid (both edges NaN)");
    if (ob.n_pix == 0) return;
    observe_on(ctx, t.st, t.wav, t.R, t.n_wav, edge_lo, edge_hi, num_out, den_out, chi2_out, n_used_out);
  });
}

int32_t prom_spectrum_observe(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                              double edge_lo, double edge_hi, double* num_out, double* den_out, double* chi2_out,
                              int64_t* n_used_out) {
  return guarded(ctx, [&] {
    prom::ObsDev& ob = ctx->obs;
    observe_check(ob, "prom_spectrum_observe", edge_lo, edge_hi, chi2_out || n_used_out);
    // (the edges are checked, and a table without pixels returns, before the uploads: not spectrum_args)
    PROM_REQUIRE(n_orb == ob.n_orb, "prom_spectrum_observe: n_orb differs from the observation's");
    spectrum_check("prom_spectrum_observe", n_wav, wav, wav && R);
    PROM_REQUIRE((edge_lo != edge_lo || edge_lo <= wav[0]) && (edge_hi != edge_hi || edge_hi >= wav[n_wav - 1]),
                 "prom_spectrum_observe: the edges lie outside the grid");
    if (ob.n_pix == 0) return;
    const hipStream_t st = ctx->stream;
    upload(ob.wav, wav, n_wav, st);
    upload(ob.R, R, (int64_t)n_orb * n_wav, st);
    observe_on(ctx, st, ob.wav.as<double>(), ob.R.as<double>(), n_wav, edge_lo, edge_hi, num_out, den_out, chi2_out,
               n_used_out);
  });
}

int32_t prom_observe_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::ObsDev& ob = ctx->obs;
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_observe_kernel_ms: bad arguments");
    if (!ob.set || !ob.last_wav || ob.n_pix == 0)
      throw Error(PROM_E_STATE, "prom_observe_kernel_ms: no observe call to repeat");
    const hipStream_t st = ctx->stream;
    double sum = 0.0;
    time_launches(ctx, st, n_runs, 1, &sum,
               [&] { observe_launch(ctx, st, ob.last_wav, ob.last_R, ob.last_n_wav, ctx->ev[0], ctx->ev[1]); });
    *ms_out = sum / n_runs;
  });
}

// ------------------------------------------------------------------------------ velocity maps
int32_t prom_vmap_set(prom_ctx* ctx, int32_t n_orb, int32_t n_trial, const double* F) {
  return guarded(ctx, [&] {
    prom::VmDev& vm = ctx->vm;
    const prom::ObsDev& ob = ctx->obs;
    vm.set = false;
    vm.last_wav = vm.last_R = nullptr;
    PROM_REQUIRE(n_orb >= 1 && n_trial >= 1 && n_trial <= (1 << 24) && F, "prom_vmap_set: bad shape");
    if (!ob.set)
      throw Error(PROM_E_STATE, "prom_vmap_set: no observation on the context (prom_observe_set)");
    if (!ob.has_data)
      throw Error(PROM_E_STATE, "prom_vmap_set: the observation has no data and ivar (prom_observe_set)");
    if (ob.n_orb != n_orb) throw Error(PROM_E_STATE, "prom_vmap_set: the observation has another n_orb");
    const int64_t n = (int64_t)n_orb * n_trial;
    PROM_REQUIRE(n <= ((int64_t)1 << 28), "prom_vmap_set: table too large");
    for (int64_t i = 0; i < n; ++i)
      PROM_REQUIRE(F[i] > 0.0 && obs_finite(F[i]), "prom_vmap_set: trial factors must be finite and positive");
    const hipStream_t st = ctx->stream;
    upload(vm.F, F, n, st);
    vm.mom.ensure(sizeof(double) * 7 * (size_t)n);
    vm.n_used.ensure(sizeof(int64_t) * (size_t)n);
    PROM_HIP(hipStreamSynchronize(st));   // the host array is read during the call only
    vm.n_orb = n_orb;
    vm.n_trial = n_trial;
    vm.set = true;
  });
}

// one pass over the table in batches of whole trial groups (ev: events around the k_vmap launches of the first batch)
static void vmap_launch(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int32_t n_wav,
                        hipEvent_t ev0, hipEvent_t ev1) {
  prom::VmDev& vm = ctx->vm;
  const prom::ObsDev& ob = ctx->obs;
  const VmBatches b = vm_batches(ctx, vm.n_orb, vm.n_trial);
  vm.part.ensure(sizeof(double) * (size_t)prom::vm_part_doubles(vm.n_orb, b.nb_max, b.n_chunks));
  static const bool debug = std::getenv("PROM_DEBUG") != nullptr;
  if (debug)
    std::fprintf(stderr, "prom: velocity map: %d trials in %d groups, %d batches of up to %d groups, %d chunks\n",
                 vm.n_trial, b.n_groups, (b.n_groups + b.bg - 1) / b.bg, b.bg, b.n_chunks);
  for (int32_t g = 0; g < b.n_groups; g += b.bg) {
    const int32_t j_first = prom::vm_group_first(g), nb = std::min(b.nb_max, vm.n_trial - j_first);
    prom::launch_vmap(st, wav, vm.q.as<double>(), R, n_wav, ob.lam.as<double>(), ob.sig.as<double>(), ob.k,
                      ob.data.as<double>(), ob.ivar.as<double>(), vm.F.as<double>(), ob.n_pix, vm.n_orb, vm.n_trial,
                      j_first, nb, vm.part.as<double>(), g == 0 ? ev0 : nullptr, g == 0 ? ev1 : nullptr);
    prom::launch_vmap_reduce(st, vm.part.as<double>(), ob.n_pix, vm.n_orb, vm.n_trial, j_first, nb,
                             vm.mom.as<double>(), vm.n_used.as<int64_t>());
  }
}

// the shared tail of the two map calls: q of the whole grid, the batches and the copies back, on stream st
static void vmap_on(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int64_t n_wav, double* mom_out,
                    int64_t* n_used_out) {
  prom::VmDev& vm = ctx->vm;
  const int64_t n = (int64_t)vm.n_orb * vm.n_trial;
  if (ctx->obs.n_pix == 0) return zero_moments(n, mom_out, n_used_out);   // no pixel is used: every moment 0
  const double nan = std::nan("");
  vm.q.ensure(sizeof(double) * (size_t)n_wav);
  prom::launch_observe_q(st, wav, (int32_t)n_wav, nan, nan, vm.q.as<double>());
  vmap_launch(ctx, st, wav, R, (int32_t)n_wav, nullptr, nullptr);
  vm.last_wav = wav;
  vm.last_R = R;
  vm.last_n_wav = (int32_t)n_wav;
  if (mom_out) download(mom_out, vm.mom, 7 * n, st);
  if (n_used_out) download(n_used_out, vm.n_used, n, st);
  PROM_HIP(hipStreamSynchronize(st));
}

static void vmap_check(prom_ctx* ctx, const char* who) {
  if (!ctx->vm.set || !ctx->obs.set || !ctx->obs.has_data || ctx->obs.n_orb != ctx->vm.n_orb)
    throw Error(PROM_E_STATE, std::string(who) + ": no trial table on the context (prom_vmap_set; a later "
                                                 "prom_observe_set or a prom_transit_set with another n_orb drops it)");
}

int32_t prom_transit_vmap(prom_ctx* ctx, double* mom_out, int64_t* n_used_out) {
  return guarded(ctx, [&] {
    vmap_check(ctx, "prom_transit_vmap");
    const TransitArgs t = transit_args(ctx, "prom_transit_vmap", ctx->vm.n_orb, "the trial table");
    vmap_on(ctx, t.st, t.wav, t.R, t.n_wav, mom_out, n_used_out);
  });
}

int32_t prom_spectrum_vmap(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                           double* mom_out, int64_t* n_used_out) {
  return guarded(ctx, [&] {
    prom::VmDev& vm = ctx->vm;
    vmap_check(ctx, "prom_spectrum_vmap");
    const hipStream_t st = spectrum_args(ctx, "prom_spectrum_vmap", n_orb, vm.n_orb, "the trial table's", n_wav, wav, R,
                                         vm.wav, vm.R, [&] { vm.last_wav = vm.last_R = nullptr; });
    vmap_on(ctx, st, vm.wav.as<double>(), vm.R.as<double>(), n_wav, mom_out, n_used_out);
  });
}

int32_t prom_vmap_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::VmDev& vm = ctx->vm;
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_vmap_kernel_ms: bad arguments");
    if (!vm.set || !ctx->obs.set || !vm.last_wav || ctx->obs.n_pix == 0)
      throw Error(PROM_E_STATE, "prom_vmap_kernel_ms: no map call to repeat");
    const hipStream_t st = ctx->stream;
    // k_vmap of the first batch (the whole table when it fits the scratch cap), scaled to the table by trial count
    const double scale = first_batch_scale(vm.n_trial, vm_batches(ctx, vm.n_orb, vm.n_trial).nb_max);
    double sum = 0.0;
    time_launches(ctx, st, n_runs, 1, &sum,
               [&] { vmap_launch(ctx, st, vm.last_wav, vm.last_R, vm.last_n_wav, ctx->ev[0], ctx->ev[1]); });
    *ms_out = scale * sum / n_runs;
  });
}

// ------------------------------------------------------------------------------ broadened spectra
int32_t prom_broaden_set(prom_ctx* ctx, int32_t n_k, double b0, double s, const double* K) {
  return guarded(ctx, [&] {
    prom::BrDev& br = ctx->br;
    br.set = false;
    br.current = false;   // R_b was formed with the kernel that leaves
    br.last_wav = br.last_q = br.last_R = nullptr;
    br.last_out = nullptr;
    if (n_k == 0) return;
    PROM_REQUIRE(n_k >= 2 && n_k <= prom::kBrMaxNodes && K, "prom_broaden_set: n_k must be 0 or lie in [2, 1025]");
    PROM_REQUIRE(obs_finite(b0), "prom_broaden_set: b0 must be finite");
    PROM_REQUIRE(obs_finite(s) && s > 0.0, "prom_broaden_set: s must be finite and > 0");
    bool any = false;
    for (int32_t i = 0; i < n_k; ++i) {
      PROM_REQUIRE(obs_finite(K[i]) && K[i] >= 0.0, "prom_broaden_set: K must be finite and >= 0");
      any = any || K[i] > 0.0;
    }
    PROM_REQUIRE(any, "prom_broaden_set: K must not be all zero");
    std::vector<prom::BrRec> rec((size_t)n_k);
    for (int32_t i = 0; i < n_k; ++i) rec[i] = prom::BrRec{K[i], i + 1 < n_k ? K[i + 1] - K[i] : 0.0};
    const hipStream_t st = ctx->stream;
    for (auto t : ctx->streams) PROM_HIP(hipStreamSynchronize(t));   // (a launch in flight may read the old records)
    upload(br.rec, rec.data(), n_k, st);
    PROM_HIP(hipStreamSynchronize(st));   // the host array is read during the call only
    br.n_k = n_k;
    br.b0 = b0;
    br.s = s;
    br.set = true;
  });
}

// q of the whole grid and k_broaden on stream st
static void broaden_launch(prom_ctx* ctx, hipStream_t st, const double* wav, double* q, const double* R, int32_t n_wav,
                           int32_t n_orb, double* out) {
  prom::BrDev& br = ctx->br;
  const double nan = std::nan("");
  prom::launch_observe_q(st, wav, n_wav, nan, nan, q);
  prom::launch_broaden(st, wav, q, R, n_wav, n_orb, br.rec.as<prom::BrRec>(), prom::BrKern{br.b0, br.s, br.n_k}, out,
                       nullptr, nullptr);
  br.last_wav = wav;
  br.last_q = q;
  br.last_R = R;
  br.last_out = out;
  br.last_n_wav = n_wav;
  br.last_n_orb = n_orb;
}

int32_t prom_spectrum_broaden(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                              double* Rb_out) {
  return guarded(ctx, [&] {
    prom::BrDev& br = ctx->br;
    if (!br.set) throw Error(PROM_E_STATE, "prom_spectrum_broaden: no kernel on the context (prom_broaden_set)");
    // (any n_orb, an output that must be there and a positive grid: not spectrum_args)
    PROM_REQUIRE(n_orb >= 1 && n_orb <= 65535, "prom_spectrum_broaden: bad n_orb");
    spectrum_check("prom_spectrum_broaden", n_wav, wav, wav && R && Rb_out);
    PROM_REQUIRE(wav[0] > 0.0 && obs_finite(1.0 / wav[0]),
                 "prom_spectrum_broaden: wavelengths must be > 0 (and 1 / wav finite)");
    const hipStream_t st = ctx->stream;
    const int64_t n = (int64_t)n_orb * n_wav;
    br.last_wav = br.last_q = br.last_R = nullptr;   // (the uploads may move the buffers the last call read)
    br.last_out = nullptr;
    upload(br.wav, wav, n_wav, st);
    upload(br.R, R, n, st);
    br.sq.ensure(sizeof(double) * (size_t)n_wav);
    br.out.ensure(sizeof(double) * (size_t)n);
    broaden_launch(ctx, st, br.wav.as<double>(), br.sq.as<double>(), br.R.as<double>(), (int32_t)n_wav, n_orb,
                   br.out.as<double>());
    download(Rb_out, br.out, n, st);
    PROM_HIP(hipStreamSynchronize(st));
  });
}

int32_t prom_transit_broaden(prom_ctx* ctx) {
  return guarded(ctx, [&] {
    prom::TransitDev& tr = ctx->tr;
    prom::BrDev& br = ctx->br;
    if (!br.set) throw Error(PROM_E_STATE, "prom_transit_broaden: no kernel on the context (prom_broaden_set)");
    // (the run's own R, never R_b, and no table whose n_orb could differ: not transit_args)
    if (!tr.ran) throw Error(PROM_E_STATE, "prom_transit_broaden: no completed run");
    const hipStream_t st = ctx->streams[tr.last];
    // R_b and q are one buffer each: an earlier broaden on another stream must be through with them
    if (br.stream && br.stream != st) PROM_HIP(hipStreamSynchronize(br.stream));
    const size_t bytes = sizeof(double) * (size_t)tr.n_orb * (size_t)tr.n_wav;
    if (bytes > br.Rb.cap || sizeof(double) * (size_t)tr.n_wav > br.q.cap) {
      // the buffers move: nothing may read the old ones any more, and no measurement aid may repeat a call on them
      for (auto t : ctx->streams) PROM_HIP(hipStreamSynchronize(t));
      const double* old = br.Rb.as<double>();
      if (old && ctx->obs.last_R == old) ctx->obs.last_wav = ctx->obs.last_R = nullptr;
      if (old && ctx->vm.last_R == old) ctx->vm.last_wav = ctx->vm.last_R = nullptr;
      if (old && ctx->ex.last_R == old) {
        ctx->ex.last_wav = ctx->ex.last_R = nullptr;
        ctx->ex.dt_ran = ctx->ex.hp_ran = ctx->ex.od_ran = false;
      }
      br.last_wav = br.last_q = br.last_R = nullptr;
      br.last_out = nullptr;
    }
    br.current = false;
    br.q.ensure(sizeof(double) * (size_t)tr.n_wav);
    br.Rb.ensure(bytes);
    broaden_launch(ctx, st, tr.wav.as<double>(), br.q.as<double>(), tr.slot[tr.last].R.as<double>(), (int32_t)tr.n_wav,
                   tr.n_orb, br.Rb.as<double>());
    br.stream = st;
    br.current = true;
  });
}

int32_t prom_transit_broadened(prom_ctx* ctx, double* Rb_out) {
  return guarded(ctx, [&] {
    prom::TransitDev& tr = ctx->tr;
    prom::BrDev& br = ctx->br;
    if (!tr.ran || !br.current)
      throw Error(PROM_E_STATE, "prom_transit_broadened: no broadened spectrum of the last run (prom_transit_broaden)");
    PROM_REQUIRE(Rb_out, "prom_transit_broadened: null output");
    const hipStream_t st = br.stream;
    download(Rb_out, br.Rb, (int64_t)tr.n_orb * tr.n_wav, st);
    PROM_HIP(hipStreamSynchronize(st));
  });
}

int32_t prom_broaden_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::BrDev& br = ctx->br;
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_broaden_kernel_ms: bad arguments");
    if (!br.set || !br.last_wav) throw Error(PROM_E_STATE, "prom_broaden_kernel_ms: no broaden call to repeat");
    const hipStream_t st = ctx->stream;
    double sum = 0.0;
    time_launches(ctx, st, n_runs, 1, &sum, [&] {
      prom::launch_broaden(st, br.last_wav, br.last_q, br.last_R, br.last_n_wav, br.last_n_orb,
                           br.rec.as<prom::BrRec>(), prom::BrKern{br.b0, br.s, br.n_k}, br.last_out, ctx->ev[0],
                           ctx->ev[1]);
    });
    *ms_out = sum / n_runs;
  });
}

}  // extern "C"
