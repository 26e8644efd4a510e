// C-ABI layer, the exposures' side: the exposure table, its filter, high-pass and orders and the chain every filtered
// call runs (declared in include/prom_hip.h; the injections' side is prom_api_inject.hip, which runs the chain through
// prom_api_chain.h).  Host code only: argument checks, copies and kernel launches on the context's streams.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "prom_api_chain.h"
#include "detrend_index.h"
#include "highpass_index.h"
#include "order_index.h"
#include "filter_index.h"
#include "order_sysrem_index.h"

namespace prom::api {

void highpass_launch(const prom::ExDev& ex, hipStream_t st, double* model, int64_t n_rows, int32_t n_pix, hipEvent_t ev0,
                     hipEvent_t ev1) {
  if (ex.hp_kind == 1)
    prom::launch_median(st, model, ex.hp_seg.as<int32_t>(), ex.hp_perm.as<int32_t>(), ex.hp_half, ex.hp_mode, n_rows,
                        ex.hp_n_seg, n_pix, ev0, ev1);
  else
    prom::launch_highpass(st, model, ex.hp_seg.as<int32_t>(), ex.hp_perm.as<int32_t>(), ex.hp_g.as<double>(),
                          ex.hp_half, ex.hp_den, ex.hp_mode, n_rows, ex.hp_n_seg, n_pix, ev0, ev1);
}

void record_last(prom::ExDev& ex, const double* wav, const double* R, int64_t n_wav, Ran ran, int32_t detrend) {
  ex.last_wav = wav;
  ex.last_R = R;
  ex.last_n_wav = (int32_t)n_wav;
  ex.dt_ran = ran == Ran::detrend;
  ex.hp_ran = ran == Ran::highpass;
  ex.od_ran = ran == Ran::orders;
  if (ran == Ran::highpass) ex.hp_detrend = detrend;
}

void expose_launch(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int32_t n_wav, bool want_mom,
                   double* model, hipEvent_t ev0, hipEvent_t ev1) {
  prom::ExDev& ex = ctx->ex;
  const prom::ObsDev& ob = ctx->obs;
  const VmBatches b = vm_batches(ctx, ex.n_exp, ex.n_trial);
  ex.part.ensure(sizeof(double) * (size_t)prom::vm_part_doubles(ex.n_exp, b.nb_max, b.n_chunks));
  static const bool debug = std::getenv("PROM_DEBUG") != nullptr;
  if (debug)
    std::fprintf(stderr, "prom: exposures: %d trials in %d groups, %d batches of up to %d groups, %d chunks\n",
                 ex.n_trial, b.n_groups, (b.n_groups + b.bg - 1) / b.bg, b.bg, b.n_chunks);
  for (int32_t g = 0; g < b.n_groups; g += b.bg) {
    const int32_t j_first = prom::vm_group_first(g), nb = std::min(b.nb_max, ex.n_trial - j_first);
    prom::launch_expose(st, wav, ex.q.as<double>(), R, n_wav, ob.lam.as<double>(), ob.sig.as<double>(), ob.k,
                        ex.row.as<int32_t>(), ex.a.as<double>(), ex.F.as<double>(), ex.data.as<double>(),
                        ex.ivar.as<double>(), ob.n_pix, ex.n_exp, ex.n_trial, ex.n_tap, j_first, nb,
                        ex.part.as<double>(), model, g == 0 ? ev0 : nullptr, g == 0 ? ev1 : nullptr);
    if (want_mom)
      prom::launch_vmap_reduce(st, ex.part.as<double>(), ob.n_pix, ex.n_exp, ex.n_trial, j_first, nb,
                               ex.mom.as<double>(), ex.n_used.as<int64_t>());
  }
}

void moments_launch(prom_ctx* ctx, hipStream_t st, const double* data, hipEvent_t ev0, hipEvent_t ev1,
                    const double* model) {
  prom::ExDev& ex = ctx->ex;
  if (!model) model = ex.model.as<double>();
  const prom::ObsDev& ob = ctx->obs;
  const VmBatches b = vm_batches(ctx, ex.n_exp, ex.n_trial);
  ex.part.ensure(sizeof(double) * (size_t)prom::vm_part_doubles(ex.n_exp, b.nb_max, b.n_chunks));
  static const bool debug = std::getenv("PROM_DEBUG") != nullptr;
  if (debug)
    std::fprintf(stderr, "prom: detrended moments: %d trials in %d groups, %d batches of up to %d groups, %d chunks\n",
                 ex.n_trial, b.n_groups, (b.n_groups + b.bg - 1) / b.bg, b.bg, b.n_chunks);
  for (int32_t g = 0; g < b.n_groups; g += b.bg) {
    const int32_t j_first = prom::vm_group_first(g), nb = std::min(b.nb_max, ex.n_trial - j_first);
    prom::launch_model_moments(st, model, ex.flag.as<uint8_t>(), data, ex.ivar.as<double>(), ob.n_pix,
                               ex.n_exp, ex.n_trial, j_first, nb, ex.part.as<double>(), g == 0 ? ev0 : nullptr,
                               g == 0 ? ev1 : nullptr);
    prom::launch_vmap_reduce(st, ex.part.as<double>(), ob.n_pix, ex.n_exp, ex.n_trial, j_first, nb, ex.mom.as<double>(),
                             ex.n_used.as<int64_t>());
  }
}

namespace {

// the batches of whole trial groups of the per-order records under the scratch cap
struct OdBatches {
  int32_t n_groups, bg, nb_max;
};
OdBatches od_batches(const prom_ctx* ctx) {
  const prom::ExDev& ex = ctx->ex;
  OdBatches b;
  b.n_groups = prom::od_groups(ex.n_trial);
  b.bg = prom::od_batch_groups(ctx->vmap_scratch_bytes, ex.n_exp, ex.od_n_seg, b.n_groups);
  b.nb_max = std::min(b.bg * prom::kOdTrials, ex.n_trial);
  return b;
}

}  // namespace

void orders_launch(prom_ctx* ctx, hipStream_t st, const double* data, double* orec_mom_out, int64_t* orec_n_used_out,
                   hipEvent_t* ev, const double* model) {
  prom::ExDev& ex = ctx->ex;
  if (!model) model = ex.model.as<double>();
  const int32_t n_pix = ctx->obs.n_pix, n_seg = ex.od_n_seg;
  const OdBatches b = od_batches(ctx);
  ex.od_rec.ensure(sizeof(double) * (size_t)prom::od_record_doubles(ex.n_exp, b.nb_max, n_seg));
  ex.od_tot.ensure(sizeof(double) * (size_t)prom::kOdTotals * ex.n_exp * ex.n_trial);
  static const bool debug = std::getenv("PROM_DEBUG") != nullptr;
  if (debug)
    std::fprintf(stderr, "prom: per-order moments: %d trials in %d groups, %d batches of up to %d groups, %d orders\n",
                 ex.n_trial, b.n_groups, (b.n_groups + b.bg - 1) / b.bg, b.bg, n_seg);
  const bool want = orec_mom_out || orec_n_used_out;
  std::vector<double> host;
  if (want) host.resize((size_t)prom::od_record_doubles(ex.n_exp, b.nb_max, n_seg));
  for (int32_t g = 0; g < b.n_groups; g += b.bg) {
    const int32_t j_first = prom::od_group_first(g), nb = std::min(b.nb_max, ex.n_trial - j_first);
    prom::launch_order_moments(st, model, ex.flag.as<uint8_t>(), data, ex.ivar.as<double>(),
                               ex.od_seg.as<int32_t>(), ex.od_perm.as<int32_t>(), n_pix, ex.n_exp, ex.n_trial, j_first,
                               nb, n_seg, ex.od_rec.as<double>(), ev && g == 0 ? ev[0] : nullptr,
                               ev && g == 0 ? ev[1] : nullptr);
    prom::launch_order_totals(st, ex.od_rec.as<double>(), ex.od_keep.as<uint8_t>(), ex.n_exp, ex.n_trial, j_first, nb,
                              n_seg, ex.od_tot.as<double>(), ev && g == 0 ? ev[2] : nullptr,
                              ev && g == 0 ? ev[3] : nullptr);
    if (!want) continue;
    download(host.data(), ex.od_rec, prom::od_record_doubles(ex.n_exp, nb, n_seg), st);
    PROM_HIP(hipStreamSynchronize(st));   // (the next batch writes the same buffer)
    for (int32_t e = 0; e < ex.n_exp; ++e)
      for (int32_t jb = 0; jb < nb; ++jb)
        for (int32_t s = 0; s < n_seg; ++s) {
          const double* rec = host.data() + prom::od_record(e, jb, s, nb, n_seg);
          const int64_t to = ((int64_t)e * ex.n_trial + j_first + jb) * n_seg + s;
          if (orec_mom_out) std::copy(rec, rec + 7, orec_mom_out + 7 * to);
          if (orec_n_used_out) std::memcpy(orec_n_used_out + to, rec + 7, sizeof(int64_t));
        }
  }
}

namespace {

// no pixel: every moment, record and total 0 and no model value
void zero_outputs(const prom::ExDev& ex, const ExOut& o) {
  const int64_t n = (int64_t)ex.n_exp * ex.n_trial;
  zero_moments(n, o.mom, o.n_used);
  zero_moments(n * ex.od_n_seg, o.orec_mom, o.orec_n_used);
  if (o.tot) std::fill(o.tot, o.tot + prom::kOdTotals * n, 0.0);
}

// the copies back (the per-order records have gone batch by batch) and the end of the call
void download_outputs(prom_ctx* ctx, hipStream_t st, const ExOut& o) {
  prom::ExDev& ex = ctx->ex;
  const int64_t n = (int64_t)ex.n_exp * ex.n_trial;
  if (o.mom) download(o.mom, ex.mom, 7 * n, st);
  if (o.n_used) download(o.n_used, ex.n_used, n, st);
  if (o.tot) download(o.tot, ex.od_tot, prom::kOdTotals * n, st);
  if (o.model) download(o.model, ex.model, n * ctx->obs.n_pix, st);
  PROM_HIP(hipStreamSynchronize(st));
}

}  // namespace

bool chain_prepare(prom_ctx* ctx, const ChainCall& c, int64_t n_wav) {
  prom::ExDev& ex = ctx->ex;
  const int32_t n_pix = ctx->obs.n_pix;
  const int64_t n = (int64_t)ex.n_exp * ex.n_trial;
  if (c.ran == Ran::orders) ex.od_ran = false;
  if (n_pix == 0) {
    zero_outputs(ex, c.out);
    return false;
  }
  if (!c.always && !c.out.any()) return false;
  if (c.orders && prom::od_workgroups(ex.n_exp, 1, ex.od_n_seg) > kMaxGrid)
    throw Error(PROM_E_ARG, "k_order_moments: n_exp n_seg too large for one launch");
  if (c.highpass && prom::hp_workgroups(n, ex.hp_n_seg) > kMaxGrid)
    throw Error(PROM_E_ARG, "k_highpass: n_exp n_trial n_seg too large for one launch");
  if (c.detrend && prom::dt_workgroups(ex.n_trial, n_pix) > kMaxGrid)
    throw Error(PROM_E_ARG, "k_detrend: n_trial n_pix too large for one launch");
  ex.q.ensure(sizeof(double) * (size_t)n_wav);
  try {   // the whole table's model is resident at once: it is not batched
    ex.model.ensure(sizeof(double) * (size_t)(n * n_pix));
  } catch (const Error& err) {
    throw Error(err.code, std::string(err.what()) + ": " + c.noun + " the model of all " + std::to_string(ex.n_trial) +
                              " trials in device memory; give fewer trials per call");
  }
  ex.flag.ensure((size_t)ex.n_trial * n_pix);
  return true;
}

void chain_unfiltered(prom_ctx* ctx, hipStream_t st, const ChainCall& c, const double* wav, const double* R,
                      int32_t n_wav, const hipEvent_t* hp_ev) {
  prom::ExDev& ex = ctx->ex;
  expose_launch(ctx, st, wav, R, n_wav, false, ex.model.as<double>(), nullptr, nullptr);
  if (c.highpass)
    highpass_launch(ex, st, ex.model.as<double>(), (int64_t)ex.n_exp * ex.n_trial, ctx->obs.n_pix,
                    hp_ev ? hp_ev[0] : nullptr, hp_ev ? hp_ev[1] : nullptr);
}

namespace {

// 2: the final model: the unfiltered one, then the filter in place or every column flagged filterable (hp_ev, dt_ev:
// events around k_highpass and k_detrend).  The filters work in place, so an aid that repeats one forms the model again
// each time
void chain_model(prom_ctx* ctx, hipStream_t st, const ChainCall& c, const double* wav, const double* R, int32_t n_wav,
                 const hipEvent_t* hp_ev = nullptr, const hipEvent_t* dt_ev = nullptr) {
  prom::ExDev& ex = ctx->ex;
  const int32_t n_pix = ctx->obs.n_pix;
  chain_unfiltered(ctx, st, c, wav, R, n_wav, hp_ev);
  if (c.detrend)
    prom::launch_detrend(st, ex.model.as<double>(), c.U->as<double>(), c.W->as<double>(), ex.flag.as<uint8_t>(),
                         ex.n_exp, c.n_comp, ex.n_trial, n_pix, dt_ev ? dt_ev[0] : nullptr, dt_ev ? dt_ev[1] : nullptr,
                         nullptr, c.seg_of);
  else
    PROM_HIP(hipMemsetAsync(ex.flag.as<uint8_t>(), 1, (size_t)ex.n_trial * n_pix, st));
}

// 3: the moments, the state the call leaves, the per-order kernels and the copies back, in this order
void chain_finish(prom_ctx* ctx, hipStream_t st, const ChainCall& c, const double* wav, const double* R, int64_t n_wav) {
  prom::ExDev& ex = ctx->ex;
  const bool forget = c.ran == Ran::none;
  if (c.out.moments()) moments_launch(ctx, st, c.data->as<double>(), nullptr, nullptr);
  record_last(ex, forget ? nullptr : wav, forget ? nullptr : R, n_wav, c.ran, c.detrend);
  if (c.out.orders()) orders_launch(ctx, st, c.data->as<double>(), c.out.orec_mom, c.out.orec_n_used, nullptr);
  download_outputs(ctx, st, c.out);
}

}  // namespace

void chain_go(prom_ctx* ctx, hipStream_t st, const ChainCall& c, const double* wav, const double* R, int64_t n_wav) {
  const double nan = std::nan("");
  prom::launch_observe_q(st, wav, (int32_t)n_wav, nan, nan, ctx->ex.q.as<double>());
  chain_model(ctx, st, c, wav, R, (int32_t)n_wav);
  chain_finish(ctx, st, c, wav, R, n_wav);
}

}  // namespace prom::api

using namespace prom::api;

namespace {

// segments over the observation's pixels (the high-pass's, the orders'): seg_first runs from 0 to n_pix strictly
// ascending and perm is a permutation; without pixels one empty segment
void segments_check(const char* who, int32_t n_pix, int32_t n_seg, const int32_t* seg_first, const int32_t* perm) {
  const std::string w(who);
  if (n_pix == 0) {   // no pixel: no segment can hold one; the calls give zeros
    PROM_REQUIRE(n_seg == 1 && seg_first[0] == 0 && seg_first[1] == 0, w + ": without pixels seg_first must be {0, 0}");
    return;
  }
  PROM_REQUIRE(n_seg <= n_pix && seg_first[0] == 0 && seg_first[n_seg] == n_pix,
               w + ": seg_first must run from 0 to n_pix");
  for (int32_t i = 0; i < n_seg; ++i)
    PROM_REQUIRE(seg_first[i + 1] > seg_first[i], w + ": seg_first must be strictly ascending");
  std::vector<char> seen((size_t)n_pix, 0);
  for (int32_t i = 0; i < n_pix; ++i) {
    PROM_REQUIRE(perm[i] >= 0 && perm[i] < n_pix && !seen[(size_t)perm[i]],
                 w + ": perm must be a permutation of 0 .. n_pix - 1");
    seen[(size_t)perm[i]] = 1;
  }
}

// an exposure entry's spectrum: the last run's, or the caller's in the table's wav / R buffers (od: a per-order entry)
TransitArgs ex_args(prom_ctx* ctx, const char* who, const Spectrum& s, bool od = false) {
  prom::ExDev& ex = ctx->ex;
  if (s.source == 2) return transit_args(ctx, who, ex.n_orb, "the exposure table");
  const hipStream_t st =
      spectrum_args(ctx, who, s.n_orb, ex.n_orb, "the observation's", s.n_wav, s.wav, s.R, ex.wav, ex.R, [&] {
        ex.last_wav = ex.last_R = nullptr;
        if (od) ex.od_ran = false;
      });
  return TransitArgs{st, ex.wav.as<double>(), ex.R.as<double>(), s.n_wav};
}

ExOut plain_out(double* mom, int64_t* n_used, double* model) {
  return ExOut{mom, n_used, nullptr, nullptr, nullptr, model};
}

// a call on the resident filter and the table's own data
ChainCall resident_call(prom_ctx* ctx, bool highpass, bool detrend, bool orders, Ran ran, const char* noun,
                        const ExOut& out) {
  prom::ExDev& ex = ctx->ex;
  return ChainCall{highpass, detrend, orders, &ex.U, &ex.W, ex.n_comp, &ex.data, ran, false, noun, out,
                   ex.dt_n_seg > 0 ? ex.dt_seg_of.as<int32_t>() : nullptr};
}

// the shared tail of the detrended, high-pass and per-order entries
void chain_on(prom_ctx* ctx, const TransitArgs& t, const ChainCall& c) {
  if (chain_prepare(ctx, c, t.n_wav)) chain_go(ctx, t.st, c, t.wav, t.R, t.n_wav);
}

// ---- one body per family: its state checks, the spectrum's, then the call ------------------------------------------------
// the plain expose calls: the moments are fused into k_expose and the model is kept on request only, so this is not the
// chain
void expose_entry(prom_ctx* ctx, const char* who, const Spectrum& s, const ExOut& o) {
  prom::ExDev& ex = ctx->ex;
  expose_check(ctx, who);
  const TransitArgs t = ex_args(ctx, who, s);
  if (ctx->obs.n_pix == 0) return zero_outputs(ex, o);
  if (!o.any()) return;
  const double nan = std::nan("");
  ex.q.ensure(sizeof(double) * (size_t)t.n_wav);
  if (o.model) ex.model.ensure(sizeof(double) * (size_t)ex.n_exp * ex.n_trial * ctx->obs.n_pix);
  prom::launch_observe_q(t.st, t.wav, (int32_t)t.n_wav, nan, nan, ex.q.as<double>());
  expose_launch(ctx, t.st, t.wav, t.R, (int32_t)t.n_wav, o.moments(), o.model ? ex.model.as<double>() : nullptr,
                nullptr, nullptr);
  record_last(ex, t.wav, t.R, t.n_wav, Ran::none, 0);
  download_outputs(ctx, t.st, o);
}

ChainCall detrend_call(prom_ctx* ctx, const ExOut& out) {
  return resident_call(ctx, false, true, false, Ran::detrend, "the detrended exposures keep", out);
}

void detrended_entry(prom_ctx* ctx, const char* who, const Spectrum& s, const ExOut& o) {
  expose_check(ctx, who);
  if (!ctx->ex.dt_set)
    throw Error(PROM_E_STATE, std::string(who) + ": no filter on the context (prom_detrend_set; a later "
                                                 "prom_expose_set, or whatever drops the exposure table, drops it)");
  chain_on(ctx, ex_args(ctx, who, s), detrend_call(ctx, o));
}

ChainCall highpass_call(prom_ctx* ctx, int32_t detrend, const ExOut& out) {
  return resident_call(ctx, true, detrend != 0, false, Ran::highpass, "the high-pass filtered exposures keep", out);
}

void highpass_entry(prom_ctx* ctx, const char* who, const Spectrum& s, int32_t detrend, const ExOut& o) {
  expose_check(ctx, who);
  if (!ctx->ex.hp_set)
    throw Error(PROM_E_STATE, std::string(who) + ": no high-pass on the context (prom_highpass_set; a later "
                                                 "prom_expose_set, or whatever drops the exposure table, drops it)");
  if (detrend != 0 && detrend != 1) throw Error(PROM_E_ARG, std::string(who) + ": detrend must be 0 or 1");
  if (detrend && !ctx->ex.dt_set)
    throw Error(PROM_E_STATE, std::string(who) + ": detrend = 1 without a filter on the context (prom_detrend_set)");
  chain_on(ctx, ex_args(ctx, who, s), highpass_call(ctx, detrend, o));
}

void orders_entry(prom_ctx* ctx, const char* who, const Spectrum& s, int32_t highpass, int32_t detrend, const ExOut& o) {
  expose_check(ctx, who);
  if (!ctx->ex.od_set)
    throw Error(PROM_E_STATE, std::string(who) + ": no orders on the context (prom_orders_set; a later "
                                                 "prom_expose_set, or whatever drops the exposure table, drops them)");
  if (highpass != 0 && highpass != 1) throw Error(PROM_E_ARG, std::string(who) + ": highpass must be 0 or 1");
  if (detrend != 0 && detrend != 1) throw Error(PROM_E_ARG, std::string(who) + ": detrend must be 0 or 1");
  if (highpass && !ctx->ex.hp_set)
    throw Error(PROM_E_STATE, std::string(who) + ": highpass = 1 without a high-pass on the context (prom_highpass_set)");
  if (detrend && !ctx->ex.dt_set)
    throw Error(PROM_E_STATE, std::string(who) + ": detrend = 1 without a filter on the context (prom_detrend_set)");
  chain_on(ctx, ex_args(ctx, who, s, true),
           resident_call(ctx, highpass != 0, detrend != 0, true, Ran::orders, "the per-order moments keep", o));
}

// ---- what the four filter sets share (n_seg = 0: one basis, the entries without `orders`) -------------------------------
// the state the call drops and the checks of its shape
void detrend_begin(prom_ctx* ctx, const char* who, bool orders, int32_t n_exp, int32_t n_comp, int32_t n_seg) {
  prom::ExDev& ex = ctx->ex;
  const std::string w(who);
  ex.dt_set = ex.dt_ran = false;
  ex.dt_n_seg = 0;
  if (ctx->rc.last == 1) ctx->rc.last = 0;
  table_check(ctx, who);
  if (orders && !ex.od_set) throw Error(PROM_E_STATE, w + ": no orders on the context (prom_orders_set)");
  PROM_REQUIRE(n_exp == ex.n_exp, w + ": n_exp differs from the exposure table's");
  PROM_REQUIRE(n_comp >= 1 && n_comp <= prom::kDtMaxComp, w + ": n_comp must lie in [1, 16]");
  PROM_REQUIRE(n_seg == (orders ? ex.od_n_seg : 0), w + ": n_seg differs from the resident orders'");
}

// U, [n_seg][n_exp][n_comp] or [n_exp][n_comp], and seg_of of the resident orders on the device
void detrend_basis(prom_ctx* ctx, const char* who, int32_t n_exp, int32_t n_comp, int32_t n_seg, const double* U,
                   hipStream_t st) {
  prom::ExDev& ex = ctx->ex;
  const std::string w(who);
  const int64_t nu = (int64_t)std::max(n_seg, 1) * n_exp * n_comp;
  PROM_REQUIRE(U, w + ": U missing");
  for (int64_t i = 0; i < nu; ++i) PROM_REQUIRE(obs_finite(U[i]), w + ": U must be finite");
  upload(ex.U, U, nu, st);
  if (n_seg == 0) return;
  const int32_t n_pix = ctx->obs.n_pix;
  std::vector<int32_t> seg_of((size_t)std::max(n_pix, 1), 0);
  prom::fo_seg_of(n_seg, ex.od_seg_host.data(), ex.od_perm_host.data(), seg_of.data());
  upload(ex.dt_seg_of, seg_of.data(), (int64_t)n_pix, st);
  PROM_HIP(hipStreamSynchronize(st));   // (seg_of is a local)
}

// a set: the caller's W beside U
void detrend_set(prom_ctx* ctx, const char* who, bool orders, int32_t n_exp, int32_t n_comp, int32_t n_seg,
                 const double* U, const double* W) {
  prom::ExDev& ex = ctx->ex;
  const std::string w(who);
  const hipStream_t st = ctx->stream;
  const int64_t nw = (int64_t)n_comp * n_exp * ctx->obs.n_pix;
  detrend_begin(ctx, who, orders, n_exp, n_comp, n_seg);
  if (!orders) PROM_REQUIRE(U && (nw == 0 || W), w + ": U and W missing");
  detrend_basis(ctx, who, n_exp, n_comp, n_seg, U, st);
  PROM_REQUIRE(nw == 0 || W, w + ": W missing");
  for (int64_t i = 0; i < nw; ++i) PROM_REQUIRE(obs_finite(W[i]), w + ": W must be finite");
  upload(ex.W, W, nw, st);
  PROM_HIP(hipStreamSynchronize(st));   // the host arrays are read during the call only
  ex.n_comp = n_comp;
  ex.dt_n_seg = n_seg;
  ex.dt_set = true;
}

// a build: W of (U, the table's ivar) on the device, for prom_filter_kernel_ms to repeat
void detrend_build(prom_ctx* ctx, const char* who, bool orders, int32_t n_exp, int32_t n_comp, int32_t n_seg,
                   const double* U, double* W_out) {
  prom::ExDev& ex = ctx->ex;
  const hipStream_t st = ctx->stream;
  const int32_t n_pix = ctx->obs.n_pix;
  const int64_t nw = (int64_t)n_comp * n_exp * n_pix;
  detrend_begin(ctx, who, orders, n_exp, n_comp, n_seg);
  detrend_basis(ctx, who, n_exp, n_comp, n_seg, U, st);
  ex.W.ensure(sizeof(double) * (size_t)std::max<int64_t>(nw, 1));
  if (n_seg)
    prom::launch_filter_weights_orders(st, ex.U.as<double>(), ex.ivar.as<double>(), ex.dt_seg_of.as<int32_t>(),
                                       ex.W.as<double>(), n_exp, n_comp, n_pix, nullptr, nullptr);
  else
    prom::launch_filter_weights(st, ex.U.as<double>(), ex.ivar.as<double>(), ex.W.as<double>(), n_exp, n_comp, n_pix,
                                nullptr, nullptr);
  if (W_out) download(W_out, ex.W, nw, st);
  PROM_HIP(hipStreamSynchronize(st));   // the host array is read during the call only
  ex.n_comp = n_comp;
  ex.dt_n_seg = n_seg;
  ex.dt_set = true;
  if (n_pix > 0) {
    ctx->rc.last = 1;
    ctx->rc.last_n_comp = n_comp;
  }
}

// ---- what the two high-pass sets share (g: the weighted mean's taps, null: the median) -----------------------------------
void highpass_set(prom_ctx* ctx, const char* who, int32_t n_pix, int32_t n_seg, const int32_t* seg_first,
                  const int32_t* perm, int32_t half_width, const double* g, bool median, int32_t mode) {
  prom::ExDev& ex = ctx->ex;
  const std::string w(who);
  ex.hp_set = ex.hp_ran = false;
  table_check(ctx, who);
  PROM_REQUIRE(n_pix == ctx->obs.n_pix, w + ": n_pix differs from the observation's");
  PROM_REQUIRE(n_seg >= 1 && seg_first && (n_pix == 0 || perm), w + ": segments missing");
  PROM_REQUIRE(half_width >= 0 && half_width <= prom::kHpMaxHalf && (median || g),
               w + ": half_width must lie in [0, 512]");
  PROM_REQUIRE(mode == 0 || mode == 1, w + ": mode must be 0 (subtract) or 1 (divide)");
  segments_check(who, n_pix, n_seg, seg_first, perm);
  const hipStream_t st = ctx->stream;
  if (!median) {
    for (int32_t d = 0; d <= half_width; ++d)
      PROM_REQUIRE(obs_finite(g[d]) && g[d] >= 0.0, w + ": g must be finite and >= 0");
    PROM_REQUIRE(g[0] > 0.0, w + ": g[0] must be > 0");
    upload(ex.hp_g, g, (int64_t)half_width + 1, st);
    ex.hp_den = prom::hp_den_full(g, half_width);
  }
  upload(ex.hp_seg, seg_first, (int64_t)n_seg + 1, st);
  upload(ex.hp_perm, perm, (int64_t)n_pix, st);
  PROM_HIP(hipStreamSynchronize(st));   // the host arrays are read during the call only
  ex.hp_n_seg = n_seg;
  ex.hp_half = half_width;
  ex.hp_mode = mode;
  ex.hp_kind = median ? 1 : 0;
  ex.hp_set = true;
}

// the spectrum the last call read, for an aid to repeat it
bool no_last_call(const prom_ctx* ctx) {
  return !ctx->ex.set || !ctx->obs.set || !ctx->ex.last_wav || ctx->obs.n_pix == 0;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------ exposures
int32_t prom_expose_set(prom_ctx* ctx, int32_t n_exp, int32_t n_trial, int32_t n_tap, const int32_t* row,
                        const double* a, const double* F, const double* data, const double* ivar) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    const prom::ObsDev& ob = ctx->obs;
    ex.set = false;
    ex.dt_set = ex.dt_ran = false;   // a filter belongs to the table it was set for
    ex.hp_set = ex.hp_ran = false;   // ... and so does a high-pass
    ex.od_set = ex.od_ran = false;   // ... and the orders of the per-order moments
    ctx->sy.set = false;             // ... and the raw exposures of the injections
    ctx->sy.last_source = 0;
    ctx->rc.last = 0;
    ex.last_wav = ex.last_R = nullptr;
    PROM_REQUIRE(n_exp >= 1 && n_exp <= 65535 && n_trial >= 1 && n_trial <= (1 << 24) && n_tap >= 1 &&
                     n_tap <= (1 << 16) && row && a && F,
                 "prom_expose_set: bad shape");
    if (!ob.set) throw Error(PROM_E_STATE, "prom_expose_set: no observation on the context (prom_observe_set)");
    PROM_REQUIRE(ob.n_pix == 0 || (data && ivar), "prom_expose_set: data and ivar missing");
    const int64_t nt = (int64_t)n_exp * n_tap, nf = nt * n_trial, nd = (int64_t)n_exp * ob.n_pix;
    PROM_REQUIRE(nf <= ((int64_t)1 << 28), "prom_expose_set: table too large");
    for (int64_t i = 0; i < nt; ++i) {
      PROM_REQUIRE(row[i] >= 0 && row[i] < ob.n_orb, "prom_expose_set: a tap's row lies outside [0, n_orb)");
      PROM_REQUIRE(a[i] >= 0.0 && obs_finite(a[i]), "prom_expose_set: tap weights must be finite and >= 0");
    }
    for (int64_t i = 0; i < nf; ++i)
      PROM_REQUIRE(F[i] > 0.0 && obs_finite(F[i]), "prom_expose_set: factors must be finite and positive");
    const hipStream_t st = ctx->stream;
    upload(ex.row, row, nt, st);
    upload(ex.a, a, nt, st);
    upload(ex.F, F, nf, st);
    upload(ex.data, data, nd, st);
    upload(ex.ivar, ivar, nd, st);
    ex.mom.ensure(sizeof(double) * 7 * (size_t)n_exp * n_trial);
    ex.n_used.ensure(sizeof(int64_t) * (size_t)n_exp * n_trial);
    PROM_HIP(hipStreamSynchronize(st));   // the host arrays are read during the call only
    ex.n_orb = ob.n_orb;
    ex.n_exp = n_exp;
    ex.n_trial = n_trial;
    ex.n_tap = n_tap;
    ex.set = true;
  });
}

int32_t prom_transit_expose(prom_ctx* ctx, double* mom_out, int64_t* n_used_out, double* model_out) {
  return guarded(ctx, [&] {
    expose_entry(ctx, "prom_transit_expose", kLastRun, plain_out(mom_out, n_used_out, model_out));
  });
}

int32_t prom_spectrum_expose(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                             double* mom_out, int64_t* n_used_out, double* model_out) {
  return guarded(ctx, [&] {
    expose_entry(ctx, "prom_spectrum_expose", callers(n_orb, n_wav, wav, R), plain_out(mom_out, n_used_out, model_out));
  });
}

int32_t prom_expose_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_expose_kernel_ms: bad arguments");
    if (no_last_call(ctx)) throw Error(PROM_E_STATE, "prom_expose_kernel_ms: no expose call to repeat");
    // k_expose of the first batch (the whole table when it fits the scratch cap), scaled to the table by trial count;
    // moments only, no model store
    const double scale = first_batch_scale(ex.n_trial, vm_batches(ctx, ex.n_exp, ex.n_trial).nb_max);
    double sum = 0.0;
    time_launches(ctx, ctx->stream, n_runs, 1, &sum, [&] {
      expose_launch(ctx, ctx->stream, ex.last_wav, ex.last_R, ex.last_n_wav, true, nullptr, ctx->ev[0], ctx->ev[1]);
    });
    *ms_out = scale * sum / n_runs;
  });
}

// ------------------------------------------------------------------------------ detrended exposures
int32_t prom_detrend_set(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, const double* U, const double* W) {
  return guarded(ctx, [&] { detrend_set(ctx, "prom_detrend_set", false, n_exp, n_comp, 0, U, W); });
}

int32_t prom_detrend_set_orders(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, int32_t n_seg, const double* U,
                                const double* W) {
  return guarded(ctx, [&] { detrend_set(ctx, "prom_detrend_set_orders", true, n_exp, n_comp, n_seg, U, W); });
}

int32_t prom_detrend_build(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, const double* U, double* W_out) {
  return guarded(ctx, [&] { detrend_build(ctx, "prom_detrend_build", false, n_exp, n_comp, 0, U, W_out); });
}

int32_t prom_detrend_build_orders(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, int32_t n_seg, const double* U,
                                  double* W_out) {
  return guarded(ctx, [&] { detrend_build(ctx, "prom_detrend_build_orders", true, n_exp, n_comp, n_seg, U, W_out); });
}

int32_t prom_transit_expose_detrended(prom_ctx* ctx, double* mom_out, int64_t* n_used_out, double* model_out) {
  return guarded(ctx, [&] {
    detrended_entry(ctx, "prom_transit_expose_detrended", kLastRun, plain_out(mom_out, n_used_out, model_out));
  });
}

int32_t prom_spectrum_expose_detrended(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                       double* mom_out, int64_t* n_used_out, double* model_out) {
  return guarded(ctx, [&] {
    detrended_entry(ctx, "prom_spectrum_expose_detrended", callers(n_orb, n_wav, wav, R),
                    plain_out(mom_out, n_used_out, model_out));
  });
}

int32_t prom_detrend_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_detrend_kernel_ms: bad arguments");
    if (no_last_call(ctx) || !ex.dt_set || !ex.dt_ran)
      throw Error(PROM_E_STATE, "prom_detrend_kernel_ms: no detrended call to repeat");
    // the unfiltered model is formed again (untimed) before k_detrend (timed, the whole table); k_model_moments of the
    // first batch, scaled to the table by trial count
    const double scale = first_batch_scale(ex.n_trial, vm_batches(ctx, ex.n_exp, ex.n_trial).nb_max);
    const ChainCall c = detrend_call(ctx, ExOut{});
    double sum[2];
    time_launches(ctx, ctx->stream, n_runs, 2, sum, [&] {
      chain_model(ctx, ctx->stream, c, ex.last_wav, ex.last_R, ex.last_n_wav, nullptr, &ctx->ev[0]);
      moments_launch(ctx, ctx->stream, ex.data.as<double>(), ctx->ev[2], ctx->ev[3]);
    });
    ms_out[0] = sum[0] / n_runs;
    ms_out[1] = scale * sum[1] / n_runs;
  });
}

// ------------------------------------------------------------------------------ high-pass filtered exposures
int32_t prom_highpass_set(prom_ctx* ctx, int32_t n_pix, int32_t n_seg, const int32_t* seg_first, const int32_t* perm,
                          int32_t half_width, const double* g, int32_t mode) {
  return guarded(ctx, [&] {
    highpass_set(ctx, "prom_highpass_set", n_pix, n_seg, seg_first, perm, half_width, g, false, mode);
  });
}

int32_t prom_highpass_set_median(prom_ctx* ctx, int32_t n_pix, int32_t n_seg, const int32_t* seg_first,
                                 const int32_t* perm, int32_t half_width, int32_t mode) {
  return guarded(ctx, [&] {
    highpass_set(ctx, "prom_highpass_set_median", n_pix, n_seg, seg_first, perm, half_width, nullptr, true, mode);
  });
}

int32_t prom_transit_expose_highpass(prom_ctx* ctx, int32_t detrend, double* mom_out, int64_t* n_used_out,
                                     double* model_out) {
  return guarded(ctx, [&] {
    highpass_entry(ctx, "prom_transit_expose_highpass", kLastRun, detrend, plain_out(mom_out, n_used_out, model_out));
  });
}

int32_t prom_spectrum_expose_highpass(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                      int32_t detrend, double* mom_out, int64_t* n_used_out, double* model_out) {
  return guarded(ctx, [&] {
    highpass_entry(ctx, "prom_spectrum_expose_highpass", callers(n_orb, n_wav, wav, R), detrend,
                   plain_out(mom_out, n_used_out, model_out));
  });
}

int32_t prom_highpass_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_highpass_kernel_ms: bad arguments");
    if (no_last_call(ctx) || !ex.hp_set || !ex.hp_ran || (ex.hp_detrend && !ex.dt_set))
      throw Error(PROM_E_STATE, "prom_highpass_kernel_ms: no high-pass call to repeat");
    // the unfiltered model is formed again (untimed) before k_highpass (timed, the whole table)
    const ChainCall c = highpass_call(ctx, ex.hp_detrend, ExOut{});
    double sum = 0.0;
    time_launches(ctx, ctx->stream, n_runs, 1, &sum, [&] {
      chain_model(ctx, ctx->stream, c, ex.last_wav, ex.last_R, ex.last_n_wav, &ctx->ev[0]);
    });
    ms_out[0] = sum / n_runs;
  });
}

// ------------------------------------------------------------------------------ per-order moments
int32_t prom_orders_set(prom_ctx* ctx, int32_t n_pix, int32_t n_seg, const int32_t* seg_first, const int32_t* perm,
                        const uint8_t* keep) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    ex.od_set = ex.od_ran = false;
    if (ex.dt_n_seg > 0) {   // a per-order filter belongs to the orders it was set for
      ex.dt_set = ex.dt_ran = false;
      ex.dt_n_seg = 0;
      if (ctx->rc.last == 1) ctx->rc.last = 0;
    }
    table_check(ctx, "prom_orders_set");
    PROM_REQUIRE(n_pix == ctx->obs.n_pix, "prom_orders_set: n_pix differs from the observation's");
    PROM_REQUIRE(n_seg >= 1 && seg_first && keep && (n_pix == 0 || perm), "prom_orders_set: orders missing");
    segments_check("prom_orders_set", n_pix, n_seg, seg_first, perm);
    for (int32_t i = 0; i < n_seg; ++i) PROM_REQUIRE(keep[i] <= 1, "prom_orders_set: keep must be 0 or 1");
    const hipStream_t st = ctx->stream;
    upload(ex.od_seg, seg_first, (int64_t)n_seg + 1, st);
    upload(ex.od_perm, perm, (int64_t)n_pix, st);
    upload(ex.od_keep, keep, (int64_t)n_seg, st);
    PROM_HIP(hipStreamSynchronize(st));   // the host arrays are read during the call only
    ex.od_n_seg = n_seg;
    ex.od_n_max = prom::os_n_max(n_seg, seg_first);
    ex.od_seg_host.assign(seg_first, seg_first + n_seg + 1);
    ex.od_perm_host.assign(perm, perm + n_pix);
    ex.od_set = true;
  });
}

int32_t prom_transit_expose_orders(prom_ctx* ctx, int32_t highpass, int32_t detrend, double* mom_out,
                                   int64_t* n_used_out, double* orec_mom_out, int64_t* orec_n_used_out, double* tot_out,
                                   double* model_out) {
  return guarded(ctx, [&] {
    orders_entry(ctx, "prom_transit_expose_orders", kLastRun, highpass, detrend,
                 ExOut{mom_out, n_used_out, orec_mom_out, orec_n_used_out, tot_out, model_out});
  });
}

int32_t prom_spectrum_expose_orders(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                    int32_t highpass, int32_t detrend, double* mom_out, int64_t* n_used_out,
                                    double* orec_mom_out, int64_t* orec_n_used_out, double* tot_out,
                                    double* model_out) {
  return guarded(ctx, [&] {
    orders_entry(ctx, "prom_spectrum_expose_orders", callers(n_orb, n_wav, wav, R), highpass, detrend,
                 ExOut{mom_out, n_used_out, orec_mom_out, orec_n_used_out, tot_out, model_out});
  });
}

int32_t prom_orders_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_orders_kernel_ms: bad arguments");
    if (!ex.set || !ex.od_set || !ex.od_ran || !ctx->obs.set || ctx->obs.n_pix == 0)
      throw Error(PROM_E_STATE, "prom_orders_kernel_ms: no per-order call to repeat");
    // the two kernels read the final model and the flags the last call left; the first batch, scaled to the table by
    // trial count
    const double scale = first_batch_scale(ex.n_trial, od_batches(ctx).nb_max);
    double sum[2];
    time_launches(ctx, ctx->stream, n_runs, 2, sum,
                 [&] { orders_launch(ctx, ctx->stream, ex.data.as<double>(), nullptr, nullptr, ctx->ev); });
    ms_out[0] = scale * sum[0] / n_runs;
    ms_out[1] = scale * sum[1] / n_runs;
  });
}

}  // extern "C"
