// C-ABI layer, the injections' side: the raw exposures, clean / inject, the filter's weights, the recovery and the
// injection grids (declared in include/prom_hip.h).  One runner, inject_buffers and inject_steps, stands behind every
// call: a single clean, inject or recover call is the grid of one.  The recovery runs the exposures' chain
// (prom_api_chain.h, prom_api_expose.hip).  Host code only: argument checks, copies and kernel launches on the context's
// streams.
#include <cstdio>
#include <cstdlib>

#include "prom_api_chain.h"
#include "highpass_index.h"
#include "order_index.h"
#include "sysrem_index.h"
#include "filter_index.h"
#include "grid_index.h"
#include "order_sysrem_index.h"

using namespace prom::api;

namespace {

// an injection's spectrum: none (clean), the last run's, or the caller's in the raw exposures' wav / R buffers
TransitArgs sy_args(prom_ctx* ctx, const char* who, const Spectrum& s) {
  prom::SyDev& sy = ctx->sy;
  if (s.source == 1) return TransitArgs{ctx->stream, nullptr, nullptr, 0};
  if (s.source == 2) return transit_args(ctx, who, ctx->ex.n_orb, "the exposure table");
  const hipStream_t st = spectrum_args(ctx, who, s.n_orb, ctx->ex.n_orb, "the observation's", s.n_wav, s.wav, s.R, sy.wav,
                                       sy.R, [&] { sy.last_source = 0; });
  sy.last_n_orb = s.n_orb;
  return TransitArgs{st, sy.wav.as<double>(), sy.R.as<double>(), s.n_wav};
}

// what a clean / inject call asks for (source: the Spectrum's; a grid's trial and scale are 0, its list has its own checks)
struct SyCall {
  int32_t source, trial, highpass, n_comp, n_iter, ones;
  double scale;
  int32_t orders;   // 1: SYSREM per resident order (prom_orders_set), U gains the order dimension
};

// the batch items of one injection and their width: the resident orders and the longest of them, or the table
int32_t sy_items(const prom_ctx* ctx, const SyCall& c) { return c.orders ? ctx->ex.od_n_seg : 1; }
int32_t sy_width(const prom_ctx* ctx, const SyCall& c) { return c.orders ? ctx->ex.od_n_max : ctx->sy.n_pix; }

void sysrem_check(prom_ctx* ctx, const char* who, const SyCall& c) {
  const std::string w(who);
  expose_check(ctx, who);
  if (!ctx->sy.set)
    throw Error(PROM_E_STATE, w + ": no raw exposures on the context (prom_sysrem_set; a later prom_expose_set, or "
                                  "whatever drops the exposure table, drops them)");
  if (c.highpass != 0 && c.highpass != 1) throw Error(PROM_E_ARG, w + ": highpass must be 0 or 1");
  if (c.ones != 0 && c.ones != 1) throw Error(PROM_E_ARG, w + ": ones must be 0 or 1");
  if (c.n_comp < 0 || c.n_comp + c.ones < 1 || c.n_comp + c.ones > prom::kSyMaxComp)
    throw Error(PROM_E_ARG, w + ": n_comp >= 0 and 1 <= n_comp + ones <= 16");
  if (c.n_iter < 1) throw Error(PROM_E_ARG, w + ": n_iter must be >= 1");
  if (c.source != 1) {
    if (c.trial < 0 || c.trial >= ctx->ex.n_trial) throw Error(PROM_E_ARG, w + ": trial outside [0, n_trial)");
    if (!std::isfinite(c.scale)) throw Error(PROM_E_ARG, w + ": scale must be finite");
  }
  if (c.highpass && !ctx->ex.hp_set)
    throw Error(PROM_E_STATE, w + ": highpass = 1 without a high-pass on the context (prom_highpass_set)");
  if (c.orders && !ctx->ex.od_set)
    throw Error(PROM_E_STATE, w + ": no orders on the context (prom_orders_set)");
  if (c.orders && ctx->ex.od_n_seg > prom::kGrMaxBatch)
    throw Error(PROM_E_ARG, w + ": more than 65535 orders");
}

// ---- the runner of every injection ----------------------------------------------------------------------------------------
// the work buffers of up to nb injections at once (a single call: nb = 1), the only place that sizes them; a clean call
// forms no model and asks for none of the model's buffers
void inject_buffers(prom_ctx* ctx, const SyCall& c, int32_t nb, int64_t n_wav, bool recover) {
  prom::SyDev& sy = ctx->sy;
  const prom::ExDev& ex = ctx->ex;
  const int32_t n_exp = sy.n_exp, n_pix = sy.n_pix, n_cols = c.n_comp + c.ones;
  const int32_t width = sy_width(ctx, c);
  const size_t B = (size_t)nb, n = (size_t)n_exp * n_pix, work = (size_t)(n_exp * prom::sy_pitch(width));
  const size_t items = B * (size_t)sy_items(ctx, c);   // (per order: an item per order of every injection)
  sy.D.ensure(sizeof(double) * B * n);
  sy.out.ensure(sizeof(double) * B * n);
  sy.r.ensure(sizeof(double) * items * work);
  sy.w.ensure(sizeof(double) * items * work);
  sy.a.ensure(sizeof(double) * items * n_exp);
  sy.ended.ensure(sizeof(int32_t) * items * prom::kGrFlags);
  sy.part.ensure(2 * sizeof(double) * items * n_exp * prom::sy_tiles(width));
  sy.U.ensure(sizeof(double) * items * n_exp * n_cols);
  if (recover) ctx->rc.W.ensure(sizeof(double) * B * n_cols * n);
  if (c.source == 1) return;
  sy.q.ensure(sizeof(double) * (size_t)n_wav);
  sy.Fj.ensure(sizeof(double) * B * n_exp * ex.n_tap);
  sy.model.ensure(sizeof(double) * B * n);
  sy.epart.ensure(sizeof(double) *
                  (size_t)prom::vm_part_doubles(n_exp, vm_batches(ctx, n_exp, nb).nb_max, prom::vm_chunks(n_pix)));
}

// the steps of the injections [b0, b0 + nb) of the list in sy.trial / sy.scale, nothing waits: D (injected, high-passed),
// out (cleaned) and U of the sub-batch stay in sy.D, sy.out and sy.U as [nb][...].  A clean call (nb = 1) copies raw
// in the injection's place.  ev: six events around the injection, the high-pass and SYSREM
void inject_steps(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int64_t n_wav, const SyCall& c,
                  int32_t b0, int32_t nb, hipEvent_t* ev = nullptr) {
  prom::SyDev& sy = ctx->sy;
  prom::ExDev& ex = ctx->ex;
  const prom::ObsDev& ob = ctx->obs;
  const int32_t n_exp = sy.n_exp, n_pix = sy.n_pix;
  if (ev) PROM_HIP(hipEventRecord(ev[0], st));
  if (c.source != 1) {
    const double nan = std::nan("");
    if (b0 == 0) prom::launch_observe_q(st, wav, (int32_t)n_wav, nan, nan, sy.q.as<double>());   // (of the whole list)
    // the models of the listed trials: their factors as a table of nb trials, through k_expose unchanged
    prom::launch_gather_grid(st, ex.F.as<double>(), sy.Fj.as<double>(), sy.trial.as<int32_t>() + b0, n_exp, ex.n_trial,
                             ex.n_tap, nb);
    const VmBatches vb = vm_batches(ctx, n_exp, nb);
    for (int32_t g = 0; g < vb.n_groups; g += vb.bg) {
      const int32_t j_first = prom::vm_group_first(g), nj = std::min(vb.nb_max, nb - j_first);
      prom::launch_expose(st, wav, sy.q.as<double>(), R, (int32_t)n_wav, ob.lam.as<double>(), ob.sig.as<double>(), ob.k,
                          ex.row.as<int32_t>(), ex.a.as<double>(), sy.Fj.as<double>(), ex.data.as<double>(),
                          ex.ivar.as<double>(), n_pix, n_exp, nb, ex.n_tap, j_first, nj, sy.epart.as<double>(),
                          sy.model.as<double>(), nullptr, nullptr);
    }
    prom::launch_inject_grid(st, sy.raw.as<double>(), sy.model.as<double>(), sy.scale.as<double>() + b0,
                             sy.D.as<double>(), n_exp, n_pix, nb);
  } else {
    PROM_HIP(hipMemcpyAsync(sy.D.p, sy.raw.p, sizeof(double) * (size_t)n_exp * n_pix, hipMemcpyDeviceToDevice, st));
  }
  if (ev) PROM_HIP(hipEventRecord(ev[1], st));
  if (ev) PROM_HIP(hipEventRecord(ev[2], st));
  if (c.highpass) highpass_launch(ex, st, sy.D.as<double>(), (int64_t)nb * n_exp, n_pix);
  if (ev) PROM_HIP(hipEventRecord(ev[3], st));
  if (ev) PROM_HIP(hipEventRecord(ev[4], st));
  if (c.orders)
    prom::launch_sysrem_orders(st, sy.D.as<double>(), ex.ivar.as<double>(), ex.od_seg.as<int32_t>(),
                               ex.od_perm.as<int32_t>(), sy.r.as<double>(), sy.w.as<double>(), sy.a.as<double>(),
                               sy.ended.as<int32_t>(), sy.part.as<double>(), sy.U.as<double>(), sy.out.as<double>(),
                               n_exp, n_pix, ex.od_n_seg, ex.od_n_max, c.n_comp, c.n_iter, c.ones, nb);
  else
    prom::launch_sysrem(st, sy.D.as<double>(), ex.ivar.as<double>(), sy.r.as<double>(), sy.w.as<double>(),
                        sy.a.as<double>(), sy.ended.as<int32_t>(), sy.part.as<double>(), sy.U.as<double>(),
                        sy.out.as<double>(), n_exp, n_pix, c.n_comp, c.n_iter, c.ones, nb);
  if (ev) PROM_HIP(hipEventRecord(ev[5], st));
}

// no pixel: every component of each of `rows` rows of U ends at once
void zero_U(const SyCall& c, int64_t rows, double* U_out) {
  const int32_t n_cols = c.n_comp + c.ones;
  if (!U_out) return;
  for (int64_t i = 0; i < rows; ++i)
    for (int32_t k = 0; k < n_cols; ++k) U_out[i * n_cols + k] = (c.ones && k == 0) ? 1.0 : 0.0;
}

// ---- clean and inject: the grid of one ------------------------------------------------------------------------------------
// the shared tail of the clean / inject calls (ev: the runner's events, and the call runs even without an output;
// recover: a recover call goes on on the same stream, so the call runs whatever the outputs, sizes W and does not wait)
void sysrem_on(prom_ctx* ctx, const TransitArgs& t, const SyCall& c, double* U_out, double* cleaned_out,
               double* injected_out, hipEvent_t* ev, bool recover = false) {
  prom::SyDev& sy = ctx->sy;
  const int32_t n_exp = sy.n_exp, n_pix = sy.n_pix;
  const int64_t n = (int64_t)n_exp * n_pix, nu = (int64_t)sy_items(ctx, c) * n_exp * (c.n_comp + c.ones);
  if (n_pix == 0) return zero_U(c, (int64_t)sy_items(ctx, c) * n_exp, U_out);
  if (!recover && !ev && !U_out && !cleaned_out && !injected_out) return;
  if (ctx->rc.last == 2) ctx->rc.last = 0;   // (U may move or change its shape)
  if (c.highpass && prom::hp_workgroups(n_exp, ctx->ex.hp_n_seg) > kMaxGrid)   // (before anything is launched)
    throw Error(PROM_E_ARG, "k_highpass: n_exp n_seg too large for one launch");
  inject_buffers(ctx, c, 1, t.n_wav, recover);
  if (c.source != 1) {   // the list of one entry; its host side lives as long as the context, so no wait covers the copies
    sy.one_trial = c.trial;
    sy.one_scale = c.scale;
    upload(sy.trial, &sy.one_trial, 1, t.st);
    upload(sy.scale, &sy.one_scale, 1, t.st);
  }
  inject_steps(ctx, t.st, t.wav, t.R, t.n_wav, c, 0, 1, ev);
  sy.last_source = c.source;
  sy.last_trial = c.trial;
  sy.last_scale = c.scale;
  sy.last_highpass = c.highpass;
  sy.last_n_comp = c.n_comp;
  sy.last_n_iter = c.n_iter;
  sy.last_ones = c.ones;
  sy.last_n_wav = t.n_wav;
  sy.last_orders = c.orders;
  if (U_out) download(U_out, sy.U, nu, t.st);
  if (cleaned_out) download(cleaned_out, sy.out, n, t.st);
  if (injected_out) download(injected_out, sy.D, n, t.st);
  if (!recover) PROM_HIP(hipStreamSynchronize(t.st));
}

void inject_entry(prom_ctx* ctx, const char* who, const Spectrum& s, SyCall c, double* U_out, double* cleaned_out,
                  double* injected_out) {
  c.source = s.source;
  sysrem_check(ctx, who, c);
  sysrem_on(ctx, sy_args(ctx, who, s), c, U_out, cleaned_out, injected_out, nullptr);
}

// ---- the recovery -------------------------------------------------------------------------------------------------------
void recover_check(prom_ctx* ctx, const char* who, const SyCall& c, int32_t orders) {
  const std::string w(who);
  sysrem_check(ctx, who, c);
  if (orders != 0 && orders != 1) throw Error(PROM_E_ARG, w + ": orders must be 0 or 1");
  if (orders && !ctx->ex.od_set)
    throw Error(PROM_E_STATE, w + ": orders = 1 without orders on the context (prom_orders_set)");
}

// the chain (highpass, detrend = 1) with the cleaned data in the place of the table's and (U, W) of the injection in the
// place of the resident filter
ChainCall recover_call(prom_ctx* ctx, const SyCall& c, int32_t orders, const ExOut& out) {
  return ChainCall{c.highpass != 0, true, orders != 0, &ctx->sy.U, &ctx->rc.W, c.n_comp + c.ones, &ctx->sy.out, Ran::none,
                   true, "the recovery keeps", out};
}

// the shared tail of the two recover calls: the inject call's steps, W of (U, ivar), then the chain.  Without `orders`
// the per-order outputs are not looked at
void recover_on(prom_ctx* ctx, const TransitArgs& t, const SyCall& c, int32_t orders, ExOut out, double* U_out) {
  prom::ExDev& ex = ctx->ex;
  prom::RcDev& rc = ctx->rc;
  const int32_t n_pix = ctx->obs.n_pix, n_cols = c.n_comp + c.ones;
  if (!orders) out.orec_mom = out.tot = nullptr;
  if (!orders) out.orec_n_used = nullptr;
  const ChainCall cc = recover_call(ctx, c, orders, out);
  if (n_pix == 0) sysrem_on(ctx, t, c, U_out, nullptr, nullptr, nullptr);   // no pixel: the inject call's U
  if (!chain_prepare(ctx, cc, t.n_wav)) return;
  // the last calls' q, models and flags go: the aids of the expose calls have nothing to repeat
  record_last(ex, nullptr, nullptr, 0, Ran::none, 0);
  // 1: the inject call's steps; the cleaned data stay in sy.out and U in sy.U
  sysrem_on(ctx, t, c, U_out, nullptr, nullptr, nullptr, true);
  // 2: W of (U, the table's ivar)
  prom::launch_filter_weights(t.st, ctx->sy.U.as<double>(), ex.ivar.as<double>(), rc.W.as<double>(), ex.n_exp, n_cols,
                              n_pix, nullptr, nullptr);
  rc.last = 2;
  rc.last_n_comp = n_cols;
  // 3: the final model and the moments against the cleaned data
  chain_go(ctx, t.st, cc, t.wav, t.R, t.n_wav);
}

void recover_entry(prom_ctx* ctx, const char* who, const Spectrum& s, SyCall c, int32_t orders, const ExOut& out,
                   double* U_out) {
  c.source = s.source;
  recover_check(ctx, who, c, orders);
  recover_on(ctx, sy_args(ctx, who, s), c, orders, out, U_out);
}

// ---- injection grids ------------------------------------------------------------------------------------------------------
// a list of injections: entry b is (trial[b], scale[b])
struct GridList {
  int32_t n_inj;
  const int32_t* trial;
  const double* scale;
};

// the cap on the work buffers of a sub-batch, read at every grid call
int64_t grid_cap_bytes() {
  double mb = 4096.0;
  if (const char* e = std::getenv("PROM_GRID_SCRATCH_MB")) {
    const double v = std::atof(e);
    if (v > 0.0 && v < 1.0e7) mb = v;
  }
  return std::max<int64_t>(1, (int64_t)(mb * 1048576.0));
}

// the refusals of the list, after the single calls' own
void grid_check(prom_ctx* ctx, const char* who, const GridList& g) {
  const std::string w(who);
  if (g.n_inj < 0) throw Error(PROM_E_ARG, w + ": n_inj must be >= 0");
  if (g.n_inj > 0 && (!g.trial || !g.scale)) throw Error(PROM_E_ARG, w + ": trial and scale missing");
  for (int32_t b = 0; b < g.n_inj; ++b) {
    if (g.trial[b] < 0 || g.trial[b] >= ctx->ex.n_trial)
      throw Error(PROM_E_ARG, w + ": trial outside [0, n_trial) in entry " + std::to_string(b));
    if (!std::isfinite(g.scale[b])) throw Error(PROM_E_ARG, w + ": scale must be finite in entry " + std::to_string(b));
  }
}

// injections of a sub-batch under the cap, and the launches of a sub-batch that grow with it, before anything runs
int32_t grid_plan(prom_ctx* ctx, const SyCall& c, int32_t n_inj, bool recover) {
  const prom::ExDev& ex = ctx->ex;
  const int64_t per = c.orders ? prom::os_injection_bytes(ex.n_exp, ctx->obs.n_pix, ex.od_n_seg, ex.od_n_max,
                                                          c.n_comp + c.ones, ex.n_tap)
                               : prom::gr_injection_bytes(ex.n_exp, ctx->obs.n_pix, c.n_comp + c.ones, ex.n_tap, recover);
  const int32_t nb = c.orders ? prom::os_sub_batch(grid_cap_bytes(), per, n_inj, ex.od_n_seg)
                              : prom::gr_sub_batch(grid_cap_bytes(), per, n_inj);
  if (c.highpass && prom::hp_workgroups((int64_t)nb * ex.n_exp, ex.hp_n_seg) > kMaxGrid)
    throw Error(PROM_E_ARG, "k_highpass: n_inj n_exp n_seg too large for one launch");
  static const bool debug = std::getenv("PROM_DEBUG") != nullptr;
  if (debug)
    std::fprintf(stderr, "prom: injection grid: %d injections in %d sub-batches of up to %d, %lld bytes each\n", n_inj,
                 prom::gr_sub_batches(n_inj, nb), nb, (long long)per);
  return nb;
}

// what every grid call does before its sub-batches: the work buffers hold a sub-batch from here on, so
// prom_sysrem_kernel_ms has no call to repeat, nor has prom_filter_kernel_ms after a recover call; the buffers of
// sub-batches of up to nb injections, and the list on the device (the sub-batches' waits cover the caller's arrays)
void grid_begin(prom_ctx* ctx, hipStream_t st, const SyCall& c, const GridList& g, int32_t nb, int64_t n_wav,
                bool recover) {
  ctx->sy.last_source = 0;
  if (ctx->rc.last == 2) ctx->rc.last = 0;
  inject_buffers(ctx, c, nb, n_wav, recover);
  upload(ctx->sy.trial, g.trial, g.n_inj, st);
  upload(ctx->sy.scale, g.scale, g.n_inj, st);
}

// the shared tail of the two inject grid calls
void inject_grid_on(prom_ctx* ctx, const TransitArgs& t, const SyCall& c, const GridList& g, double* U_out,
                    double* cleaned_out, double* injected_out) {
  prom::SyDev& sy = ctx->sy;
  const int32_t n_exp = sy.n_exp, n_pix = sy.n_pix;
  const int64_t n = (int64_t)n_exp * n_pix, nu = (int64_t)sy_items(ctx, c) * n_exp * (c.n_comp + c.ones);
  if (n_pix == 0) return zero_U(c, (int64_t)g.n_inj * sy_items(ctx, c) * n_exp, U_out);
  if (g.n_inj == 0 || (!U_out && !cleaned_out && !injected_out)) return;
  const int32_t nb_max = grid_plan(ctx, c, g.n_inj, false);
  grid_begin(ctx, t.st, c, g, nb_max, t.n_wav, false);
  for (int32_t s = 0; s < prom::gr_sub_batches(g.n_inj, nb_max); ++s) {
    const int32_t b0 = prom::gr_sub_first(s, nb_max), nb = prom::gr_sub_count(s, nb_max, g.n_inj);
    inject_steps(ctx, t.st, t.wav, t.R, t.n_wav, c, b0, nb);
    if (U_out) download(U_out + b0 * nu, sy.U, nb * nu, t.st);
    if (cleaned_out) download(cleaned_out + b0 * n, sy.out, nb * n, t.st);
    if (injected_out) download(injected_out + b0 * n, sy.D, nb * n, t.st);
    PROM_HIP(hipStreamSynchronize(t.st));   // (the next sub-batch writes the same buffers; the last: the end of the call)
  }
}

void inject_grid_entry(prom_ctx* ctx, const char* who, const Spectrum& s, SyCall c, const GridList& g, double* U_out,
                       double* cleaned_out, double* injected_out) {
  c.source = s.source;
  sysrem_check(ctx, who, c);
  grid_check(ctx, who, g);
  inject_grid_on(ctx, sy_args(ctx, who, s), c, g, U_out, cleaned_out, injected_out);
}

// the shared tail of the two recover grid calls: the model of every trial before the filter once (the chain's first
// half) into ex.model, which then stays; per sub-batch the runner's steps and W of every (U[b], ivar); per injection
// the filter out of place into rc.model and the moments against cleaned[b]
void recover_grid_on(prom_ctx* ctx, const TransitArgs& t, const SyCall& c, int32_t orders, const GridList& g,
                     double* mom_out, int64_t* n_used_out, double* tot_out, double* U_out) {
  prom::ExDev& ex = ctx->ex;
  prom::SyDev& sy = ctx->sy;
  prom::RcDev& rc = ctx->rc;
  const hipStream_t st = t.st;
  const int32_t n_pix = ctx->obs.n_pix, n_exp = ex.n_exp, n_cols = c.n_comp + c.ones;
  const int64_t nu = (int64_t)n_exp * n_cols, nm = (int64_t)n_exp * ex.n_trial;
  if (!orders) tot_out = nullptr;
  if (n_pix == 0) {   // no pixel: zeros, and the inject call's U
    zero_moments(g.n_inj * nm, mom_out, n_used_out);
    if (tot_out) std::fill(tot_out, tot_out + prom::kOdTotals * g.n_inj * nm, 0.0);
    return zero_U(c, (int64_t)g.n_inj * n_exp, U_out);
  }
  if (g.n_inj == 0) return;
  const ChainCall cc = recover_call(ctx, c, orders, ExOut{});
  const int32_t nb_max = grid_plan(ctx, c, g.n_inj, true);
  chain_prepare(ctx, cc, t.n_wav);
  try {   // the filtered model of one injection beside the unfiltered one
    rc.model.ensure(sizeof(double) * (size_t)(nm * n_pix));
  } catch (const Error& err) {
    throw Error(err.code, std::string(err.what()) + ": the recovery grid keeps a second model of all " +
                              std::to_string(ex.n_trial) + " trials in device memory; give fewer trials per call");
  }
  record_last(ex, nullptr, nullptr, 0, Ran::none, 0);
  grid_begin(ctx, st, c, g, nb_max, t.n_wav, true);
  const double nan = std::nan("");
  prom::launch_observe_q(st, t.wav, (int32_t)t.n_wav, nan, nan, ex.q.as<double>());
  chain_unfiltered(ctx, st, cc, t.wav, t.R, (int32_t)t.n_wav);
  for (int32_t s = 0; s < prom::gr_sub_batches(g.n_inj, nb_max); ++s) {
    const int32_t b0 = prom::gr_sub_first(s, nb_max), nb = prom::gr_sub_count(s, nb_max, g.n_inj);
    inject_steps(ctx, st, t.wav, t.R, t.n_wav, c, b0, nb);
    if (U_out) download(U_out + b0 * nu, sy.U, nb * nu, st);
    prom::launch_filter_weights(st, sy.U.as<double>(), ex.ivar.as<double>(), rc.W.as<double>(), n_exp, n_cols, n_pix,
                                nullptr, nullptr, nb);
    for (int32_t b = 0; b < nb; ++b) {
      const double* cleaned = sy.out.as<double>() + prom::gr_data(b, n_exp, n_pix);
      prom::launch_detrend(st, rc.model.as<double>(), sy.U.as<double>() + prom::gr_u(b, n_exp, n_cols),
                           rc.W.as<double>() + prom::gr_w(b, n_cols, n_exp, n_pix), ex.flag.as<uint8_t>(), n_exp, n_cols,
                           ex.n_trial, n_pix, nullptr, nullptr, ex.model.as<double>());
      if (mom_out || n_used_out) moments_launch(ctx, st, cleaned, nullptr, nullptr, rc.model.as<double>());
      if (mom_out) download(mom_out + 7 * nm * (b0 + b), ex.mom, 7 * nm, st);
      if (n_used_out) download(n_used_out + nm * (b0 + b), ex.n_used, nm, st);
      if (tot_out) {
        orders_launch(ctx, st, cleaned, nullptr, nullptr, nullptr, rc.model.as<double>());
        download(tot_out + prom::kOdTotals * nm * (b0 + b), ex.od_tot, prom::kOdTotals * nm, st);
      }
    }
    PROM_HIP(hipStreamSynchronize(st));   // (the next sub-batch writes the same buffers; the last: the end of the call)
  }
}

void recover_grid_entry(prom_ctx* ctx, const char* who, const Spectrum& s, SyCall c, int32_t orders, const GridList& g,
                        double* mom_out, int64_t* n_used_out, double* tot_out, double* U_out) {
  c.source = s.source;
  recover_check(ctx, who, c, orders);
  grid_check(ctx, who, g);
  recover_grid_on(ctx, sy_args(ctx, who, s), c, orders, g, mom_out, n_used_out, tot_out, U_out);
}

// ---- the filter's weights of a caller's U and ivar (orders: a basis per order, pixel p takes that of seg_of[p]) -----------
void filter_weights(prom_ctx* ctx, const char* who, bool orders, int32_t n_exp, int32_t n_comp, int32_t n_pix,
                    int32_t n_seg, const int32_t* seg_of, const double* U, const double* ivar, double* W_out) {
  prom::RcDev& rc = ctx->rc;
  const std::string w(who);
  PROM_REQUIRE(n_comp >= 1 && n_comp <= prom::kDtMaxComp, w + ": n_comp must lie in [1, 16]");
  PROM_REQUIRE(n_exp >= 1 && n_pix >= 0 && n_seg >= 1,
               w + (orders ? ": n_exp and n_seg must be >= 1 and n_pix >= 0" : ": n_exp must be >= 1 and n_pix >= 0"));
  const int64_t nu = (int64_t)n_seg * n_exp * n_comp, ni = (int64_t)n_exp * n_pix, nw = ni * n_comp;
  PROM_REQUIRE(U && (n_pix == 0 || (ivar && W_out && (seg_of || !orders))),
               w + (orders ? ": U, seg_of, ivar or W_out missing" : ": U, ivar or W_out missing"));
  for (int64_t i = 0; i < nu; ++i) PROM_REQUIRE(obs_finite(U[i]), w + ": U must be finite");
  for (int32_t p = 0; orders && p < n_pix; ++p)
    PROM_REQUIRE(seg_of[p] >= 0 && seg_of[p] < n_seg, w + ": seg_of outside [0, n_seg)");
  if (n_pix == 0) return;
  const hipStream_t st = ctx->stream;
  upload(rc.fU, U, nu, st);
  upload(rc.fivar, ivar, ni, st);
  if (orders) upload(rc.fseg, seg_of, (int64_t)n_pix, st);
  rc.fW.ensure(sizeof(double) * (size_t)nw);
  if (orders)
    prom::launch_filter_weights_orders(st, rc.fU.as<double>(), rc.fivar.as<double>(), rc.fseg.as<int32_t>(),
                                       rc.fW.as<double>(), n_exp, n_comp, n_pix, nullptr, nullptr);
  else
    prom::launch_filter_weights(st, rc.fU.as<double>(), rc.fivar.as<double>(), rc.fW.as<double>(), n_exp, n_comp, n_pix,
                                nullptr, nullptr);
  download(W_out, rc.fW, nw, st);
  PROM_HIP(hipStreamSynchronize(st));
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------ injection and SYSREM
int32_t prom_sysrem_set(prom_ctx* ctx, int32_t n_exp, int32_t n_pix, const double* raw) {
  return guarded(ctx, [&] {
    prom::SyDev& sy = ctx->sy;
    sy.set = false;
    sy.last_source = 0;
    table_check(ctx, "prom_sysrem_set");
    PROM_REQUIRE(n_exp == ctx->ex.n_exp && n_pix == ctx->obs.n_pix,
                 "prom_sysrem_set: raw must be [n_exp][n_pix] of the exposure table");
    PROM_REQUIRE(n_exp <= prom::kSyMaxExp, "prom_sysrem_set: more than 4096 exposures");
    const int64_t n = (int64_t)n_exp * n_pix;
    PROM_REQUIRE(n == 0 || raw, "prom_sysrem_set: raw missing");
    const hipStream_t st = ctx->stream;
    upload(sy.raw, raw, n, st);
    PROM_HIP(hipStreamSynchronize(st));   // the host array is read during the call only
    sy.n_exp = n_exp;
    sy.n_pix = n_pix;
    sy.set = true;
  });
}

int32_t prom_sysrem_clean(prom_ctx* ctx, int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out,
                          double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    inject_entry(ctx, "prom_sysrem_clean", kNoSpectrum, SyCall{0, 0, highpass, n_comp, n_iter, ones, 0.0, 0}, U_out,
                 cleaned_out, injected_out);
  });
}

int32_t prom_transit_inject(prom_ctx* ctx, int32_t trial, double scale, int32_t highpass, int32_t n_comp, int32_t n_iter,
                            int32_t ones, double* U_out, double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    inject_entry(ctx, "prom_transit_inject", kLastRun, SyCall{0, trial, highpass, n_comp, n_iter, ones, scale, 0}, U_out,
                 cleaned_out, injected_out);
  });
}

int32_t prom_spectrum_inject(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                             int32_t trial, double scale, int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones,
                             double* U_out, double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    inject_entry(ctx, "prom_spectrum_inject", callers(n_orb, n_wav, wav, R),
                 SyCall{0, trial, highpass, n_comp, n_iter, ones, scale, 0}, U_out, cleaned_out, injected_out);
  });
}

// SYSREM per order: the same calls with every resident order (prom_orders_set) cleaned on its own; U_out gains the
// order dimension, [n_seg][n_exp][n_comp + ones]
int32_t prom_sysrem_clean_orders(prom_ctx* ctx, int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones,
                                 double* U_out, double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    inject_entry(ctx, "prom_sysrem_clean_orders", kNoSpectrum, SyCall{0, 0, highpass, n_comp, n_iter, ones, 0.0, 1},
                 U_out, cleaned_out, injected_out);
  });
}

int32_t prom_transit_inject_orders(prom_ctx* ctx, int32_t trial, double scale, int32_t highpass, int32_t n_comp,
                                   int32_t n_iter, int32_t ones, double* U_out, double* cleaned_out,
                                   double* injected_out) {
  return guarded(ctx, [&] {
    inject_entry(ctx, "prom_transit_inject_orders", kLastRun, SyCall{0, trial, highpass, n_comp, n_iter, ones, scale, 1},
                 U_out, cleaned_out, injected_out);
  });
}

int32_t prom_spectrum_inject_orders(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                    int32_t trial, double scale, int32_t highpass, int32_t n_comp, int32_t n_iter,
                                    int32_t ones, double* U_out, double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    inject_entry(ctx, "prom_spectrum_inject_orders", callers(n_orb, n_wav, wav, R),
                 SyCall{0, trial, highpass, n_comp, n_iter, ones, scale, 1}, U_out, cleaned_out, injected_out);
  });
}

int32_t prom_sysrem_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::SyDev& sy = ctx->sy;
    prom::TransitDev& tr = ctx->tr;
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_sysrem_kernel_ms: bad arguments");
    const bool table = table_present(ctx) && sy.set && sy.n_pix > 0;
    if (!table || sy.last_source == 0 || (sy.last_highpass && !ctx->ex.hp_set) || (sy.last_orders && !ctx->ex.od_set) ||
        (sy.last_source == 2 && (!tr.ran || ctx->ex.n_orb != tr.n_orb || tr.n_wav != sy.last_n_wav)) ||
        (sy.last_source == 3 && sy.last_n_orb != ctx->ex.n_orb))
      throw Error(PROM_E_STATE, "prom_sysrem_kernel_ms: no clean or inject call to repeat");
    const SyCall c{sy.last_source, sy.last_trial, sy.last_highpass, sy.last_n_comp, sy.last_n_iter, sy.last_ones,
                   sy.last_scale, sy.last_orders};
    const TransitArgs t{ctx->stream, c.source == 2 ? tr.wav.as<double>() : sy.wav.as<double>(),
                        c.source == 2 ? transit_R(ctx) : sy.R.as<double>(), sy.last_n_wav};
    double sum[3];   // the injection, the high-pass, SYSREM
    time_launches(ctx, ctx->stream, n_runs, 3, sum,
                  [&] { sysrem_on(ctx, t, c, nullptr, nullptr, nullptr, ctx->ev); });
    ms_out[0] = sum[2] / n_runs;
    ms_out[1] = c.source != 1 ? sum[0] / n_runs : std::nan("");
    ms_out[2] = c.highpass ? sum[1] / n_runs : std::nan("");
  });
}

// ------------------------------------------------------------------------------ the filter's weights and the recovery
int32_t prom_filter_weights(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, int32_t n_pix, const double* U,
                            const double* ivar, double* W_out) {
  return guarded(ctx, [&] {
    filter_weights(ctx, "prom_filter_weights", false, n_exp, n_comp, n_pix, 1, nullptr, U, ivar, W_out);
  });
}

int32_t prom_filter_weights_orders(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, int32_t n_pix, int32_t n_seg,
                                   const int32_t* seg_of, const double* U, const double* ivar, double* W_out) {
  return guarded(ctx, [&] {
    filter_weights(ctx, "prom_filter_weights_orders", true, n_exp, n_comp, n_pix, n_seg, seg_of, U, ivar, W_out);
  });
}

int32_t prom_filter_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::RcDev& rc = ctx->rc;
    prom::ExDev& ex = ctx->ex;
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_filter_kernel_ms: bad arguments");
    const bool table = table_present(ctx) && ctx->obs.n_pix > 0;
    const bool built = rc.last == 1 && ex.dt_set && ex.n_comp == rc.last_n_comp;
    const bool recovered = rc.last == 2 && ctx->sy.set && ctx->sy.last_source != 0 &&
                           ctx->sy.last_n_comp + ctx->sy.last_ones == rc.last_n_comp;
    if (!table || !(built || recovered))
      throw Error(PROM_E_STATE, "prom_filter_kernel_ms: no build or recover call to repeat");
    // the kernel writes the W it wrote before, from the same inputs: the same bits
    const double* U = built ? ex.U.as<double>() : ctx->sy.U.as<double>();
    double* W = built ? ex.W.as<double>() : rc.W.as<double>();
    double sum = 0.0;
    time_launches(ctx, ctx->stream, n_runs, 1, &sum, [&] {
      if (built && ex.dt_n_seg > 0)   // (a per-order build: its own instantiation)
        prom::launch_filter_weights_orders(ctx->stream, U, ex.ivar.as<double>(), ex.dt_seg_of.as<int32_t>(), W,
                                           ex.n_exp, rc.last_n_comp, ctx->obs.n_pix, ctx->ev[0], ctx->ev[1]);
      else
        prom::launch_filter_weights(ctx->stream, U, ex.ivar.as<double>(), W, ex.n_exp, rc.last_n_comp, ctx->obs.n_pix,
                                    ctx->ev[0], ctx->ev[1]);
    });
    ms_out[0] = sum / n_runs;
  });
}

int32_t prom_transit_recover(prom_ctx* ctx, int32_t trial, double scale, int32_t highpass, int32_t n_comp,
                             int32_t n_iter, int32_t ones, int32_t orders, double* mom_out, int64_t* n_used_out,
                             double* orec_mom_out, int64_t* orec_n_used_out, double* tot_out, double* U_out,
                             double* model_out) {
  return guarded(ctx, [&] {
    recover_entry(ctx, "prom_transit_recover", kLastRun, SyCall{0, trial, highpass, n_comp, n_iter, ones, scale, 0},
                  orders, ExOut{mom_out, n_used_out, orec_mom_out, orec_n_used_out, tot_out, model_out}, U_out);
  });
}

int32_t prom_spectrum_recover(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                              int32_t trial, double scale, int32_t highpass, int32_t n_comp, int32_t n_iter,
                              int32_t ones, int32_t orders, double* mom_out, int64_t* n_used_out,
                              double* orec_mom_out, int64_t* orec_n_used_out, double* tot_out, double* U_out,
                              double* model_out) {
  return guarded(ctx, [&] {
    recover_entry(ctx, "prom_spectrum_recover", callers(n_orb, n_wav, wav, R),
                  SyCall{0, trial, highpass, n_comp, n_iter, ones, scale, 0}, orders,
                  ExOut{mom_out, n_used_out, orec_mom_out, orec_n_used_out, tot_out, model_out}, U_out);
  });
}

// ------------------------------------------------------------------------------ injection grids
int32_t prom_transit_inject_grid(prom_ctx* ctx, int32_t n_inj, const int32_t* trial, const double* scale,
                                 int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out,
                                 double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    inject_grid_entry(ctx, "prom_transit_inject_grid", kLastRun, SyCall{0, 0, highpass, n_comp, n_iter, ones, 0.0, 0},
                      GridList{n_inj, trial, scale}, U_out, cleaned_out, injected_out);
  });
}

int32_t prom_spectrum_inject_grid(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                  int32_t n_inj, const int32_t* trial, const double* scale, int32_t highpass,
                                  int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out, double* cleaned_out,
                                  double* injected_out) {
  return guarded(ctx, [&] {
    inject_grid_entry(ctx, "prom_spectrum_inject_grid", callers(n_orb, n_wav, wav, R),
                      SyCall{0, 0, highpass, n_comp, n_iter, ones, 0.0, 0}, GridList{n_inj, trial, scale}, U_out,
                      cleaned_out, injected_out);
  });
}

// SYSREM per order over a grid: entry b is what the per-order inject call gives for (trial[b], scale[b]); U_out is
// [n_inj][n_seg][n_exp][n_comp + ones]
int32_t prom_transit_inject_grid_orders(prom_ctx* ctx, int32_t n_inj, const int32_t* trial, const double* scale,
                                        int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out,
                                        double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    inject_grid_entry(ctx, "prom_transit_inject_grid_orders", kLastRun,
                      SyCall{0, 0, highpass, n_comp, n_iter, ones, 0.0, 1}, GridList{n_inj, trial, scale}, U_out,
                      cleaned_out, injected_out);
  });
}

int32_t prom_spectrum_inject_grid_orders(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                         int32_t n_inj, const int32_t* trial, const double* scale, int32_t highpass,
                                         int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out,
                                         double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    inject_grid_entry(ctx, "prom_spectrum_inject_grid_orders", callers(n_orb, n_wav, wav, R),
                      SyCall{0, 0, highpass, n_comp, n_iter, ones, 0.0, 1}, GridList{n_inj, trial, scale}, U_out,
                      cleaned_out, injected_out);
  });
}

int32_t prom_transit_recover_grid(prom_ctx* ctx, int32_t n_inj, const int32_t* trial, const double* scale,
                                  int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, int32_t orders,
                                  double* mom_out, int64_t* n_used_out, double* tot_out, double* U_out) {
  return guarded(ctx, [&] {
    recover_grid_entry(ctx, "prom_transit_recover_grid", kLastRun, SyCall{0, 0, highpass, n_comp, n_iter, ones, 0.0, 0},
                       orders, GridList{n_inj, trial, scale}, mom_out, n_used_out, tot_out, U_out);
  });
}

int32_t prom_spectrum_recover_grid(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                   int32_t n_inj, const int32_t* trial, const double* scale, int32_t highpass,
                                   int32_t n_comp, int32_t n_iter, int32_t ones, int32_t orders, double* mom_out,
                                   int64_t* n_used_out, double* tot_out, double* U_out) {
  return guarded(ctx, [&] {
    recover_grid_entry(ctx, "prom_spectrum_recover_grid", callers(n_orb, n_wav, wav, R),
                       SyCall{0, 0, highpass, n_comp, n_iter, ones, 0.0, 0}, orders, GridList{n_inj, trial, scale},
                       mom_out, n_used_out, tot_out, U_out);
  });
}

}  // extern "C"
