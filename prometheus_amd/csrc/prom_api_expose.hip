// C-ABI layer, the exposures' side: the exposure table, its filter, high-pass and orders, the chain every filtered call
// runs, SYSREM, the filter's weights and the recovery (declared in include/prom_hip.h).  Host code only: argument
// checks, copies and kernel launches on the context's streams.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "prom_api_shared.h"
#include "detrend_index.h"
#include "highpass_index.h"
#include "order_index.h"
#include "sysrem_index.h"
#include "filter_index.h"
#include "grid_index.h"
#include "order_sysrem_index.h"

namespace {

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

// an exposure entry's arguments from a caller's spectrum, in the table's wav / R buffers (od: a per-order entry)
hipStream_t ex_spectrum(prom_ctx* ctx, const char* who, int32_t n_orb, int64_t n_wav, const double* wav,
                        const double* R, bool od = false) {
  prom::ExDev& ex = ctx->ex;
  return spectrum_args(ctx, who, n_orb, ex.n_orb, "the observation's", n_wav, wav, R, ex.wav, ex.R, [&] {
    ex.last_wav = ex.last_R = nullptr;
    if (od) ex.od_ran = false;
  });
}

// ... and an injection's, in the raw exposures' buffers
hipStream_t sy_spectrum(prom_ctx* ctx, const char* who, int32_t n_orb, int64_t n_wav, const double* wav,
                        const double* R) {
  prom::SyDev& sy = ctx->sy;
  const hipStream_t st = spectrum_args(ctx, who, n_orb, ctx->ex.n_orb, "the observation's", n_wav, wav, R, sy.wav, sy.R,
                                       [&] { sy.last_source = 0; });
  sy.last_n_orb = n_orb;
  return st;
}

TransitArgs ex_transit(prom_ctx* ctx, const char* who) {
  return transit_args(ctx, who, ctx->ex.n_orb, "the exposure table");
}

// ---- what every exposure call shares -----------------------------------------------------------------------------------
// the caller's arrays of an exposure call (null: not asked for); the per-order ones stay null outside those calls
struct ExOut {
  double* mom;
  int64_t* n_used;
  double* orec_mom;
  int64_t* orec_n_used;
  double* tot;
  double* model;
  bool moments() const { return mom || n_used; }
  bool orders() const { return orec_mom || orec_n_used || tot; }
  bool any() const { return moments() || orders() || model; }
};

ExOut plain_out(double* mom, int64_t* n_used, double* model) {
  return ExOut{mom, n_used, nullptr, nullptr, nullptr, model};
}

// no pixel: every moment, record and total 0 and no model value
void zero_outputs(const prom::ExDev& ex, const ExOut& o) {
  const int64_t n = (int64_t)ex.n_exp * ex.n_trial;
  zero_moments(n, o.mom, o.n_used);
  zero_moments(n * ex.od_n_seg, o.orec_mom, o.orec_n_used);
  if (o.tot) std::fill(o.tot, o.tot + prom::kOdTotals * n, 0.0);
}

// the resident high-pass, whichever kind it is (the weighted mean of prom_highpass_set or the median of
// prom_highpass_set_median), over n_rows rows of `model` in place
void highpass_launch(const prom::ExDev& ex, hipStream_t st, double* model, int64_t n_rows, int32_t n_pix,
                     hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr) {
  if (ex.hp_kind == 1)
    prom::launch_median(st, model, ex.hp_seg.as<int32_t>(), ex.hp_perm.as<int32_t>(), ex.hp_half, ex.hp_mode, n_rows,
                        ex.hp_n_seg, n_pix, ev0, ev1);
  else
    prom::launch_highpass(st, model, ex.hp_seg.as<int32_t>(), ex.hp_perm.as<int32_t>(), ex.hp_g.as<double>(),
                          ex.hp_half, ex.hp_den, ex.hp_mode, n_rows, ex.hp_n_seg, n_pix, ev0, ev1);
}

// which *_kernel_ms aid may repeat the call that ends
enum class Ran { none, detrend, highpass, orders };

// the "last call" state: the spectrum the call read (null: nothing to repeat) and the one aid that may repeat it
void record_last(prom::ExDev& ex, const double* wav, const double* R, int64_t n_wav, Ran ran, int32_t detrend) {
  ex.last_wav = wav;
  ex.last_R = R;
  ex.last_n_wav = (int32_t)n_wav;
  ex.dt_ran = ran == Ran::detrend;
  ex.hp_ran = ran == Ran::highpass;
  ex.od_ran = ran == Ran::orders;
  if (ran == Ran::highpass) ex.hp_detrend = detrend;
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

// one pass over the table in batches of whole trial groups (ev: events around the k_expose launch of the first batch)
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

// the shared tail of the two plain expose calls on stream st: the moments are fused into k_expose and the model is
// kept on request only, so this is not the chain below
void expose_on(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int64_t n_wav, const ExOut& o) {
  prom::ExDev& ex = ctx->ex;
  if (ctx->obs.n_pix == 0) return zero_outputs(ex, o);
  if (!o.any()) return;
  const double nan = std::nan("");
  ex.q.ensure(sizeof(double) * (size_t)n_wav);
  if (o.model) ex.model.ensure(sizeof(double) * (size_t)ex.n_exp * ex.n_trial * ctx->obs.n_pix);
  prom::launch_observe_q(st, wav, (int32_t)n_wav, nan, nan, ex.q.as<double>());
  expose_launch(ctx, st, wav, R, (int32_t)n_wav, o.moments(), o.model ? ex.model.as<double>() : nullptr, nullptr,
                nullptr);
  record_last(ex, wav, R, n_wav, Ran::none, 0);
  download_outputs(ctx, st, o);
}

// ---- the chain of the filtered calls ------------------------------------------------------------------------------------
// q, k_expose without moments into ex.model, the high-pass and the filter in place (or every column flagged
// filterable), k_model_moments, the per-order kernels, the copies back.  A call says which stages run and on what:
struct ChainCall {
  bool highpass, detrend, orders;   // the stages (orders: a per-order call, whose kernels run when their outputs are asked)
  const DevBuf *U, *W;              // the filter of the detrend stage, [n_exp][n_comp] and [n_comp][n_exp][n_pix] ...
  int32_t n_comp;                   // ... of n_comp components
  const DevBuf* data;               // what the moments are taken against, [n_exp][n_pix]
  Ran ran;                          // the aid that may repeat the call (none: the recovery, which also forgets the spectrum)
  bool always;                      // the call runs whatever the outputs (the recovery)
  const char* noun;                 // the out-of-memory message's "<noun> the model of all ... trials"
  ExOut out;
  const int32_t* seg_of;            // a per-order filter: U is [n_seg][n_exp][n_comp] and pixel p takes the basis of
                                    // order seg_of[p] (on the device); left out or null: one basis
};

// a call on the resident filter and the table's own data
ChainCall resident_call(prom_ctx* ctx, bool highpass, bool detrend, bool orders, Ran ran, const char* noun,
                        const ExOut& out) {
  prom::ExDev& ex = ctx->ex;
  return ChainCall{highpass, detrend, orders, &ex.U, &ex.W, ex.n_comp, &ex.data, ran, false, noun, out,
                   ex.dt_n_seg > 0 ? ex.dt_seg_of.as<int32_t>() : nullptr};
}

// the moments of the model in ex.model against `data`, in batches of whole trial groups (ev: events around the first
// batch's k_model_moments; model: another buffer of ex.model's shape, a recovery grid's)
void moments_launch(prom_ctx* ctx, hipStream_t st, const double* data, hipEvent_t ev0, hipEvent_t ev1,
                    const double* model = nullptr) {
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

// k_order_moments + k_order_totals over the final model in ex.model against `data`, in batches of whole trial groups
// under the scratch cap (one group at least); a batch's records go to the caller's arrays when they are wanted (ev:
// events around the two kernels of the first batch; model: as moments_launch's)
void orders_launch(prom_ctx* ctx, hipStream_t st, const double* data, double* orec_mom_out, int64_t* orec_n_used_out,
                   hipEvent_t* ev, const double* model = nullptr) {
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

// 1: whether the call runs at all (false: the outputs are filled and there is nothing to do), the refusals of every
// stage that will run, before anything is launched, and the buffers of the whole table
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

// 2: the final model: the unfiltered model of the whole table into ex.model (k_expose without moments), the high-pass
// in place, then the filter in place or every column flagged filterable (hp_ev, dt_ev: events around k_highpass and
// k_detrend).  The filters work in place, so an aid that repeats one forms the model again each time
void chain_model(prom_ctx* ctx, hipStream_t st, const ChainCall& c, const double* wav, const double* R, int32_t n_wav,
                 const hipEvent_t* hp_ev = nullptr, const hipEvent_t* dt_ev = nullptr) {
  prom::ExDev& ex = ctx->ex;
  const int32_t n_pix = ctx->obs.n_pix;
  expose_launch(ctx, st, wav, R, n_wav, false, ex.model.as<double>(), nullptr, nullptr);
  if (c.highpass)
    highpass_launch(ex, st, ex.model.as<double>(), (int64_t)ex.n_exp * ex.n_trial, n_pix, hp_ev ? hp_ev[0] : nullptr,
                    hp_ev ? hp_ev[1] : nullptr);
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

// q of the whole grid, then 2 and 3
void chain_go(prom_ctx* ctx, hipStream_t st, const ChainCall& c, const double* wav, const double* R, int64_t n_wav) {
  const double nan = std::nan("");
  prom::launch_observe_q(st, wav, (int32_t)n_wav, nan, nan, ctx->ex.q.as<double>());
  chain_model(ctx, st, c, wav, R, (int32_t)n_wav);
  chain_finish(ctx, st, c, wav, R, n_wav);
}

// the shared tail of the detrended, high-pass and per-order calls, on stream st
void chain_on(prom_ctx* ctx, hipStream_t st, const ChainCall& c, const double* wav, const double* R, int64_t n_wav) {
  if (chain_prepare(ctx, c, n_wav)) chain_go(ctx, st, c, wav, R, n_wav);
}

// ---- the families' own checks and descriptions ---------------------------------------------------------------------------
void detrend_check(prom_ctx* ctx, const char* who) {
  expose_check(ctx, who);
  if (!ctx->ex.dt_set)
    throw Error(PROM_E_STATE, std::string(who) + ": no filter on the context (prom_detrend_set; a later "
                                                 "prom_expose_set, or whatever drops the exposure table, drops it)");
}

ChainCall detrend_call(prom_ctx* ctx, const ExOut& out) {
  return resident_call(ctx, false, true, false, Ran::detrend, "the detrended exposures keep", out);
}

void highpass_check(prom_ctx* ctx, const char* who, int32_t detrend) {
  expose_check(ctx, who);
  if (!ctx->ex.hp_set)
    throw Error(PROM_E_STATE, std::string(who) + ": no high-pass on the context (prom_highpass_set; a later "
                                                 "prom_expose_set, or whatever drops the exposure table, drops it)");
  if (detrend != 0 && detrend != 1) throw Error(PROM_E_ARG, std::string(who) + ": detrend must be 0 or 1");
  if (detrend && !ctx->ex.dt_set)
    throw Error(PROM_E_STATE, std::string(who) + ": detrend = 1 without a filter on the context (prom_detrend_set)");
}

ChainCall highpass_call(prom_ctx* ctx, int32_t detrend, const ExOut& out) {
  return resident_call(ctx, true, detrend != 0, false, Ran::highpass, "the high-pass filtered exposures keep", out);
}

void orders_check(prom_ctx* ctx, const char* who, int32_t highpass, int32_t detrend) {
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
}

ChainCall orders_call(prom_ctx* ctx, int32_t highpass, int32_t detrend, const ExOut& out) {
  return resident_call(ctx, highpass != 0, detrend != 0, true, Ran::orders, "the per-order moments keep", out);
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
    expose_check(ctx, "prom_transit_expose");
    const TransitArgs t = ex_transit(ctx, "prom_transit_expose");
    expose_on(ctx, t.st, t.wav, t.R, t.n_wav, plain_out(mom_out, n_used_out, model_out));
  });
}

int32_t prom_spectrum_expose(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                             double* mom_out, int64_t* n_used_out, double* model_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    expose_check(ctx, "prom_spectrum_expose");
    const hipStream_t st = ex_spectrum(ctx, "prom_spectrum_expose", n_orb, n_wav, wav, R);
    expose_on(ctx, st, ex.wav.as<double>(), ex.R.as<double>(), n_wav,
              plain_out(mom_out, n_used_out, model_out));
  });
}

int32_t prom_expose_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_expose_kernel_ms: bad arguments");
    if (!ex.set || !ctx->obs.set || !ex.last_wav || ctx->obs.n_pix == 0)
      throw Error(PROM_E_STATE, "prom_expose_kernel_ms: no expose call to repeat");
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
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    ex.dt_set = ex.dt_ran = false;
    if (ctx->rc.last == 1) ctx->rc.last = 0;
    table_check(ctx, "prom_detrend_set");
    PROM_REQUIRE(n_exp == ex.n_exp, "prom_detrend_set: n_exp differs from the exposure table's");
    PROM_REQUIRE(n_comp >= 1 && n_comp <= prom::kDtMaxComp, "prom_detrend_set: n_comp must lie in [1, 16]");
    const int64_t nu = (int64_t)n_exp * n_comp, nw = nu * ctx->obs.n_pix;
    PROM_REQUIRE(U && (nw == 0 || W), "prom_detrend_set: U and W missing");
    for (int64_t i = 0; i < nu; ++i) PROM_REQUIRE(obs_finite(U[i]), "prom_detrend_set: U must be finite");
    for (int64_t i = 0; i < nw; ++i) PROM_REQUIRE(obs_finite(W[i]), "prom_detrend_set: W must be finite");
    const hipStream_t st = ctx->stream;
    upload(ex.U, U, nu, st);
    upload(ex.W, W, nw, st);
    PROM_HIP(hipStreamSynchronize(st));   // the host arrays are read during the call only
    ex.n_comp = n_comp;
    ex.dt_n_seg = 0;
    ex.dt_set = true;
  });
}

namespace {

// what the two per-order filter sets share: the checks, seg_of of the resident orders and U[n_seg][n_exp][n_comp] on
// the device; the filter is not resident until the caller says so
void detrend_orders_begin(prom_ctx* ctx, const char* who, int32_t n_exp, int32_t n_comp, int32_t n_seg, const double* U,
                          hipStream_t st) {
  prom::ExDev& ex = ctx->ex;
  const std::string w(who);
  ex.dt_set = ex.dt_ran = false;
  ex.dt_n_seg = 0;
  if (ctx->rc.last == 1) ctx->rc.last = 0;
  table_check(ctx, who);
  if (!ex.od_set) throw Error(PROM_E_STATE, w + ": no orders on the context (prom_orders_set)");
  PROM_REQUIRE(n_exp == ex.n_exp, w + ": n_exp differs from the exposure table's");
  PROM_REQUIRE(n_comp >= 1 && n_comp <= prom::kDtMaxComp, w + ": n_comp must lie in [1, 16]");
  PROM_REQUIRE(n_seg == ex.od_n_seg, w + ": n_seg differs from the resident orders'");
  const int64_t nu = (int64_t)n_seg * n_exp * n_comp;
  PROM_REQUIRE(U, w + ": U missing");
  for (int64_t i = 0; i < nu; ++i) PROM_REQUIRE(obs_finite(U[i]), w + ": U must be finite");
  const int32_t n_pix = ctx->obs.n_pix;
  std::vector<int32_t> seg_of((size_t)std::max(n_pix, 1), 0);
  prom::fo_seg_of(n_seg, ex.od_seg_host.data(), ex.od_perm_host.data(), seg_of.data());
  upload(ex.U, U, nu, st);
  upload(ex.dt_seg_of, seg_of.data(), (int64_t)n_pix, st);
  PROM_HIP(hipStreamSynchronize(st));   // (seg_of is a local; U is read during the call only)
}

}  // namespace

int32_t prom_detrend_set_orders(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, int32_t n_seg, const double* U,
                                const double* W) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    const hipStream_t st = ctx->stream;
    const int64_t nw = (int64_t)n_comp * n_exp * ctx->obs.n_pix;
    detrend_orders_begin(ctx, "prom_detrend_set_orders", n_exp, n_comp, n_seg, U, st);
    PROM_REQUIRE(nw == 0 || W, "prom_detrend_set_orders: W missing");
    for (int64_t i = 0; i < nw; ++i) PROM_REQUIRE(obs_finite(W[i]), "prom_detrend_set_orders: W must be finite");
    upload(ex.W, W, nw, st);
    PROM_HIP(hipStreamSynchronize(st));   // the host arrays are read during the call only
    ex.n_comp = n_comp;
    ex.dt_n_seg = n_seg;
    ex.dt_set = true;
  });
}

int32_t prom_transit_expose_detrended(prom_ctx* ctx, double* mom_out, int64_t* n_used_out, double* model_out) {
  return guarded(ctx, [&] {
    detrend_check(ctx, "prom_transit_expose_detrended");
    const TransitArgs t = ex_transit(ctx, "prom_transit_expose_detrended");
    chain_on(ctx, t.st, detrend_call(ctx, plain_out(mom_out, n_used_out, model_out)), t.wav, t.R,
             t.n_wav);
  });
}

int32_t prom_spectrum_expose_detrended(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                       double* mom_out, int64_t* n_used_out, double* model_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    detrend_check(ctx, "prom_spectrum_expose_detrended");
    const hipStream_t st = ex_spectrum(ctx, "prom_spectrum_expose_detrended", n_orb, n_wav, wav, R);
    chain_on(ctx, st, detrend_call(ctx, plain_out(mom_out, n_used_out, model_out)),
             ex.wav.as<double>(), ex.R.as<double>(), n_wav);
  });
}

int32_t prom_detrend_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_detrend_kernel_ms: bad arguments");
    if (!ex.set || !ex.dt_set || !ex.dt_ran || !ctx->obs.set || !ex.last_wav || ctx->obs.n_pix == 0)
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
    prom::ExDev& ex = ctx->ex;
    ex.hp_set = ex.hp_ran = false;
    table_check(ctx, "prom_highpass_set");
    PROM_REQUIRE(n_pix == ctx->obs.n_pix, "prom_highpass_set: n_pix differs from the observation's");
    PROM_REQUIRE(n_seg >= 1 && seg_first && (n_pix == 0 || perm), "prom_highpass_set: segments missing");
    PROM_REQUIRE(half_width >= 0 && half_width <= prom::kHpMaxHalf && g,
                 "prom_highpass_set: half_width must lie in [0, 512]");
    PROM_REQUIRE(mode == 0 || mode == 1, "prom_highpass_set: mode must be 0 (subtract) or 1 (divide)");
    segments_check("prom_highpass_set", n_pix, n_seg, seg_first, perm);
    for (int32_t d = 0; d <= half_width; ++d)
      PROM_REQUIRE(obs_finite(g[d]) && g[d] >= 0.0, "prom_highpass_set: g must be finite and >= 0");
    PROM_REQUIRE(g[0] > 0.0, "prom_highpass_set: g[0] must be > 0");
    const hipStream_t st = ctx->stream;
    upload(ex.hp_seg, seg_first, (int64_t)n_seg + 1, st);
    upload(ex.hp_perm, perm, (int64_t)n_pix, st);
    upload(ex.hp_g, g, (int64_t)half_width + 1, st);
    PROM_HIP(hipStreamSynchronize(st));   // the host arrays are read during the call only
    ex.hp_n_seg = n_seg;
    ex.hp_half = half_width;
    ex.hp_mode = mode;
    ex.hp_den = prom::hp_den_full(g, half_width);
    ex.hp_kind = 0;
    ex.hp_set = true;
  });
}

int32_t prom_highpass_set_median(prom_ctx* ctx, int32_t n_pix, int32_t n_seg, const int32_t* seg_first,
                                 const int32_t* perm, int32_t half_width, int32_t mode) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    ex.hp_set = ex.hp_ran = false;
    table_check(ctx, "prom_highpass_set_median");
    PROM_REQUIRE(n_pix == ctx->obs.n_pix, "prom_highpass_set_median: n_pix differs from the observation's");
    PROM_REQUIRE(n_seg >= 1 && seg_first && (n_pix == 0 || perm), "prom_highpass_set_median: segments missing");
    PROM_REQUIRE(half_width >= 0 && half_width <= prom::kHpMaxHalf,
                 "prom_highpass_set_median: half_width must lie in [0, 512]");
    PROM_REQUIRE(mode == 0 || mode == 1, "prom_highpass_set_median: mode must be 0 (subtract) or 1 (divide)");
    segments_check("prom_highpass_set_median", n_pix, n_seg, seg_first, perm);
    const hipStream_t st = ctx->stream;
    upload(ex.hp_seg, seg_first, (int64_t)n_seg + 1, st);
    upload(ex.hp_perm, perm, (int64_t)n_pix, st);
    PROM_HIP(hipStreamSynchronize(st));   // the host arrays are read during the call only
    ex.hp_n_seg = n_seg;
    ex.hp_half = half_width;
    ex.hp_mode = mode;
    ex.hp_kind = 1;
    ex.hp_set = true;
  });
}

int32_t prom_transit_expose_highpass(prom_ctx* ctx, int32_t detrend, double* mom_out, int64_t* n_used_out,
                                     double* model_out) {
  return guarded(ctx, [&] {
    highpass_check(ctx, "prom_transit_expose_highpass", detrend);
    const TransitArgs t = ex_transit(ctx, "prom_transit_expose_highpass");
    chain_on(ctx, t.st, highpass_call(ctx, detrend, plain_out(mom_out, n_used_out, model_out)),
             t.wav, t.R, t.n_wav);
  });
}

int32_t prom_spectrum_expose_highpass(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                      int32_t detrend, double* mom_out, int64_t* n_used_out, double* model_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    highpass_check(ctx, "prom_spectrum_expose_highpass", detrend);
    const hipStream_t st = ex_spectrum(ctx, "prom_spectrum_expose_highpass", n_orb, n_wav, wav, R);
    chain_on(ctx, st, highpass_call(ctx, detrend, plain_out(mom_out, n_used_out, model_out)),
             ex.wav.as<double>(), ex.R.as<double>(), n_wav);
  });
}

int32_t prom_highpass_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_highpass_kernel_ms: bad arguments");
    if (!ex.set || !ex.hp_set || !ex.hp_ran || !ctx->obs.set || !ex.last_wav || ctx->obs.n_pix == 0 ||
        (ex.hp_detrend && !ex.dt_set))
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
    orders_check(ctx, "prom_transit_expose_orders", highpass, detrend);
    const TransitArgs t = ex_transit(ctx, "prom_transit_expose_orders");
    const ExOut out{mom_out, n_used_out, orec_mom_out, orec_n_used_out, tot_out, model_out};
    chain_on(ctx, t.st, orders_call(ctx, highpass, detrend, out), t.wav, t.R, t.n_wav);
  });
}

int32_t prom_spectrum_expose_orders(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                    int32_t highpass, int32_t detrend, double* mom_out, int64_t* n_used_out,
                                    double* orec_mom_out, int64_t* orec_n_used_out, double* tot_out,
                                    double* model_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    orders_check(ctx, "prom_spectrum_expose_orders", highpass, detrend);
    const hipStream_t st = ex_spectrum(ctx, "prom_spectrum_expose_orders", n_orb, n_wav, wav, R, true);
    const ExOut out{mom_out, n_used_out, orec_mom_out, orec_n_used_out, tot_out, model_out};
    chain_on(ctx, st, orders_call(ctx, highpass, detrend, out), ex.wav.as<double>(), ex.R.as<double>(), n_wav);
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

namespace {

// what a clean / inject call asks for (source 1: clean, 2: the last run's R, 3: a caller's spectrum)
struct SyCall {
  int32_t source, trial, highpass, n_comp, n_iter, ones;
  double scale;
  int32_t orders;   // 1: SYSREM per resident order (prom_orders_set), U gains the order dimension (left out: 0)
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

// the shared tail of the clean / inject calls on stream st (ev: six events around the injection, the high-pass and
// SYSREM, and the call runs even without an output; wait = false: a recover call goes on on the same stream, so the call
// runs whatever the outputs and does not wait)
void sysrem_on(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int64_t n_wav, const SyCall& c,
               double* U_out, double* cleaned_out, double* injected_out, hipEvent_t* ev, bool wait = true) {
  prom::SyDev& sy = ctx->sy;
  prom::ExDev& ex = ctx->ex;
  const prom::ObsDev& ob = ctx->obs;
  const int32_t n_exp = sy.n_exp, n_pix = sy.n_pix, n_cols = c.n_comp + c.ones;
  const int32_t items = sy_items(ctx, c), width = sy_width(ctx, c);   // (per order: the orders, n_max wide)
  const int64_t n = (int64_t)n_exp * n_pix;
  if (n_pix == 0) {   // no pixel: every component ends at once
    if (U_out)
      for (int64_t e = 0; e < (int64_t)items * n_exp; ++e)
        for (int32_t k = 0; k < n_cols; ++k) U_out[e * n_cols + k] = (c.ones && k == 0) ? 1.0 : 0.0;
    return;
  }
  if (wait && !ev && !U_out && !cleaned_out && !injected_out) return;
  if (ctx->rc.last == 2) ctx->rc.last = 0;   // (U may move or change its shape)
  if (c.highpass && prom::hp_workgroups(n_exp, ex.hp_n_seg) > kMaxGrid)   // (before anything is launched)
    throw Error(PROM_E_ARG, "k_highpass: n_exp n_seg too large for one launch");
  const int64_t pitch = prom::sy_pitch(width);
  sy.D.ensure(sizeof(double) * (size_t)n);
  sy.out.ensure(sizeof(double) * (size_t)n);
  sy.r.ensure(sizeof(double) * (size_t)items * (size_t)(n_exp * pitch));
  sy.w.ensure(sizeof(double) * (size_t)items * (size_t)(n_exp * pitch));
  sy.a.ensure(sizeof(double) * (size_t)items * n_exp);
  sy.ended.ensure(sizeof(int32_t) * (size_t)items * prom::kGrFlags);
  sy.part.ensure(2 * sizeof(double) * (size_t)items * n_exp * prom::sy_tiles(width));
  sy.U.ensure(sizeof(double) * (size_t)items * n_exp * n_cols);
  if (ev) PROM_HIP(hipEventRecord(ev[0], st));
  if (c.source != 1) {
    // the model of trial `trial` alone: its factors as a table of one trial, through k_expose unchanged
    const double nan = std::nan("");
    sy.q.ensure(sizeof(double) * (size_t)n_wav);
    sy.Fj.ensure(sizeof(double) * (size_t)n_exp * ex.n_tap);
    sy.model.ensure(sizeof(double) * (size_t)n);
    sy.epart.ensure(sizeof(double) * (size_t)prom::vm_part_doubles(n_exp, 1, prom::vm_chunks(n_pix)));
    prom::launch_observe_q(st, wav, (int32_t)n_wav, nan, nan, sy.q.as<double>());
    prom::launch_sysrem_gather(st, ex.F.as<double>(), sy.Fj.as<double>(), n_exp, ex.n_trial, ex.n_tap, c.trial);
    prom::launch_expose(st, wav, sy.q.as<double>(), R, (int32_t)n_wav, ob.lam.as<double>(), ob.sig.as<double>(), ob.k,
                        ex.row.as<int32_t>(), ex.a.as<double>(), sy.Fj.as<double>(), ex.data.as<double>(),
                        ex.ivar.as<double>(), n_pix, n_exp, 1, ex.n_tap, 0, 1, sy.epart.as<double>(),
                        sy.model.as<double>(), nullptr, nullptr);
    prom::launch_inject(st, sy.raw.as<double>(), sy.model.as<double>(), c.scale, sy.D.as<double>(), n);
  } else {
    PROM_HIP(hipMemcpyAsync(sy.D.p, sy.raw.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
  }
  if (ev) PROM_HIP(hipEventRecord(ev[1], st));
  if (ev) PROM_HIP(hipEventRecord(ev[2], st));
  if (c.highpass)
    highpass_launch(ex, st, sy.D.as<double>(), n_exp, n_pix);
  if (ev) PROM_HIP(hipEventRecord(ev[3], st));
  if (ev) PROM_HIP(hipEventRecord(ev[4], st));
  if (c.orders)
    prom::launch_sysrem_orders(st, sy.D.as<double>(), ex.ivar.as<double>(), ex.od_seg.as<int32_t>(),
                               ex.od_perm.as<int32_t>(), sy.r.as<double>(), sy.w.as<double>(), sy.a.as<double>(),
                               sy.ended.as<int32_t>(), sy.part.as<double>(), sy.U.as<double>(), sy.out.as<double>(),
                               n_exp, n_pix, items, width, c.n_comp, c.n_iter, c.ones);
  else
    prom::launch_sysrem(st, sy.D.as<double>(), ex.ivar.as<double>(), sy.r.as<double>(), sy.w.as<double>(),
                        sy.a.as<double>(), sy.ended.as<int32_t>(), sy.part.as<double>(), sy.U.as<double>(),
                        sy.out.as<double>(), n_exp, n_pix, c.n_comp, c.n_iter, c.ones);
  if (ev) PROM_HIP(hipEventRecord(ev[5], st));
  sy.last_source = c.source;
  sy.last_trial = c.trial;
  sy.last_scale = c.scale;
  sy.last_highpass = c.highpass;
  sy.last_n_comp = c.n_comp;
  sy.last_n_iter = c.n_iter;
  sy.last_ones = c.ones;
  sy.last_n_wav = n_wav;
  sy.last_orders = c.orders;
  if (U_out) download(U_out, sy.U, (int64_t)items * n_exp * n_cols, st);
  if (cleaned_out) download(cleaned_out, sy.out, n, st);
  if (injected_out) download(injected_out, sy.D, n, st);
  if (wait) PROM_HIP(hipStreamSynchronize(st));
}

}  // namespace

int32_t prom_sysrem_clean(prom_ctx* ctx, int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out,
                          double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    const SyCall c{1, 0, highpass, n_comp, n_iter, ones, 0.0};
    sysrem_check(ctx, "prom_sysrem_clean", c);
    sysrem_on(ctx, ctx->stream, nullptr, nullptr, 0, c, U_out, cleaned_out, injected_out, nullptr);
  });
}

int32_t prom_transit_inject(prom_ctx* ctx, int32_t trial, double scale, int32_t highpass, int32_t n_comp, int32_t n_iter,
                            int32_t ones, double* U_out, double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    const SyCall c{2, trial, highpass, n_comp, n_iter, ones, scale};
    sysrem_check(ctx, "prom_transit_inject", c);
    const TransitArgs t = ex_transit(ctx, "prom_transit_inject");
    sysrem_on(ctx, t.st, t.wav, t.R, t.n_wav, c, U_out, cleaned_out, injected_out, nullptr);
  });
}

int32_t prom_spectrum_inject(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                             int32_t trial, double scale, int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones,
                             double* U_out, double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    prom::SyDev& sy = ctx->sy;
    const SyCall c{3, trial, highpass, n_comp, n_iter, ones, scale};
    sysrem_check(ctx, "prom_spectrum_inject", c);
    const hipStream_t st = sy_spectrum(ctx, "prom_spectrum_inject", n_orb, n_wav, wav, R);
    sysrem_on(ctx, st, sy.wav.as<double>(), sy.R.as<double>(), n_wav, c, U_out, cleaned_out, injected_out, nullptr);
  });
}

// SYSREM per order: the same calls with every resident order (prom_orders_set) cleaned on its own; U_out gains the
// order dimension, [n_seg][n_exp][n_comp + ones]
int32_t prom_sysrem_clean_orders(prom_ctx* ctx, int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones,
                                 double* U_out, double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    const SyCall c{1, 0, highpass, n_comp, n_iter, ones, 0.0, 1};
    sysrem_check(ctx, "prom_sysrem_clean_orders", c);
    sysrem_on(ctx, ctx->stream, nullptr, nullptr, 0, c, U_out, cleaned_out, injected_out, nullptr);
  });
}

int32_t prom_transit_inject_orders(prom_ctx* ctx, int32_t trial, double scale, int32_t highpass, int32_t n_comp,
                                   int32_t n_iter, int32_t ones, double* U_out, double* cleaned_out,
                                   double* injected_out) {
  return guarded(ctx, [&] {
    const SyCall c{2, trial, highpass, n_comp, n_iter, ones, scale, 1};
    sysrem_check(ctx, "prom_transit_inject_orders", c);
    const TransitArgs t = ex_transit(ctx, "prom_transit_inject_orders");
    sysrem_on(ctx, t.st, t.wav, t.R, t.n_wav, c, U_out, cleaned_out, injected_out, nullptr);
  });
}

int32_t prom_spectrum_inject_orders(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                    int32_t trial, double scale, int32_t highpass, int32_t n_comp, int32_t n_iter,
                                    int32_t ones, double* U_out, double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    prom::SyDev& sy = ctx->sy;
    const SyCall c{3, trial, highpass, n_comp, n_iter, ones, scale, 1};
    sysrem_check(ctx, "prom_spectrum_inject_orders", c);
    const hipStream_t st = sy_spectrum(ctx, "prom_spectrum_inject_orders", n_orb, n_wav, wav, R);
    sysrem_on(ctx, st, sy.wav.as<double>(), sy.R.as<double>(), n_wav, c, U_out, cleaned_out, injected_out, nullptr);
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
    const double* wav = c.source == 2 ? tr.wav.as<double>() : sy.wav.as<double>();
    const double* R = c.source == 2 ? transit_R(ctx) : sy.R.as<double>();
    double sum[3];   // the injection, the high-pass, SYSREM
    time_launches(ctx, ctx->stream, n_runs, 3, sum, [&] {
      sysrem_on(ctx, ctx->stream, wav, R, sy.last_n_wav, c, nullptr, nullptr, nullptr, ctx->ev);
    });
    ms_out[0] = sum[2] / n_runs;
    ms_out[1] = c.source != 1 ? sum[0] / n_runs : std::nan("");
    ms_out[2] = c.highpass ? sum[1] / n_runs : std::nan("");
  });
}

// ------------------------------------------------------------------------------ the filter's weights and the recovery
int32_t prom_filter_weights(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, int32_t n_pix, const double* U,
                            const double* ivar, double* W_out) {
  return guarded(ctx, [&] {
    prom::RcDev& rc = ctx->rc;
    PROM_REQUIRE(n_comp >= 1 && n_comp <= prom::kDtMaxComp, "prom_filter_weights: n_comp must lie in [1, 16]");
    PROM_REQUIRE(n_exp >= 1 && n_pix >= 0, "prom_filter_weights: n_exp must be >= 1 and n_pix >= 0");
    const int64_t nu = (int64_t)n_exp * n_comp, ni = (int64_t)n_exp * n_pix, nw = nu * n_pix;
    PROM_REQUIRE(U && (n_pix == 0 || (ivar && W_out)), "prom_filter_weights: U, ivar or W_out missing");
    for (int64_t i = 0; i < nu; ++i) PROM_REQUIRE(obs_finite(U[i]), "prom_filter_weights: U must be finite");
    if (n_pix == 0) return;
    const hipStream_t st = ctx->stream;
    upload(rc.fU, U, nu, st);
    upload(rc.fivar, ivar, ni, st);
    rc.fW.ensure(sizeof(double) * (size_t)nw);
    prom::launch_filter_weights(st, rc.fU.as<double>(), rc.fivar.as<double>(), rc.fW.as<double>(), n_exp, n_comp, n_pix,
                                nullptr, nullptr);
    download(W_out, rc.fW, nw, st);
    PROM_HIP(hipStreamSynchronize(st));
  });
}

int32_t prom_detrend_build(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, const double* U, double* W_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    ex.dt_set = ex.dt_ran = false;
    if (ctx->rc.last == 1) ctx->rc.last = 0;
    table_check(ctx, "prom_detrend_build");
    PROM_REQUIRE(n_exp == ex.n_exp, "prom_detrend_build: n_exp differs from the exposure table's");
    PROM_REQUIRE(n_comp >= 1 && n_comp <= prom::kDtMaxComp, "prom_detrend_build: n_comp must lie in [1, 16]");
    const int32_t n_pix = ctx->obs.n_pix;
    const int64_t nu = (int64_t)n_exp * n_comp, nw = nu * n_pix;
    PROM_REQUIRE(U, "prom_detrend_build: U missing");
    for (int64_t i = 0; i < nu; ++i) PROM_REQUIRE(obs_finite(U[i]), "prom_detrend_build: U must be finite");
    const hipStream_t st = ctx->stream;
    upload(ex.U, U, nu, st);
    ex.W.ensure(sizeof(double) * (size_t)std::max<int64_t>(nw, 1));
    prom::launch_filter_weights(st, ex.U.as<double>(), ex.ivar.as<double>(), ex.W.as<double>(), n_exp, n_comp, n_pix,
                                nullptr, nullptr);
    if (W_out) download(W_out, ex.W, nw, st);
    PROM_HIP(hipStreamSynchronize(st));   // the host array is read during the call only
    ex.n_comp = n_comp;
    ex.dt_n_seg = 0;
    ex.dt_set = true;
    if (n_pix > 0) {
      ctx->rc.last = 1;
      ctx->rc.last_n_comp = n_comp;
    }
  });
}

int32_t prom_filter_weights_orders(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, int32_t n_pix, int32_t n_seg,
                                   const int32_t* seg_of, const double* U, const double* ivar, double* W_out) {
  return guarded(ctx, [&] {
    prom::RcDev& rc = ctx->rc;
    PROM_REQUIRE(n_comp >= 1 && n_comp <= prom::kDtMaxComp, "prom_filter_weights_orders: n_comp must lie in [1, 16]");
    PROM_REQUIRE(n_exp >= 1 && n_pix >= 0 && n_seg >= 1,
                 "prom_filter_weights_orders: n_exp and n_seg must be >= 1 and n_pix >= 0");
    const int64_t nu = (int64_t)n_seg * n_exp * n_comp, ni = (int64_t)n_exp * n_pix, nw = ni * n_comp;
    PROM_REQUIRE(U && (n_pix == 0 || (ivar && W_out && seg_of)),
                 "prom_filter_weights_orders: U, seg_of, ivar or W_out missing");
    for (int64_t i = 0; i < nu; ++i) PROM_REQUIRE(obs_finite(U[i]), "prom_filter_weights_orders: U must be finite");
    for (int32_t p = 0; p < n_pix; ++p)
      PROM_REQUIRE(seg_of[p] >= 0 && seg_of[p] < n_seg, "prom_filter_weights_orders: seg_of outside [0, n_seg)");
    if (n_pix == 0) return;
    const hipStream_t st = ctx->stream;
    upload(rc.fU, U, nu, st);
    upload(rc.fivar, ivar, ni, st);
    upload(rc.fseg, seg_of, (int64_t)n_pix, st);
    rc.fW.ensure(sizeof(double) * (size_t)nw);
    prom::launch_filter_weights_orders(st, rc.fU.as<double>(), rc.fivar.as<double>(), rc.fseg.as<int32_t>(),
                                       rc.fW.as<double>(), n_exp, n_comp, n_pix, nullptr, nullptr);
    download(W_out, rc.fW, nw, st);
    PROM_HIP(hipStreamSynchronize(st));
  });
}

int32_t prom_detrend_build_orders(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, int32_t n_seg, const double* U,
                                  double* W_out) {
  return guarded(ctx, [&] {
    prom::ExDev& ex = ctx->ex;
    const hipStream_t st = ctx->stream;
    const int32_t n_pix = ctx->obs.n_pix;
    const int64_t nw = (int64_t)n_comp * n_exp * n_pix;
    detrend_orders_begin(ctx, "prom_detrend_build_orders", n_exp, n_comp, n_seg, U, st);
    ex.W.ensure(sizeof(double) * (size_t)std::max<int64_t>(nw, 1));
    prom::launch_filter_weights_orders(st, ex.U.as<double>(), ex.ivar.as<double>(), ex.dt_seg_of.as<int32_t>(),
                                       ex.W.as<double>(), n_exp, n_comp, n_pix, nullptr, nullptr);
    if (W_out) download(W_out, ex.W, nw, st);
    PROM_HIP(hipStreamSynchronize(st));
    ex.n_comp = n_comp;
    ex.dt_n_seg = n_seg;
    ex.dt_set = true;
    if (n_pix > 0) {
      ctx->rc.last = 1;
      ctx->rc.last_n_comp = n_comp;
    }
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

namespace {

void recover_check(prom_ctx* ctx, const char* who, const SyCall& c, int32_t orders) {
  const std::string w(who);
  sysrem_check(ctx, who, c);
  if (orders != 0 && orders != 1) throw Error(PROM_E_ARG, w + ": orders must be 0 or 1");
  if (orders && !ctx->ex.od_set)
    throw Error(PROM_E_STATE, w + ": orders = 1 without orders on the context (prom_orders_set)");
}

// the shared tail of the two recover calls on stream st: the inject call's steps, W of (U, ivar), then the chain
// (highpass, detrend = 1) with the cleaned data in the place of the table's and (U, W) in the place of the resident
// filter.  Without `orders` the per-order outputs are not looked at
void recover_on(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int64_t n_wav, const SyCall& c,
                int32_t orders, ExOut out, double* U_out) {
  prom::ExDev& ex = ctx->ex;
  prom::SyDev& sy = ctx->sy;
  prom::RcDev& rc = ctx->rc;
  const int32_t n_pix = ctx->obs.n_pix, n_exp = ex.n_exp, n_cols = c.n_comp + c.ones;
  if (!orders) out.orec_mom = out.tot = nullptr;
  if (!orders) out.orec_n_used = nullptr;
  const ChainCall cc{c.highpass != 0, true, orders != 0, &sy.U, &rc.W, n_cols, &sy.out, Ran::none, true,
                     "the recovery keeps", out};
  if (n_pix == 0) sysrem_on(ctx, st, wav, R, n_wav, c, U_out, nullptr, nullptr, nullptr);   // no pixel: the inject call's U
  if (!chain_prepare(ctx, cc, n_wav)) return;
  rc.W.ensure(sizeof(double) * (size_t)n_cols * n_exp * n_pix);
  // the last calls' q, models and flags go: the aids of the expose calls have nothing to repeat
  record_last(ex, nullptr, nullptr, 0, Ran::none, 0);
  // 1: the inject call's steps; the cleaned data stay in sy.out and U in sy.U
  sysrem_on(ctx, st, wav, R, n_wav, c, U_out, nullptr, nullptr, nullptr, false);
  // 2: W of (U, the table's ivar)
  prom::launch_filter_weights(st, sy.U.as<double>(), ex.ivar.as<double>(), rc.W.as<double>(), n_exp, n_cols, n_pix,
                              nullptr, nullptr);
  rc.last = 2;
  rc.last_n_comp = n_cols;
  // 3: the final model and the moments against the cleaned data
  chain_go(ctx, st, cc, wav, R, n_wav);
}

}  // namespace

int32_t prom_transit_recover(prom_ctx* ctx, int32_t trial, double scale, int32_t highpass, int32_t n_comp,
                             int32_t n_iter, int32_t ones, int32_t orders, double* mom_out, int64_t* n_used_out,
                             double* orec_mom_out, int64_t* orec_n_used_out, double* tot_out, double* U_out,
                             double* model_out) {
  return guarded(ctx, [&] {
    const SyCall c{2, trial, highpass, n_comp, n_iter, ones, scale};
    recover_check(ctx, "prom_transit_recover", c, orders);
    const TransitArgs t = ex_transit(ctx, "prom_transit_recover");
    recover_on(ctx, t.st, t.wav, t.R, t.n_wav, c, orders,
               ExOut{mom_out, n_used_out, orec_mom_out, orec_n_used_out, tot_out, model_out}, U_out);
  });
}

int32_t prom_spectrum_recover(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                              int32_t trial, double scale, int32_t highpass, int32_t n_comp, int32_t n_iter,
                              int32_t ones, int32_t orders, double* mom_out, int64_t* n_used_out,
                              double* orec_mom_out, int64_t* orec_n_used_out, double* tot_out, double* U_out,
                              double* model_out) {
  return guarded(ctx, [&] {
    prom::SyDev& sy = ctx->sy;
    const SyCall c{3, trial, highpass, n_comp, n_iter, ones, scale};
    recover_check(ctx, "prom_spectrum_recover", c, orders);
    const hipStream_t st = sy_spectrum(ctx, "prom_spectrum_recover", n_orb, n_wav, wav, R);
    recover_on(ctx, st, sy.wav.as<double>(), sy.R.as<double>(), n_wav, c, orders,
               ExOut{mom_out, n_used_out, orec_mom_out, orec_n_used_out, tot_out, model_out}, U_out);
  });
}

// ------------------------------------------------------------------------------ injection grids
namespace {

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

// the refusals of the list, after the single calls' own (c holds a trial and a scale that pass them)
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

// the work buffers of sub-batches of up to nb injections, and the list on the device
void grid_buffers(prom_ctx* ctx, hipStream_t st, const SyCall& c, const GridList& g, int32_t nb, int64_t n_wav,
                  bool recover) {
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
  sy.q.ensure(sizeof(double) * (size_t)n_wav);
  sy.Fj.ensure(sizeof(double) * B * n_exp * ex.n_tap);
  sy.model.ensure(sizeof(double) * B * n);
  sy.epart.ensure(sizeof(double) *
                  (size_t)prom::vm_part_doubles(n_exp, vm_batches(ctx, n_exp, nb).nb_max, prom::vm_chunks(n_pix)));
  if (recover) ctx->rc.W.ensure(sizeof(double) * B * n_cols * n);
  upload(sy.trial, g.trial, g.n_inj, st);
  upload(sy.scale, g.scale, g.n_inj, st);
}

// the inject call's steps for the injections [b0, b0 + nb) of the list, nothing waits: D (injected, high-passed),
// out (cleaned) and U of the sub-batch stay in sy.D, sy.out and sy.U as [nb][...]
void grid_clean(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int64_t n_wav, const SyCall& c,
                int32_t b0, int32_t nb) {
  prom::SyDev& sy = ctx->sy;
  prom::ExDev& ex = ctx->ex;
  const prom::ObsDev& ob = ctx->obs;
  const int32_t n_exp = sy.n_exp, n_pix = sy.n_pix;
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
  if (c.highpass)
    highpass_launch(ex, st, sy.D.as<double>(), (int64_t)nb * n_exp, n_pix);
  if (c.orders)
    prom::launch_sysrem_orders(st, sy.D.as<double>(), ex.ivar.as<double>(), ex.od_seg.as<int32_t>(),
                               ex.od_perm.as<int32_t>(), sy.r.as<double>(), sy.w.as<double>(), sy.a.as<double>(),
                               sy.ended.as<int32_t>(), sy.part.as<double>(), sy.U.as<double>(), sy.out.as<double>(),
                               n_exp, n_pix, ex.od_n_seg, ex.od_n_max, c.n_comp, c.n_iter, c.ones, nb);
  else
    prom::launch_sysrem(st, sy.D.as<double>(), ex.ivar.as<double>(), sy.r.as<double>(), sy.w.as<double>(),
                        sy.a.as<double>(), sy.ended.as<int32_t>(), sy.part.as<double>(), sy.U.as<double>(),
                        sy.out.as<double>(), n_exp, n_pix, c.n_comp, c.n_iter, c.ones, nb);
}

// no pixel: every component of every entry ends at once
void grid_zero_U(const SyCall& c, int32_t n_exp, int64_t n_inj, double* U_out) {
  const int32_t n_cols = c.n_comp + c.ones;
  if (!U_out) return;
  for (int64_t i = 0; i < (int64_t)n_inj * n_exp; ++i)
    for (int32_t k = 0; k < n_cols; ++k) U_out[i * n_cols + k] = (c.ones && k == 0) ? 1.0 : 0.0;
}

// what a grid call leaves: the work buffers hold a sub-batch, so prom_sysrem_kernel_ms has no call to repeat, nor has
// prom_filter_kernel_ms after a recover call
void grid_forget(prom_ctx* ctx) {
  ctx->sy.last_source = 0;
  if (ctx->rc.last == 2) ctx->rc.last = 0;
}

// the shared tail of the two inject grid calls on stream st
void inject_grid_on(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int64_t n_wav, const SyCall& c,
                    const GridList& g, double* U_out, double* cleaned_out, double* injected_out) {
  prom::SyDev& sy = ctx->sy;
  const int32_t n_exp = sy.n_exp, n_pix = sy.n_pix, n_cols = c.n_comp + c.ones;
  const int64_t n = (int64_t)n_exp * n_pix, nu = (int64_t)sy_items(ctx, c) * n_exp * n_cols;
  if (n_pix == 0) return grid_zero_U(c, n_exp, (int64_t)g.n_inj * sy_items(ctx, c), U_out);
  if (g.n_inj == 0 || (!U_out && !cleaned_out && !injected_out)) return;
  const int32_t nb_max = grid_plan(ctx, c, g.n_inj, false);
  grid_forget(ctx);
  grid_buffers(ctx, st, c, g, nb_max, n_wav, false);
  const double nan = std::nan("");
  prom::launch_observe_q(st, wav, (int32_t)n_wav, nan, nan, sy.q.as<double>());
  for (int32_t s = 0; s < prom::gr_sub_batches(g.n_inj, nb_max); ++s) {
    const int32_t b0 = prom::gr_sub_first(s, nb_max), nb = prom::gr_sub_count(s, nb_max, g.n_inj);
    grid_clean(ctx, st, wav, R, n_wav, c, b0, nb);
    if (U_out) download(U_out + b0 * nu, sy.U, nb * nu, st);
    if (cleaned_out) download(cleaned_out + b0 * n, sy.out, nb * n, st);
    if (injected_out) download(injected_out + b0 * n, sy.D, nb * n, st);
    PROM_HIP(hipStreamSynchronize(st));   // (the next sub-batch writes the same buffers; the last: the end of the call)
  }
}

// the shared tail of the two recover grid calls on stream st: the final model of every trial before the filter once
// (k_expose, k_highpass) into ex.model, which then stays; per sub-batch the inject grid's steps and W of every (U[b],
// ivar); per injection the filter out of place into rc.model and the moments against cleaned[b]
void recover_grid_on(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int64_t n_wav, const SyCall& c,
                     int32_t orders, const GridList& g, double* mom_out, int64_t* n_used_out, double* tot_out,
                     double* U_out) {
  prom::ExDev& ex = ctx->ex;
  prom::SyDev& sy = ctx->sy;
  prom::RcDev& rc = ctx->rc;
  const int32_t n_pix = ctx->obs.n_pix, n_exp = ex.n_exp, n_cols = c.n_comp + c.ones;
  const int64_t nu = (int64_t)n_exp * n_cols, nm = (int64_t)n_exp * ex.n_trial;
  if (!orders) tot_out = nullptr;
  if (n_pix == 0) {   // no pixel: zeros, and the inject call's U
    zero_moments(g.n_inj * nm, mom_out, n_used_out);
    if (tot_out) std::fill(tot_out, tot_out + prom::kOdTotals * g.n_inj * nm, 0.0);
    return grid_zero_U(c, n_exp, g.n_inj, U_out);
  }
  if (g.n_inj == 0) return;
  const ChainCall cc{c.highpass != 0, true, orders != 0, &sy.U, &rc.W, n_cols, &sy.out, Ran::none, true,
                     "the recovery keeps", ExOut{}};
  const int32_t nb_max = grid_plan(ctx, c, g.n_inj, true);
  chain_prepare(ctx, cc, n_wav);
  try {   // the filtered model of one injection beside the unfiltered one
    rc.model.ensure(sizeof(double) * (size_t)(nm * n_pix));
  } catch (const Error& err) {
    throw Error(err.code, std::string(err.what()) + ": the recovery grid keeps a second model of all " +
                              std::to_string(ex.n_trial) + " trials in device memory; give fewer trials per call");
  }
  record_last(ex, nullptr, nullptr, 0, Ran::none, 0);
  grid_forget(ctx);
  grid_buffers(ctx, st, c, g, nb_max, n_wav, true);
  const double nan = std::nan("");
  prom::launch_observe_q(st, wav, (int32_t)n_wav, nan, nan, sy.q.as<double>());
  prom::launch_observe_q(st, wav, (int32_t)n_wav, nan, nan, ex.q.as<double>());
  expose_launch(ctx, st, wav, R, (int32_t)n_wav, false, ex.model.as<double>(), nullptr, nullptr);
  if (c.highpass)
    highpass_launch(ex, st, ex.model.as<double>(), nm, n_pix);
  for (int32_t s = 0; s < prom::gr_sub_batches(g.n_inj, nb_max); ++s) {
    const int32_t b0 = prom::gr_sub_first(s, nb_max), nb = prom::gr_sub_count(s, nb_max, g.n_inj);
    grid_clean(ctx, st, wav, R, n_wav, c, b0, nb);
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

// a SyCall whose trial and scale pass the single calls' checks: the list has its own
SyCall grid_call(int32_t source, int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, int32_t orders = 0) {
  return SyCall{source, 0, highpass, n_comp, n_iter, ones, 0.0, orders};
}

}  // namespace

int32_t prom_transit_inject_grid(prom_ctx* ctx, int32_t n_inj, const int32_t* trial, const double* scale,
                                 int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out,
                                 double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    const SyCall c = grid_call(2, highpass, n_comp, n_iter, ones);
    const GridList g{n_inj, trial, scale};
    sysrem_check(ctx, "prom_transit_inject_grid", c);
    grid_check(ctx, "prom_transit_inject_grid", g);
    const TransitArgs t = ex_transit(ctx, "prom_transit_inject_grid");
    inject_grid_on(ctx, t.st, t.wav, t.R, t.n_wav, c, g, U_out, cleaned_out, injected_out);
  });
}

int32_t prom_spectrum_inject_grid(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                  int32_t n_inj, const int32_t* trial, const double* scale, int32_t highpass,
                                  int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out, double* cleaned_out,
                                  double* injected_out) {
  return guarded(ctx, [&] {
    prom::SyDev& sy = ctx->sy;
    const SyCall c = grid_call(3, highpass, n_comp, n_iter, ones);
    const GridList g{n_inj, trial, scale};
    sysrem_check(ctx, "prom_spectrum_inject_grid", c);
    grid_check(ctx, "prom_spectrum_inject_grid", g);
    const hipStream_t st = sy_spectrum(ctx, "prom_spectrum_inject_grid", n_orb, n_wav, wav, R);
    inject_grid_on(ctx, st, sy.wav.as<double>(), sy.R.as<double>(), n_wav, c, g, U_out, cleaned_out, injected_out);
  });
}

// SYSREM per order over a grid: entry b is what the per-order inject call gives for (trial[b], scale[b]); U_out is
// [n_inj][n_seg][n_exp][n_comp + ones]
int32_t prom_transit_inject_grid_orders(prom_ctx* ctx, int32_t n_inj, const int32_t* trial, const double* scale,
                                        int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out,
                                        double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    const SyCall c = grid_call(2, highpass, n_comp, n_iter, ones, 1);
    const GridList g{n_inj, trial, scale};
    sysrem_check(ctx, "prom_transit_inject_grid_orders", c);
    grid_check(ctx, "prom_transit_inject_grid_orders", g);
    const TransitArgs t = ex_transit(ctx, "prom_transit_inject_grid_orders");
    inject_grid_on(ctx, t.st, t.wav, t.R, t.n_wav, c, g, U_out, cleaned_out, injected_out);
  });
}

int32_t prom_spectrum_inject_grid_orders(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                         int32_t n_inj, const int32_t* trial, const double* scale, int32_t highpass,
                                         int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out,
                                         double* cleaned_out, double* injected_out) {
  return guarded(ctx, [&] {
    prom::SyDev& sy = ctx->sy;
    const SyCall c = grid_call(3, highpass, n_comp, n_iter, ones, 1);
    const GridList g{n_inj, trial, scale};
    sysrem_check(ctx, "prom_spectrum_inject_grid_orders", c);
    grid_check(ctx, "prom_spectrum_inject_grid_orders", g);
    const hipStream_t st = sy_spectrum(ctx, "prom_spectrum_inject_grid_orders", n_orb, n_wav, wav, R);
    inject_grid_on(ctx, st, sy.wav.as<double>(), sy.R.as<double>(), n_wav, c, g, U_out, cleaned_out, injected_out);
  });
}

int32_t prom_transit_recover_grid(prom_ctx* ctx, int32_t n_inj, const int32_t* trial, const double* scale,
                                  int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, int32_t orders,
                                  double* mom_out, int64_t* n_used_out, double* tot_out, double* U_out) {
  return guarded(ctx, [&] {
    const SyCall c = grid_call(2, highpass, n_comp, n_iter, ones);
    const GridList g{n_inj, trial, scale};
    recover_check(ctx, "prom_transit_recover_grid", c, orders);
    grid_check(ctx, "prom_transit_recover_grid", g);
    const TransitArgs t = ex_transit(ctx, "prom_transit_recover_grid");
    recover_grid_on(ctx, t.st, t.wav, t.R, t.n_wav, c, orders, g, mom_out, n_used_out, tot_out, U_out);
  });
}

int32_t prom_spectrum_recover_grid(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                   int32_t n_inj, const int32_t* trial, const double* scale, int32_t highpass,
                                   int32_t n_comp, int32_t n_iter, int32_t ones, int32_t orders, double* mom_out,
                                   int64_t* n_used_out, double* tot_out, double* U_out) {
  return guarded(ctx, [&] {
    prom::SyDev& sy = ctx->sy;
    const SyCall c = grid_call(3, highpass, n_comp, n_iter, ones);
    const GridList g{n_inj, trial, scale};
    recover_check(ctx, "prom_spectrum_recover_grid", c, orders);
    grid_check(ctx, "prom_spectrum_recover_grid", g);
    const hipStream_t st = sy_spectrum(ctx, "prom_spectrum_recover_grid", n_orb, n_wav, wav, R);
    recover_grid_on(ctx, st, sy.wav.as<double>(), sy.R.as<double>(), n_wav, c, orders, g, mom_out, n_used_out, tot_out,
                    U_out);
  });
}

}  // extern "C"
