// What the recovery (prom_api_inject.hip) needs from the chain of the filtered exposure calls: declared here, defined
// once in prom_api_expose.hip.  Host code only.
#pragma once

#include "prom_api_shared.h"

namespace prom::api {

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

// which *_kernel_ms aid may repeat the call that ends
enum class Ran { none, detrend, highpass, orders };

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

// the "last call" state: the spectrum the call read (null: nothing to repeat) and the one aid that may repeat it
void record_last(prom::ExDev& ex, const double* wav, const double* R, int64_t n_wav, Ran ran, int32_t detrend);

// one pass over the table in batches of whole trial groups (ev: events around the k_expose launch of the first batch)
void expose_launch(prom_ctx* ctx, hipStream_t st, const double* wav, const double* R, int32_t n_wav, bool want_mom,
                   double* model, hipEvent_t ev0, hipEvent_t ev1);

// the resident high-pass, whichever kind it is (the weighted mean of prom_highpass_set or the median of
// prom_highpass_set_median), over n_rows rows of `model` in place
void highpass_launch(const prom::ExDev& ex, hipStream_t st, double* model, int64_t n_rows, int32_t n_pix,
                     hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// the moments of the model in ex.model against `data`, in batches of whole trial groups (ev: events around the first
// batch's k_model_moments; model: another buffer of ex.model's shape, a recovery grid's)
void moments_launch(prom_ctx* ctx, hipStream_t st, const double* data, hipEvent_t ev0, hipEvent_t ev1,
                    const double* model = nullptr);

// k_order_moments + k_order_totals over the final model in ex.model against `data`, in batches of whole trial groups
// under the scratch cap (one group at least); a batch's records go to the caller's arrays when they are wanted (ev:
// events around the two kernels of the first batch; model: as moments_launch's)
void orders_launch(prom_ctx* ctx, hipStream_t st, const double* data, double* orec_mom_out, int64_t* orec_n_used_out,
                   hipEvent_t* ev, const double* model = nullptr);

// 1: whether the call runs at all (false: the outputs are filled and there is nothing to do), the refusals of every
// stage that will run, before anything is launched, and the buffers of the whole table
bool chain_prepare(prom_ctx* ctx, const ChainCall& c, int64_t n_wav);

// 2, its first half: the model of every trial before the filter, into ex.model: k_expose without moments, then the
// high-pass in place (hp_ev: events around k_highpass); q of the grid is in ex.q
void chain_unfiltered(prom_ctx* ctx, hipStream_t st, const ChainCall& c, const double* wav, const double* R,
                      int32_t n_wav, const hipEvent_t* hp_ev = nullptr);

// q of the whole grid, then 2 and 3: the final model, the moments, the state the call leaves, the per-order kernels and
// the copies back
void chain_go(prom_ctx* ctx, hipStream_t st, const ChainCall& c, const double* wav, const double* R, int64_t n_wav);

}  // namespace prom::api
