// The filter's weights on the device (prom_filter_weights / prom_detrend_build / prom_*_recover):
// W[k][e][p] = (N_p^-1 U^T diag(v_p))[k][e] with N_p = U^T diag(v_p) U, per pixel p, by a Cholesky factorisation of
// N_p's lower triangle.  Definition in prom_hip.h ("the filter's weights on the device"); the arithmetic is
// filter_index.h's fw_weights, shared with the host harness.
//
// k_filter_weights: a thread owns one pixel, a workgroup is one wave of kFwTile consecutive pixels, so ivar[e][p] is
// read and W[k][e][p] stored along p.  The kernel is compiled once per K (a ladder of 16, as k_detrend's): the
// K (K + 1) / 2 entries of the triangle, y and x are never indexed at run time; the launch bound of one wave lets it
// take the unified file of 512 registers.  Up to K = 14 the triangle stays in registers; K = 15 and 16 (136 doubles
// and x: the compiler spilled) keep the rows from kFwRegRows on in LDS as [entry][lane], which is conflict-free, so
// no instantiation uses scratch (the table is in DESIGN.md, "Recovery on the device").  U[e][.] is uniform over the
// wave: scalar loads.  Pass 1 walks the exposures and forms N, the factorisation runs in place,
// pass 2 solves every weighted exposure without storing (an x that is not finite zeroes the whole pixel, and a W
// entry is to be written once), pass 3 solves again and stores.  There is no cross-lane arithmetic, no atomic, no
// barrier and no hand-off between workgroups, so a pixel's bits depend on its own column alone.  blockIdx.y is the
// injection of a recovery grid: U[b] is read and W[b] written (grid_index.h), ivar is shared; every other call is the
// batch of one.
//
// k_filter_weights_orders is the per-order instantiation (prom_filter_weights_orders, prom_detrend_build_orders;
// prom_hip.h "SYSREM per order on the device"): the same function text with the U pointer moved per lane by
// seg_of[p] n_exp K, so pixel p is filtered with the basis of its own order.  U is then no longer uniform over the
// wave: the compiler loads it with vector loads into registers of the lane, which is why the ladder has a threshold
// of its own (kFwRegCompOrders).  It is a kernel of its own and not a template flag of k_filter_weights, so the
// single-basis instantiations, their arguments included, are what they were.
#include "prom_internal.h"
#include "filter_index.h"
#include "grid_index.h"
#include "order_sysrem_index.h"

namespace prom {

static_assert(kFwTile == 64, "a workgroup of k_filter_weights is one wave along p");

// the triangle's entries an instantiation keeps in registers: all of them up to kFwRegComp components, the rows
// below kFwRegRows above (the rest in LDS, 41,472 bytes at K = 16)
constexpr int kFwRegComp = 14, kFwRegRows = 10;
constexpr int fw_reg_entries(int K) { return K <= kFwRegComp ? fw_entries(K) : fw_entries(kFwRegRows); }

template <int K>
__global__ void __launch_bounds__(kFwTile) k_filter_weights(const double* __restrict__ U,
                                                             const double* __restrict__ ivar, double* __restrict__ W,
                                                             int32_t n_exp, int32_t n_pix) {
  const int32_t p = fw_pixel(blockIdx.x, threadIdx.x);
  if (p >= n_pix) return;
  constexpr int NR = fw_reg_entries(K), NM = fw_entries(K) - NR;
  __shared__ double lds[NM > 0 ? NM * kFwTile : 1];
  const int32_t b = blockIdx.y;
  U += gr_u(b, n_exp, K);
  W += gr_w(b, K, n_exp, n_pix);
  FwTri<NR> L;
  L.mem = lds + threadIdx.x;
  L.pitch = kFwTile;
  fw_weights<K, NR>(L, U, ivar + ex_data(0, p, n_pix), W + dt_w(0, 0, p, n_exp, n_pix), n_pix, n_exp);
}

// the per-order ladder: with U in vector registers the triangle stays in registers up to kFwRegCompOrders components,
// and above that the rows below kFwRegRowsOrders (K = 16 spilled with the single-basis ladder's 10 rows)
constexpr int kFwRegCompOrders = 12, kFwRegRowsOrders = 8;
constexpr int fw_reg_entries_orders(int K) {
  return K <= kFwRegCompOrders ? fw_entries(K) : fw_entries(kFwRegRowsOrders);
}

template <int K>
__global__ void __launch_bounds__(kFwTile) k_filter_weights_orders(const double* __restrict__ U,
                                                                    const double* __restrict__ ivar,
                                                                    const int32_t* __restrict__ seg_of,
                                                                    double* __restrict__ W, int32_t n_exp,
                                                                    int32_t n_pix) {
  const int32_t p = fw_pixel(blockIdx.x, threadIdx.x);
  if (p >= n_pix) return;
  constexpr int NR = fw_reg_entries_orders(K), NM = fw_entries(K) - NR;
  __shared__ double lds[NM > 0 ? NM * kFwTile : 1];
  U += fo_u(seg_of[p], n_exp, K);   // the basis of p's own order
  FwTri<NR> L;
  L.mem = lds + threadIdx.x;
  L.pitch = kFwTile;
  fw_weights<K, NR>(L, U, ivar + ex_data(0, p, n_pix), W + dt_w(0, 0, p, n_exp, n_pix), n_pix, n_exp);
}

void launch_filter_weights_orders(hipStream_t s, const double* U, const double* ivar, const int32_t* seg_of, double* W,
                                  int32_t n_exp, int32_t n_comp, int32_t n_pix, hipEvent_t ev0, hipEvent_t ev1) {
  if (n_pix <= 0 || n_exp <= 0) return;
  if (n_comp < 1 || n_comp > kDtMaxComp) throw Error(PROM_E_ARG, "k_filter_weights: n_comp outside [1, 16]");
  const dim3 grid((uint32_t)fw_tiles(n_pix));
  if (ev0) PROM_HIP(hipEventRecord(ev0, s));
  switch (n_comp) {
#define PROM_FW_CASE(K)                                                                                            \
  case K:                                                                                                          \
    hipLaunchKernelGGL((k_filter_weights_orders<K>), grid, dim3(kFwTile), 0, s, U, ivar, seg_of, W, n_exp, n_pix); \
    break;
    PROM_FW_CASE(1) PROM_FW_CASE(2) PROM_FW_CASE(3) PROM_FW_CASE(4) PROM_FW_CASE(5) PROM_FW_CASE(6) PROM_FW_CASE(7)
    PROM_FW_CASE(8) PROM_FW_CASE(9) PROM_FW_CASE(10) PROM_FW_CASE(11) PROM_FW_CASE(12) PROM_FW_CASE(13)
    PROM_FW_CASE(14) PROM_FW_CASE(15) PROM_FW_CASE(16)
#undef PROM_FW_CASE
  }
  PROM_HIP(hipGetLastError());
  if (ev1) PROM_HIP(hipEventRecord(ev1, s));
}

void launch_filter_weights(hipStream_t s, const double* U, const double* ivar, double* W, int32_t n_exp, int32_t n_comp,
                           int32_t n_pix, hipEvent_t ev0, hipEvent_t ev1, int32_t n_inj) {
  if (n_pix <= 0 || n_exp <= 0 || n_inj <= 0) return;
  if (n_inj > kGrMaxBatch) throw Error(PROM_E_ARG, "k_filter_weights: more than 65535 injections in one launch");
  if (n_comp < 1 || n_comp > kDtMaxComp) throw Error(PROM_E_ARG, "k_filter_weights: n_comp outside [1, 16]");
  const dim3 grid((uint32_t)fw_tiles(n_pix), (uint32_t)n_inj);
  if (ev0) PROM_HIP(hipEventRecord(ev0, s));
  switch (n_comp) {
#define PROM_FW_CASE(K)                                                                                  \
  case K:                                                                                                \
    hipLaunchKernelGGL((k_filter_weights<K>), grid, dim3(kFwTile), 0, s, U, ivar, W, n_exp, n_pix);      \
    break;
    PROM_FW_CASE(1) PROM_FW_CASE(2) PROM_FW_CASE(3) PROM_FW_CASE(4) PROM_FW_CASE(5) PROM_FW_CASE(6) PROM_FW_CASE(7)
    PROM_FW_CASE(8) PROM_FW_CASE(9) PROM_FW_CASE(10) PROM_FW_CASE(11) PROM_FW_CASE(12) PROM_FW_CASE(13)
    PROM_FW_CASE(14) PROM_FW_CASE(15) PROM_FW_CASE(16)
#undef PROM_FW_CASE
  }
  PROM_HIP(hipGetLastError());
  if (ev1) PROM_HIP(hipEventRecord(ev1, s));
}

}  // namespace prom
