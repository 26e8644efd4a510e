// Injection and SYSREM on the device (prom_sysrem_set / prom_sysrem_clean / prom_transit_inject /
// prom_spectrum_inject): a trial's model multiplied into the raw exposures, the resident high-pass along each order,
// then the alternating least-squares fits of SYSREM, component by component.  Definitions in prom_hip.h.
//
//   k_gather_grid    Fj[e][b][tap] = F[e][trial[b]][tap]: the factors of the listed trials, so that ...
//   k_expose         (prom_expose.hip, unchanged) ... forms model[e][b][p] of those trials alone, with B in n_trial's place
//   k_inject_grid    D[b][e][p] from raw[e][p], model[e][b][p] and scale[b]
//   k_highpass       (prom_highpass.hip, unchanged, on request) D in place, as a model of B trials
//   k_sysrem_prep    w[e][p] and r[e][p] of the pitched work buffers from D and ivar; the padding gets w = 0, r = +0
//   k_sysrem_fill    a[e] and U[e][col] = one value (a component's first a; the column of ones)
//   k_sysrem_step    a workgroup (one wave) owns a tile of kSyTile pixel columns and keeps c_p in registers: it walks
//                    the exposures once for c = fit_c(a), then again for the tile's partials of fit_a(c),
//                    part[e][tile]; the last step of a component subtracts a c from r in the second walk instead
//   k_sysrem_rows    one workgroup: per exposure the tiles' partials in the fixed shape, a_e, the norm, a / norm into
//                    a[e] and U[e][col]; a norm that is not > 0 ends the component: its flag in device memory makes
//                    the component's later launches return at once, so the host never waits inside the loop
//   k_sysrem_finish  cleaned[e][p] = r where w > 0, else D
//
// k_sysrem_step reads r and w twice per launch, coalesced along p (a lane's kSyVec pixels are one vector, a wave reads
// 64 kSyVec consecutive doubles of a row); the second walk finds most of the tile in the caches.  a[e] and the flag
// are uniform over the workgroup.  The only cross-lane arithmetic is the butterfly of the row sums, whose shape
// sysrem_index.h fixes as a function of n_pix alone.  No atomics, no LDS in the step, plain vector stores.
//
// The injection grids (prom_*_inject_grid / prom_*_recover_grid) run the same five SYSREM kernels: blockIdx.y is the
// injection b, every per-injection buffer is [B][the single call's], and a kernel moves its pointers to b's slice
// (grid_index.h) before it does what it did.  The single call is the batch of one, literally: the C-ABI layer has one
// runner (prom_api_inject.hip, inject_steps), and a single call gives it a list of one entry, so every kernel here is one
// batched text with B = 1 and offset 0.  A component that ends sets flag `col` of b's own row of `ended`, so it stops
// b's later launches and nobody else's.
//
// SYSREM per order (prom_sysrem_clean_orders, prom_*_inject_orders, prom_*_inject_grid_orders): an order is one more
// batch item.  Item y = b n_seg + s of the work buffers is order s of injection b, n_max = max n_s wide
// (order_sysrem_index.h); k_sysrem_fill, k_sysrem_step and k_sysrem_rows run unchanged over n_inj n_seg items.
//   k_sysrem_prep_orders    w and r of item y from D[b][e][perm[first_s + i]], the padding beyond n_s as above
//   k_sysrem_finish_orders  cleaned[b][e][perm[first_s + i]] of item y; perm is a permutation, so every entry of the
//                           cleaned data is written exactly once
#include "prom_internal.h"
#include "sysrem_index.h"
#include "grid_index.h"
#include "order_sysrem_index.h"

namespace prom {

static_assert(kSyBlock == 64, "a k_sysrem_step workgroup is one wave: the butterfly is the whole tile");
static_assert(kSyRowsBlock % 64 == 0 && kSyRowsBlock <= 1024, "k_sysrem_rows: whole waves in one workgroup");

struct alignas(kSyVec * 8) SyVecD {
  double x[kSyVec];
};

__global__ void __launch_bounds__(kSyFlatBlock) k_gather_grid(const double* __restrict__ F, double* __restrict__ Fj,
                                                              const int32_t* __restrict__ trial, int32_t n_exp,
                                                              int32_t n_trial, int32_t n_tap, int32_t n_inj) {
  const int64_t i = (int64_t)blockIdx.x * kSyFlatBlock + threadIdx.x;
  if (i >= (int64_t)n_exp * n_tap) return;
  const int32_t b = blockIdx.y;
  const int32_t e = (int32_t)(i / n_tap), tap = (int32_t)(i % n_tap);
  Fj[gr_gather_to(e, b, tap, n_inj, n_tap)] = F[gr_gather_from(e, trial[b], tap, n_trial, n_tap)];
}

__global__ void __launch_bounds__(kSyFlatBlock) k_inject_grid(const double* __restrict__ raw,
                                                              const double* __restrict__ model,
                                                              const double* __restrict__ scale, double* __restrict__ D,
                                                              int32_t n_exp, int32_t n_pix, int32_t n_inj) {
  const int64_t i = (int64_t)blockIdx.x * kSyFlatBlock + threadIdx.x;
  if (i >= (int64_t)n_exp * n_pix) return;
  const int32_t b = blockIdx.y;
  const int32_t e = (int32_t)(i / n_pix), p = (int32_t)(i % n_pix);
  D[gr_inject_to(b, e, p, n_exp, n_pix)] =
      sy_inject(raw[ex_data(e, p, n_pix)], model[gr_inject_model(e, b, p, n_inj, n_pix)], scale[b]);
}

__global__ void __launch_bounds__(kSyFlatBlock) k_sysrem_prep(const double* __restrict__ D, const double* __restrict__ ivar,
                                                              double* __restrict__ r, double* __restrict__ w,
                                                              int32_t n_exp, int32_t n_pix, int64_t pitch) {
  const int64_t i = (int64_t)blockIdx.x * kSyFlatBlock + threadIdx.x;
  if (i >= (int64_t)n_exp * pitch) return;
  const int32_t b = blockIdx.y;   // the injection: its D, r and w (ivar is shared)
  D += gr_data(b, n_exp, n_pix);
  r += gr_work(b, n_exp, pitch);
  w += gr_work(b, n_exp, pitch);
  const int32_t e = (int32_t)(i / pitch), p = (int32_t)(i % pitch);
  double wv = 0.0, rv = 0.0;
  if (p < n_pix) {
    const double d = D[ex_data(e, p, n_pix)];
    wv = sy_weight(ivar[ex_data(e, p, n_pix)], d);
    if (wv > 0.0) rv = d;
  }
  w[sy_at(e, p, pitch)] = wv;
  r[sy_at(e, p, pitch)] = rv;
}

__global__ void __launch_bounds__(kSyFlatBlock) k_sysrem_fill(double* __restrict__ a, double* __restrict__ U, int32_t n_exp,
                                                              int32_t col, int32_t n_cols, double value) {
  const int32_t e = blockIdx.x * kSyFlatBlock + threadIdx.x;
  if (e >= n_exp) return;
  const int32_t b = blockIdx.y;
  a[gr_a(b, n_exp) + e] = value;
  U[gr_u(b, n_exp, n_cols) + sy_u(e, col, n_cols)] = value;
}

constexpr int kSyRowsAhead = 4;   // exposures of the second walk in flight at once

// part[e0 .. e0 + N - 1][tile] of the lane's tile from its c: N exposures' loads, lane sums and butterflies side by side
template <int N>
__device__ __forceinline__ void sy_step_partials(const double* __restrict__ r, const double* __restrict__ w,
                                                 const double (&c)[kSyVec], double2* __restrict__ part, int32_t e0,
                                                 int32_t p, int64_t pitch, int32_t lane, int32_t tile, int32_t n_tiles) {
  SyVecD wv[N], rv[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    wv[i] = *reinterpret_cast<const SyVecD*>(w + sy_at(e0 + i, p, pitch));
    rv[i] = *reinterpret_cast<const SyVecD*>(r + sy_at(e0 + i, p, pitch));
  }
  double tn[N], td[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    tn[i] = td[i] = 0.0;
#pragma unroll
    for (int v = 0; v < kSyVec; ++v) sy_fit_add(wv[i].x[v], rv[i].x[v], c[v], &tn[i], &td[i]);
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      tn[i] = sy_add(tn[i], __shfl_xor(tn[i], m, 64));
      td[i] = sy_add(td[i], __shfl_xor(td[i], m, 64));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) part[sy_part(e0 + i, tile, n_tiles)] = make_double2(tn[i], td[i]);
  }
}

template <bool LAST>
__global__ void __launch_bounds__(kSyBlock) k_sysrem_step(double* __restrict__ r, const double* __restrict__ w,
                                                          const double* __restrict__ a,
                                                          const int32_t* __restrict__ ended, double2* __restrict__ part,
                                                          int32_t n_exp, int64_t pitch, int32_t n_tiles) {
  const int32_t b = blockIdx.y;   // the injection: its flag, r, w, a and partials
  if (ended[gr_flag(b, 0)]) return;   // (uniform: the component's norm was not > 0)
  r += gr_work(b, n_exp, pitch);
  w += gr_work(b, n_exp, pitch);
  a += gr_a(b, n_exp);
  part += gr_part(b, n_exp, n_tiles);
  const int32_t lane = threadIdx.x, tile = blockIdx.x;
  const int32_t p = sy_pixel(tile, lane);
  // c = fit_c(a) of this lane's pixels, in ascending e
  double num[kSyVec], den[kSyVec], c[kSyVec];
#pragma unroll
  for (int v = 0; v < kSyVec; ++v) num[v] = den[v] = 0.0;
#pragma unroll 4
  for (int32_t e = 0; e < n_exp; ++e) {
    const SyVecD wv = *reinterpret_cast<const SyVecD*>(w + sy_at(e, p, pitch));
    const SyVecD rv = *reinterpret_cast<const SyVecD*>(r + sy_at(e, p, pitch));
    const double ae = a[e];
#pragma unroll
    for (int v = 0; v < kSyVec; ++v) sy_fit_add(wv.x[v], rv.x[v], ae, &num[v], &den[v]);
  }
#pragma unroll
  for (int v = 0; v < kSyVec; ++v) c[v] = sy_ratio(num[v], den[v]);
  // the second walk: the subtraction, or the tile's partials of fit_a(c), kSyRowsAhead exposures at a time (their
  // loads and butterflies are independent of each other; every exposure's sums keep their own shape)
  if (LAST) {
#pragma unroll 4
    for (int32_t e = 0; e < n_exp; ++e) {
      const SyVecD wv = *reinterpret_cast<const SyVecD*>(w + sy_at(e, p, pitch));
      SyVecD rv = *reinterpret_cast<const SyVecD*>(r + sy_at(e, p, pitch));
      const double ae = a[e];
#pragma unroll
      for (int v = 0; v < kSyVec; ++v) rv.x[v] = sy_residual(wv.x[v], rv.x[v], ae, c[v]);
      *reinterpret_cast<SyVecD*>(r + sy_at(e, p, pitch)) = rv;
    }
  } else {
    int32_t e = 0;
    for (; e + kSyRowsAhead <= n_exp; e += kSyRowsAhead)
      sy_step_partials<kSyRowsAhead>(r, w, c, part, e, p, pitch, lane, tile, n_tiles);
    for (; e < n_exp; ++e) sy_step_partials<1>(r, w, c, part, e, p, pitch, lane, tile, n_tiles);
  }
}

__global__ void __launch_bounds__(kSyRowsBlock) k_sysrem_rows(const double2* __restrict__ part, double* __restrict__ a,
                                                              double* __restrict__ U, int32_t* __restrict__ ended,
                                                              int32_t n_exp, int32_t n_tiles, int32_t col,
                                                              int32_t n_cols) {
  __shared__ double sA[kSyMaxExp];
  __shared__ double sNorm;
  const int32_t b = blockIdx.x;   // the injection: one workgroup each; its flag, partials, a and U
  ended += gr_flag(b, 0);
  if (*ended) return;   // (every thread reads the flag before the first barrier; thread 0 sets it after the last)
  part += gr_part(b, n_exp, n_tiles);
  a += gr_a(b, n_exp);
  U += gr_u(b, n_exp, n_cols);
  const int32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int32_t e = wave; e < n_exp; e += kSyRowsBlock / 64) {
    double tn = 0.0, td = 0.0;
    const int32_t cnt = sy_rows_count(lane, n_tiles);
    for (int32_t i = 0; i < cnt; ++i) {
      const double2 pt = part[sy_part(e, sy_rows_tile(lane, i), n_tiles)];
      tn = sy_add(tn, pt.x);
      td = sy_add(td, pt.y);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      tn = sy_add(tn, __shfl_xor(tn, m, 64));
      td = sy_add(td, __shfl_xor(td, m, 64));
    }
    if (lane == 0) sA[e] = sy_ratio(tn, td);
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int32_t e = 0; e < n_exp; ++e) s = sy_add(s, sy_mul(sA[e], sA[e]));
    sNorm = sy_sqrt(s);
  }
  __syncthreads();
  const double norm = sNorm;
  const bool ok = norm > 0.0;
  for (int32_t e = tid; e < n_exp; e += kSyRowsBlock) {
    const double v = ok ? sy_div(sA[e], norm) : 0.0;
    a[e] = v;
    U[sy_u(e, col, n_cols)] = v;
  }
  if (!ok && tid == 0) *ended = 1;
}

__global__ void __launch_bounds__(kSyFlatBlock) k_sysrem_finish(const double* __restrict__ D, const double* __restrict__ r,
                                                                const double* __restrict__ w, double* __restrict__ out,
                                                                int32_t n_exp, int32_t n_pix, int64_t pitch) {
  const int64_t i = (int64_t)blockIdx.x * kSyFlatBlock + threadIdx.x;
  if (i >= (int64_t)n_exp * n_pix) return;
  const int32_t b = blockIdx.y;
  D += gr_data(b, n_exp, n_pix);
  out += gr_data(b, n_exp, n_pix);
  r += gr_work(b, n_exp, pitch);
  w += gr_work(b, n_exp, pitch);
  const int32_t e = (int32_t)(i / n_pix), p = (int32_t)(i % n_pix);
  const int64_t at = sy_at(e, p, pitch);
  out[ex_data(e, p, n_pix)] = w[at] > 0.0 ? r[at] : D[ex_data(e, p, n_pix)];
}

__global__ void __launch_bounds__(kSyFlatBlock) k_sysrem_prep_orders(
    const double* __restrict__ D, const double* __restrict__ ivar, const int32_t* __restrict__ seg_first,
    const int32_t* __restrict__ perm, double* __restrict__ r, double* __restrict__ w, int32_t n_exp, int32_t n_pix,
    int32_t n_seg, int64_t pitch) {
  const int64_t t = (int64_t)blockIdx.x * kSyFlatBlock + threadIdx.x;
  if (t >= (int64_t)n_exp * pitch) return;
  const int32_t y = blockIdx.y;   // the item: order s of injection b
  const int32_t b = os_item_injection(y, n_seg), s = os_item_order(y, n_seg);
  const int32_t e = (int32_t)(t / pitch), i = (int32_t)(t % pitch);
  const int32_t n_s = seg_first[s + 1] - seg_first[s];
  double wv = 0.0, rv = 0.0;
  if (i < n_s) {
    const int32_t p = perm[os_slot(seg_first, s, i)];
    const double d = D[os_data(b, e, p, n_exp, n_pix)];
    wv = sy_weight(ivar[ex_data(e, p, n_pix)], d);
    if (wv > 0.0) rv = d;
  }
  w[os_work(y, e, i, n_exp, pitch)] = wv;
  r[os_work(y, e, i, n_exp, pitch)] = rv;
}

__global__ void __launch_bounds__(kSyFlatBlock) k_sysrem_finish_orders(
    const double* __restrict__ D, const double* __restrict__ r, const double* __restrict__ w,
    const int32_t* __restrict__ seg_first, const int32_t* __restrict__ perm, double* __restrict__ out, int32_t n_exp,
    int32_t n_pix, int32_t n_seg, int32_t n_max, int64_t pitch) {
  const int64_t t = (int64_t)blockIdx.x * kSyFlatBlock + threadIdx.x;
  if (t >= (int64_t)n_exp * n_max) return;
  const int32_t y = blockIdx.y;
  const int32_t b = os_item_injection(y, n_seg), s = os_item_order(y, n_seg);
  const int32_t e = (int32_t)(t / n_max), i = (int32_t)(t % n_max);
  if (i >= seg_first[s + 1] - seg_first[s]) return;
  const int32_t p = perm[os_slot(seg_first, s, i)];
  const int64_t at = os_work(y, e, i, n_exp, pitch), da = os_data(b, e, p, n_exp, n_pix);
  out[da] = w[at] > 0.0 ? r[at] : D[da];
}

static uint32_t flat_grid(int64_t n, const char* who) {
  const int64_t wgs = sy_flat_workgroups(n);
  if (wgs > (((int64_t)1 << 31) - 1)) throw Error(PROM_E_ARG, std::string(who) + ": too many entries for one launch");
  return (uint32_t)wgs;
}

void launch_gather_grid(hipStream_t s, const double* F, double* Fj, const int32_t* trial, int32_t n_exp, int32_t n_trial,
                        int32_t n_tap, int32_t n_inj) {
  if (n_exp <= 0 || n_tap <= 0 || n_inj <= 0) return;
  hipLaunchKernelGGL(k_gather_grid, dim3(flat_grid((int64_t)n_exp * n_tap, "k_gather_grid"), (uint32_t)n_inj),
                     dim3(kSyFlatBlock), 0, s, F, Fj, trial, n_exp, n_trial, n_tap, n_inj);
  PROM_HIP(hipGetLastError());
}

void launch_inject_grid(hipStream_t s, const double* raw, const double* model, const double* scale, double* D,
                        int32_t n_exp, int32_t n_pix, int32_t n_inj) {
  if (n_exp <= 0 || n_pix <= 0 || n_inj <= 0) return;
  hipLaunchKernelGGL(k_inject_grid, dim3(flat_grid((int64_t)n_exp * n_pix, "k_inject_grid"), (uint32_t)n_inj),
                     dim3(kSyFlatBlock), 0, s, raw, model, scale, D, n_exp, n_pix, n_inj);
  PROM_HIP(hipGetLastError());
}

// the components of `items` batch items n_pix wide, between the prep and the finish kernel: the column of ones, then
// per component the first a, n_iter steps and row sums, and the subtraction
static void sysrem_components(hipStream_t s, double* r, double* w, double* a, int32_t* ended, double2* pt, double* U,
                              int32_t n_exp, int32_t n_pix, int32_t n_comp, int32_t n_iter, int32_t ones,
                              int32_t items) {
  const int32_t n_cols = n_comp + ones, n_tiles = sy_tiles(n_pix);
  const int64_t pitch = sy_pitch(n_pix);
  const uint32_t B = (uint32_t)items;   // the item is blockIdx.y (blockIdx.x of the one-workgroup k_sysrem_rows)
  const dim3 fill_grid((uint32_t)sy_flat_workgroups(n_exp), B), tiles((uint32_t)n_tiles, B);
  int32_t col = 0;
  if (ones) {
    hipLaunchKernelGGL(k_sysrem_fill, fill_grid, dim3(kSyFlatBlock), 0, s, a, U, n_exp, col, n_cols, 1.0);
    hipLaunchKernelGGL((k_sysrem_step<true>), tiles, dim3(kSyBlock), 0, s, r, w, a, ended + col, pt, n_exp, pitch,
                       n_tiles);
    ++col;
  }
  for (int32_t k = 0; k < n_comp; ++k, ++col) {
    hipLaunchKernelGGL(k_sysrem_fill, fill_grid, dim3(kSyFlatBlock), 0, s, a, U, n_exp, col, n_cols, sy_first_a(n_exp));
    for (int32_t it = 0; it < n_iter; ++it) {
      hipLaunchKernelGGL((k_sysrem_step<false>), tiles, dim3(kSyBlock), 0, s, r, w, a, ended + col, pt, n_exp, pitch,
                         n_tiles);
      hipLaunchKernelGGL(k_sysrem_rows, dim3(B), dim3(kSyRowsBlock), 0, s, pt, a, U, ended + col, n_exp, n_tiles, col,
                         n_cols);
    }
    hipLaunchKernelGGL((k_sysrem_step<true>), tiles, dim3(kSyBlock), 0, s, r, w, a, ended + col, pt, n_exp, pitch,
                       n_tiles);
  }
}

void launch_sysrem(hipStream_t s, const double* D, const double* ivar, double* r, double* w, double* a, int32_t* ended,
                   double* part, double* U, double* out, int32_t n_exp, int32_t n_pix, int32_t n_comp, int32_t n_iter,
                   int32_t ones, int32_t n_inj) {
  if (n_pix <= 0 || n_exp <= 0 || n_inj <= 0) return;
  if (n_exp > kSyMaxExp) throw Error(PROM_E_ARG, "k_sysrem_rows: n_exp above 4096");
  if (n_inj > kGrMaxBatch) throw Error(PROM_E_ARG, "k_sysrem_step: more than 65535 injections in one launch");
  const int64_t pitch = sy_pitch(n_pix);
  const uint32_t B = (uint32_t)n_inj;   // the injection is blockIdx.y
  PROM_HIP(hipMemsetAsync(ended, 0, sizeof(int32_t) * kGrFlags * (size_t)n_inj, s));
  hipLaunchKernelGGL(k_sysrem_prep, dim3(flat_grid((int64_t)n_exp * pitch, "k_sysrem_prep"), B), dim3(kSyFlatBlock), 0,
                     s, D, ivar, r, w, n_exp, n_pix, pitch);
  sysrem_components(s, r, w, a, ended, reinterpret_cast<double2*>(part), U, n_exp, n_pix, n_comp, n_iter, ones, n_inj);
  hipLaunchKernelGGL(k_sysrem_finish, dim3(flat_grid((int64_t)n_exp * n_pix, "k_sysrem_finish"), B),
                     dim3(kSyFlatBlock), 0, s, D, r, w, out, n_exp, n_pix, pitch);
  PROM_HIP(hipGetLastError());
}

void launch_sysrem_orders(hipStream_t s, const double* D, const double* ivar, const int32_t* seg_first,
                          const int32_t* perm, double* r, double* w, double* a, int32_t* ended, double* part, double* U,
                          double* out, int32_t n_exp, int32_t n_pix, int32_t n_seg, int32_t n_max, int32_t n_comp,
                          int32_t n_iter, int32_t ones, int32_t n_inj) {
  if (n_pix <= 0 || n_exp <= 0 || n_inj <= 0 || n_seg <= 0 || n_max <= 0) return;
  if (n_exp > kSyMaxExp) throw Error(PROM_E_ARG, "k_sysrem_rows: n_exp above 4096");
  if ((int64_t)n_inj * n_seg > kGrMaxBatch)
    throw Error(PROM_E_ARG, "k_sysrem_step: more than 65535 (injection, order) items in one launch");
  const int64_t pitch = sy_pitch(n_max);
  const int32_t items = n_inj * n_seg;
  const uint32_t B = (uint32_t)items;   // the item y = b n_seg + s is blockIdx.y
  PROM_HIP(hipMemsetAsync(ended, 0, sizeof(int32_t) * kGrFlags * (size_t)items, s));
  hipLaunchKernelGGL(k_sysrem_prep_orders, dim3(flat_grid((int64_t)n_exp * pitch, "k_sysrem_prep_orders"), B),
                     dim3(kSyFlatBlock), 0, s, D, ivar, seg_first, perm, r, w, n_exp, n_pix, n_seg, pitch);
  sysrem_components(s, r, w, a, ended, reinterpret_cast<double2*>(part), U, n_exp, n_max, n_comp, n_iter, ones, items);
  hipLaunchKernelGGL(k_sysrem_finish_orders, dim3(flat_grid((int64_t)n_exp * n_max, "k_sysrem_finish_orders"), B),
                     dim3(kSyFlatBlock), 0, s, D, r, w, seg_first, perm, out, n_exp, n_pix, n_seg, n_max, pitch);
  PROM_HIP(hipGetLastError());
}

}  // namespace prom
