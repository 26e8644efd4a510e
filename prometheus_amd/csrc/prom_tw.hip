// k_sigma_tw: the Doppler-shifted cross-section lookups and transmission curves over target windows.
#include "prom_tc.h"
#include "tw_index.h"
#include "tw_stage.h"

namespace prom {

// ---- sigma lookups + transmission curves over target windows (the default with orbital Doppler shift) ----
// The targets t = shift_o lambda_w of all rows, not the wavelengths, are cut into windows (host: prom_window.hip):
// window b holds, per row o, the contiguous wavelengths w in [W[b][o], W[b+1][o]) whose targets fall in the
// window's target interval (at most a few hundred per row).  Per species the table nodes those targets reach are
// one slice, staged once per window for every row: no Doppler-spread overlap between neighbouring windows' slices
// and no second workgroup staging the same slice for other rows.  The wavelengths the rows read, [lw0, lw1), are
// staged with them: the item loop then issues no vector load, only its stores (on gfx9 a load's vmcnt wait also
// waits for every earlier store: a global wavelength load per item cost each item a store round trip).  Slices and
// wavelengths share kTwLds doubles of LDS (22 KB: 24 bytes a node, 8 a wavelength), carved per window by the host.
// Work items are (row, 64 wavelengths) with the row wave-uniform: its Doppler factor, curve header and coefficients
// are scalar loads.  Per species slice (SigSeg kind & 3): 1 staged, with the host-verified linear guess (one LDS
// round: x_g, x_{g+1} and the record; a second only for lanes one node off); 3 staged without a guess (a slice
// across a change of node spacing: bisection in LDS); 2 the guess into the global records (a slice larger than the
// LDS) or 0 none (targets outside the table): the window goes to the second pass.  The second pass also takes the rows
// whose curve header says non-finite columns (flag 2, the reference's chord order) or a table truncated at the host's
// octave cap (flag 4, the exact sum beyond it): numpy's bracket from the table's directory, per point.  Every path
// evaluates fl(chi E_k) e^a (or E_k e^a - offset) of numpy's bracket k, so R does not depend on the windows: bitwise
// equal to k_sigma_tc's and for any wavelength or phase shard.
// What a wave needs before its first chunk is kept short: the staging reads the window's stage record (tw_stage.h,
// derived per set from the plan: one scalar load instead of a classification of every pool entry against every
// slice), a row's curve scalars are one batch of scalar loads held for all its chunks (TcRow, prom_tc.h), and the
// first pass is split outermost by wavelength source, so the staged instance's loops wait for no vector memory.

template <int NSIG, int D, bool MG, int RP>
__global__ void __launch_bounds__(kBlock) k_sigma_tw(const SigTabs4 tabv, const SigTabDev* __restrict__ tabp,
                                                     const PolyCoef pc, const double* __restrict__ wav,
                                                     int64_t n_wav, int32_t n_rows, const SigSeg* __restrict__ wseg,
                                                     const int32_t* __restrict__ wrow, const TwStage* __restrict__ wstg,
                                                     int32_t n_win, const TcArgs ta,
                                                     const double* __restrict__ hdr, const double* __restrict__ shift,
                                                     const double* __restrict__ ctab, double* __restrict__ Rout) {
  // (hdr, shift, ctab, Rout: TcArgs' hdr, tabv.t[0].shift, tab and R as __restrict__ parameters -- with the kernel's
  // stores provably elsewhere, the row's header and Doppler factor become scalar loads)
  static_assert(D > 0, "polynomial lookups only (coarse tables take k_sigma_tc)");
  // LDS: [0, 2 tot) the records {(chi) E_k, L_k} (species s at 2 pad), then tot + NSIG node x's (species s at pad + s:
  // x_lo .. x_{lo+m}), then the window's wavelengths (tw_stage.h: tw_lds_x, tw_lds_lam)
  __shared__ double2 lds2[kTwLds / 2 + 32];   // (+ 64 doubles: the staged wavelengths' padding, read past lw1)
  double* const lds = reinterpret_cast<double*>(lds2);
  // XCD-aware: workgroup ids round-robin over the 8 XCDs; XCD x takes windows [x per, (x + 1) per) in order, so
  // neighbouring windows (whose rows read overlapping wavelengths) share an L2
  const int32_t per = (n_win + 7) >> 3;
  const int32_t b = (int32_t)(blockIdx.x & 7) * per + (int32_t)(blockIdx.x >> 3);
  if (b >= n_win) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the window's stage record (tw_stage.h: one scalar load) and, for the first pass' guesses, its slices
  const TwStage st = wstg[b];
  SigSeg sg[NSIG];
#pragma unroll
  for (int s = 0; s < NSIG; ++s) sg[s] = wseg[(int64_t)b * NSIG + s];
  const bool wrare = (st.mode & kTwRare) != 0;      // (some species without a slice: second pass for the whole window)
  const bool wexact = (st.mode & kTwExact) != 0;    // (every guess is numpy's bracket at every target: k_tw_exact)
  const bool wsearch = (st.mode & kTwSearch) != 0;  // (some staged slice without a guess, kind 3: bisection in LDS)
  const int32_t tot = st.tot;                       // staged nodes (kinds 1 and 3)
  const int32_t lw0 = st.lw0, nlam = st.nlam;       // (nlam = 0: wavelengths from global memory)
  double2* const sel = lds2;
  double* const slam = lds + tw_lds_lam(tot, NSIG);
  // stage the slices and the wavelengths; every load issued before the first LDS write, none behind a test: a
  // thread past the pool's (the wavelengths') end loads entry 0 (the first wavelength) again and writes nothing, so
  // the loads stay one batch with one wait.  Pool entry i belongs to species #{s : bnd[s] <= i}: one classification
  // per entry, then its record base and abundance by selects -- from VGPR copies made once per thread (a select
  // takes no scalar operand beside its mask: each would be copied again per entry)
  {
    constexpr int NQ = (kTwLds / 3 + kBlock - 1) / kBlock;
    constexpr int NL = (kTwLamCap + kBlock - 1) / kBlock;
    const double4* recv[NSIG];   // species s' record of pool entry 0
    double chiv[NSIG];
#pragma unroll
    for (int s = 0; s < NSIG; ++s) {
      recv[s] = tabv.t[s].rec + st.off[s];
      chiv[s] = MG ? tabv.t[s].chi : 1.0;
      if constexpr (NSIG > 1) asm volatile("" : "+v"(recv[s]), "+v"(chiv[s]));
    }
    double lq[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int32_t i = tid + j * kBlock;
      lq[j] = (wav + lw0)[(uint32_t)(i < nlam ? i : 0)];
    }
    double4 q[NQ];
    int32_t sp[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int32_t i = tid + j * kBlock;
      const uint32_t iq = i < tot ? i : 0;
      sp[j] = tw_stage_species(st.bnd, NSIG, (int32_t)iq);
      const double4* rr = recv[0];
#pragma unroll
      for (int s = 1; s < NSIG; ++s) rr = sp[j] == s ? recv[s] : rr;
      q[j] = rr[iq];
    }
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int32_t i = tid + j * kBlock;
      if (i >= tot) continue;
      double e = q[j].y;
      if constexpr (MG) {
        double chi = chiv[0];
#pragma unroll
        for (int s = 1; s < NSIG; ++s) chi = sp[j] == s ? chiv[s] : chi;
        e = chi * e;
      }
      // x_i and the upper node x_{i+1} after it: the slot of the species' next entry, which writes the same bits
      // (a record's upper node is the next record's node), or after its last entry the slice's last upper node
      double* const xi = lds + tw_lds_x(tot, i, sp[j]);
      xi[0] = q[j].x;
      xi[1] = q[j].w;
      lds[2 * i] = e;
      lds[2 * i + 1] = q[j].z;
    }
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int32_t i = tid + j * kBlock;
      if (i < nlam) slam[i] = lq[j];
    }
  }
  __syncthreads();
  double choff = 0.0;
  if constexpr (MG) {
#pragma unroll
    for (int s = 0; s < NSIG; ++s) choff += tabv.t[s].chi * tabv.t[s].offset;
  }
  const int32_t* __restrict__ wa = wrow + (int64_t)b * n_rows;
  const int32_t* __restrict__ wz = wa + n_rows;
  // first pass: windows whose every species has a staged, guessed slice (kind 1), rows whose curve is complete (header
  // flags 2 and 4 clear).  Waves take whole rows (or row pairs) round robin, each row's Doppler factor and curve header
  // loaded once into scalar registers, then the rows' chunks of 64 wavelengths
  if (!wrare) {
    // per species, hoisted by hand (the compiler keeps them as per-lookup arithmetic otherwise): the slice's LDS
    // bases from the stage record (lookup address = g * 8 + base), and the guess's offset and the polynomial's leading
    // coefficient held in VGPRs (a 64-bit FMA takes one scalar operand: either would be copied to VGPRs before every use)
    const double* xsb[NSIG];
    const double2* elb[NSIG];
    double xsv[NSIG];
#pragma unroll
    for (int s = 0; s < NSIG; ++s) {
      xsb[s] = lds + tw_stage_xbase(st.base[s]);
      elb[s] = sel + tw_stage_elbase(st.base[s]);
      xsv[s] = sg[s].xs;
      asm volatile("" : "+v"(xsv[s]));
    }
    double cdv = pc.c[D];
    asm volatile("" : "+v"(cdv));
    int32_t lg = ta.lg;   // (held from here: left to the compiler, the arguments are loaded again for every row)
    int64_t rstride = n_wav;
    asm volatile("" : "+s"(lg), "+s"(rstride));
    // NP points per lane at once: rows a and b (RP = 2: a row pair, the two rows' chunks k side by side -- two
    // independent lookup chains per lane), with each row's Doppler factor, curve scalars, table and R row in scalar
    // registers for all its chunks
    struct RowS {
      TcRow c;
      double* Rrow;
      double sh;
      int32_t w0, w1;
      bool rare;   // (header flags 2 or 4: the second pass takes the row)
    };
    // one batch of scalar loads per row -- the header's flags, N_max, tfrac and tail coefficients, the Doppler factor
    // and the row's wavelength range, none behind a test of another -- and one wait: the empty asm takes them all,
    // so the loads stay together ahead of the second-pass test and the chunks reload none of them
    auto row_of = [&](int32_t o) {
      RowS r;
      const double* __restrict__ h = hdr + (int64_t)o * kTcHdr;
      r.c.h = h;
      r.c.tabo = ctab + (int64_t)o * lg * kTcD;
      r.c.nmax = h[kTcHNmax];
      r.c.tf = h[kTcHTfrac];
#pragma unroll
      for (int e = 0; e < 5; ++e) r.c.t[e] = h[kTcHT0 + e];
      double t5 = h[kTcHT0 + 5], fl = h[kTcHFlags];
      r.sh = shift[o];
      r.w0 = wa[o];
      r.w1 = wz[o];
      asm volatile(""
                   : "+s"(r.c.nmax), "+s"(r.c.tf), "+s"(r.c.t[0]), "+s"(r.c.t[1]), "+s"(r.c.t[2]), "+s"(r.c.t[3]),
                     "+s"(r.c.t[4]), "+s"(t5), "+s"(fl), "+s"(r.sh), "+s"(r.w0), "+s"(r.w1));
      r.rare = tc_flags_second_pass(fl);
      r.c.t5v = t5;
      asm volatile("" : "+v"(r.c.t5v));   // (the leading coefficient in VGPRs: one FMA may read one scalar pair)
      r.Rrow = Rout + (int64_t)o * rstride + lane;   // (this lane's column of the row)
      return r;
    };
    // MODE 0: every guess exact; 1: guesses with the one-node test; 2: as 1, kind-3 slices by bisection.  c0[p]: the
    // chunk's first wavelength (stores only where c0[p] + lane < w1), lam[p] the lane's wavelength
    auto chunk = [&](const RowS* rs, auto np_tag, const int32_t* c0, const double* lam, auto mode_tag) {
      constexpr int NP = decltype(np_tag)::value;
      constexpr int MODE = decltype(mode_tag)::value;
      constexpr bool EX = MODE == 0;
      double t[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) t[p] = rs[p].sh * lam[p];
      // every species' x_g (x_{g+1}) and record in one LDS round, then, unless every guess is exact, the rare
      // one-node corrections, then the e^a polynomials.  (tw_guess clamps at m - 2 only: the dispatch below computes
      // chunks of rows with wavelengths in the window only, every wavelength a lane reads is one of its row's or a
      // later one, and every target of the row lies in the slice, so fma(t, inv, xs) > -1 and the guess is >= 0.
      // Lanes past the row's end that fall into the stage's 64 entries of padding hold no wavelength at all: whatever
      // they look up, they store nothing)
      int32_t g[NP][NSIG];
      double x0[NP][NSIG], x1[NP][NSIG];
      double2 e[NP][NSIG];
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int s = 0; s < NSIG; ++s) {
          g[p][s] = tw_guess(t[p], sg[s].inv, xsv[s], sg[s].m);
          x0[p][s] = xsb[s][g[p][s]];
          if constexpr (!EX) x1[p][s] = xsb[s][g[p][s] + 1];
          e[p][s] = elb[s][g[p][s]];
        }
      if constexpr (!EX) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int s = 0; s < NSIG; ++s) {
            if (MODE == 2 && (sg[s].kind & 3) == 3) {
              // numpy's bracket, the largest k <= m - 2 with x_k <= t, by bisection over the staged slice
              int32_t k = 0;
              for (int32_t st2 = 1 << (31 - __builtin_clz((uint32_t)(sg[s].m - 1) | 1u)); st2 > 0; st2 >>= 1)
                if (k + st2 <= sg[s].m - 2 && xsb[s][k + st2] <= t[p]) k += st2;
              x0[p][s] = xsb[s][k];
              e[p][s] = elb[s][k];
              continue;
            }
            const bool lo = t[p] < x0[p][s], hi = t[p] >= x1[p][s];   // (no short-circuit: that would chain the reads)
            if (lo | hi) {
              const int32_t k = lo ? g[p][s] - 1 : g[p][s] + 1;
              x0[p][s] = xsb[s][k];
              e[p][s] = elb[s][k];
            }
          }
      }
      double acc[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        acc[p] = 0.0;
#pragma unroll
        for (int s = 0; s < NSIG; ++s) {
          const double a = e[p][s].y * (t[p] - x0[p][s]);
          double q = __builtin_fma(cdv, a, pc.c[D - 1]);   // (exp_taylor<D>, the leading coefficient from a VGPR)
#pragma unroll
          for (int k = D - 2; k >= 0; --k) q = __builtin_fma(q, a, pc.c[k]);
          if constexpr (MG) acc[p] = __builtin_fma(e[p][s].x, q, acc[p]);
          else acc[p] = __builtin_fma(e[p][s].x, q, -tabv.t[s].offset);
        }
        if constexpr (MG) acc[p] -= choff;
      }
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const double v = tc_eval_full_r(acc[p], rs[p].c);
        if (c0[p] + lane < rs[p].w1) rs[p].Rrow[c0[p]] = v;
      }
    };
    // the NP rows' chunks k = k0, k0 + G, ...: the wavelengths from the LDS stage (STAGED: no vector load in the row
    // and chunk loops, so no wait in them for the earlier stores either), else loaded up to four chunks at a time
    // before any of them is computed (one vmcnt wait -- which also waits for the earlier stores -- per batch).  A
    // row with fewer chunks than its partner computes a clamped chunk (tw_chunk_read: its first) and stores nothing;
    // every row here has w0 < w1 (tw_index.h)
    auto rows = [&](const RowS* rs, auto np_tag, int32_t k0, int32_t G, auto mode_tag, auto staged_tag) {
      constexpr int NP = decltype(np_tag)::value;
      int32_t nch = 0;
#pragma unroll
      for (int p = 0; p < NP; ++p) nch = max(nch, tw_chunks(rs[p].w0, rs[p].w1));
      if constexpr (decltype(staged_tag)::value) {
        for (int32_t k = k0; k < nch; k += G) {
          int32_t c0[NP];
          double lam[NP];
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            c0[p] = tw_chunk_first(rs[p].w0, k);
            lam[p] = slam[tw_lam_staged(rs[p].w0, rs[p].w1, k, lane, lw0)];
          }
          chunk(rs, np_tag, c0, lam, mode_tag);
        }
      } else {
        constexpr int B = 4 / NP;
        for (int32_t k = k0; k < nch; k += B * G) {
          double lam[B][NP];
#pragma unroll
          for (int j = 0; j < B; ++j)
#pragma unroll
            for (int p = 0; p < NP; ++p) lam[j][p] = wav[tw_lam_global(rs[p].w0, rs[p].w1, k + j * G, lane)];
#pragma unroll
          for (int j = 0; j < B; ++j) {
            if (k + j * G >= nch) break;
            int32_t c0[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) c0[p] = tw_chunk_first(rs[p].w0, k + j * G);
            chunk(rs, np_tag, c0, lam[j], mode_tag);
          }
        }
      }
    };
    // the pass for one wavelength source: the split is outermost, so the staged instance's row loop is its own code
    auto first_pass = [&](auto staged_tag) {
      auto rows_mode = [&](const RowS* rs, auto np_tag, int32_t k0, int32_t G) {
        if (wexact) rows(rs, np_tag, k0, G, std::integral_constant<int, 0>{}, staged_tag);
        else if (!wsearch) rows(rs, np_tag, k0, G, std::integral_constant<int, 1>{}, staged_tag);
        else rows(rs, np_tag, k0, G, std::integral_constant<int, 2>{}, staged_tag);
      };
      if constexpr (RP == 1) {
        const int32_t G = tw_waves_per_unit(n_rows);   // waves per row
        for (int32_t o = __builtin_amdgcn_readfirstlane(wv / G); o < n_rows; o += 4 / G) {
          const RowS r1[1] = {row_of(o)};
          if (r1[0].rare) continue;   // (second pass)
          rows_mode(r1, std::integral_constant<int, 1>{}, wv % G, G);
        }
      } else {
        // row pairs (2q, 2q + 1) round robin over the waves (G waves per pair when there are fewer than 4 pairs); a
        // pair with one row absent (in the second pass, past n_rows or without wavelengths in this window) runs its
        // other row alone, a pair of two absent rows nothing: no chunk of an empty row is ever computed
        const int32_t P = (n_rows + 1) >> 1;
        const int32_t G = tw_waves_per_unit(P);
        for (int32_t q = __builtin_amdgcn_readfirstlane(wv / G); q < P; q += 4 / G) {
          const int32_t oa = 2 * q, ob = 2 * q + 1;
          const RowS a = row_of(oa), z = row_of(ob < n_rows ? ob : oa);   // (past the last row: loaded from oa, absent)
          const bool ra = tw_row_absent(a.rare, a.w0, a.w1);
          const bool rb = ob >= n_rows || tw_row_absent(z.rare, z.w0, z.w1);
          const int32_t pr = tw_pair_rows(ra, rb);
          if (pr == 3) {
            const RowS r2[2] = {a, z};
            rows_mode(r2, std::integral_constant<int, 2>{}, wv % G, G);
          } else if (pr != 0) {
            const RowS r1[1] = {pr == 1 ? a : z};
            rows_mode(r1, std::integral_constant<int, 1>{}, wv % G, G);
          }
        }
      }
    };
    if (nlam > 0) first_pass(std::true_type{});
    else first_pass(std::false_type{});
  }
  // second pass: the rest (kinds 0, 2, 3, rows with header flags 2 or 4), numpy's bracket per
  // point from the table's directory; items (row o, chunk c of 64 wavelengths) to waves round robin
  auto run_pass = [&](auto pass_tag) {
    constexpr int pass = decltype(pass_tag)::value;
    // the next item of this pass at or after (o, c): its row's wavelength range, or o = n_rows
    auto next_item = [&](int32_t& o, int32_t& c, int32_t& w0, int32_t& w1) {
      o = __builtin_amdgcn_readfirstlane(o);
      c = __builtin_amdgcn_readfirstlane(c);
      while (o < n_rows) {
        const bool rare = wrare || ((int32_t)hdr[(int64_t)o * kTcHdr + kTcHFlags] & 6) != 0;
        if (rare == (pass == 1)) {
          w0 = __builtin_amdgcn_readfirstlane(wa[o]);
          w1 = __builtin_amdgcn_readfirstlane(wz[o]);
          const int32_t nch = (w1 - w0 + 63) >> 6;
          if (c < nch) return;
          c = __builtin_amdgcn_readfirstlane(c - nch);
        }
        o = __builtin_amdgcn_readfirstlane(o + 1);
      }
    };
    int32_t on = 0, cn = wv, w0n = 0, w1n = 0;
    next_item(on, cn, w0n, w1n);
    while (on < n_rows) {
      const int32_t o = __builtin_amdgcn_readfirstlane(on), w1 = __builtin_amdgcn_readfirstlane(w1n);
      const int32_t w = __builtin_amdgcn_readfirstlane(w0n + cn * 64) + lane;
      const bool live = w < w1;
      const double lam = wav[live ? w : w1 - 1];
      cn += 4;
      next_item(on, cn, w0n, w1n);
      const double t = shift[o] * lam;
      const double* h = hdr + (int64_t)o * kTcHdr;
      double acc = 0.0, v;
      {
        // second pass: numpy's bracket per point; zr (merged species, non-finite columns): some chi_s sigma_s not > 0
        bool zr = false;
#pragma unroll
        for (int s = 0; s < NSIG; ++s) {
          const SigTabDev& tb = tabp[s];   // (from memory here: the argument copy's fields would stay live in SGPRs)
          if (t >= tb.xfirst && t < tb.xlast) {
            const double4 q = tb.rec[bracket_of(t, tb)];
            const double ex = exp_taylor<D>(q.z * (t - q.x), pc);
            if constexpr (MG) {
              acc = __builtin_fma(tb.chi * q.y, ex, acc);
              zr = zr || !(tb.chi * __builtin_fma(q.y, ex, -tb.offset) > 0.0);
            } else {
              acc = __builtin_fma(q.y, ex, -tb.offset);
            }
          } else {
            const double sv = sigma_poly_of(t, tb, pc, D);   // (numpy's end rules)
            if constexpr (MG) {
              acc = __builtin_fma(tb.chi, sv + tb.offset, acc);
              zr = zr || !(tb.chi * sv > 0.0);
            } else {
              acc = sv;
            }
          }
        }
        if constexpr (MG) acc -= choff;
        const double Y = acc;
        // non-finite columns (flag 2): the reference's chord order with ocml exp (k_sigma_tc's rule); else the curve,
        // or beyond a truncated table the exact sum in chord order (tc_eval's) -- one chord loop for both
        const bool nf = ((int32_t)h[kTcHFlags] & 2) != 0;
        const double q = Y * h[kTcHNmax];
        const int32_t L = (int32_t)h[kTcHL];
        const int32_t j = q <= 1.0e300 ? tc_exponent(q) - kTcExpEps : 0x7fffffff;
        const bool beyond = !nf && q >= kTcEps && q == q && j >= L && !((int32_t)h[kTcHFlags] & 1);
        if (!nf && !beyond) {
          v = tc_eval_full(Y, h, ctab + (int64_t)o * ta.lg * kTcD);
        } else {
          const double fs = h[kTcHFsum];
          const double a = tc_chord_sum(Y, nf, zr, fs, ta.flags + (int64_t)o * ta.n_pr, ta.ncol + (int64_t)o * ta.n_pr,
                                        ta.fout, ta.n_pr);
          if (beyond && ta.evals) atomicAdd(&ta.evals[threadIdx.x & 63], (unsigned long long)(int32_t)h[kTcHNact]);
          v = nf ? (a + h[kTcHTfrac] * fs) / fs : h[kTcHTfrac] + a;
        }
      }
      if (live) Rout[(int64_t)o * n_wav + w] = v;
    }
  };
  run_pass(std::integral_constant<int, 1>{});
}

// per set (prom_transit_set, after new windows): a window's guessed slices (kind 1) are exact (kind |= 4) when every
// guess is numpy's bracket at every target the window's rows look up (k_seg_exact's test on the windows): k_sigma_tw
// then reads x_g and the record only, with no bracket test.  The window's stage record takes kTwExact with them when
// every species' slice is a guessed one (tw_stage_of's rule on the marked slices)
template <int NSIG>
__global__ void __launch_bounds__(kBlock) k_tw_exact(const SigTabs4 tabv, const double* __restrict__ wav,
                                                     int32_t n_rows, SigSeg* __restrict__ wseg,
                                                     const int32_t* __restrict__ wrow, TwStage* __restrict__ wstg) {
  const int32_t b = blockIdx.x;
  const int32_t* wa = wrow + (int64_t)b * n_rows;
  const int32_t* wz = wa + n_rows;
  __shared__ int32_t bad;
  if (threadIdx.x == 0) bad = 0;
  bool all1 = true;   // every species' slice a guessed one: the window is exact when they all are
#pragma unroll
  for (int s = 0; s < NSIG; ++s) all1 = all1 && (wseg[(int64_t)b * NSIG + s].kind & 3) == 1;
  __syncthreads();
  bool ok = true;
  for (int32_t o = 0; o < n_rows; ++o) {
    const int32_t w0 = wa[o], w1 = wz[o];
    for (int32_t w = w0 + (int32_t)threadIdx.x; w < w1; w += kBlock) {
      const double t = tabv.t[0].shift[o] * wav[w];
#pragma unroll
      for (int s = 0; s < NSIG; ++s) {
        const SigSeg sg = wseg[(int64_t)b * NSIG + s];
        if ((sg.kind & 3) != 1) continue;
        const int32_t g = seg_guess(t, sg.xs, sg.inv, sg.m);
        const double* __restrict__ X = tabv.t[s].x + sg.lo;
        int32_t a = 0, c = sg.m - 1;   // X[a] <= t < X[c]: the window's slice bounds every target
        while (c - a > 1) {
          const int32_t mid = (a + c) >> 1;
          if (X[mid] <= t) a = mid; else c = mid;
        }
        ok = ok && a == g;
      }
    }
  }
  if (!ok) bad = 1;   // (benign race: every writer stores 1)
  __syncthreads();
  if (threadIdx.x < NSIG && !bad) {
    SigSeg& sg = wseg[(int64_t)b * NSIG + threadIdx.x];
    if ((sg.kind & 3) == 1) sg.kind |= 4;
  }
  if (threadIdx.x == 0 && !bad && all1) wstg[b].mode |= kTwExact;   // (the stage record's mode follows the marks)
}

void launch_tw_exact(hipStream_t s, TransitDev& tr, int32_t nsig) {
  if (!tr.tw_ok || tr.n_tw <= 0) return;
  SigSeg* twseg = tr.tw_seg.as<SigSeg>();
  const int32_t* twrow = tr.tw_row.as<int32_t>();
  TwStage* twstg = tr.tw_stage.as<TwStage>();
#define PROM_TWE(NS)                                                                                            \
  hipLaunchKernelGGL((k_tw_exact<NS>), dim3((unsigned)tr.n_tw), dim3(kBlock), 0, s, tr.sigtab_v, tr.wav.as<double>(), \
                     tr.n_orb, twseg, twrow, twstg)
  switch (nsig) {
    case 1: PROM_TWE(1); break;
    case 2: PROM_TWE(2); break;
    case 3: PROM_TWE(3); break;
    default: PROM_TWE(4); break;
  }
#undef PROM_TWE
  PROM_HIP(hipGetLastError());
}

void launch_sigma_tw(hipStream_t s, TransitDev& tr, int32_t nsig, int32_t deg, const TcArgs& ta, hipEvent_t ev0,
                     hipEvent_t ev1) {
  const unsigned nbw = (unsigned)(((int64_t)tr.n_tw + 7) / 8 * 8);   // one workgroup per window, XCD-interleaved ids
  const SigSeg* twseg = tr.tw_seg.as<SigSeg>();
  const int32_t* twrow = tr.tw_row.as<int32_t>();
  const TwStage* twstg = tr.tw_stage.as<TwStage>();
  const PolyCoef& pc = poly_coef();
  const SigTabs4& tabv = tr.sigtab_v;
  const SigTabDev* tabp = tr.sigtab.as<SigTabDev>();   // (the same descriptors in device memory: the second pass)
  const double* wav = tr.wav.as<double>();
  const int32_t n_rows = tr.n_orb;
  const int64_t n_wav = tr.n_wav;
  PROM_REQUIRE(deg > 0 && n_rows >= 2 && tr.n_tw > 0, "k_sigma_tw: polynomial lookups with orbital Doppler rows");
  // row pairs per wave in the first pass (two lookup chains per lane) for one species: 64 VGPRs either way, C4x10
  // 47-48 against 49-52 us (profiles/r06u_*); several species: single rows (three species with pairs: 98 VGPRs, 4 waves
  // per SIMD, C3 39.5 against 37.2 us).  PROM_TW_RP (read once): 1 or 2 forces either
  static const int rp_env = [] { const char* e = std::getenv("PROM_TW_RP"); return e ? std::atoi(e) : 0; }();
  const int rp = rp_env == 1 || rp_env == 2 ? rp_env : (nsig == 1 ? 2 : 1);
#define PROM_TWK(NS, DG, MGV)                                                                                        \
  if (rp == 2)                                                                                                       \
    hipExtLaunchKernelGGL((k_sigma_tw<NS, DG, MGV, 2>), dim3(nbw), dim3(kBlock), 0, s, ev0, ev1, 0, tabv, tabp, pc, wav, \
                          n_wav, n_rows, twseg, twrow, twstg, tr.n_tw, ta, ta.hdr, tabv.t[0].shift, ta.tab, ta.R);   \
  else                                                                                                               \
    hipExtLaunchKernelGGL((k_sigma_tw<NS, DG, MGV, 1>), dim3(nbw), dim3(kBlock), 0, s, ev0, ev1, 0, tabv, tabp, pc, wav, \
                          n_wav, n_rows, twseg, twrow, twstg, tr.n_tw, ta, ta.hdr, tabv.t[0].shift, ta.tab, ta.R)
#define PROM_TWD(NS, MGV)                 \
  if (deg <= 8) { PROM_TWK(NS, 8, MGV); } \
  else { PROM_TWK(NS, 14, MGV); }
  switch (nsig) {
    case 1: PROM_TWD(1, false) break;
    case 2: PROM_TWD(2, true) break;
    case 3: PROM_TWD(3, true) break;
    default: PROM_TWD(4, true) break;
  }
#undef PROM_TWD
#undef PROM_TWK
  PROM_HIP(hipGetLastError());
}

}  // namespace prom
