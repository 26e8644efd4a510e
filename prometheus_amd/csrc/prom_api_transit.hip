// The transit entries of the C-ABI layer: prom_transit_set, run, kernel_ms, result, columns and band_stats.  Host code
// only.  prom_transit_set is a sequence of file-local steps, the member functions of one SetState; the arithmetic the
// kernels trust (sigma segments, mirror pairs, star slices, polynomial degree) is prom_segments.hip's, the target
// windows prom_window.hip's.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "prom_api_shared.h"
#include "tw_stage.h"

namespace {

// prom_transit_set's inputs: small arrays are appended to a host image at add() (the callers' temporaries
// may die before the flush) and reach the device as one DMA of [descriptors | data] plus one scatter kernel,
// instead of a pageable copy each; large arrays are copied directly (one DMA when they sit in the pinned
// pool, e.g. the wavelength grid of a Transit)
struct Stager {
  static constexpr size_t kSmall = (size_t)256 << 10;
  std::vector<char> img;
  std::vector<std::pair<DevBuf*, int64_t>> ent;   // destination, offset in img
  std::vector<int64_t> len;
  template <class T>
  void add(DevBuf& b, const T* h, int64_t n, hipStream_t s) {
    b.ensure(sizeof(T) * (size_t)std::max<int64_t>(n, 1));
    if (n <= 0) return;
    const size_t bytes = sizeof(T) * (size_t)n;
    if (bytes > kSmall) {
      PROM_HIP(hipMemcpyAsync(b.p, h, bytes, hipMemcpyHostToDevice, s));
      return;
    }
    const size_t off = (img.size() + 15) & ~(size_t)15;
    img.resize(off + bytes);
    std::memcpy(img.data() + off, h, bytes);
    ent.push_back({&b, (int64_t)off});
    len.push_back((int64_t)bytes);
  }
  template <class T>
  void add(DevBuf& b, const std::vector<T>& v, hipStream_t s) { add(b, v.data(), (int64_t)v.size(), s); }
  void flush(prom_ctx* ctx, hipStream_t s) {
    if (ent.empty()) return;
    const size_t n = ent.size();
    const size_t head = (sizeof(prom::ScatterDesc) * n + 255) & ~(size_t)255;
    const size_t total = head + img.size();
    if (ctx->upin_cap < total) {
      // nothing reads the old staging: every set ends with a stream synchronisation
      if (ctx->upin) PROM_HIP(hipHostFree(ctx->upin));
      ctx->upin = nullptr;
      ctx->upin_cap = 0;
      const size_t cap = std::max<size_t>(total * 2, (size_t)1 << 20);
      PROM_HIP(hipHostMalloc(&ctx->upin, cap, hipHostMallocDefault));
      ctx->upin_cap = cap;
    }
    ctx->ustage.ensure(ctx->upin_cap);
    char* dbase = static_cast<char*>(ctx->ustage.p);
    auto* d = static_cast<prom::ScatterDesc*>(ctx->upin);
    for (size_t i = 0; i < n; ++i) d[i] = prom::ScatterDesc{ent[i].first->p, (int64_t)head + ent[i].second, len[i]};
    std::memcpy(static_cast<char*>(ctx->upin) + head, img.data(), img.size());
    PROM_HIP(hipMemcpyAsync(dbase, ctx->upin, total, hipMemcpyHostToDevice, s));
    prom::launch_scatter(s, dbase, reinterpret_cast<const prom::ScatterDesc*>(dbase), (int32_t)n);
    img.clear();
    ent.clear();
    len.clear();
  }
};

// an environment switch that is on unless set to 0 / off unless set to a non-zero number
bool env_not0(const char* name) {
  const char* e = std::getenv(name);
  return !(e && std::atoi(e) == 0);
}
bool env_on(const char* name) {
  const char* e = std::getenv(name);
  return e && std::atoi(e) != 0;
}

// What the steps of prom_transit_set share: the call's arguments, the staged uploads, the scenarios' per-phase arrays
// and counts, the per-set environment switches that do not live in TransitDev, and the sigma-segment cache key of
// this set (committed at the end, after the device copy succeeded)
struct SetState {
  prom_ctx* ctx;
  const prom_transit_problem* pb;
  prom::TransitDev& tr;
  hipStream_t s;
  Stager stg;
  int64_t n_orb = 0, tab_total = 0;
  int32_t n_atoms = 0, n_mol = 0;
  std::vector<double> bx, by, sh;   // [n_sc][n_orb]
  // PROM_MOL_MIRROR, PROM_SIGMA_ROWS=0, PROM_SEG_DIR, PROM_TW=0, PROM_SIG_POLY, PROM_TW_EXACT, PROM_DEBUG;
  // PROM_TC_LG (INT_MAX: unset), PROM_TC_PARTS (0: unset)
  bool mir_on, no_guess, use_dir, tw_off, sig_poly, tw_exact, debug;
  int tc_lg_cap, tc_parts;
  bool seg_key_new = false, seg_key_keep = false;
  std::vector<double> new_key_sh;
  std::vector<uint64_t> new_key_gen;
  // the steps, in prom_transit_set's order
  void read_options(), collect_scenarios(), pair_chords(), stage_inputs(), normalise_columns(), sigma_segments(),
      target_windows(), poly_degree(), stellar_setup(), density_tables(), slot_buffers(), finish_set();
};

// 1. reads pb; leaves nothing: throws on a request without its arrays
void check_request(const prom_transit_problem* pb) {
  PROM_REQUIRE(pb->n_wav >= 1 && pb->wavelength, "transit: need >= 1 wavelength");
  PROM_REQUIRE(pb->n_pr >= 1 && pb->n_orb >= 1 && pb->chord_y && pb->chord_z && pb->chord_fout,
               "transit: need chords and phases");
  PROM_REQUIRE(pb->n_x >= 1 && pb->x, "transit: need line-of-sight samples");
  PROM_REQUIRE(pb->planet_y, "transit: planet_y missing");
  PROM_REQUIRE(pb->n_moons >= 0 && (pb->n_moons == 0 || (pb->moon_y && pb->moon_R)), "transit: moons");
  PROM_REQUIRE(pb->n_scenarios >= 1 && pb->scenarios, "transit: need >= 1 density scenario");
  PROM_REQUIRE(pb->n_wav <= ((int64_t)65535 << 8), "transit: n_wav too large for one shard");
}

// 2. reads pb's sizes and options and the per-set environment; leaves the sizes, options and switches in tr and
// here, the context's other residents told that the problem changed, every stream idle and the old graphs dropped
void SetState::read_options() {
  tr.n_wav = pb->n_wav;
  tr.n_pr = pb->n_pr;
  n_orb = tr.n_orb = pb->n_orb;
  if (ctx->obs.set && ctx->obs.n_orb != pb->n_orb) ctx->obs.set = false;   // the observation's phases are gone
  ctx->obs.last_wav = ctx->obs.last_R = nullptr;   // (this set may move the buffers the last observe call read)
  if (ctx->vm.set && ctx->vm.n_orb != pb->n_orb) ctx->vm.set = false;      // ... and the trial table's with them
  ctx->vm.last_wav = ctx->vm.last_R = nullptr;
  if (ctx->ex.set && ctx->ex.n_orb != pb->n_orb) ctx->ex.set = false;      // ... and the exposure table's rows
  ctx->ex.last_wav = ctx->ex.last_R = nullptr;
  ctx->br.last_wav = ctx->br.last_q = ctx->br.last_R = nullptr;   // ... and those prom_transit_broaden read
  ctx->br.last_out = nullptr;
  tr.n_x = pb->n_x;
  tr.n_sc = pb->n_scenarios;
  tr.n_moons = pb->n_moons;
  tr.delta_x = pb->delta_x;
  tr.planet_R = pb->planet_R;
  tr.cull_tau = pb->cull_tau > 0.0 ? pb->cull_tau : std::ldexp(1.0, -60);
  for (auto st : ctx->streams) PROM_HIP(hipStreamSynchronize(st));   // pipelined runs may still read the old problem
  drop_graphs(tr);   // captured against the old problem's buffers and arguments
  tr.exp_mode = (pb->options & PROM_OPT_OCML_EXP) ? 0 : 1;
  tr.merge = (pb->options & PROM_OPT_NO_MERGE) == 0;
  tr.window = (pb->options & PROM_OPT_NO_WINDOW) == 0;
  // measured on MI355X (tools/host_overhead.py, C2): hipGraphLaunch costs the host ~16 us per run
  // against ~8.5 us for the three direct launches, so graphs are opt-in (PROM_GRAPH=1)
  tr.graphs = env_on("PROM_GRAPH");
  tr.plan = env_not0("PROM_TAU_PLAN");
  tr.species_merge_ok = env_not0("PROM_SPECIES_MERGE");   // narrowed by normalise_columns
  tr.tcurve = env_not0("PROM_TCURVE");                    // narrowed by normalise_columns
  // the per-run switches of the windowed path, read here rather than in every prom_transit_run (getenv scans
  // the environment: ~1 us a call on the GPU box's hosts, against ~8.5 us for a run's three launches)
  const char* fk = std::getenv("PROM_SIGMA_FORK");
  tr.env_fork = fk ? (std::atoi(fk) != 0 ? 1 : 0) : -1;
  tr.env_stagger = env_on("PROM_SIG_STAGGER");
  tr.col_spec = env_not0("PROM_COL_SPEC");
  tr.mol_stage = env_not0("PROM_MOL_STAGE");
  mir_on = env_not0("PROM_MOL_MIRROR");
  // PROM_SIGMA_ROWS=0 (validation): every block without a guess -- per-target directory lookups (sigma_of) everywhere,
  // numpy.interp + exp10 rows
  no_guess = !env_not0("PROM_SIGMA_ROWS");
  // PROM_SEG_DIR=0 (comparisons): no bucket directories.  Like no_guess, such segments are neither reused nor
  // committed as the key, so toggling the switch between sets with the same tables never measures the other
  use_dir = env_not0("PROM_SEG_DIR");
  tw_off = !env_not0("PROM_TW");   // (read at every set): 0 never
  sig_poly = env_not0("PROM_SIG_POLY");
  tw_exact = env_not0("PROM_TW_EXACT");   // 0: no exact marks on the windows' slices, for comparisons
  debug = std::getenv("PROM_DEBUG") != nullptr;
  // PROM_TC_LG (tests): a lower octave cap, so that points above the table take the exact per-point sum;
  // PROM_TC_PARTS (profiling): k_tc_build's part count
  const char* lg = std::getenv("PROM_TC_LG");
  tc_lg_cap = lg ? std::atoi(lg) : INT_MAX;
  const char* parts = std::getenv("PROM_TC_PARTS");
  tc_parts = parts ? std::atoi(parts) : 0;
}

// 3. reads pb's scenarios and the context's tables; leaves tr.terms, dens, mslots, atom_sigma_max, tab_off and the
// counts, and here the scenarios' body positions and Doppler factors and the length of the tabulated densities
void SetState::collect_scenarios() {
  PROM_REQUIRE(pb->n_pr < (1 << 24), "transit: n_pr must be < 2^24");
  tr.terms.clear();
  tr.dens.clear();
  tr.mslots.clear();
  tr.atom_sigma_max.clear();
  tr.tab_off.assign(tr.n_sc, -1);
  bx.resize(tr.n_sc * n_orb);
  by.resize(tr.n_sc * n_orb);
  sh.resize(tr.n_sc * n_orb);
  for (int32_t sc = 0; sc < tr.n_sc; ++sc) {
    const prom_scenario& sn = pb->scenarios[sc];
    PROM_REQUIRE(valid_kind(sn.density.kind), "transit: unknown density kind");
    tr.dens.push_back(to_dev(sn.density));
    PROM_REQUIRE(sn.shift, "transit: scenario shift[] missing");
    if (sn.density.kind == PROM_DENSITY_TABULATED) {
      PROM_REQUIRE(sn.n_tabulated, "transit: tabulated scenario without n_tabulated");
      tr.tab_off[sc] = tab_total;
      tab_total += n_orb * tr.n_pr * tr.n_x;
    } else if (sn.density.kind == PROM_DENSITY_GRIDDED) {
      int64_t gnx, gny, gnz, glen;
      PROM_REQUIRE(sn.n_tabulated && gridded_dims(sn.density, &gnx, &gny, &gnz, &glen),
                   "transit: gridded scenario needs p = {n_gx, n_gy, n_gz} (>= 2 each) and the packed grid");
      tr.tab_off[sc] = tab_total;
      tab_total += glen;
    } else {
      PROM_REQUIRE(sn.body_x && sn.body_y, "transit: scenario body position missing");
    }
    for (int64_t o = 0; o < n_orb; ++o) {
      bx[sc * n_orb + o] = sn.body_x ? sn.body_x[o] : 0.0;
      by[sc * n_orb + o] = sn.body_y ? sn.body_y[o] : 0.0;
      sh[sc * n_orb + o] = sn.shift[o];
    }
    PROM_REQUIRE(sn.n_constituents >= 0 && (sn.n_constituents == 0 || sn.constituents), "transit: constituents");
    for (int32_t k = 0; k < sn.n_constituents; ++k) {
      const prom_constituent& C = sn.constituents[k];
      prom::TermDev t{};
      t.scenario = sc;
      t.is_molecule = C.is_molecule ? 1 : 0;
      t.table = C.table_id;
      t.chi = C.chi;
      if (t.is_molecule) {
        PROM_REQUIRE(table_ok(ctx->mtables, C.table_id), "transit: unknown molecular table id");
        t.slot = n_mol++;
        const prom::MolTable& mt = ctx->mtables[C.table_id];
        prom::MolSlotDev md{};
        md.P = mt.P.as<double>(); md.T = mt.T.as<double>(); md.W = mt.W.as<double>(); md.V = mt.V.as<double>();
        md.n_p = mt.n_p; md.n_t = mt.n_t; md.n_w = mt.n_w;
        md.offset = mt.offset;
        md.fill = std::log10(mt.offset);
        md.temp = sn.T;
        md.chi = C.chi;
        md.scenario = sc;
        tr.mslots.push_back(md);
      } else {
        PROM_REQUIRE(table_ok(ctx->tables, C.table_id), "transit: unknown table id");
        t.slot = n_atoms++;
        const prom::AtomTable& tb = ctx->tables[C.table_id];
        tr.atom_sigma_max.push_back((std::pow(10.0, tb.ymax) - tb.offset) * (1.0 + 1e-9));
      }
      tr.terms.push_back(t);
    }
  }
  tr.n_atoms = n_atoms;
  tr.n_mol = n_mol;
  tr.n_terms = (int32_t)tr.terms.size();
}

// 4. reads pb's grid and chords; leaves them staged for tr.wav, cy, cz, cfout, and the chords' mirror images (for
// k_mol_list's merging of equal molecular records) in tr.mirror_h / n_mirror, staged for tr.mirror
void SetState::pair_chords() {
  stg.add(tr.wav, pb->wavelength, tr.n_wav, s);
  stg.add(tr.cy, pb->chord_y, tr.n_pr, s);
  stg.add(tr.cz, pb->chord_z, tr.n_pr, s);
  stg.add(tr.cfout, pb->chord_fout, tr.n_pr, s);
  tr.mirror_h.assign((size_t)tr.n_pr, -1);
  tr.n_mirror = 0;
  if (mir_on && tr.n_pr <= prom::kMolMirrorMax)
    tr.n_mirror = prom::pair_mirrors(pb->chord_y, pb->chord_z, tr.n_pr, tr.mirror_h);
  stg.add(tr.mirror, tr.mirror_h.data(), tr.n_pr, s);
}

// 4b. reads pb's remaining per-phase arrays, bx / by / sh and tr.terms, atom_sigma_max, mslots; leaves them staged
// and every molecular slot's bilinear records built at its temperature (k_mol_gt into tr.mol_g)
void SetState::stage_inputs() {
  stg.add(tr.x, pb->x, tr.n_x, s);
  stg.add(tr.planet_y, pb->planet_y, n_orb, s);
  stg.add(tr.moon_y, pb->moon_y, (int64_t)tr.n_moons * n_orb, s);
  stg.add(tr.moon_R, pb->moon_R, tr.n_moons, s);
  stg.add(tr.body_x, bx, s);
  stg.add(tr.body_y, by, s);
  stg.add(tr.shift, sh, s);
  stg.add(tr.terms_dev, tr.terms, s);
  stg.add(tr.sigma_max_dev, tr.atom_sigma_max, s);
  // the molecular tables at each slot's temperature, one 32-byte bilinear record per (P interval, lambda'
  // interval) (k_mol_gt: two 16-byte loads per sample in k_tau_mol)
  int64_t g_total = 0;
  for (const auto& md : tr.mslots) g_total += 2 * (int64_t)std::max(md.n_p - 1, 1) * (md.n_w - 1);
  if (g_total > 0) tr.mol_g.ensure(sizeof(double2) * (size_t)g_total);
  int64_t g_off = 0;
  for (auto& md : tr.mslots) {
    md.k_B = pb->k_B > 0.0 ? pb->k_B : 1.381 * std::pow(10.0, -16);
    md.shift = tr.shift.as<double>() + (int64_t)md.scenario * n_orb;
    md.G = tr.mol_g.as<double2>() + g_off;
    g_off += 2 * (int64_t)std::max(md.n_p - 1, 1) * (md.n_w - 1);
    prom::launch_mol_gt(s, md);
  }
  stg.add(tr.molslot, tr.mslots, s);
}

// c = 1 / bound where the bound can normalise a column: {c, 1 / c}, zeros where it cannot; *ok cleared when the bound
// overflows (integrate without windows / without merging)
void norm_of(double bound, double* ncoef, double* nscale, bool* ok) {
  const double c = (bound > 0.0 && std::isfinite(bound)) ? 1.0 / bound : 0.0;
  if (!std::isfinite(bound) || (bound > 0.0 && !(c > 0.0))) *ok = false;
  *ncoef = std::isfinite(c) ? c : 0.0;
  *nscale = (c > 0.0 && std::isfinite(c)) ? bound : 0.0;
}

// 5. reads the scenarios' densities, tr.terms and the tables; leaves the column normalisation (tr.sigtab staged,
// sigtab_v, qbound_v), the species merge (species_merge_ok, sigtab_m, colargs_m.t, sigma_max_m staged, qbound_m), the
// curve switch with its octave cap (tcurve, tc_ybound, tc_lg), uniform_shift, and tr.window narrowed
void SetState::normalise_columns() {
  // per-scenario density bound n_ref (every built-in model peaks at p[0] = n_0 on its domain;
  // tabulated: the largest finite value) -> column normalisation c_s = 1 / (chi_s n_ref n_x dx)
  std::vector<double> nref(tr.n_sc, 0.0);
  auto finite_max = [](const double* v, int64_t i0, int64_t i1) {
    double m = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
      const double a = std::fabs(v[i]);
      if (std::isfinite(a) && a > m) m = a;
    }
    return m;
  };
  for (int32_t sc = 0; sc < tr.n_sc; ++sc) {
    const prom_scenario& sn = pb->scenarios[sc];
    if (sn.density.kind == PROM_DENSITY_TABULATED) {
      nref[sc] = finite_max(sn.n_tabulated, 0, n_orb * tr.n_pr * tr.n_x);
    } else if (sn.density.kind == PROM_DENSITY_GRIDDED) {
      // a trilinear value is a convex combination of corners (weights sum to 1 within rounding)
      int64_t gnx, gny, gnz, glen;
      gridded_dims(sn.density, &gnx, &gny, &gnz, &glen);
      nref[sc] = finite_max(sn.n_tabulated, gnx + gny + gnz, glen) * (1.0 + 1e-9);
    } else {
      // p[0] bounds the built-in profile only where it decays away from its body
      if (!prom::density_bounded(sn.density.kind, sn.density.p)) tr.window = false;
      nref[sc] = std::fabs(sn.density.p[0]) * (1.0 + 1e-9);
    }
  }
  for (const auto& t : tr.terms)   // negative mixing ratios give negative columns: no envelopes
    if (!t.is_molecule && !(t.chi >= 0.0)) tr.window = false;
  std::vector<prom::SigTabDev> st;
  for (const auto& t : tr.terms) {
    if (t.is_molecule) continue;
    const prom::AtomTable& tb = ctx->tables[t.table];
    // an overflowing bound cannot normalise the columns: integrate without windows
    double c, inv;
    norm_of(std::fabs(t.chi) * nref[t.scenario] * (double)tr.n_x * tr.delta_x, &c, &inv, &tr.window);
    st.push_back({tb.x.as<double>(), tb.y.as<double>(), tb.n, tb.offset,
                  tr.shift.as<double>() + (int64_t)t.scenario * n_orb, tb.dir.as<int32_t>(), tb.n_dir, 0,
                  tb.dir_x0, tb.dir_inv_h, c, inv, t.chi, tb.hx.front(), tb.hx.back(), tb.rec.as<double4>()});
  }
  // species merging: one scenario carries every atomic constituent (and there are >= 2 of them)
  int32_t sc0 = -1;
  bool one_sc = n_atoms >= 2 && n_mol == 0;
  double smax_m = 0.0;
  for (const auto& t : tr.terms) {
    if (t.is_molecule) continue;
    if (sc0 < 0) sc0 = t.scenario;
    if (t.scenario != sc0 || !(std::isfinite(t.chi) && t.chi >= 0.0)) one_sc = false;
    smax_m += t.chi * tr.atom_sigma_max[t.slot];
  }
  tr.species_merge_ok = tr.species_merge_ok && one_sc && tr.n_sc <= 4;
  if (tr.species_merge_ok) {
    tr.sigtab_m = prom::SigTabs4{};
    tr.sigtab_m.t[0] = st[0];
    norm_of(nref[sc0] * (double)tr.n_x * tr.delta_x, &tr.sigtab_m.t[0].ncoef, &tr.sigtab_m.t[0].nscale,
            &tr.species_merge_ok);
    if (!std::isfinite(smax_m)) tr.species_merge_ok = false;
    tr.sigtab_m.t[0].chi = 1.0;
    tr.colargs_m = prom::ColArgs{};
    prom::TermDev tm{};
    tm.scenario = sc0;
    tm.is_molecule = 0;
    tm.slot = 0;
    tm.table = -1;
    tm.chi = 1.0;
    tr.colargs_m.t[0] = tm;
    stg.add(tr.sigma_max_m, &smax_m, 1, s);
    tr.qbound_m = smax_m * tr.sigtab_m.t[0].nscale;
  }
  stg.add(tr.sigtab, st, s);
  tr.qbound_v = 0.0;
  for (size_t i = 0; i < st.size(); ++i) tr.qbound_v += tr.atom_sigma_max[i] * st[i].nscale;
  // transmission curves (prom_tcurve.hip): one effective absorber on the fast column path, windows allowed
  // (PROM_OPT_NO_WINDOW / OCML_EXP keep the exact validation paths), no stellar spectrum (tr.star is assigned later)
  tr.tcurve = tr.tcurve && prom::cols8_path(tr) && tr.exp_mode && tr.window && !pb->has_star && n_atoms >= 1 &&
              (n_atoms == 1 || tr.species_merge_ok);
  // Y bound (merged: sum_s chi_s sigma_max_s; one species: sigma_max) and the octave cap of the tables:
  // q = Y N_max <= Y_bound * (the column bound 1 / c), one octave of margin
  const double yb = !tr.tcurve ? 0.0 : (n_atoms == 1 ? tr.atom_sigma_max[0] : smax_m);
  const double nb = !tr.tcurve ? 0.0 : (n_atoms == 1 ? st[0].nscale : tr.sigtab_m.t[0].nscale);
  tr.tc_ybound = (std::isfinite(yb) && yb > 0.0) ? yb : 0.0;
  const double qb = yb * nb;
  int lg = prom::kTcMaxOctaves;
  if (std::isfinite(qb) && qb > 0.0) lg = std::max(1, std::min(prom::kTcMaxOctaves, std::ilogb(qb) + 7 + 2));
  tr.tc_lg = std::max(1, std::min(lg, tc_lg_cap));
  // PROM_OPT_DOPPLER_ROWS: one sigma row per phase even when the factors are equal (a phase shard of a
  // problem with orbital Doppler shift takes the full problem's sigma path: bitwise equal rows)
  tr.uniform_shift = !(pb->options & PROM_OPT_DOPPLER_ROWS);
  for (const auto& t : tr.terms) {
    if (t.is_molecule) continue;
    for (int64_t o = 1; o < n_orb; ++o)
      if (!(sh[t.scenario * n_orb + o] == sh[t.scenario * n_orb])) tr.uniform_shift = false;
  }
  tr.sigtab_v = prom::SigTabs4{};
  for (size_t i = 0; i < st.size() && i < 4; ++i) tr.sigtab_v.t[i] = st[i];
}

// 6b. target windows (k_sigma_tw, prom_window.hip): every atomic slot on one set of Doppler factors (one scenario),
// n_orb >= 2; built with the sigma segments (the same inputs) and kept when they are reused.  Reads the grid, the
// tables' nodes and sh; leaves tr.tw_seg, tw_row, tw_stage staged and n_tw, tw_ok, tw_new.  The default: C4x10
// k_sigma_tw 47-48 us against k_sigma_tc's 60, pipelined step 0.062 against 0.065 ms; C3 (three merged species)
// steps 0.0366-0.0374 against 0.0370-0.0384 ms on the same boxes, reads 46 against 79 MB per launch, though
// 36-37 against 32 us isolated (profiles/r06t_*, r06u_*)
void SetState::target_windows() {
  tr.tw_ok = false;
  tr.n_tw = 0;
  std::vector<const std::vector<double>*> tabs;
  int32_t sc_tw = -1;
  bool one = n_orb >= 2;
  for (const auto& t : tr.terms) {
    if (t.is_molecule) continue;
    if (sc_tw < 0) sc_tw = t.scenario;
    for (int64_t o = 0; o < n_orb; ++o)
      if (!(sh[t.scenario * n_orb + o] == sh[sc_tw * n_orb + o])) one = false;
    tabs.push_back(&ctx->tables[t.table].hx);
  }
  if (!one || sc_tw < 0 || tw_off) return;
  // (profiling knobs, read once: wavelengths per row, points per window, LDS doubles per workgroup).  The point
  // cap scales with the rows: a window's wavelengths span its rows' Doppler spread (C4x10: ~600) on top of a row's
  // own, so many-phase windows of 64 wavelengths a row spend most of their staging there -- C4x10p128 1.07 ms per
  // step at 8,192 points, 0.67 ms at 32,768 (128 rows x 256), C4x10p64 0.40 / 0.34 ms (profiles/r06w_*)
  // wavelengths per row: 256, and up to 768 for few rows (a window's staging then serves more points): C4x10
  // (8 rows) 0.0605-0.0613 ms per step at 256, 0.0563-0.0575 at 512, 0.0544 at 768; C4 0.0118 / 0.0111-0.0113;
  // C4x10p64 (64 rows) 0.343 at 256, 0.366 at 512; C3 unchanged (its windows end at the LDS budget)
  static const int rowcap_env = [] { const char* e = std::getenv("PROM_TW_ROWCAP"); return e ? std::max(1, std::atoi(e)) : 0; }();
  const int rowcap = rowcap_env > 0 ? rowcap_env : std::max(256, std::min(768, (int)(4096 / std::max<int64_t>(1, n_orb)) / 64 * 64));
  static const int64_t pmax_env = [] { const char* e = std::getenv("PROM_TW_PMAX"); return e ? (int64_t)std::max(1, std::atoi(e)) : (int64_t)0; }();
  const int64_t pmax = pmax_env > 0 ? pmax_env : std::max<int64_t>(8192, (int64_t)rowcap * n_orb);
  static const int lamcap = [] {   // (wavelengths staged per window at most; 0: never)
    const char* e = std::getenv("PROM_TW_LAMCAP");
    return e ? std::max(0, std::min(prom::kTwLamCap, std::atoi(e))) : prom::kTwLamCap;
  }();
  static const int lds = [] {
    const char* e = std::getenv("PROM_TW_LDS");
    return e ? std::max(16, std::min(prom::kTwLds, std::atoi(e))) : prom::kTwLds;
  }();
  std::vector<prom::SigSeg> twseg;
  std::vector<int32_t> twrow, twlam;
  int32_t nw = 0;
  if (!prom::build_target_windows(pb->wavelength, tr.n_wav, sh.data() + (int64_t)sc_tw * n_orb, (int32_t)n_orb, tabs,
                                  lds, lamcap, rowcap, pmax, twseg, twrow, twlam, nw))
    return;
  stg.add(tr.tw_seg, twseg, s);
  stg.add(tr.tw_row, twrow, s);
  // the windows' stage records (tw_stage.h), from the finished plan; k_tw_exact marks them with the slices
  std::vector<prom::TwStage> twstg((size_t)nw);
  for (int32_t b = 0; b < nw; ++b)
    twstg[b] = prom::tw_stage_of(twseg.data() + (int64_t)b * (int64_t)tabs.size(), (int32_t)tabs.size(), twlam[2 * b],
                                 twlam[2 * b + 1]);
  stg.add(tr.tw_stage, twstg, s);
  tr.n_tw = nw;
  tr.tw_ok = true;
  tr.tw_new = true;
  if (debug) {
    int64_t k[4] = {0, 0, 0, 0};
    for (const auto& e : twseg) k[e.kind & 3] += 1;
    int64_t lam_st = 0, lam_n = 0;   // windows whose wavelengths are staged; their wavelengths
    for (int32_t b = 0; b < nw; ++b)
      if (twlam[2 * b + 1] > twlam[2 * b]) {
        ++lam_st;
        lam_n += twlam[2 * b + 1] - twlam[2 * b];
      }
    std::fprintf(stderr, "[prom] target windows: %d (slices: %lld staged, %lld global, %lld staged unguessed, "
                 "%lld outside the table; wavelengths staged in %lld windows, %.1f per window)\n", nw,
                 (long long)k[1], (long long)k[2], (long long)k[3], (long long)k[0], (long long)lam_st,
                 lam_st ? (double)lam_n / (double)lam_st : 0.0);
  }
}

// 6. sigma segments of the Doppler rows (every path with resampled rows reads them, with or without orbital Doppler
// shift).  Reads the grid, the atomic tables' nodes and generations and sh; leaves tr.sig_seg, sig_seg4, sig_dir,
// sig_fb, sig_fb_tc staged with their counts and sig_seg_ok -- or the last set's, when its key matches -- the target
// windows, tr.seg_key_valid cleared and this set's key here
void SetState::sigma_segments() {
  tr.sig_seg_ok = false;
  std::vector<double> key_sh;
  std::vector<uint64_t> key_gen;
  std::vector<const std::vector<double>*> tabs;
  std::vector<const double*> shifts;
  for (const auto& t : tr.terms) {
    if (t.is_molecule) continue;
    key_gen.push_back(ctx->tables[t.table].gen);
    key_sh.insert(key_sh.end(), sh.begin() + t.scenario * n_orb, sh.begin() + (t.scenario + 1) * n_orb);
    tabs.push_back(&ctx->tables[t.table].hx);
    shifts.push_back(sh.data() + t.scenario * n_orb);
  }
  const bool seg_reuse = !no_guess && use_dir && tr.seg_key_valid && key_gen == tr.seg_key_gen &&
                         key_sh == tr.seg_key_sh && (int64_t)tr.seg_key_wav.size() == tr.n_wav &&
                         std::memcmp(tr.seg_key_wav.data(), pb->wavelength, sizeof(double) * tr.n_wav) == 0;
  // reused segments stay valid only if this set completes; a throw below must not leave the key
  // pointing at buffers a later (failed) set may have reallocated
  tr.seg_key_valid = false;
  seg_key_keep = seg_reuse;   // the stored key stays as it is (re-validated at the end)
  if (seg_reuse) {
    tr.sig_seg_ok = true;
    if (tw_off) tr.tw_ok = false;
    else if (!tr.tw_ok) target_windows();
    return;
  }
  tr.tw_ok = false;
  prom::SigmaSegments g;
  if (!prom::build_sigma_segments(pb->wavelength, tr.n_wav, tabs, shifts, n_orb, use_dir, no_guess, g)) return;
  tr.sig_noguess = g.noguess;
  stg.add(tr.sig_seg, g.seg, s);
  stg.add(tr.sig_seg4, g.seg4, s);
  stg.add(tr.sig_dir, g.sdir, s);
  if (debug) std::fprintf(stderr, "[prom] bucket directories: %zu, %zu buckets\n", (size_t)g.n_dir, g.sdir.size());
  tr.n_sig_fb = (int32_t)g.fb.size();
  tr.n_sig_fb_tc = (int32_t)g.fb_tc.size();
  if (g.fb.empty()) g.fb.push_back(0);
  if (g.fb_tc.empty()) g.fb_tc.push_back(0);
  stg.add(tr.sig_fb, g.fb, s);
  stg.add(tr.sig_fb_tc, g.fb_tc, s);
  tr.sig_seg_ok = true;
  target_windows();
  // the key is committed only after the segments have reached the device (end of the call):
  // a set that throws later must not leave a key that a retry would reuse (validation segments never)
  seg_key_new = !no_guess && use_dir;
  new_key_sh = std::move(key_sh);
  new_key_gen = std::move(key_gen);
}

// 7. reads the atomic tables' amax; leaves tr.sig_deg (0: exp10 rows; PROM_SIG_POLY=0 and PROM_SIGMA_ROWS=0 force it)
void SetState::poly_degree() {
  std::vector<double> amax;
  for (const auto& t : tr.terms)
    if (!t.is_molecule) amax.push_back(ctx->tables[t.table].amax);
  tr.sig_deg = prom::sigma_poly_degree(amax.data(), (int32_t)amax.size(), sig_poly && !no_guess);
}

// 8. reads pb's stellar arrays and the star table; leaves tr.star, star_table_id and, with a star, star_tab,
// star_uniform, the chord arrays staged for crho / cclv / cshift and the tiles' node slices for rm_slices
void SetState::stellar_setup() {
  tr.star = pb->has_star != 0;
  tr.star_table_id = tr.star ? pb->star_table : -1;
  if (!tr.star) return;
  PROM_REQUIRE(pb->chord_rho && pb->chord_clv && pb->chord_star_shift, "transit: stellar chord arrays missing");
  PROM_REQUIRE(table_ok(ctx->tables, pb->star_table), "transit: unknown star table id");
  PROM_REQUIRE(n_mol == 0 && n_atoms <= 8,
               "transit: the stellar-spectrum path takes <= 8 atomic constituents and no molecules");
  const prom::AtomTable& sb = ctx->tables[pb->star_table];
  PROM_REQUIRE(sb.offset == 0.0, "transit: the star table must have offset 0 (n_interp_log(..., 0.0))");
  tr.star_tab = prom::SigTabDev{sb.x.as<double>(), sb.y.as<double>(), sb.n, sb.offset, nullptr,
                                sb.dir.as<int32_t>(), sb.n_dir, 0, sb.dir_x0, sb.dir_inv_h, 0.0, 0.0, 0.0,
                                sb.hx.front(), sb.hx.back(), sb.rec.as<double4>()};
  stg.add(tr.crho, pb->chord_rho, tr.n_pr, s);
  stg.add(tr.cclv, pb->chord_clv, tr.n_pr, s);
  stg.add(tr.cshift, pb->chord_star_shift, tr.n_pr, s);
  double smin, smax;
  if (!prom::factor_range(pb->chord_star_shift, tr.n_pr, smin, smax)) smin = smax = std::nan("");   // no slices
  tr.star_uniform = true;
  for (int32_t i = 1; i < tr.n_pr; ++i)
    if (!(pb->chord_star_shift[i] == pb->chord_star_shift[0])) tr.star_uniform = false;
  stg.add(tr.rm_slices, prom::star_slices(pb->wavelength, tr.n_wav, sb.hx, smin, smax), s);
}

// 9. reads tr.dens, tab_off and the scenarios' tabulated densities; leaves them copied into tr.tab, tr.scdev staged
// and the by-value kernel arguments tr.colargs (terms, scenarios) and colargs_m.sc
void SetState::density_tables() {
  tr.tab.ensure(sizeof(double) * std::max<int64_t>(tab_total, 1));
  std::vector<prom::ScDevHost> sd(tr.n_sc);
  for (int32_t sc = 0; sc < tr.n_sc; ++sc) {
    sd[sc].m = tr.dens[sc];
    sd[sc].tab = tr.tab_off[sc] >= 0 ? tr.tab.as<double>() + tr.tab_off[sc] : nullptr;
  }
  stg.add(tr.scdev, sd, s);
  tr.colargs = prom::ColArgs{};
  for (int32_t i = 0; i < tr.n_sc && i < 4; ++i) tr.colargs.sc[i] = tr.colargs_m.sc[i] = sd[i];
  for (int32_t i = 0; i < tr.n_terms && i < 8; ++i) tr.colargs.t[i] = tr.terms[i];
  for (int32_t sc = 0; sc < tr.n_sc; ++sc)
    if (tr.tab_off[sc] >= 0) {
      int64_t len = n_orb * tr.n_pr * tr.n_x, gnx, gny, gnz;
      if (pb->scenarios[sc].density.kind == PROM_DENSITY_GRIDDED)
        gridded_dims(pb->scenarios[sc].density, &gnx, &gny, &gnz, &len);
      PROM_HIP(hipMemcpyAsync(tr.tab.as<double>() + tr.tab_off[sc], pb->scenarios[sc].n_tabulated,
                              sizeof(double) * len, hipMemcpyHostToDevice, s));
    }
}

// 10. reads the sizes and the routes (cols8_path, fast_path, tr.tcurve); leaves tr.depth and every slot's work
// buffers sized, and with the curves tr.tc_parts, tc_fsum and the constants of k_tc_build
void SetState::slot_buffers() {
  const int64_t nc = n_orb * tr.n_pr;
  // pipelining needs every per-run buffer in the slot (n(c, x), the molecular samples and lists are); the
  // fast atomic paths and the molecular path run pipelined, the generic atomic column path (k_ntot +
  // k_columns) and the stellar-spectrum path one slot
  const bool cols8 = prom::cols8_path(tr);
  const bool mol_pipe = n_mol > 0 && !tr.star;
  tr.depth = (prom::fast_path(tr) || mol_pipe) ? ctx->pipeline : 1;
  for (int si = 0; si < tr.depth; ++si) {
    prom::RunSlot& rs = tr.slot[si];
    if (!cols8) rs.ntot.ensure(sizeof(double) * tr.n_sc * nc * tr.n_x);
    rs.ncol.ensure(sizeof(double) * std::max<int64_t>(n_atoms, 1) * nc);
    rs.molcol.ensure(sizeof(double) * std::max<int64_t>(n_mol, 1) * nc);
    if (n_mol > 0) {
      rs.mol_smp.ensure(sizeof(double) * 4 * n_mol * nc * tr.n_x);
      rs.mol_nin.ensure(sizeof(int32_t) * n_mol * nc);
      rs.mol_lst.ensure(sizeof(double) * 4 * ((n_mol * tr.n_x + 1) * nc + (int64_t)prom::kMolListPad * n_orb));
      rs.mol_rend.ensure(sizeof(int32_t) * nc);
    }
    rs.flags.ensure(sizeof(int32_t) * nc);
    rs.recs.ensure(sizeof(double) * nc * (1 + n_atoms));
    rs.act_ip.ensure(sizeof(int32_t) * nc);
    rs.counts.ensure(sizeof(int32_t) * n_orb * prom::kCnt);
    rs.mrecs.ensure(sizeof(double) * nc * (1 + n_atoms));
    if (n_atoms >= 1 && n_atoms <= prom::kWinMaxSpecies && n_mol == 0) {
      rs.wenv.ensure(sizeof(int32_t) * n_orb * 2 * prom::kEnvN);
      rs.wmom.ensure(sizeof(double) * n_orb * (tr.n_pr + 1) *
                     std::max(prom::n_tail_moments(n_atoms), prom::n_tail_moments(1)));   // merged species: 1
    }
    rs.evals.ensure(sizeof(unsigned long long) * 64);
    // resampled cross-sections: one row per phase when the Doppler factors differ between phases
    const int64_t sig_rows = tr.uniform_shift ? 1 : n_orb;
    rs.sig.ensure(sizeof(double) * sig_rows * std::max<int64_t>(n_atoms, 1) * tr.n_wav);
    rs.zfl.ensure((size_t)(sig_rows * tr.n_wav));
    const int64_t n_wtiles = (tr.n_wav + 127) / 128;
    rs.tq.ensure(sizeof(float) * 4 * sig_rows * n_wtiles);
    rs.hlist.ensure(sizeof(int32_t) * 4 * 2 * n_orb * 2 * n_wtiles);   // small and big lists, <= 1 per half tile
    rs.hcnt.ensure(sizeof(int32_t) * 4);
    rs.trec.ensure(sizeof(int32_t) * 4 * n_orb * n_wtiles);   // {h, t, flags, 0} per (phase, tile)
    tr.taup_resident = 0;
    rs.tsum.ensure(sizeof(double) * n_orb);
    rs.fsum.ensure(sizeof(double) * n_orb);
    rs.R.ensure(sizeof(double) * n_orb * tr.n_wav);
    if (!tr.tcurve) continue;
    // k_tc_build: ~300 chords per part (C3: 8 parts; profiles/r04h_tc_build_parts.txt), at most kTcPartMax
    // parts; one part needs no hand-off between workgroups; PROM_TC_PARTS (profiling) overrides
    tr.tc_parts = (int32_t)std::max<int64_t>(1, std::min<int64_t>(prom::kTcPartMax, (tr.n_pr + 299) / 300));
    if (tc_parts > 0) tr.tc_parts = std::min(prom::kTcPartMax, tc_parts);
    // the chords' F_out total (the disk sum's denominator, the same for every phase), accumulated in long double
    // and rounded once: a float64 sum in chord order was 12 u off at 16,416 chords, which every R of the phase
    // carried (tests/test_gpu_tc_sweep.py, the tail at n_pr = 16,416)
    long double fsum = 0.0L;
    for (int32_t i = 0; i < tr.n_pr; ++i) fsum += (long double)pb->chord_fout[i];
    tr.tc_fsum = (double)fsum;
    if (!tr.tc_const.p) {
      // c_k = sum_j f_j cm[k][j] at the nodes u_j = cos(pi (j + 1/2) / 16); node factors 2^((u_k + 1) / 2)
      std::vector<double> cc(prom::kTcD * prom::kTcD + prom::kTcD);
      for (int k = 0; k < prom::kTcD; ++k)
        for (int j = 0; j < prom::kTcD; ++j)
          cc[k * prom::kTcD + j] = std::cos(M_PI * (double)k * ((double)j + 0.5) / (double)prom::kTcD) *
                                   ((k == 0 ? 1.0 : 2.0) / (double)prom::kTcD);
      for (int k = 0; k < prom::kTcD; ++k)
        cc[prom::kTcD * prom::kTcD + k] = std::exp2(0.5 * (std::cos(M_PI * ((double)k + 0.5) / (double)prom::kTcD) + 1.0));
      tr.tc_const.ensure(sizeof(double) * cc.size());
      PROM_HIP(hipMemcpy(tr.tc_const.p, cc.data(), sizeof(double) * cc.size(), hipMemcpyHostToDevice));
    }
    const int64_t n_ch = (tr.tc_lg + prom::kTcChain - 1) / prom::kTcChain;
    rs.tc_hdr.ensure(sizeof(double) * n_orb * prom::kTcHdr);
    rs.tc_tab.ensure(sizeof(double) * n_orb * tr.tc_lg * prom::kTcD);
    rs.tc_part.ensure(sizeof(double) * n_orb * n_ch * prom::kTcPartMax * prom::kTcPartVals);
    const size_t cb = sizeof(int32_t) * n_orb * n_ch;
    if (rs.tc_cnt.cap < cb) {
      rs.tc_cnt.ensure(cb);
      PROM_HIP(hipMemsetAsync(rs.tc_cnt.p, 0, rs.tc_cnt.cap, s));
    }
    rs.tc_pp.ensure(sizeof(prom::TcPart) * (size_t)std::max<int64_t>(1, n_orb * (tr.n_pr / 32)));
  }
  tr.last = 0;
}

// 11. reads everything staged; leaves it on the device, the per-set kernels run (k_rm_fout, the exact marks of new
// windows and segments), the PROM_DEBUG lines written, the stream idle and then the segment key committed
void SetState::finish_set() {
  stg.flush(ctx, s);
  if (tr.star) prom::launch_rm_fout(s, tr);   // per set: the unocculted flux of every wavelength
  if (tr.tw_new) {
    // windows built by this call: mark the slices whose guess is numpy's bracket at every target
    if (tw_exact) prom::launch_tw_exact(s, tr, n_atoms);
    tr.tw_new = false;
  }
  if (seg_key_new) {
    // segments built by this call: mark those whose guess is numpy's bracket for every target
    const int64_t nb = (tr.n_wav + prom::kSigBlockW - 1) / prom::kSigBlockW;
    tr.sig_flags.ensure(sizeof(int32_t) * nb * n_atoms);
    prom::launch_seg_exact(s, n_atoms, tr.sigtab_v, tr.wav.as<double>(), tr.n_wav, (int32_t)n_orb,
                           tr.sig_seg.as<prom::SigSeg>(), tr.sig_flags.as<int32_t>());
    if (debug) {
      std::vector<prom::SigSeg> hs(nb * n_atoms);
      PROM_HIP(hipMemcpyAsync(hs.data(), tr.sig_seg.p, sizeof(prom::SigSeg) * hs.size(), hipMemcpyDeviceToHost, s));
      PROM_HIP(hipStreamSynchronize(s));
      int64_t cnt[8] = {};
      for (const auto& e : hs) ++cnt[e.kind & 7];
      std::fprintf(stderr, "[prom] sigma segments: %lld blocks x %d species, %d oversize blocks (%d for k_sigma_tc), kinds: "
                   "none %lld, lds %lld, global %lld, lds exact %lld, global exact %lld; poly degree %d\n", (long long)nb,
                   n_atoms, tr.n_sig_fb, tr.n_sig_fb_tc, (long long)cnt[0], (long long)cnt[1], (long long)cnt[2],
                   (long long)cnt[5], (long long)cnt[6], tr.sig_deg);
    }
  }
  if (debug) {
    const prom::ColPlan cp = prom::col_plan(tr);
    std::fprintf(stderr, "[prom] column chain: transmission curves %d, phase partials %d, column kernel kind %d "
                 "(0: generic)\n", cp.tcp ? 1 : 0, cp.partials ? 1 : 0, cp.kind);
  }
  PROM_HIP(hipStreamSynchronize(s));
  if (seg_key_new) {
    tr.seg_key_wav.assign(pb->wavelength, pb->wavelength + tr.n_wav);
    tr.seg_key_sh = std::move(new_key_sh);
    tr.seg_key_gen = std::move(new_key_gen);
  }
  tr.seg_key_valid = seg_key_new || seg_key_keep;
}

}  // namespace

extern "C" {

int32_t prom_transit_set(prom_ctx* ctx, const prom_transit_problem* pb) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(pb, "prom_transit_set: null problem");
    ctx->tr.ready = false;
    ctx->tr.ran = false;
    ctx->br.current = false;   // R_b belongs to the run it was formed from
    SetState S{ctx, pb, ctx->tr, ctx->stream};
    check_request(pb);
    S.read_options();
    S.collect_scenarios();
    S.pair_chords();
    S.stage_inputs();
    S.normalise_columns();
    S.sigma_segments();
    S.poly_degree();
    S.stellar_setup();
    S.density_tables();
    S.slot_buffers();
    S.finish_set();
    ctx->tr.ready = true;
  });
}

int32_t prom_transit_run(prom_ctx* ctx, prom_transit_stats* stats) {
  return guarded(ctx, [&] {
    prom::TransitDev& tr = ctx->tr;
    if (!tr.ready) throw Error(PROM_E_STATE, "prom_transit_run: call prom_transit_set first");
    int variant = 0;
    hipEvent_t* ev = ctx->ev;
    const bool timed = ctx->timing && (ctx->window_runs++ % ctx->timing_stride) == 0;
    if (timed) {
      const size_t need = 4 * (size_t)(ctx->timed_runs + 1);
      while (ctx->tev.size() < need) {
        hipEvent_t e;
        PROM_HIP(hipEventCreate(&e));
        ctx->tev.push_back(e);
      }
      ev = &ctx->tev[4 * (size_t)ctx->timed_runs];
      constexpr int32_t kTsCap = 8192;   // workgroups a tau launch may stamp
      if (ctx->tsbuf.size() <= (size_t)ctx->timed_runs) {
        ctx->tsbuf.emplace_back();
        ctx->tsbuf.back().ensure(sizeof(unsigned long long) * 2 * kTsCap);
      }
      if (ctx->ts_blocks.size() <= (size_t)ctx->timed_runs) ctx->ts_blocks.resize(ctx->timed_runs + 1);
      ctx->tr.ts_out = ctx->tsbuf[ctx->timed_runs].as<unsigned long long>();
      ctx->tr.ts_cap = kTsCap;
      ctx->tr.ts_blocks = 0;
      ++ctx->timed_runs;
    }
    tr.count_evals = stats != nullptr;
    // pipelined problems alternate slots and streams: this run's column / ordering kernels overlap the
    // previous run's tau kernel; a slot is reused two runs later, after its stream's previous run
    const int si = (tr.last + 1) % tr.depth;
    const hipStream_t st = ctx->streams[si];
    prom::RunSlot& rs = tr.slot[si];
    // the slot's second stream: the one `depth` away (free when depth <= kMaxSlots / 2).  The fork shortens
    // one run (sigma rows beside k_columns8 / k_order) but costs pipelined throughput (C4 7.3e10 -> 3.8e10
    // pts/s, C3 unchanged: profiles/r02w_pipeline_sweep.txt), so it is the default for unpipelined
    // problems only; PROM_SIGMA_FORK=0/1 forces it off/on
    const bool fork_ok = tr.depth <= prom::kMaxSlots / 2 && (tr.env_fork >= 0 ? tr.env_fork != 0 : tr.depth == 1);
    rs.aux = fork_ok ? ctx->streams[si + tr.depth] : nullptr;
    rs.ev_fork = fork_ok ? ctx->fork_ev[si] : nullptr;
    rs.ev_join = fork_ok ? ctx->join_ev[si] : nullptr;
    // staggered kernel order on alternate slots (PROM_SIG_STAGGER=1): odd slots queue the Doppler sigma
    // rows after k_order, so their latency-bound ordering overlaps the even slots' full-chip kernels
    rs.sig_late = tr.depth > 1 && (si & 1) && tr.env_stagger;
    if (stats) PROM_HIP(hipMemsetAsync(rs.evals.p, 0, sizeof(unsigned long long) * 64, st));
    if (!stats && !timed && tr.graphs && tr.depth > 1) {
      // untimed fast-path run: replay the slot's graph (captured here the first time)
      if (!tr.gexec[si]) {
        hipGraph_t g = nullptr;
        PROM_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        try {
          prom::launch_transit(st, tr, rs, ctx->tables, ctx->mtables, nullptr, &variant, false);
        } catch (...) {
          (void)hipStreamEndCapture(st, &g);
          if (g) (void)hipGraphDestroy(g);
          throw;
        }
        PROM_HIP(hipStreamEndCapture(st, &g));
        const hipError_t ie = hipGraphInstantiate(&tr.gexec[si], g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        PROM_HIP(ie);
      }
      PROM_HIP(hipGraphLaunch(tr.gexec[si], st));
    } else {
      prom::launch_transit(st, tr, rs, ctx->tables, ctx->mtables, (stats || timed) ? ev : nullptr, &variant,
                           stats != nullptr);
    }
    tr.last = si;
    tr.count_evals = false;
    if (timed) ctx->ts_blocks[ctx->timed_runs - 1] = tr.ts_blocks;
    tr.ts_out = nullptr;
    tr.ts_blocks = 0;

    tr.ran = true;
    ctx->br.current = false;   // the transit observe calls read this run's R until prom_transit_broaden is called again
    if (stats) {
      std::memset(stats, 0, sizeof(*stats));
      PROM_HIP(hipEventSynchronize(ev[3]));
      float a = 0, b = 0, c = 0, t = 0;
      PROM_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
      PROM_HIP(hipEventElapsedTime(&b, ev[1], ev[2]));
      PROM_HIP(hipEventElapsedTime(&c, ev[2], ev[3]));
      PROM_HIP(hipEventElapsedTime(&t, ev[0], ev[3]));
      stats->ms_density = a;
      stats->ms_sigma = b;
      stats->ms_tau = c;
      stats->ms_total = t;
      const int K = prom::kCnt;
      std::vector<int32_t> cnt(tr.n_orb * K);
      download(cnt.data(), rs.counts, (int64_t)cnt.size(), st);
      unsigned long long ev64[64];
      download(ev64, rs.evals, 64, st);
      PROM_HIP(hipStreamSynchronize(st));
      int64_t unwindowed = 0, counted = 0;
      for (int32_t o = 0; o < tr.n_orb; ++o) {
        const bool sorted = cnt[o * K + 5] != 0;
        const bool exact = cnt[o * K + 3] != 0;
        const int64_t recs = sorted ? cnt[o * K + 4] : cnt[o * K];
        stats->active_chords += cnt[o * K];
        stats->transparent_chords += cnt[o * K + 1];
        stats->blocked_chords += cnt[o * K + 2];
        stats->tau_records += recs;
        if (exact) stats->tau_kernel_variant_exact_phases += 1;
        // the device counters cover the non-exact phases of the atomic fast kernel
        if (exact || tr.n_mol > 0 || !tr.exp_mode || tr.n_atoms > prom::kWinMaxSpecies || tr.star) unwindowed += recs;
      }
      for (int i = 0; i < 64; ++i) counted += (int64_t)ev64[i];
      if (std::getenv("PROM_DEBUG") && rs.trec.p && rs.hcnt.p && rs.tq.p) {
        const int64_t n_wtiles = (tr.n_wav + 127) / 128;
        std::vector<int32_t> trv(4 * tr.n_orb * n_wtiles), hc(4);
        std::vector<float> tqv(4 * n_wtiles * tr.n_orb);
        download(trv.data(), rs.trec, (int64_t)trv.size(), st);
        download(hc.data(), rs.hcnt, 4, st);
        download(tqv.data(), rs.tq, (int64_t)tqv.size(), st);
        PROM_HIP(hipStreamSynchronize(st));
        long long win = 0, fl = 0;
        double tqs = 0.0;
        for (int64_t i = 0; i < tr.n_orb * n_wtiles; ++i) { win += trv[4 * i + 1] - trv[4 * i]; fl += trv[4 * i + 2]; }
        for (float v : tqv) tqs += v;
        std::fprintf(stderr, "prom: windows sum %lld flags sum %lld heavy small %d big %d tq sum %.9g\n", win, fl, hc[0],
                     hc[1], tqs);
        // heavy entries' record counts: small list, then big list (hcap = n_orb * 2 * n_tiles entries each)
        const int64_t hcap = (int64_t)tr.n_orb * 2 * n_wtiles;
        for (int b = 0; b < 2; ++b) {
          const int32_t ne = hc[b];
          if (ne <= 0 || !rs.hlist.p) continue;
          std::vector<int32_t> hl(4 * (size_t)ne);
          PROM_HIP(hipMemcpy(hl.data(), rs.hlist.as<int32_t>() + 4 * (b ? hcap : 0), sizeof(int32_t) * hl.size(),
                             hipMemcpyDeviceToHost));
          long long sum = 0;
          int32_t mx = 0;
          std::vector<int32_t> hist(8, 0);   // records: <=64, <=128, <=256, <=512, <=1024, <=2048, <=4096, more
          for (int32_t i = 0; i < ne; ++i) {
            const int32_t n = hl[4 * i + 2] - hl[4 * i + 1];
            sum += n;
            mx = std::max(mx, n);
            int k = 0;
            while (k < 7 && n > (64 << k)) ++k;
            ++hist[k];
          }
          std::fprintf(stderr, "prom: %s entries %d records sum %lld max %d  hist(<=64,128,..,4096,more) %d %d %d %d %d %d %d %d\n",
                       b ? "big" : "small", ne, sum, mx, hist[0], hist[1], hist[2], hist[3], hist[4], hist[5], hist[6],
                       hist[7]);
        }
      }
      if (std::getenv("PROM_DEBUG"))
        for (int32_t o = 0; o < tr.n_orb; ++o)
          std::fprintf(stderr, "prom: phase %d active %d records %d candidates %d sort %d largest slot %d\n", o,
                       cnt[o * K], cnt[o * K + 4], cnt[o * K + 7] & 8191, (cnt[o * K + 7] >> 13) & 3,
                       cnt[o * K + 7] >> 16);
      stats->chord_lambda_evals = stats->active_chords * tr.n_wav;
      stats->exp_evals = counted + unwindowed * tr.n_wav;
      stats->tau_kernel_variant = variant;
    }
  });
}

int32_t prom_transit_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out) {
  return guarded(ctx, [&] {
    prom::TransitDev& tr = ctx->tr;
    if (!tr.ready) throw Error(PROM_E_STATE, "prom_transit_kernel_ms: call prom_transit_set first");
    PROM_REQUIRE(n_runs >= 1 && ms_out, "prom_transit_kernel_ms: bad arguments");
    for (auto st : ctx->streams) PROM_HIP(hipStreamSynchronize(st));
    std::vector<hipEvent_t> ev(2 * PROM_K_COUNT);
    for (auto& e : ev) PROM_HIP(hipEventCreate(&e));
    std::vector<double> sum(PROM_K_COUNT, 0.0);
    std::vector<int32_t> cnt(PROM_K_COUNT, 0);
    const hipStream_t st = ctx->streams[0];
    prom::RunSlot& rs = tr.slot[0];
    rs.aux = nullptr;
    rs.ev_fork = rs.ev_join = nullptr;
    rs.sig_late = false;
    int variant = 0;
    try {
      for (int32_t r = 0; r < n_runs; ++r) {
        tr.kprof = ev.data();
        tr.kprof_mask = 0;
        prom::launch_transit(st, tr, rs, ctx->tables, ctx->mtables, nullptr, &variant, false);
        tr.kprof = nullptr;
        PROM_HIP(hipStreamSynchronize(st));
        for (int k = 0; k < PROM_K_COUNT; ++k) {
          if (!(tr.kprof_mask & (1u << k))) continue;
          float ms = 0.0f;
          PROM_HIP(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
          sum[k] += ms;
          ++cnt[k];
        }
      }
    } catch (...) {
      tr.kprof = nullptr;
      for (auto e : ev) (void)hipEventDestroy(e);
      throw;
    }
    for (auto e : ev) PROM_HIP(hipEventDestroy(e));
    tr.last = 0;
    tr.ran = true;
    ctx->br.current = false;
    for (int k = 0; k < PROM_K_COUNT; ++k) ms_out[k] = cnt[k] ? sum[k] / cnt[k] : std::nan("");
  });
}

int32_t prom_transit_result(prom_ctx* ctx, double* R_out) {
  return guarded(ctx, [&] {
    prom::TransitDev& tr = ctx->tr;
    if (!tr.ran) throw Error(PROM_E_STATE, "prom_transit_result: no completed run");
    PROM_REQUIRE(R_out, "prom_transit_result: null output");
    for (auto st : ctx->streams) PROM_HIP(hipStreamSynchronize(st));
    const size_t bytes = sizeof(double) * (size_t)tr.n_orb * (size_t)tr.n_wav;
    const char* src = static_cast<const char*>(tr.slot[tr.last].R.p);
    if (prom::pinned_holds(R_out, bytes)) {
      // page-locked destination (prom_host_alloc): DMA straight into it, split over PROM_D2H_SPLIT streams
      const char* e = std::getenv("PROM_D2H_SPLIT");
      const size_t k = (size_t)std::max(1, std::min(prom::kMaxSlots, e ? std::atoi(e) : 1));
      const size_t part = ((bytes + k - 1) / k + 4095) & ~(size_t)4095;
      for (size_t i = 0; i < k && i * part < bytes; ++i)
        PROM_HIP(hipMemcpyAsync(reinterpret_cast<char*>(R_out) + i * part, src + i * part,
                                std::min(part, bytes - i * part), hipMemcpyDeviceToHost, ctx->streams[i]));
      for (size_t i = 0; i < k; ++i) PROM_HIP(hipStreamSynchronize(ctx->streams[i]));
      return;
    }
    // D2H in chunks into pinned staging (one DMA per chunk, full link rate) while host threads copy the
    // finished chunks out to the caller's (pageable) array: the copy-out overlaps the transfer and runs on
    // several cores instead of one
    constexpr size_t kChunk = (size_t)2 << 20;
    const size_t n_chunks = (bytes + kChunk - 1) / kChunk;
    if (ctx->pin_cap < bytes) {
      if (ctx->pin) PROM_HIP(hipHostFree(ctx->pin));
      ctx->pin = nullptr;
      ctx->pin_cap = 0;
      PROM_HIP(hipHostMalloc(&ctx->pin, bytes, hipHostMallocDefault));
      ctx->pin_cap = bytes;
    }
    while (ctx->pin_ev.size() < n_chunks) {
      hipEvent_t e;
      PROM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      ctx->pin_ev.push_back(e);
    }
    char* pin = static_cast<char*>(ctx->pin);
    for (size_t c = 0; c < n_chunks; ++c) {
      const size_t off = c * kChunk, len = std::min(kChunk, bytes - off);
      PROM_HIP(hipMemcpyAsync(pin + off, src + off, len, hipMemcpyDeviceToHost, ctx->stream));
      PROM_HIP(hipEventRecord(ctx->pin_ev[c], ctx->stream));
    }
    const size_t n_thr = std::min<size_t>(n_chunks, 8);
    std::vector<hipError_t> errs(n_thr, hipSuccess);
    auto copier = [&](size_t t) {
      for (size_t c = t; c < n_chunks; c += n_thr) {
        const hipError_t e = hipEventSynchronize(ctx->pin_ev[c]);
        if (e != hipSuccess) { errs[t] = e; return; }
        const size_t off = c * kChunk, len = std::min(kChunk, bytes - off);
        std::memcpy(reinterpret_cast<char*>(R_out) + off, pin + off, len);
      }
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < n_thr; ++t) pool.emplace_back(copier, t);
    copier(0);
    for (auto& th : pool) th.join();
    for (auto e : errs) PROM_HIP(e);
  });
}

int32_t prom_transit_columns(prom_ctx* ctx, double* N_out) {
  return guarded(ctx, [&] {
    prom::TransitDev& tr = ctx->tr;
    if (!tr.ran) throw Error(PROM_E_STATE, "prom_transit_columns: no completed run");
    PROM_REQUIRE(N_out, "prom_transit_columns: null output");
    for (auto st : ctx->streams) PROM_HIP(hipStreamSynchronize(st));
    download(N_out, tr.slot[tr.last].ncol, (int64_t)tr.n_atoms * tr.n_orb * tr.n_pr, ctx->stream);
    PROM_HIP(hipStreamSynchronize(ctx->stream));
  });
}

int32_t prom_transit_band_stats(prom_ctx* ctx, int32_t n_bands, const double* bounds, double* sum_out,
                                int64_t* count_out, double* max_out) {
  return guarded(ctx, [&] {
    prom::TransitDev& tr = ctx->tr;
    if (!tr.ran) throw Error(PROM_E_STATE, "prom_transit_band_stats: no completed run");
    PROM_REQUIRE(n_bands >= 0 && (n_bands == 0 || bounds) && sum_out && count_out && max_out,
                 "prom_transit_band_stats: bad arguments");
    const int32_t n_orb = tr.n_orb;
    // the last run's stream orders the reduction after it; scratch[0..2] are free between calls
    const hipStream_t st = ctx->streams[tr.last];
    upload(ctx->scratch[0], bounds, (int64_t)n_orb * n_bands * 2, st);
    ctx->scratch[1].ensure(sizeof(double) * n_orb);
    ctx->scratch[2].ensure(sizeof(int64_t) * n_orb);
    ctx->scratch[3].ensure(sizeof(double) * n_orb);
    prom::launch_band_stats(st, tr.slot[tr.last].R.as<double>(), tr.wav.as<double>(), n_orb, tr.n_wav, n_bands,
                            ctx->scratch[0].as<double>(), ctx->scratch[1].as<double>(),
                            ctx->scratch[2].as<int64_t>(), ctx->scratch[3].as<double>());
    download(sum_out, ctx->scratch[1], n_orb, st);
    download(count_out, ctx->scratch[2], n_orb, st);
    download(max_out, ctx->scratch[3], n_orb, st);
    PROM_HIP(hipStreamSynchronize(st));
  });
}

}  // extern "C"
