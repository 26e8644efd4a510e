/*
 * prom_hip.h -- C-ABI of libprom_hip.so, the MI355X (gfx950) transit radiative-transfer core.
 *
 * The reference (CrazeXD/Prometheus) is pure Python with a duck-typed plugin protocol and no
 * FFI.  Each entry point below replaces one function (or one fused group of functions) on its
 * per-(orbital phase, wavelength) optical-depth path; the file:line it replaces is cited next to
 * it (paths relative to the reference tree).  A Python binding over ctypes lives in
 * prometheus_amd/_native.py; the stub a maintainer would add to the reference is in INTEGRATION.md.
 *
 * Conventions
 *   - Plain C types only: int32_t/int64_t sizes, double arrays (IEEE binary64, C order).
 *   - Every function returns PROM_OK (0) or a negative prom_status; the message of the last failure
 *     on a context is prom_last_error(ctx).  No exception crosses the ABI.
 *   - Host pointers passed in are read during the call only (inputs are copied to device memory
 *     owned by the context); output pointers are host buffers the caller owns.
 *   - One context per device.  Calls on different contexts may run concurrently from different host
 *     threads; a context is not re-entrant.  The library keeps no global mutable state.
 */
#ifndef PROM_HIP_H
#define PROM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PROM_ABI_VERSION 6

typedef struct prom_ctx prom_ctx;

enum prom_status {
  PROM_OK = 0,
  PROM_E_ARG = -1,      /* invalid argument (shape, null pointer, unknown id/kind) */
  PROM_E_HIP = -2,      /* HIP runtime error (device missing, launch failure, ...) */
  PROM_E_NOMEM = -3,    /* device allocation failed */
  PROM_E_STATE = -4     /* call out of order (e.g. prom_transit_run before prom_transit_set) */
};

/* ---- context ------------------------------------------------------------------------------- */
int32_t prom_abi_version(void);
int32_t prom_device_count(int32_t* count);
int32_t prom_create(int32_t device, prom_ctx** out);
void prom_destroy(prom_ctx* ctx);
const char* prom_last_error(const prom_ctx* ctx);
int32_t prom_synchronize(prom_ctx* ctx);

/* ---- log-sigma lookup tables ----------------------------------------------------------------
 * A table is the (x, log10(sigma + offset)) pair that the reference stores in an interp1d object
 * (AtmosphericConstituent.constructLookupFunction, gasProperties.py:694-715).  Tables live in
 * device memory, identified by an id local to the context. */

/* Upload a precomputed table (x strictly as given, must be non-decreasing). */
int32_t prom_table_upload(prom_ctx* ctx, int64_t n, const double* x, const double* log_sigma,
                          double offset, int32_t* table_id);

/* Build the table on the device: sigma(x) = sum over lines, in the given order, of
 *   (pi e^2 / (m_e c)) f_l * voigt_profile(c/x - c/lambda_l, sigma_v/lambda_l, gamma_l)
 * then log10(sigma + offset).  Replaces calculateVoigtProfile + constructLookupFunction
 * (gasProperties.py:672-715); line_coef[l] = (pi e^2/(m_e c)) * f_l computed by the caller in
 * the reference's evaluation order.  log_sigma_out (host, n) may be NULL. */
int32_t prom_table_build_voigt(prom_ctx* ctx, int64_t n, const double* x, int32_t n_lines,
                               const double* line_wavelength, const double* line_gamma,
                               const double* line_coef, double sigma_v, double c_light,
                               double offset, int32_t* table_id, double* log_sigma_out);

/* sigma(x) itself (no log, no table): calculateVoigtProfile (gasProperties.py:672-692). */
int32_t prom_voigt_sigma(prom_ctx* ctx, int64_t n, const double* x, int32_t n_lines,
                         const double* line_wavelength, const double* line_gamma,
                         const double* line_coef, double sigma_v, double c_light,
                         double* sigma_out);

/* out[i] = 10^(interp(targets[i], table)) - offset with numpy.interp semantics (clamping, exact
 * node hits): n_interp_log (gasProperties.py:34-51) / AtmosphericConstituent.getSigmaAbs (:727-735). */
int32_t prom_table_lookup(prom_ctx* ctx, int32_t table_id, int64_t n_targets, const double* targets,
                          double* out);

/* Release a table's device memory; its id is reused by a later upload.  The reference drops its
 * interp1d objects with the constituent (gasProperties.py:694-715, :34-51 builds one per call); a
 * transit problem set on this context that reads the table is invalidated (prom_transit_run then
 * fails with PROM_E_STATE until prom_transit_set is called again). */
int32_t prom_table_free(prom_ctx* ctx, int32_t table_id);
/* Live tables on the context (atomic, molecular) and the device bytes they hold. */
int32_t prom_table_count(prom_ctx* ctx, int32_t* n_atomic, int32_t* n_molecular, int64_t* device_bytes);

/* ---- molecular tables (MolecularConstituent, gasProperties.py:765-818) ----------------------
 * Axes in the reference's units after its conversions: P [dyn cm^-2] (= p[Pa] * 10), T [K],
 * wavelength [cm] (= 1/bin_edges reversed, increasing); log_sigma[n_p][n_t][n_w] = log10(xsec + offset)
 * on those axes.  Lookup is trilinear in (P, T, wavelength) with RegularGridInterpolator(
 * bounds_error=False, fill_value=log10(offset)) semantics; P is clipped below at 1e-4. */
int32_t prom_molecular_upload(prom_ctx* ctx, int32_t n_p, const double* P, int32_t n_t, const double* T,
                              int64_t n_w, const double* wavelength, const double* log_sigma,
                              double offset, int32_t* table_id);
/* getSigmaAbs: sigma[c][x][w] for P[c][x], fixed T, wavelength[c][w] (gasProperties.py:789-818). */
int32_t prom_molecular_sigma(prom_ctx* ctx, int32_t table_id, int64_t n_chords, int32_t n_x,
                             const double* P, double T, int64_t n_wav, const double* wavelength,
                             double* sigma_out);
/* Release a molecular table (see prom_table_free). */
int32_t prom_molecular_free(prom_ctx* ctx, int32_t table_id);

/* ---- density scenarios (calculateNumberDensity, gasProperties.py:143-516) ------------------- */
enum prom_density_kind {
  PROM_DENSITY_BAROMETRIC = 1,  /* :143-161  p = {n_0, R, H}                                     */
  PROM_DENSITY_HYDROSTATIC = 2, /* :185-204  p = {n_0, R, G*mu*M, k_B*T, Jeans_0}                */
  PROM_DENSITY_POWERLAW = 3,    /* :228-244, :311-330, :356-374  p = {n_0, R, q} (planet or moon) */
  PROM_DENSITY_TORUS = 4,       /* :491-516  p = {n_0, a_torus, 4*H_torus, H_torus}              */
  PROM_DENSITY_TABULATED = 5,   /* any other plugin: n(c, x) evaluated by the caller              */
  PROM_DENSITY_GRIDDED = 6      /* SerpensExosphere :548-601: scipy RegularGridInterpolator (linear,
                                   bounds_error) of a 3-D grid at (x - body_x, y - body_y, z);
                                   p = {n_gx, n_gy, n_gz}, grid in prom_scenario.n_tabulated as
                                   [gx[n_gx], gy[n_gy], gz[n_gz], values[n_gx][n_gy][n_gz]]        */
};

typedef struct prom_density_model {
  int32_t kind;
  int32_t reserved;
  double p[8];   /* scalars precomputed on the host in the reference's evaluation order */
} prom_density_model;

/* n[c][x] at chords with sky-plane coordinates (y[c], z[c]) = rho*(sin phi, cos phi) and density
 * centre (body_x[c], body_y[c]) (the planet's or moon's getPosition at that chord's phase). */
int32_t prom_number_density(prom_ctx* ctx, const prom_density_model* model, int32_t n_x,
                            const double* x, int64_t n_chords, const double* y, const double* z,
                            const double* body_x, const double* body_y, double* n_out);

/* SerpensExosphere.InterpolatedDensity (gasProperties.py:583-601; scipy RegularGridInterpolator, method
 * linear): out[i] = trilinear value of values[n_gx][n_gy][n_gz] on the ascending axes gx, gy, gz at
 * (px[i], py[i], pz[i]), in scipy's corner order.  A point outside the grid in any dimension gives NaN
 * (the reference raises: bounds_error=True). */
int32_t prom_gridded_density(prom_ctx* ctx, int32_t n_gx, const double* gx, int32_t n_gy, const double* gy,
                             int32_t n_gz, const double* gz, const double* values, int64_t n_points,
                             const double* px, const double* py, const double* pz, double* out);

/* ---- the fused transit integrator (Transit.sumOverChords, gasProperties.py:1160-1258, with
 *      Atmosphere.getLOSopticalDepth_Batch :885-956 and the density / sigma lookups inside) ----- */
typedef struct prom_constituent {
  int32_t table_id;      /* atomic: lookup-table id; molecular: molecular-table id */
  int32_t is_molecule;
  double chi;            /* mixing ratio (1.0 for exospheres) */
} prom_constituent;

typedef struct prom_scenario {
  prom_density_model density;
  const double* body_x;        /* [n_orb] density centre per phase (planet or moon)          */
  const double* body_y;        /* [n_orb]                                                     */
  const double* shift;         /* [n_orb] Doppler factor per phase (constants.py:31-45)       */
  const double* n_tabulated;   /* TABULATED: n[c][x] in the reference's chord order
                                  (c = ip * n_orb + o, geometryHandler.py:202-207);
                                  GRIDDED: the packed axes and values (prom_density_kind)      */
  double T;                    /* molecular constituents: lookup temperature                  */
  int32_t n_constituents;
  int32_t reserved;
  const prom_constituent* constituents;
} prom_scenario;

typedef struct prom_transit_problem {
  int64_t n_wav;               /* wavelengths of this shard                                   */
  const double* wavelength;    /* [n_wav] cm                                                  */
  int32_t n_pr;                /* chord positions per phase = phi_steps * rho_steps           */
  int32_t n_orb;               /* orbital phases                                              */
  const double* chord_y;       /* [n_pr] rho sin(phi), phi-major order                        */
  const double* chord_z;       /* [n_pr] rho cos(phi)                                         */
  const double* chord_fout;    /* [n_pr] F_out = rho * F_star * clv (flat star)               */
  int32_t n_x;                 /* line-of-sight samples                                       */
  int32_t n_scenarios;
  const double* x;             /* [n_x] cm                                                    */
  double delta_x;
  const double* planet_y;      /* [n_orb] planet y per phase: blocked if sqrt(dy^2+z^2) < R   */
  double planet_R;
  int32_t n_moons;
  int32_t reserved;
  const double* moon_y;        /* [n_moons][n_orb]: blocked if dy^2 + z^2 < R_m^2             */
  const double* moon_R;        /* [n_moons]                                                   */
  const prom_scenario* scenarios;
  double cull_tau;             /* chords whose tau upper bound is below this are transparent
                                  (exp(-tau) == 1 to the last ulp); <= 0 selects 2^-60       */
  int32_t options;             /* PROM_OPT_* bit set                                          */
  int32_t reserved2;
  double k_B;                  /* Boltzmann constant for P = n k_B T of molecular lookups
                                  (<= 0: the reference's 1.381e-16, constants.py:17)          */
  /* Stellar spectrum (gasProperties.py:1180-1219): with has_star != 0 the flux of chord c at
   * wavelength w is F = rho_c * (F_star(lambda_w / s_c) * clv_c), F_star(t) = 10^interp(t, star
   * table) (n_interp_log with offset 0, :34-51) and s_c = calculateDopplerShift(vsini rho_c / R_star
   * cos(phi_c - phi_rot)) (the Rossiter-McLaughlin shift, :1183-1184); chord_fout is then unused.
   * has_star == 0 keeps the flat star (F_star = 1, :1210-1211).  Atomic constituents only. */
  int32_t has_star;
  int32_t star_table;          /* table id (prom_table_upload of Fstar_function.x, .y; offset 0) */
  const double* chord_rho;     /* [n_pr] rho                                                  */
  const double* chord_clv;     /* [n_pr] 1 - u1 (1 - mu) - u2 (1 - mu)^2                       */
  const double* chord_star_shift;  /* [n_pr] s_c                                              */
} prom_transit_problem;

/* prom_transit_problem.options */
#define PROM_OPT_OCML_EXP 1    /* use the ocml exp() in the tau kernel instead of the table-driven exp */
#define PROM_OPT_NO_MERGE 2    /* integrate every active chord (no merging of equal-column chords) */
#define PROM_OPT_NO_WINDOW 4   /* evaluate exp(-tau) for every record at every wavelength (no saturated-
                                  head skip, no tail moments; see DESIGN.md "windowed integration") */
#define PROM_OPT_DOPPLER_ROWS 8 /* one Doppler sigma row per orbital phase even when the phases' factors are
                                  equal (a phase shard of a Doppler-shifted problem: the full problem's path,
                                  so its R rows are the full run's bit for bit) */

typedef struct prom_transit_stats {
  double ms_total;             /* device time of the last prom_transit_run (hipEvents)        */
  double ms_density;           /* density + column-density + culling kernels                  */
  double ms_sigma;             /* sigma resample kernel                                       */
  double ms_tau;               /* fused tau -> exp -> disk-sum kernel                         */
  int64_t active_chords;       /* chord-phase pairs integrated (all phases)                   */
  int64_t transparent_chords;  /* chord-phase pairs folded in as exp(-tau) = 1                */
  int64_t blocked_chords;
  int64_t chord_lambda_evals;  /* active_chords * n_wav                                        */
  int64_t tau_records;         /* chord records the tau kernel integrates (after merging)     */
  int64_t exp_evals;           /* exp evaluations of the fused kernel (counted on the device:
                                  the windowed kernel evaluates only the records of each
                                  wavefront's tau window; tau_records * n_wav without windows;
                                  molecular problems add the 10^v of every in-table sample)   */
  int32_t tau_kernel_variant;  /* which integration path the run took: tens = path, units = effective atomic
                                  species the path's kernels see (1 when species are merged into one absorber,
                                  0 when more than 4).  Tens (prom_transit.hip launch_transit):
                                    0  exact chord-order validation kernel k_tau with the ocml exp
                                       (PROM_OPT_OCML_EXP, and phases with a non-finite column);
                                    1  k_tau with the table exp (generic path; with molecular constituents:
                                       k_mol_list + k_tau_mol);
                                    2  windowed integration k_tau_w (k_order windows, per-tile records);
                                    3  planned windowed integration k_tau_p (k_order + k_windows heavy lists);
                                    4  stellar spectrum / CLV / RM rotation k_tau_rm;
                                    8  transmission curves, the default for one effective absorber:
                                       k_columns8 -> k_tc_build -> k_sigma_tc (prom_tcurve.hip; no orbital
                                       Doppler shift between the phases, one phase, or coarse tables);
                                    9  transmission curves with the Doppler-shifted lookups over target
                                       windows: k_columns8 -> k_tc_build -> k_sigma_tw (prom_tw.hip)       */
  int32_t tau_kernel_variant_exact_phases;  /* phases integrated on the exact (ocml) path because a
                                               column density was not finite                      */
} prom_transit_stats;

/* Copy a problem to the device (all host arrays are read during the call). */
int32_t prom_transit_set(prom_ctx* ctx, const prom_transit_problem* problem);
/* Run the integrator on the device; R stays in device memory.  stats may be NULL (with stats the
 * call waits for the run).  Runs are asynchronous: consecutive runs of a problem on the atomic paths
 * rotate over PROM_PIPELINE (default 4) internal streams and work-buffer slots, so the kernels of one run
 * (on the default path k_columns8 -> k_tc_build -> k_sigma_tc) overlap those of the runs before it; each
 * run is complete and independent.  prom_transit_result, prom_synchronize and prom_transit_set wait for
 * all of them. */
int32_t prom_transit_run(prom_ctx* ctx, prom_transit_stats* stats);
/* Copy R[n_orb][n_wav] (row-major) of the last run to a host buffer.  A buffer from prom_host_alloc
 * takes one DMA at the link rate; any other buffer is filled through the context's pinned staging. */
int32_t prom_transit_result(prom_ctx* ctx, double* R_out);

/* Page-locked host memory for results (ABI 4).  Process-wide pool, independent of contexts: a freed
 * buffer is kept for the next request of a similar size (size <= capacity <= 2 size), so a caller that
 * takes a fresh output array per call pays neither hipHostMalloc nor page faults.  Pinned bytes (in use +
 * cached) are capped at PROM_PINNED_CAP_MB (default 4096): past the cap PROM_E_NOMEM, and the caller falls
 * back to ordinary memory.  Replaces the reference's np.zeros result arrays (gasProperties.py:1165-1166). */
int32_t prom_host_alloc(int64_t bytes, void** out);
/* Return a prom_host_alloc buffer to the pool (PROM_E_ARG for any other pointer). */
int32_t prom_host_free(void* p);
/* Column densities N[s][o][ip] of the last run (atomic constituents in scenario order); testing aid.  With the species
 * merged into one effective absorber (tau_kernel_variant's units digit 1 for several atomic constituents) only slot 0
 * is written, and it holds the chi = 1 column. */
int32_t prom_transit_columns(prom_ctx* ctx, double* N_out);

/* Band statistics of the last run's R on the device, for light curves (the band-averaged transit
 * depth of mainRetrieval.py:76-93) without copying R to the host.  Phase o selects the wavelengths
 * with bounds[o][b][0] <= lambda <= bounds[o][b][1] for any band b; sum_out[o] is the sum of R over
 * them, count_out[o] their number and max_out[o] the maximum of R over ALL wavelengths of the problem
 * (NaN if any R is NaN, like numpy.max).  Over wavelength shards the sums and counts add and the
 * maxima combine with max; the light curve is (sum / count) / max. */
int32_t prom_transit_band_stats(prom_ctx* ctx, int32_t n_bands, const double* bounds, double* sum_out,
                                int64_t* count_out, double* max_out);

/* ---- observation of a spectrum on the device -------------------------------------------------
 * What a retrieval does with R before it compares it with data, over R as it lies in device memory: the
 * convolution with the spectrograph's Gaussian line-spread function, the sampling on the detector's pixels (per
 * phase in a frame scaled by f[o], e.g. the planet's rest frame) and the chi-square.  All float64; the roundings
 * named here are part of the definition.
 *
 *   trapezoid weights    q_w = (hi_w - lo_w) / 2, lo_w = wav[w-1] (w = 0: edge_lo, or wav[0] when edge_lo is NaN),
 *                        hi_w likewise at the top: the weights of the WHOLE grid when a shard or chunk passes the
 *                        grid points just outside it as edges (NaN: there is none)
 *   pixel in the model frame   L = fl(lam[p] f[o]), S = fl(sig[p] f[o]), c = fl(k S)   (f NULL: all 1)
 *   support              the w with |wav[w] - L| <= c (difference in float64, both ends inclusive)
 *   weight               g_w = exp(-0.5 z z), z = (wav[w] - L) / S
 *   partial sums         num[o][p] = sum g_w q_w R[o][w], den[o][p] = sum g_w q_w over the support, in an order
 *                        fixed by the kernel (no floating-point atomics: two calls agree bit for bit).  An empty
 *                        support gives 0 and 0; a NaN in R reaches exactly the pixels whose support holds it
 *   model spectrum       M = (sum over shards of num) / (sum over shards of den); den == 0: NaN, no coverage
 *   chi-square           pixel (o, p) is used when ivar is finite and > 0, data is finite and den > 0;
 *                        chi2[o] = sum over used pixels of ivar (M - data)^2 in a fixed order, n_used[o] their
 *                        number.  Formed on the device only when the call sees the whole grid (both edges NaN);
 *                        with an edge given a request for it is PROM_E_ARG and the caller forms it from the
 *                        combined partials.
 * The pixel's own width is not modelled: the caller folds it into sig. */

/* Make the observation resident on the context: pixel centres lam[n_pix] (non-decreasing) and Gaussian widths
 * sig[n_pix] > 0 in cm, the truncation k > 0 in units of sigma, n_orb phases, and optionally the frame factors
 * f[n_orb] > 0 (NULL: all 1) and data[n_orb][n_pix] with ivar[n_orb][n_pix] (NULL: no chi-square).  A retrieval
 * uploads it once.  A later prom_transit_set with another n_orb drops it (the observe calls then fail with
 * PROM_E_STATE). */
int32_t prom_observe_set(prom_ctx* ctx, int32_t n_pix, const double* lam, const double* sig, double k, int32_t n_orb,
                         const double* f, const double* data, const double* ivar);
/* Observe the last run's R on its stream (as prom_transit_band_stats does).  Every output may be NULL; only the
 * requested ones are copied back: num_out, den_out [n_orb][n_pix], chi2_out [n_orb], n_used_out [n_orb].  With
 * n_pix == 0 the call returns PROM_OK and touches nothing. */
int32_t prom_transit_observe(prom_ctx* ctx, double edge_lo, double edge_hi, double* num_out, double* den_out,
                             double* chi2_out, int64_t* n_used_out);
/* The same for a spectrum the caller supplies: wav[n_wav] ascending, R[n_orb][n_wav], n_orb the observation's. */
int32_t prom_spectrum_observe(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                              double edge_lo, double edge_hi, double* num_out, double* den_out, double* chi2_out,
                              int64_t* n_used_out);
/* Measurement aid (tools/observe_bench.py), not for callers: mean device duration in milliseconds of k_observe over
 * n_runs repetitions of the last observe call's launch (events around its dispatch).  PROM_E_STATE when there is
 * no such call since the last prom_observe_set or prom_transit_set. */
int32_t prom_observe_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out);

/* ---- velocity maps on the device -------------------------------------------------------------
 * The observation's model spectrum in many trial frames at once, compared with the data: for every phase o and
 * trial j of a resident table F[n_orb][n_trial] of frame factors (a grid of trial velocities, or a (Kp, Vsys)
 * grid), the seven inverse-variance weighted moments of model against data.  Chi-square, chi-square with a free
 * scale, the weighted cross-correlation and a Brogi & Line log-likelihood follow from them on the host
 * (prometheus_amd/observation.py, VelocityMap).  All float64; the roundings named here are part of the definition.
 *
 *   inputs               the resident observation (prom_observe_set) with data and ivar; the table F, every entry
 *                        finite and > 0; a spectrum wav[n_wav], R[n_orb][n_wav] that covers the whole grid (both
 *                        edges NaN in the trapezoid weights: there are no shard partials)
 *   frame of trial (o, j)  F[o][j] alone is the factor; the observation's own f[o] is not applied.  Pixel p has
 *                        L = fl(lam[p] F[o][j]), S = fl(sig[p] F[o][j]), c = fl(k S); the support, the weights g and
 *                        q, num, den and M = num / den are those of the observation's definition above with f[o]
 *                        replaced by F[o][j] (num and den added over the support in an order fixed by the kernel)
 *   used pixels          ivar[o][p] finite and > 0, data[o][p] finite, den > 0 (the chi-square's rule)
 *   moments              over the used pixels, with iv = ivar and d = data:
 *                          m0 = sum iv          m1 = sum fl(iv M)         m2 = sum fl(iv d)
 *                          m3 = sum fl(fl(iv M) M)   m4 = sum fl(fl(iv M) d)   m5 = sum fl(fl(iv d) d)
 *                          m6 = sum fl(iv fl((M - d)^2)), formed directly and not from the others
 *                        and n_used (int64), their number
 *   order, edge cases    the order of every sum is fixed by the kernels (no floating-point atomics); with no used
 *                        pixel every moment is 0 and n_used is 0; a used pixel with NaN M makes m1, m3, m4 and m6
 *                        of that (o, j) NaN and leaves m0, m2, m5 and n_used alone
 *   independence         the eight numbers of trial (o, j) depend only on the spectrum, the observation and the
 *                        value F[o][j]: not on n_trial, the column's position in the table, the other columns,
 *                        whether a support was read from LDS or from global memory, or how the launcher splits the
 *                        table into batches.  Two calls agree bit for bit. */

/* Make the trial table F[n_orb][n_trial] resident.  n_trial >= 1 and every entry finite and > 0, otherwise
 * PROM_E_ARG; the context must hold an observation with data and the same n_orb, otherwise PROM_E_STATE.  A later
 * prom_observe_set, or a prom_transit_set with another n_orb, drops the table (the map calls then fail with
 * PROM_E_STATE). */
int32_t prom_vmap_set(prom_ctx* ctx, int32_t n_orb, int32_t n_trial, const double* F);
/* The map over the last run's R on its stream (as prom_transit_observe): mom_out [n_orb][n_trial][7] and
 * n_used_out [n_orb][n_trial]; either may be NULL.  The partial records of the kernel take
 * n_orb * n_trial * ceil(ceil(n_pix / 32) / 16) * 64 bytes of device scratch, capped at 256 MiB, or at
 * PROM_VMAP_SCRATCH_MB megabytes (fractions allowed) from the environment at context creation: a larger table runs in
 * batches of whole groups of 8 trials (one group at least), with the same results bit for bit.  (The one other cap
 * read from the environment is PROM_GRID_SCRATCH_MB, megabytes of work buffers of an injection grid's sub-batch,
 * default 4096, read at every grid call: "injection grids on the device" below.) */
int32_t prom_transit_vmap(prom_ctx* ctx, double* mom_out, int64_t* n_used_out);
/* The same for a spectrum the caller supplies: wav[n_wav] finite and ascending, R[n_orb][n_wav], n_orb the table's
 * (the checks of prom_spectrum_observe). */
int32_t prom_spectrum_vmap(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                           double* mom_out, int64_t* n_used_out);
/* Measurement aid (tools/vmap_bench.py), not for callers: mean device duration in milliseconds of k_vmap over n_runs
 * repetitions of the last map call (events around the first batch's dispatch, scaled by n_trial over the batch's
 * trials when the table runs in several batches).  PROM_E_STATE when there is no such call since the last
 * prom_transit_set, prom_observe_set or prom_vmap_set. */
int32_t prom_vmap_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out);

/* ---- exposures on the device -----------------------------------------------------------------
 * Data at any phase, smeared over its duration.  An exposure is a weighted sum of a few taps; a tap is a row of R
 * read in its own frame: the row's model spectrum M at a factor F.  Interpolation between neighbouring model phases
 * is two taps, the average over an exposure's duration n_sub such pairs, trial velocities put a trial axis on the
 * factors (prometheus_amd/observation.py, exposure_taps).  All float64; the roundings named here are part of the
 * definition.
 *
 *   inputs               the resident observation (prom_observe_set): only its pixels lam, sig, k and its n_orb are
 *                        used, not its own f, data and ivar; a spectrum wav[n_wav], R[n_orb][n_wav] that covers the
 *                        whole grid (both edges NaN, as for the maps); a resident exposure table with n_exp >= 1,
 *                        n_trial >= 1, n_tap >= 1:
 *                          row[n_exp][n_tap]          int32, every entry in [0, n_orb)
 *                          a[n_exp][n_tap]            finite and >= 0
 *                          F[n_exp][n_trial][n_tap]   finite and > 0
 *                          data[n_exp][n_pix], ivar[n_exp][n_pix]   in the device's pixel order
 *   taps                 tap i of (e, j) is live when a[e][i] > 0.  A dead tap is skipped altogether: it is never
 *                        read and adds nothing, a NaN in its row does not matter (the padding rule).  A live tap's
 *                        pixel has L = fl(lam[p] F[e][j][i]), S = fl(sig[p] F[e][j][i]), c = fl(k S); the support,
 *                        the weights g and q, num_i, den_i and M_i = num_i / den_i are those of the observation's
 *                        definition on row row[e][i], added in the order the velocity map uses for the same pixel
 *                        and factor
 *   exposure model       M_e[p] starts from the first live tap's fl(a_i M_i); each later live tap's fl(a_i M_i) is
 *                        added in ascending i.  It is not renormalised: the host makes the weights sum to 1
 *   used pixels          (e, j, p) is used when ivar[e][p] is finite and > 0, data[e][p] is finite, at least one tap
 *                        is live and every live tap has den_i > 0
 *   moments              the seven moments and n_used of the velocity map, formed with M_e, data[e] and ivar[e];
 *                        with no used pixel zeros; a used pixel with NaN M_e makes m1, m3, m4 and m6 NaN and leaves
 *                        the rest alone
 *   models on request    model[e][j][p] = M_e; NaN where the pixel has no live tap or a live tap has den_i = 0.  Data
 *                        and ivar play no part in it
 *   independence         the numbers of (e, j) depend only on the spectrum, the pixels, exposure e's live taps in
 *                        order (their rows, weights and F[e][j][.]), data[e] and ivar[e]: not on n_exp, n_trial,
 *                        n_tap or the position of e or j, other exposures or trials, dead taps wherever they stand,
 *                        whether a support was read from LDS or from global memory, or the launcher's batches.  Two
 *                        calls agree bit for bit; there are no floating-point atomics
 *   degenerate case      n_exp = n_orb, one tap, row[e][0] = e and a = 1: the eight numbers are prom_spectrum_vmap's
 *                        for the table F[e][j], bit for bit (fl(1 M) = M, and the first live tap starts the sum) */

/* Make the exposure table resident.  PROM_E_ARG when a shape or value rule above is broken (n_exp <= 65535,
 * n_tap <= 65536, n_exp n_trial n_tap <= 2^28); PROM_E_STATE without a resident observation.  A later
 * prom_observe_set, or a prom_transit_set with another n_orb, drops the table (the expose calls then fail with
 * PROM_E_STATE). */
int32_t prom_expose_set(prom_ctx* ctx, int32_t n_exp, int32_t n_trial, int32_t n_tap, const int32_t* row,
                        const double* a, const double* F, const double* data, const double* ivar);
/* The exposures over the last run's R on its stream: mom_out [n_exp][n_trial][7], n_used_out [n_exp][n_trial],
 * model_out [n_exp][n_trial][n_pix].  Each may be NULL and is then neither formed nor copied.  The partial records
 * take n_exp * n_trial * ceil(ceil(n_pix / 32) / 16) * 64 bytes of device scratch under the map's cap
 * (PROM_VMAP_SCRATCH_MB): a larger table runs in batches of whole groups of 8 trials, with the same results bit
 * for bit. */
int32_t prom_transit_expose(prom_ctx* ctx, double* mom_out, int64_t* n_used_out, double* model_out);
/* The same for a spectrum the caller supplies (the checks of prom_spectrum_vmap; n_orb is the observation's). */
int32_t prom_spectrum_expose(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                             double* mom_out, int64_t* n_used_out, double* model_out);
/* Measurement aid (tools/expose_bench.py), not for callers: mean device duration in milliseconds of k_expose
 * (moments only) over n_runs repetitions of the last expose call, as prom_vmap_kernel_ms. */
int32_t prom_expose_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out);

/* ---- detrended exposures on the device --------------------------------------------------------
 * A systematics basis projected out of the exposures' model.  Data cleaned with SYSREM or PCA have lost part of the
 * planet's signal with the tellurics, so the model goes through the same linear filter before it meets them: per
 * pixel column p, over the exposures, m' = m - U (W_p m) (Gibson et al. 2022).  The filter couples all exposures of
 * a pixel; the host makes U and W (prometheus_amd/observation.py, sysrem and filter_weights).  All float64; the
 * roundings named here are part of the definition.
 *
 *   inputs               the resident observation and exposure table (prom_expose_set), a spectrum over the whole
 *                        grid, and a resident filter with 1 <= n_comp <= 16:
 *                          U[n_exp][n_comp]           finite: the basis the data were cleaned with
 *                          W[n_comp][n_exp][n_pix]    finite, in the device's pixel order, p fastest: the basis'
 *                                                     (inverse-variance weighted) pseudo-inverse at pixel p
 *   unfiltered model     M[e][j][p] is prom_spectrum_expose's model_out value, bit for bit
 *   filterable column    column (j, p) is filterable when M[e][j][p] is not NaN for every e that has
 *                        W[k][e][p] != 0 for some k
 *   coefficients         c_k starts at +0; in ascending e every term with W[k][e][p] != 0 adds
 *                        fl(W[k][e][p] M[e][j][p]).  A term with W = 0 is skipped altogether and its M is never
 *                        read into the sum (the padding rule: masked pixels carry W = 0)
 *   filtered model       M'_e starts at M_e and takes, in ascending k, M'_e <- fl(M'_e - fl(U[e][k] c_k)): every
 *                        product and every sum is rounded on its own, there is no fused multiply-add, and a plain
 *                        numpy loop gives the same bits.  In a column that is not filterable every M'_e is NaN
 *   used pixels          (e, j, p) is used when ivar[e][p] is finite and > 0, data[e][p] is finite, the column is
 *                        filterable and M[e][j][p] is not NaN.  A NaN model value therefore always un-uses its
 *                        pixel, whatever its cause (no coverage, or a NaN in R), and never reaches a moment.  This is
 *                        deliberately simpler than the exposures' rule (a used pixel with NaN M_e makes moments
 *                        NaN there): coverage is no longer known once only the model is in memory.  The kernel
 *                        tests M'_e, which in a filterable column is NaN where M_e is; it is NaN elsewhere only
 *                        when an infinity arose (one in R, or an overflowing product), and such a pixel is unused too
 *   moments              the seven moments and n_used of the velocity map, formed with M'_e, data[e] and ivar[e];
 *                        m6 directly from (M' - d); added in the map's shape (thread t of a 32-pixel tile, a
 *                        32-lane xor butterfly per tile, tiles in order within a chunk of 16, the chunks' records
 *                        in chunk order); with no used pixel zeros
 *   models on request    model[e][j][p] = M'_e
 *   independence         the numbers of (e, j) depend only on the spectrum, the pixels, the exposures' live taps,
 *                        column j's factors F[.][j][.], the filter, data[e] and ivar[e]: not on n_trial, j's
 *                        position, other trials or the launcher's batches.  Two calls agree bit for bit; there are
 *                        no floating-point atomics
 *   degenerate case      U = 0 with any finite W, and an R and table for which no M is NaN: the eight numbers and
 *                        the model are prom_spectrum_expose's, bit for bit (fl(0 c) = 0, x - 0 = x, and the moments
 *                        are added in the same shape) */

/* Make the filter resident: U[n_exp][n_comp] and W[n_comp][n_exp][n_pix].  PROM_E_STATE without a resident exposure
 * table; PROM_E_ARG when n_exp differs from the table's, n_comp lies outside [1, 16] or an entry is not finite.
 * prom_expose_set, and whatever drops the exposure table, drops the filter (the detrended calls then fail with
 * PROM_E_STATE). */
int32_t prom_detrend_set(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, const double* U, const double* W);
/* The detrended exposures over the last run's R on its stream: the outputs and checks of prom_transit_expose, each
 * output may be NULL, n_pix = 0 gives zeros.  The unfiltered model of the whole table is formed first and filtered
 * in place, so n_exp * n_trial * n_pix * 8 bytes of device memory hold it, whatever PROM_VMAP_SCRATCH_MB says (the
 * cap still batches the moments' partial records): a table whose model does not fit fails with PROM_E_NOMEM, and the
 * remedy is fewer trials per call. */
int32_t prom_transit_expose_detrended(prom_ctx* ctx, double* mom_out, int64_t* n_used_out, double* model_out);
/* The same for a spectrum the caller supplies (the checks of prom_spectrum_expose). */
int32_t prom_spectrum_expose_detrended(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                       double* mom_out, int64_t* n_used_out, double* model_out);
/* Measurement aid (tools/detrend_bench.py), not for callers: mean device durations in milliseconds over n_runs
 * repetitions of the last detrended call: ms_out[0] k_detrend (the whole table), ms_out[1] k_model_moments (the first
 * batch, scaled as prom_vmap_kernel_ms).  The filter works in place, so each repetition forms the unfiltered model
 * again (untimed) before it.  PROM_E_STATE when there is no such call. */
int32_t prom_detrend_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out);

/* ---- high-pass filtered exposures on the device -----------------------------------------------
 * High-resolution data never keep their continuum: each exposure of each echelle order has a smooth function along
 * its pixels (a Gaussian or box running mean, tens to hundreds of pixels wide) subtracted from it or divided out of
 * it, and SYSREM runs after that.  The model goes through the same two steps in the same order before it meets the
 * data.  The high-pass couples the pixels of one exposure inside one order.  All float64; the roundings named here are
 * part of the definition.
 *
 *   inputs               the resident observation and exposure table (prom_expose_set), a spectrum over the whole
 *                        grid, and a resident high-pass:
 *                          segments (the orders)      n_seg >= 1, seg_first[n_seg + 1] and perm[n_pix], both int32:
 *                                                     seg_first strictly ascending from 0 to n_pix (no segment is
 *                                                     empty), perm a permutation of 0 .. n_pix - 1; position i of
 *                                                     segment s is the device pixel perm[seg_first[s] + i]
 *                          taps                       half_width h, 0 <= h <= 512, and g[h + 1], every entry finite
 *                                                     and >= 0, g[0] > 0: g[d] is the weight at distance d
 *                          mode                       0 subtracts, 1 divides
 *   unfiltered model     M[e][j][p] is prom_spectrum_expose's model_out value, bit for bit
 *   smooth model         in a segment of length n, at position i of one (e, j), over the window
 *                        i' in [max(0, i - h), min(n - 1, i + h)] in ascending i': num starts at +0 and adds
 *                        fl(g[|i - i'|] M_i') for every i' whose M is not NaN; den starts at +0 and adds g[|i - i'|]
 *                        for the same i'.  Every product and every sum is rounded on its own, there is no fused
 *                        multiply-add, and a plain numpy loop gives the same bits.  A NaN value is skipped altogether
 *                        (adding +0 for it gives the same bits: num and den are never -0, and a kernel may rely on
 *                        that).  B_i = fl(num / den)
 *   filtered model       M'_i = fl(M_i - B_i) in mode 0, fl(M_i / B_i) in mode 1.  M'_i is NaN exactly where M_i is
 *                        NaN: a valid M_i always has den >= g[0] > 0; what IEEE gives otherwise stands (B = 0 under
 *                        division, an infinity).  An interior window without a NaN sees the same sequence of g for
 *                        every i, so a kernel may form that den once: the bits are the same
 *   then                 on request (detrend = 1) the resident SYSREM filter runs on M' exactly as defined under
 *                        "detrended exposures on the device", with M' in the place of M
 *   used pixels          (e, j, p) is used when ivar[e][p] is finite and > 0, data[e][p] is finite, the final model
 *                        value is not NaN and, with the SYSREM filter, the column is filterable
 *   moments              the seven moments and n_used in the map's shape, as for the detrended exposures; with no
 *                        used pixel zeros
 *   models on request    model[e][j][p] = the final model
 *   independence         the numbers of (e, j) depend only on the spectrum, the pixels, exposure e's live taps and
 *                        column j's factors (with the SYSREM filter those of all exposures, as there), the high-pass,
 *                        data and ivar: not on n_trial, j's position, other trials or the launcher's batches.  Two
 *                        calls agree bit for bit; there are no floating-point atomics
 *   degenerate cases     every segment of length 1, or h = 0: B = fl(fl(g[0] M) / g[0]), which is M when g[0] is a
 *                        power of two (gaussian_taps and box_taps give 1): mode 0 gives +0 wherever M is valid, mode 1
 *                        gives 1 wherever M is valid and not 0 */

/* Make the high-pass resident.  PROM_E_STATE without a resident exposure table; PROM_E_ARG when n_pix differs from the
 * observation's or a rule above is broken (with n_pix = 0: n_seg = 1 and seg_first = {0, 0}).  prom_expose_set, and
 * whatever drops the exposure table, drops the high-pass (the calls below then fail with PROM_E_STATE). */
int32_t prom_highpass_set(prom_ctx* ctx, int32_t n_pix, int32_t n_seg, const int32_t* seg_first, const int32_t* perm,
                          int32_t half_width, const double* g, int32_t mode);
/* The high-pass filtered exposures over the last run's R on its stream: the outputs, NULL rules and checks of
 * prom_transit_expose_detrended, n_pix = 0 gives zeros.  detrend is 0 or 1 (otherwise PROM_E_ARG); with 1 the
 * resident filter of prom_detrend_set follows the high-pass, and PROM_E_STATE when there is none.  The model of the
 * whole table lies in device memory at once, as for the detrended exposures: PROM_E_NOMEM when it does not fit (the
 * remedy is fewer trials per call).  A workgroup of k_highpass owns one (exposure, trial, segment):
 * n_exp n_trial n_seg >= 2^31 is PROM_E_ARG. */
int32_t prom_transit_expose_highpass(prom_ctx* ctx, int32_t detrend, double* mom_out, int64_t* n_used_out,
                                     double* model_out);
/* The same for a spectrum the caller supplies (the checks of prom_spectrum_expose). */
int32_t prom_spectrum_expose_highpass(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                      int32_t detrend, double* mom_out, int64_t* n_used_out, double* model_out);
/* Measurement aid (tools/highpass_bench.py), not for callers: ms_out[0] is the mean device duration in milliseconds of
 * k_highpass over the whole table, over n_runs repetitions of the last high-pass call.  The filter works in place, so
 * each repetition forms the unfiltered model again (untimed) before it.  PROM_E_STATE when there is no such call. */
int32_t prom_highpass_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out);

/* ---- median high-pass on the device ---------------------------------------------------------------
 * Many pipelines remove the continuum with a running median along each order, because a median does not chase deep
 * lines or cosmic-ray residue.  The resident high-pass is of one of two kinds: the weighted mean above, or the running
 * median defined here.  Whichever was set last runs wherever "the resident high-pass" runs: prom_*_expose_highpass,
 * prom_*_expose_orders, prom_sysrem_clean, prom_*_inject, prom_*_recover, prom_*_inject_grid, prom_*_recover_grid.
 * Everything above stands with B defined as follows.  All float64.
 *
 *   window               the segments seg_first[n_seg + 1] / perm[n_pix] are the mean's, the half width 0 <= h <= 512,
 *                        the mode 0 (subtract) or 1 (divide).  At position i of a segment of length n the window holds
 *                        the values M_i' for i' in [max(0, i - h), min(n - 1, i + h)] that are not NaN: clipped at the
 *                        segment's ends as the mean's is, nothing is reflected.  c is their count
 *   order of the values  the c values sorted ascending in the IEEE order of non-NaN doubles with -0 below +0 and the
 *                        infinities as ordinary values: the order of the bit patterns under the usual order-preserving
 *                        integer key (negative: all bits flipped, otherwise: the sign bit set).  This fixes the bits
 *                        among ties, of which only the sign of zero can be seen
 *   running median       c odd: B_i is the value at index (c - 1) / 2.  c even: B_i = fl(fl(lo + hi) 0.5) with lo and hi
 *                        at the indices c / 2 - 1 and c / 2
 *   filtered model       M'_i = fl(M_i - B_i) or fl(M_i / B_i).  M'_i is NaN exactly where M_i is: a valid M_i has
 *                        c >= 1, so B exists.  What IEEE gives otherwise stands (inf - inf, +inf + -inf, 0 / 0)
 *   degenerate cases     h = 0 or n = 1: B = M
 * B is a selection, so the bits do not depend on how a kernel finds it.  numpy's nanmedian of each window equals B
 * under ==; the integer key adds the sign of zero.
 *
 * Make the median resident in the place of any high-pass set before: the checks, PROM_E_ARG / PROM_E_STATE rules and
 * lifetime of prom_highpass_set, without taps.  prom_highpass_set puts the mean back.  prom_highpass_kernel_ms times
 * whichever kind is resident (k_median or k_highpass). */
int32_t prom_highpass_set_median(prom_ctx* ctx, int32_t n_pix, int32_t n_seg, const int32_t* seg_first,
                                 const int32_t* perm, int32_t half_width, int32_t mode);

/* ---- per-order moments on the device ------------------------------------------------------------
 * The likelihood of high-resolution data is defined per spectrum, that is per (exposure, echelle order): each order
 * has its own N, its own variances of data and model and its own best-fit scale, and orders are weighted or dropped
 * one by one.  The entries above add the moments over all pixels of an exposure; these give them per order, and the
 * totals of the per-order statistics, without bringing the model over the bus.  All float64; the order of addition and
 * the roundings named here are part of the definition.
 *
 *   resident orders      n_seg >= 1, seg_first[n_seg + 1] and perm[n_pix] (int32) under prom_highpass_set's rules:
 *                        seg_first strictly ascending from 0 to n_pix, perm a permutation of 0 .. n_pix - 1; position i
 *                        of order s is the device pixel perm[seg_first[s] + i] (with n_pix = 0: n_seg = 1 and {0, 0});
 *                        keep[n_seg], uint8, 0 or 1.  The orders are independent of the resident high-pass: either
 *                        may be there without the other, and their segments may differ
 *   final model          the model of the exposures after the optional high-pass (highpass = 1) and the optional
 *                        SYSREM filter (detrend = 1), each exactly as defined in its own section, in that order
 *   record of (e, j, s)  the seven moments m0 .. m6 and n_used (int64) of the final model's row (e, j) over the
 *                        positions of order s.  A position is used when ivar is finite and > 0, data is finite, the
 *                        column's flag is set (with the SYSREM filter: the column is filterable; otherwise always) and
 *                        M == M.  Its terms are iv, fl(iv M), fl(iv d), fl(fl(iv M) M), fl(fl(iv M) d), fl(fl(iv d) d)
 *                        and fl(iv fl(fl(M - d) fl(M - d))): k_model_moments' terms and rule
 *   order of addition    the order's positions are cut into tiles of 32 consecutive positions.  In a tile 32 terms
 *                        t[0 .. 31] start from the used positions' values, +0 for an unused position and for the tail
 *                        of the last tile; for m = 1, 2, 4, 8, 16 in turn every t[l] becomes fl(t[l] + t[l ^ m]) (all l
 *                        at once), and t[0] is the tile's sum.  The tiles' sums are added in ascending tile order to a
 *                        sum that starts at +0.  There is no chunk level (k_model_moments adds 16 tiles per chunk and
 *                        then the chunks), so for ONE order with the identity perm and n_pix <= 512 the record is the
 *                        lumped record of the entries above bit for bit, and otherwise it differs by rounding
 *   independence         the eight numbers of (e, j, s) depend on the final model's row (e, j), the data and order s
 *                        only: not on n_trial, j's position, the other orders, keep or the launcher's batches.  Two
 *                        calls agree bit for bit; there are no floating-point atomics
 *   totals of (e, j)     four doubles.  Order s enters when keep[s] != 0 and its n_used >= 2.  Over the entering
 *                        orders in ascending s, each sum starting at +0: sum loglike_s, sum m6_s, sum chi2_scaled_s and
 *                        sum n_used_s (a count held in a double).  With ratio(a, b) = NaN when b == 0, else fl(a / b):
 *                          chi2_scaled_s = fl(m5 - ratio(fl(m4 m4), m3))
 *                          sf = ratio(fl(m5 - ratio(fl(m2 m2), m0)), m0),  sg = ratio(fl(m3 - ratio(fl(m1 m1), m0)), m0)
 *                          c  = ratio(fl(m4 - ratio(fl(m1 m2), m0)), m0)
 *                          loglike_s = fl(fl(-0.5 n_used) ln(fl(fl(sf - fl(2 c)) + sg)))
 *                        which is observation.VelocityMap's loglike and chi2_scaled on the order's record, rounding for
 *                        rounding, so the logarithm's argument is numpy's bit for bit; ln is the device library's.  A
 *                        NaN (or infinite) statistic of an entering order makes that total NaN (or what IEEE gives):
 *                        nothing is hidden.  No entering order: zeros
 *   lumped outputs       mom_out, n_used_out and model_out are what the existing entry with the same filters returns
 *                        (prom_*_expose, _detrended, _highpass), bit for bit; without filters that holds for a model
 *                        without NaN from R, as k_model_moments promises */

/* Make the orders resident.  PROM_E_STATE without a resident exposure table; PROM_E_ARG when n_pix differs from the
 * observation's or a rule above is broken.  The host arrays are read during the call only.  prom_expose_set, and
 * whatever drops the exposure table, drops the orders (the calls below then fail with PROM_E_STATE). */
int32_t prom_orders_set(prom_ctx* ctx, int32_t n_pix, int32_t n_seg, const int32_t* seg_first, const int32_t* perm,
                        const uint8_t* keep);
/* The per-order moments over the last run's R on its stream.  highpass and detrend are 0 or 1 (otherwise PROM_E_ARG);
 * PROM_E_STATE without resident orders, with highpass = 1 without a resident high-pass and with detrend = 1 without a
 * resident filter.  Any output may be NULL: mom_out[n_exp][n_trial][7] and n_used_out[n_exp][n_trial] (lumped),
 * orec_mom_out[n_exp][n_trial][n_seg][7], orec_n_used_out[n_exp][n_trial][n_seg], tot_out[n_exp][n_trial][4],
 * model_out[n_exp][n_trial][n_pix] (the final model).  n_pix = 0 gives zeros.  The model of the whole table lies in
 * device memory at once: PROM_E_NOMEM when it does not fit (the remedy is fewer trials per call).  The records are
 * formed in batches of whole trial groups under the PROM_VMAP_SCRATCH_MB cap.  A workgroup of k_order_moments owns one
 * (exposure, trial group, order): n_exp n_seg >= 2^31 is PROM_E_ARG. */
int32_t prom_transit_expose_orders(prom_ctx* ctx, int32_t highpass, int32_t detrend, double* mom_out,
                                   int64_t* n_used_out, double* orec_mom_out, int64_t* orec_n_used_out, double* tot_out,
                                   double* model_out);
/* The same for a spectrum the caller supplies (the checks of prom_spectrum_expose). */
int32_t prom_spectrum_expose_orders(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                    int32_t highpass, int32_t detrend, double* mom_out, int64_t* n_used_out,
                                    double* orec_mom_out, int64_t* orec_n_used_out, double* tot_out, double* model_out);
/* Measurement aid (tools/order_bench.py), not for callers: ms_out[0] and ms_out[1] are the mean device durations in
 * milliseconds of k_order_moments and k_order_totals over the whole table (the first batch scaled by trial count), over
 * n_runs repetitions on the final model the last per-order call left.  PROM_E_STATE when there is no such call. */
int32_t prom_orders_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out);

/* ---- broadened spectra on the device ------------------------------------------------------------
 * The planet's own velocity field broadens and shifts every line before the instrument sees it: the rigid rotation of
 * a tidally locked planet (the terminator ring has a double-horned profile), a day-to-night wind (a net shift), an
 * east/west limb asymmetry; an instrument's measured line-spread function has the same form.  This stage convolves R,
 * as it lies in device memory after a run, with a tabulated velocity kernel on the model's own non-uniform grid into a
 * second buffer R_b, which then takes R's place as the input of the observe, velocity-map and expose calls with all
 * their options.  A velocity-space kernel commutes with every Doppler factor those stages apply, so one pass per model
 * evaluation serves all trials, taps, filters and orders.  All float64; every product, sum and difference is rounded
 * on its own (no fused multiply-add), and the roundings named here are part of the definition.
 *
 *   inputs               wav[n_wav] finite, ascending (duplicates allowed) and > 0 (1 / wav[0] must be finite);
 *                        R[n_orb][n_wav]; a kernel K[n_k], 2 <= n_k <= 1025, every entry finite and >= 0, not all
 *                        zero, whose nodes sit at the Doppler offsets beta_i = b0 + i / s, b0 finite, s finite and > 0
 *                        (nodes per unit beta).  K is piecewise linear between its nodes and zero outside them.
 *                        The host forms D[i] = fl(K[i + 1] - K[i]) once
 *   weights              q: the observation's trapezoid weights of the whole grid (both edges NaN,
 *                        q_w = fl(fl(hi - lo) / 2) with hi, lo the neighbours or the end point itself).  There are no
 *                        shard partials
 *   per output w         r = fl(1 / wav[w])
 *   per candidate w'     d = fl(wav[w'] - wav[w]), u = fl(d r), t = fl(fl(u - b0) s)
 *   support              w' belongs when 0 <= t <= n_k - 1 (float64, both ends inclusive).  t is non-decreasing in w',
 *                        so the support is one contiguous range
 *   kernel value         i = min(floor(t), n_k - 2), a = t - i (exact), kern = fl(K[i] + fl(a D[i])) (>= 0 by the
 *                        monotonicity of rounding), g = fl(kern q[w'])
 *   sums                 num[o] and den start at +0 and take their terms in ascending w':
 *                        num[o] = fl(num[o] + fl(g R[o][w'])), den = fl(den + g)
 *   result               R_b[o][w] = num[o] / den (IEEE); NaN when den == 0, which covers an empty support (a pure
 *                        shift kernel near an end of the grid)
 *   NaN                  a NaN in R[o] reaches exactly the outputs of row o whose support holds it, members of weight
 *                        zero included (0 NaN is NaN)
 *   ends of the grid     the support is simply cut there and den normalises it
 *   independence         R_b[o][w] depends on wav, R[o] and the kernel only: not on n_orb, the row's position, how rows
 *                        are grouped, tile boundaries or whether values came from LDS or global memory.  Two calls
 *                        agree bit for bit; there are no atomics
 *   meaning              R_b(lambda) ~ int K(beta) R(lambda (1 + beta)) d beta / int K.  Absorbers at line-of-sight
 *                        velocity v (positive: away from the observer) move a line to lambda (1 + v / c), so a velocity
 *                        distribution P(v) is the kernel K(beta) = P(-beta c), to first order in v / c: the shift's
 *                        error is (v / c)^2, about 1e-9 at 10 km/s */

/* Make the kernel resident (the host array is read during the call only); n_k = 0 drops it.  PROM_E_ARG when a rule
 * above is broken.  A new kernel, or none, ends the currency of a broadened spectrum (below). */
int32_t prom_broaden_set(prom_ctx* ctx, int32_t n_k, double b0, double s, const double* K);
/* The stage on a caller's spectrum: Rb_out[n_orb][n_wav].  PROM_E_STATE without a resident kernel; PROM_E_ARG for the
 * checks of prom_spectrum_observe's spectrum and for a wavelength that is not > 0. */
int32_t prom_spectrum_broaden(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                              double* Rb_out);
/* Form R_b from the last run's R on its stream; nothing crosses the bus and the call does not wait.  From then until
 * the next prom_transit_run, prom_transit_set, prom_transit_kernel_ms or prom_broaden_set, R_b is current:
 * prom_transit_observe, prom_transit_vmap and every prom_transit_expose* read R_b in R's place (nothing else about
 * them changes), while prom_transit_result and prom_transit_band_stats keep reading R.  prom_transit_observe with an
 * edge that is not NaN then returns PROM_E_ARG: the stage needs the whole grid.  The run's wavelengths must obey the
 * rules above (as for prom_transit_observe they are not checked again).  PROM_E_STATE without a resident kernel or a
 * completed run. */
int32_t prom_transit_broaden(prom_ctx* ctx);
/* Copy the current R_b out: Rb_out[n_orb][n_wav].  PROM_E_STATE when none is current. */
int32_t prom_transit_broadened(prom_ctx* ctx, double* Rb_out);
/* Measurement aid (tools/broaden_bench.py), not for callers: ms_out[0] is the mean device duration in milliseconds of
 * k_broaden over n_runs repetitions of the last broaden call's launch.  PROM_E_STATE when there is no such call. */
int32_t prom_broaden_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out);

/* ---- injection and SYSREM on the device ---------------------------------------------------------
 * To quote a detection significance or to measure how much signal the cleaning eats, a model is multiplied into the
 * RAW exposures at a chosen trial and strength, and the result is cleaned exactly as the real data were: the
 * high-pass along each order, then SYSREM.  That is one SYSREM per injection, so it runs here on the device: U and the
 * cleaned data come back, and the caller builds the exposure table and the filter of the recovery from them.  All
 * float64.  Every product, sum, quotient and square root is rounded on its own, there is no fused multiply-add, and
 * the order of every sum named here is part of the definition.
 *
 *   inputs               the resident observation and exposure table (prom_expose_set: n_exp, n_pix, ivar), resident
 *                        raw data raw[n_exp][n_pix] in the device's pixel order, any value allowed (NaN marks a bad
 *                        pixel), n_exp <= 4096; optionally the resident high-pass (prom_highpass_set); for an
 *                        injection a spectrum over the whole grid, a trial j and a finite scale
 *   injection            M[e][p] is prom_spectrum_expose's model_out[e][j][p], bit for bit (unfiltered; formed from
 *                        the broadened R while that is current).  D[e][p] = fl(raw fl(1 + fl(scale fl(M - 1)))) where
 *                        M is not NaN, and raw where M is NaN: a pixel outside the model carries no planet.  Without
 *                        an injection D = raw
 *   high-pass            on request (highpass = 1) D goes through the resident high-pass as the model of one trial
 *                        would, row by row, exactly as defined under "high-pass filtered exposures on the device"
 *   weights              w[e][p] = ivar[e][p] when ivar is finite and > 0 and D (after the high-pass) is finite, else
 *                        0.  r = D where w > 0, else +0
 *   column fit fit_c(a)  per pixel p, num and den start at +0; in ascending e, a term with w = 0 is skipped, the others
 *                        give num = fl(num + fl(fl(w r) a_e)) and den = fl(den + fl(w fl(a_e a_e))).
 *                        c_p = fl(num / den) when den > 0, else +0
 *   row fit fit_a(c)     per exposure e the terms fl(fl(w r) c_p) of num_e and fl(w fl(c_p c_p)) of den_e over the
 *                        pixels; a term with w = 0 adds nothing.  Both sums are added in one fixed shape, a function
 *                        of n_pix alone (not of n_exp, n_comp, any environment knob or the launch), with V = 2:
 *                          lane    the pixels are cut into groups of V consecutive pixels; a group's sum starts at +0
 *                                  and takes its terms in ascending p
 *                          tile    64 consecutive groups (a tile of T = 64 V = 128 pixels; the tail of the last tile
 *                                  is groups of +0) are t[0 .. 63]; for m = 1, 2, 4, 8, 16, 32 in turn every t[l]
 *                                  becomes fl(t[l] + t[l ^ m]) (all l at once), and t[0] is the tile's partial
 *                          row     64 sums s[0 .. 63] start at +0; s[l] adds the partials of the tiles l, l + 64,
 *                                  l + 128, ... in ascending order; the same butterfly over s gives the sum
 *                        a_e = fl(num_e / den_e) when den_e > 0, else +0.  Then norm = sqrt of the sum, from +0 in
 *                        ascending e, of fl(a_e a_e).  If norm > 0 is false the component ends: its column of U is +0
 *                        and r stays as it is.  Otherwise a_e = fl(a_e / norm)
 *   component            starts with a_e = fl(1 / sqrt(n_exp)) for every e and c = fit_c(a); n_iter times a = fit_a(c)
 *                        with its normalisation, then c = fit_c(a); then r[e][p] = fl(r - fl(a_e c_p)) where w > 0.
 *                        a is the component's column of U.  With ones, first a = 1, c = fit_c(a), the same
 *                        subtraction, and a leading column of ones in U.  0 <= n_comp, 1 <= n_comp + ones <= 16,
 *                        n_iter >= 1
 *   outputs              U[n_exp][n_comp + ones]; cleaned[e][p] = r where w > 0, else the value of D as it came; on
 *                        request injected[e][p] = D after the injection and the high-pass, before SYSREM
 *   independence         an entry with w = 0 influences nothing but its own returned value.  Two calls agree bit for
 *                        bit; there are no floating-point atomics.  The result of injecting trial j does not depend on
 *                        n_trial, on j's position or on the other trials.  raw and the exposure table's data are never
 *                        written
 *   no pixel             n_pix = 0: every component ends; U is zeros behind the column of ones, nothing else is written */

/* Make the raw exposures resident (the host array is read during the call only).  PROM_E_STATE without a resident
 * exposure table; PROM_E_ARG when n_exp or n_pix differs from the table's or n_exp > 4096.  prom_expose_set, and
 * whatever drops the exposure table, drops them (the calls below then fail with PROM_E_STATE). */
int32_t prom_sysrem_set(prom_ctx* ctx, int32_t n_exp, int32_t n_pix, const double* raw);
/* SYSREM of the raw exposures without an injection.  Each output may be NULL: U_out[n_exp][n_comp + ones],
 * cleaned_out[n_exp][n_pix], injected_out[n_exp][n_pix].  highpass and ones are 0 or 1; PROM_E_ARG for a broken range;
 * PROM_E_STATE without resident raw exposures and with highpass = 1 without a resident high-pass. */
int32_t prom_sysrem_clean(prom_ctx* ctx, int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out,
                          double* cleaned_out, double* injected_out);
/* The same after injecting trial `trial` of the last run's R (its broadened R_b while that is current) at `scale`, on
 * the run's stream.  PROM_E_ARG also for a trial outside [0, n_trial) and a scale that is not finite; PROM_E_STATE also
 * without a completed run or when the table has another n_orb. */
int32_t prom_transit_inject(prom_ctx* ctx, int32_t trial, double scale, int32_t highpass, int32_t n_comp, int32_t n_iter,
                            int32_t ones, double* U_out, double* cleaned_out, double* injected_out);
/* The same for a spectrum the caller supplies (the checks of prom_spectrum_expose). */
int32_t prom_spectrum_inject(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                             int32_t trial, double scale, int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones,
                             double* U_out, double* cleaned_out, double* injected_out);
/* Measurement aid (tools/sysrem_bench.py), not for callers: mean device durations in milliseconds over n_runs
 * repetitions of the last clean or inject call: ms_out[0] the SYSREM loop (weights, every fit, the cleaned data),
 * ms_out[1] the injection (the one-trial model and D; NaN for a clean call), ms_out[2] k_highpass (NaN without it).
 * PROM_E_STATE when there is no such call. */
int32_t prom_sysrem_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out);

/* ---- the filter's weights on the device ---------------------------------------------------------
 * W of "detrended exposures on the device" formed where the basis and the inverse variances already lie: per pixel p,
 * W_p = (U^T diag(v_p) U)^-1 U^T diag(v_p), by a Cholesky factorisation of the normal matrix.  All float64.  Every
 * product, sum, difference, quotient and square root is rounded on its own (fl), there is no fused multiply-add, and
 * the order of every sum named here is part of the definition; a plain numpy loop gives the same bits
 * (tests/helpers/filter_ref.py).
 *
 *   inputs               U[n_exp][K], finite, 1 <= K <= 16, n_exp >= 1; ivar[n_exp][n_pix], any value
 *   weights              v_e = ivar[e][p] when that is finite and > 0, else +0; cnt = the number of e with v_e > 0
 *   normal matrix        only the lower triangle i >= j is formed.  Every N_ij starts at +0; in ascending e an exposure
 *                        with v_e = 0 is skipped, the others give t = fl(v_e U[e][i]) and
 *                        N_ij = fl(N_ij + fl(t U[e][j]))
 *   tolerance            dmax starts at N_00 and takes, in ascending i, every N_ii > dmax;
 *                        tol = fl(fl(K 2^-52) dmax)
 *   Cholesky             for j = 0 .. K - 1 in order: s = N_jj, then for k = 0 .. j - 1 ascending
 *                        s = fl(s - fl(L_jk L_jk)).  The pixel is singular when cnt < K or when s > tol is false for
 *                        some j (NaN and an infinite dmax therefore count as singular).  L_jj = sqrt(s).  For i > j:
 *                        s' = N_ij, then for k ascending s' = fl(s' - fl(L_ik L_jk)), and L_ij = fl(s' / L_jj)
 *   solve                for every e with v_e > 0: forward, y_i = fl((fl(v_e U[e][i]) - sum) / L_ii) where the terms
 *                        fl(L_ik y_k), k = 0 .. i - 1 ascending, are subtracted one by one, each difference rounded;
 *                        backward for i = K - 1 .. 0, x_i = fl((y_i - sum) / L_ii) with the terms fl(L_ki x_k),
 *                        k = K - 1 .. i + 1 descending, subtracted the same way.  W[k][e][p] = x_k
 *   zeros                W[k][e][p] = +0 exactly for every k when v_e = 0.  A singular pixel has W = +0 throughout,
 *                        and so has a pixel any of whose x is not finite
 *   independence         a pixel's W depends on U and on that pixel's column of ivar only: not on n_pix, the pixel's
 *                        position or the launch.  Two calls agree bit for bit; there are no atomics
 *
 * This is the device's own rule.  The host's observation.filter_weights keeps its eigenvalue rule and its bits; on
 * pixels that are not borderline the two agree to rounding.  A zero column of U (a SYSREM component that ended) makes
 * N_p singular at every pixel, here exactly as on the host: W is +0 everywhere and the filter passes the model through. */

/* The definition on arrays the caller supplies (no table is needed): W_out[n_comp][n_exp][n_pix] from U[n_exp][n_comp]
 * and ivar[n_exp][n_pix].  PROM_E_ARG for n_comp outside [1, 16], n_exp < 1, n_pix < 0, a U entry that is not finite
 * or a missing array; n_pix = 0 writes nothing. */
int32_t prom_filter_weights(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, int32_t n_pix, const double* U,
                            const double* ivar, double* W_out);
/* Make the filter resident exactly as prom_detrend_set would with the W of the definition over the exposure table's
 * ivar; W is formed on the device and comes back in W_out[n_comp][n_exp][n_pix] unless that is NULL.  The checks and
 * states are prom_detrend_set's (there is no W to check), and every detrended, high-pass (detrend = 1) and per-order
 * (detrend = 1) call afterwards behaves as after prom_detrend_set with (U, W). */
int32_t prom_detrend_build(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, const double* U, double* W_out);
/* Measurement aid (tools/recover_bench.py), not for callers: ms_out[0] = the mean device duration in milliseconds over
 * n_runs repetitions of k_filter_weights as the last prom_detrend_build or recover call launched it.  PROM_E_STATE
 * when there is no such call. */
int32_t prom_filter_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out);

/* ---- recovery on the device ---------------------------------------------------------------------
 * An injection turned into the recovery's moments in one call: three steps on one stream, one wait at the end.
 *
 *   1  the steps of the inject call with the same arguments: the cleaned data C[n_exp][n_pix] and
 *      U[n_exp][n_comp + ones] stay in device memory
 *   2  W of (U, the table's ivar) by "the filter's weights on the device", in a buffer of the recovery's own: the
 *      resident filter of prom_detrend_set / prom_detrend_build is neither read nor replaced, and raw and the
 *      table's data are never written
 *   3  the whole table's model as the expose calls form it (from R_b while that is current); with highpass = 1 the
 *      resident high-pass over it; k_detrend with (U, W); the moments with C in the place of the table's data; with
 *      orders = 1 the per-order records and totals too
 *
 *   equivalence          every output equals, bit for bit, what prom_spectrum_expose_detrended, the high-pass call with
 *                        detrend = 1 or the per-order call with detrend = 1 returns on a table with the same pixels,
 *                        rows, weights, factors and ivar, with data = C and the filter set to (U, W)
 *   outputs              mom_out[n_exp][n_trial][7], n_used_out[n_exp][n_trial]; with orders = 1
 *                        orec_mom_out[n_exp][n_trial][n_seg][7], orec_n_used_out[n_exp][n_trial][n_seg] and
 *                        tot_out[n_exp][n_trial][4] (untouched with orders = 0); U_out[n_exp][n_comp + ones];
 *                        model_out[n_exp][n_trial][n_pix].  Any of them may be NULL
 *   errors               the union of the inject call's and the per-order call's; orders must be 0 or 1, and
 *                        orders = 1 without resident orders is PROM_E_STATE
 *   no pixel             n_pix = 0 gives zeros (and the U of the inject call)
 *   memory               the model of all trials is resident at once, as for the detrended calls: PROM_E_NOMEM with
 *                        the same remedy */
int32_t prom_transit_recover(prom_ctx* ctx, int32_t trial, double scale, int32_t highpass, int32_t n_comp,
                             int32_t n_iter, int32_t ones, int32_t orders, double* mom_out, int64_t* n_used_out,
                             double* orec_mom_out, int64_t* orec_n_used_out, double* tot_out, double* U_out,
                             double* model_out);
/* The same for a spectrum the caller supplies (the checks of prom_spectrum_expose). */
int32_t prom_spectrum_recover(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                              int32_t trial, double scale, int32_t highpass, int32_t n_comp, int32_t n_iter,
                              int32_t ones, int32_t orders, double* mom_out, int64_t* n_used_out,
                              double* orec_mom_out, int64_t* orec_n_used_out, double* tot_out, double* U_out,
                              double* model_out);

/* ---- injection grids on the device --------------------------------------------------------------
 * A list of n_inj injections, entry b = (trial[b], scale[b]), cleaned (the inject grid calls) or cleaned and recovered
 * (the recover grid calls) in one call: the injections of a grid are independent, so they share every launch.
 *
 *   equivalence          entry b of every output equals, bit for bit, NaN pattern and signs of zero included, what
 *                        prom_spectrum_inject / prom_spectrum_recover (prom_transit_* for the transit calls) returns
 *                        for (trial[b], scale[b]) with the same other arguments on the same context state
 *   independence         entry b does not depend on n_inj, on b's position, on the other entries (duplicates are
 *                        allowed) or on how the call cuts the list into sub-batches.  raw, the table's data and the
 *                        resident filter are never written or replaced
 *   steps                the factors of the listed trials as a table of B trials, k_expose unchanged over it,
 *                        D[b] from raw, that model and scale[b]; the resident high-pass over the B n_exp rows; SYSREM
 *                        with the injection as a grid dimension of every launch: 2 + n_cols + n_comp (2 n_iter + 1)
 *                        launches per sub-batch, not per injection; a component that ends stops its own injection
 *                        alone.  A recover grid call forms and high-passes the model of all trials once per call,
 *                        forms W of every (U[b], ivar) in one launch, and per injection filters the model out of place
 *                        into a second buffer and takes the moments (with orders = 1 also the totals) against
 *                        cleaned[b]
 *   outputs              inject grid: U_out[n_inj][n_exp][n_comp + ones], cleaned_out[n_inj][n_exp][n_pix],
 *                        injected_out[n_inj][n_exp][n_pix].  recover grid: mom_out[n_inj][n_exp][n_trial][7],
 *                        n_used_out[n_inj][n_exp][n_trial], tot_out[n_inj][n_exp][n_trial][4] (untouched with
 *                        orders = 0), U_out[n_inj][n_exp][n_comp + ones].  Any of them may be NULL.  The per-order
 *                        records and the final model are not part of the grid calls: prom_*_recover gives them for one
 *                        point
 *   errors               the single calls', before anything is launched; PROM_E_ARG also for n_inj < 0, a missing
 *                        trial or scale array with n_inj > 0, a trial outside [0, n_trial) or a scale that is not
 *                        finite (the message names the entry), and a sub-batch too large for one launch of k_highpass
 *   empty                n_inj = 0 writes nothing and succeeds; n_pix = 0 gives per entry what the single calls give
 *   sub-batches          per injection the work buffers take about (5 + n_cols for a recovery) n_exp n_pix 8 bytes.
 *                        The list is cut into sub-batches of as many injections as fit PROM_GRID_SCRATCH_MB megabytes
 *                        (fractions allowed; default 4096), one at least and 65,535 at most; the variable is read
 *                        from the environment at every grid call.  Each sub-batch's outputs are copied to the caller's
 *                        arrays and the stream waits before the next one reuses the buffers
 *   memory               a recover grid call keeps the unfiltered and one filtered model of all trials, twice the
 *                        recover call's n_exp n_trial n_pix 8 bytes: PROM_E_NOMEM with the same remedy
 *   afterwards           the work buffers hold the last sub-batch, so prom_sysrem_kernel_ms has no call to repeat and
 *                        fails with PROM_E_STATE, as prom_filter_kernel_ms does unless a prom_detrend_build came last;
 *                        the aids of the expose calls have nothing to repeat after a recover grid call */
int32_t prom_transit_inject_grid(prom_ctx* ctx, int32_t n_inj, const int32_t* trial, const double* scale,
                                 int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out,
                                 double* cleaned_out, double* injected_out);
/* The same for a spectrum the caller supplies (the checks of prom_spectrum_expose). */
int32_t prom_spectrum_inject_grid(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                  int32_t n_inj, const int32_t* trial, const double* scale, int32_t highpass,
                                  int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out, double* cleaned_out,
                                  double* injected_out);
/* The recovery of every entry, on the last run's R (its broadened R_b while that is current). */
int32_t prom_transit_recover_grid(prom_ctx* ctx, int32_t n_inj, const int32_t* trial, const double* scale,
                                  int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, int32_t orders,
                                  double* mom_out, int64_t* n_used_out, double* tot_out, double* U_out);
/* The same for a spectrum the caller supplies (the checks of prom_spectrum_expose). */
int32_t prom_spectrum_recover_grid(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                   int32_t n_inj, const int32_t* trial, const double* scale, int32_t highpass,
                                   int32_t n_comp, int32_t n_iter, int32_t ones, int32_t orders, double* mom_out,
                                   int64_t* n_used_out, double* tot_out, double* U_out);

/* ---- SYSREM per order on the device ---------------------------------------------------------------
 * Every high-resolution pipeline runs SYSREM one echelle order at a time: each order has its own telluric and blaze
 * systematics and so its own basis U.  The calls here clean every resident order on its own in the launches of ONE
 * single call: an order is one more batch item of the SYSREM kernels, as an injection is in the grids.
 *
 *   orders               the resident orders of prom_orders_set (n_seg, seg_first, perm) cut the pixels into orders.
 *                        keep plays no part: every order is cleaned.  Order s has n_s = seg_first[s + 1] - seg_first[s]
 *                        positions, in the order perm gives them
 *   injection, high-pass D, the optional resident high-pass of D and `injected` are exactly what the single call forms
 *                        ("injection and SYSREM on the device").  They are not per order: the high-pass keeps its own
 *                        segments
 *   SYSREM per order     for order s the weights, fit_c, fit_a, the norm, ended components and the subtraction are the
 *                        single call's definition, word for word, on the table whose columns are the pixels
 *                        perm[seg_first[s] + i], i = 0 .. n_s - 1, with n_pix = n_s.  In particular the shape of a
 *                        row sum is a function of n_s alone
 *   outputs              U_out[n_seg][n_exp][n_comp + ones] (a leading [n_inj] for the grids); cleaned[e][p] comes
 *                        from p's own order; injected as the single call's
 *   independence         order s's numbers do not depend on the other orders, on n_seg or on where s sits.  A
 *                        component that ends in one order ends there alone.  With one order and the identity perm
 *                        everything equals the single call bit for bit
 *   layout               batch item y = b n_seg + s of the work buffers is order s of injection b; every item is
 *                        n_max = max n_s wide.  Padding an order from n_s to n_max appends groups and tiles whose sums
 *                        are +0; every sum starts at +0 and so is never -0, and adding +0 leaves its bits: the padded
 *                        item's row sums are the single call's on n_s pixels.  Unequal orders pay for the padding
 *                        (echelle orders have equal pixel counts); there is no compacted layout
 *   launches             those of one single call, 2 + n_cols + n_comp (2 n_iter + 1), whatever n_seg
 *   errors               the namesake's, and PROM_E_STATE without resident orders; PROM_E_ARG for more than 65,535
 *                        orders
 *   sub-batches (grids)  as the grids', with the per-injection bytes of n_seg items n_max wide, and
 *                        n_inj_sub n_seg <= 65,535
 *   no pixel             n_pix = 0: U is zeros behind the column of ones for the one order
 *   afterwards           prom_sysrem_kernel_ms repeats a per-order clean or inject call as it repeats the single ones */
int32_t prom_sysrem_clean_orders(prom_ctx* ctx, int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones,
                                 double* U_out, double* cleaned_out, double* injected_out);
int32_t prom_transit_inject_orders(prom_ctx* ctx, int32_t trial, double scale, int32_t highpass, int32_t n_comp,
                                   int32_t n_iter, int32_t ones, double* U_out, double* cleaned_out,
                                   double* injected_out);
int32_t prom_spectrum_inject_orders(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                    int32_t trial, double scale, int32_t highpass, int32_t n_comp, int32_t n_iter,
                                    int32_t ones, double* U_out, double* cleaned_out, double* injected_out);
int32_t prom_transit_inject_grid_orders(prom_ctx* ctx, int32_t n_inj, const int32_t* trial, const double* scale,
                                        int32_t highpass, int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out,
                                        double* cleaned_out, double* injected_out);
int32_t prom_spectrum_inject_grid_orders(prom_ctx* ctx, int32_t n_orb, int64_t n_wav, const double* wav, const double* R,
                                         int32_t n_inj, const int32_t* trial, const double* scale, int32_t highpass,
                                         int32_t n_comp, int32_t n_iter, int32_t ones, double* U_out,
                                         double* cleaned_out, double* injected_out);

/* The filter per order.  The filter is given U[n_seg][n_exp][K], a basis per order, and seg_of[n_pix], the order of
 * every device pixel (0 <= seg_of[p] < n_seg).
 *
 *   weights              at pixel p of order s, W[.][.][p] is "the filter's weights on the device" with U_s: a pixel's
 *                        bits equal the single-basis call given U_s
 *   filtered model       M' at p is "detrended exposures on the device" (the coefficients W_p M, then M - U c) with
 *                        U_s, bit for bit
 *   kernels              the existing function text with the U pointer moved per lane by seg_of[p] n_exp K; U is then a
 *                        vector load, no longer a scalar one.  No instantiation uses scratch (profiles/)
 *   resident filter      prom_detrend_set_orders / prom_detrend_build_orders make a per-order filter resident for the
 *                        resident orders: seg_of is formed from their perm at that moment.  After them every
 *                        detrended, high-pass (detrend = 1) and per-order-moments (detrend = 1) call filters with it.
 *                        prom_detrend_set or prom_detrend_build puts a single basis back; prom_orders_set drops a
 *                        per-order filter (the calls that need one then fail with PROM_E_STATE), and so does whatever
 *                        drops the exposure table
 *   errors               those of the single-basis namesakes; PROM_E_STATE without resident orders; PROM_E_ARG when
 *                        n_seg differs from the resident orders' or seg_of leaves [0, n_seg) */

/* The definition on arrays the caller supplies (no table is needed): W_out[n_comp][n_exp][n_pix]. */
int32_t prom_filter_weights_orders(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, int32_t n_pix, int32_t n_seg,
                                   const int32_t* seg_of, const double* U, const double* ivar, double* W_out);
/* Make the per-order filter (U[n_seg][n_exp][n_comp], W[n_comp][n_exp][n_pix]) resident. */
int32_t prom_detrend_set_orders(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, int32_t n_seg, const double* U,
                                const double* W);
/* The same with W formed on the device over the table's ivar; it comes back in W_out unless that is NULL. */
int32_t prom_detrend_build_orders(prom_ctx* ctx, int32_t n_exp, int32_t n_comp, int32_t n_seg, const double* U,
                                  double* W_out);

/* Per-kernel device durations of the transit path (ABI 5; ids 5 and 6 since ABI 6): n_runs runs of the current problem, one at a
 * time (one slot, no second stream; the stream waits after every run), each kernel timed by start/stop
 * events on its own dispatch packet (groups of kernels: the first start to the last stop).  ms_out[k] is
 * the mean duration in milliseconds of kernel k (prom_kernel_id), NaN when the path does not launch it.
 * What rocprofv3 --kernel-trace reports for one slot in flight; measurement aid for bench.py. */
enum prom_kernel_id {
  PROM_K_COLUMNS = 0,   /* densities, column densities and culling: k_columns8 (atomic paths); k_ntot +
                           k_mol_prep + k_columns (molecular and generic paths)                        */
  PROM_K_SIGMA = 1,     /* Doppler cross-section rows of the windowed paths: k_sigma_poly / k_sigma_rows */
  PROM_K_ORDER = 2,     /* per-phase chord ordering: k_order (windowed paths), k_chords (generic and
                           molecular paths)                                                            */
  PROM_K_WINDOWS = 3,   /* tile windows and heavy-entry lists: k_windows (planned windowed path)        */
  PROM_K_TAU = 4,       /* the integration kernel: k_tau / k_tau_w / k_tau_p / k_tau_rm / k_mol_list +
                           k_tau_mol                                                                   */
  PROM_K_TC_BUILD = 5,  /* transmission-curve path: every phase's curve T_o, k_tc_build                 */
  PROM_K_SIGMA_TC = 6,  /* transmission-curve path: sigma at each phase's Doppler shift and R = T_o(Y),
                           k_sigma_tc                                                                  */
  PROM_K_COUNT = 7      /* length of prom_transit_kernel_ms's ms_out                                   */
};
int32_t prom_transit_kernel_ms(prom_ctx* ctx, int32_t n_runs, double* ms_out);

/* Disk-integrated stellar flux of a rotating star (ABI 5).  Replaces the rotating branch of
 * Star.getFstarIntegrated (celestialBodies.py:299-311, through calculateRM :226-240 and calculateCLV
 * :212-224): for every wavelength, the n_cells disk cells in the reference's loop order (phi outer, rho
 * inner) are accumulated one after the other,
 *   out[w] += (((10^interp(wavelength[w] / shift[c]) * clv[c]) * dphi) * drho) * rho[c],
 * interp = numpy.interp over the star table (offset 0).  The caller gives each cell's Doppler factor
 * (calculateDopplerShift of the surface velocity) and CLV factor.  A target outside the table is an
 * error (PROM_E_ARG), as the reference's interp1d(bounds_error=True) raises. */
int32_t prom_star_disk_flux(prom_ctx* ctx, int32_t star_table, int32_t n_cells, const double* shift,
                            const double* clv, const double* rho, double dphi, double drho, int64_t n_wav,
                            const double* wavelength, double* out);

/* Live per-run timing of the tau kernel without per-run synchronisation: between prom_timing_begin
 * and prom_timing_end every timed prom_transit_run carries a HIP event pair (the ordering kernel's
 * completion -> the tau kernel's completion) and, for the planned tau kernel k_tau_p, device-clock
 * stamps of its workgroups; prom_timing_end waits for them and returns ms[run][4] =
 * {NaN, NaN, tau_events, tau_device} for up to max_runs runs (n_runs receives the count).
 * tau_events includes the tau kernel's dispatch behind the ordering kernel; tau_device is the span
 * from its first workgroup's start to its last workgroup's end (NaN for other tau kernels).  Stage times of a single run come from prom_transit_run's stats.
 * prom_timing_stride(ctx, k) (k >= 1, default 1, kept until changed) times only every k-th run of the
 * window: events on a dispatch cost the host ~13 us, more than a run's GPU time, so a throughput
 * measurement samples the kernel durations instead of timing every run. */
int32_t prom_timing_begin(prom_ctx* ctx);
int32_t prom_timing_end(prom_ctx* ctx, int32_t max_runs, double* ms, int32_t* n_runs);
int32_t prom_timing_stride(prom_ctx* ctx, int32_t stride);

#ifdef __cplusplus
}
#endif

#endif /* PROM_HIP_H */
