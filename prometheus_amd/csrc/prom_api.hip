// C-ABI layer of libprom_hip.so (declared in include/prom_hip.h).  Host code only: argument checks,
// device memory owned by the context, H2D/D2H copies and kernel launches on the context's stream.  Here: the context,
// the pinned pool, tables, densities, the stellar disk and timing (the transit entries: prom_api_transit.hip).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <exception>
#include <map>
#include <mutex>

#include "prom_api_shared.h"

namespace {

// Table slots: an upload takes the lowest free slot (freed ids are reused), so a loop that builds and
// drops tables keeps the context's device memory flat.
template <class T>
int32_t store_table(std::vector<T>& v, T&& t) {
  t.live = true;
  for (size_t i = 0; i < v.size(); ++i)
    if (!v[i].live) {
      v[i] = std::move(t);
      return (int32_t)i;
    }
  v.push_back(std::move(t));
  return (int32_t)v.size() - 1;
}

// Pinned host pool behind prom_host_alloc / prom_host_free: buffers keyed by address, each either in use
// or cached for reuse; the total (in use + cached) stays under the cap, idle buffers are released first
struct PinnedPool {
  struct Buf {
    size_t cap;
    bool used;
  };
  std::mutex mu;
  std::map<char*, Buf> bufs;
  size_t total = 0;
  size_t cap_bytes() const {
    const char* e = std::getenv("PROM_PINNED_CAP_MB");
    const long long mb = e ? std::atoll(e) : 4096;
    return (size_t)std::max(0LL, mb) << 20;
  }
  // in-use buffer holding [p, p + n)
  bool holds(const void* p, size_t n) {
    std::lock_guard<std::mutex> g(mu);
    const char* c = static_cast<const char*>(p);
    auto it = bufs.upper_bound(const_cast<char*>(c));
    if (it == bufs.begin()) return false;
    --it;
    return it->second.used && c >= it->first && c + n <= it->first + it->second.cap;
  }
};

PinnedPool& pinned_pool() {
  static PinnedPool* pool = new PinnedPool();   // never destroyed: buffers may outlive static teardown
  return *pool;
}

}  // namespace

bool prom::pinned_holds(const void* p, size_t n) { return pinned_pool().holds(p, n); }

extern "C" {

int32_t prom_host_alloc(int64_t bytes, void** out) {
  if (!out || bytes < 0) return PROM_E_ARG;
  *out = nullptr;
  PinnedPool& pp = pinned_pool();
  const size_t want = std::max<size_t>(((size_t)bytes + ((size_t)1 << 21) - 1) & ~(((size_t)1 << 21) - 1),
                                       (size_t)1 << 21);
  std::lock_guard<std::mutex> g(pp.mu);
  char* best = nullptr;
  for (auto& kv : pp.bufs)
    if (!kv.second.used && kv.second.cap >= want && kv.second.cap <= 2 * want &&
        (!best || kv.second.cap < pp.bufs[best].cap))
      best = kv.first;
  if (best) {
    pp.bufs[best].used = true;
    *out = best;
    return PROM_OK;
  }
  const size_t cap = pp.cap_bytes();
  for (auto it = pp.bufs.begin(); pp.total + want > cap && it != pp.bufs.end();) {
    if (!it->second.used) {
      (void)hipHostFree(it->first);
      pp.total -= it->second.cap;
      it = pp.bufs.erase(it);
    } else {
      ++it;
    }
  }
  if (pp.total + want > cap) return PROM_E_NOMEM;
  void* p = nullptr;
  if (hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess || !p) return PROM_E_NOMEM;
  pp.bufs[static_cast<char*>(p)] = PinnedPool::Buf{want, true};
  pp.total += want;
  *out = p;
  return PROM_OK;
}

int32_t prom_host_free(void* p) {
  PinnedPool& pp = pinned_pool();
  std::lock_guard<std::mutex> g(pp.mu);
  auto it = pp.bufs.find(static_cast<char*>(p));
  if (!p || it == pp.bufs.end() || !it->second.used) return PROM_E_ARG;
  it->second.used = false;
  return PROM_OK;
}

int32_t prom_abi_version(void) { return PROM_ABI_VERSION; }

int32_t prom_device_count(int32_t* count) {
  if (!count) return PROM_E_ARG;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return PROM_OK;
}

int32_t prom_create(int32_t device, prom_ctx** out) {
  if (!out) return PROM_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return PROM_E_HIP;
  prom_ctx* ctx = new (std::nothrow) prom_ctx();
  if (!ctx) return PROM_E_NOMEM;
  ctx->device = device;
  bool ok = hipSetDevice(device) == hipSuccess;
  for (int i = 0; ok && i < prom::kMaxSlots; ++i)
    ok = hipStreamCreateWithFlags(&ctx->streams[i], hipStreamNonBlocking) == hipSuccess;
  ctx->stream = ctx->streams[0];
  if (const char* e = std::getenv("PROM_PIPELINE")) ctx->pipeline = std::max(1, std::min(prom::kMaxSlots, std::atoi(e)));
  // (megabytes, fractions allowed; a map that needs more runs in batches of whole trial groups, one group at least)
  if (const char* e = std::getenv("PROM_VMAP_SCRATCH_MB")) {
    const double mb = std::atof(e);
    if (mb > 0.0 && mb < 1.0e6) ctx->vmap_scratch_bytes = std::max<int64_t>(1, (int64_t)(mb * 1048576.0));
  }
  if (!ok) {
    delete ctx;
    return PROM_E_HIP;
  }
  for (int i = 0; i < prom::kMaxSlots; ++i) {
    if (hipEventCreateWithFlags(&ctx->fork_ev[i], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->join_ev[i], hipEventDisableTiming) != hipSuccess) {
      prom_destroy(ctx);
      return PROM_E_HIP;
    }
  }
  for (auto& e : ctx->ev) {
    if (hipEventCreate(&e) != hipSuccess) {
      delete ctx;
      return PROM_E_HIP;
    }
  }

  *out = ctx;
  return PROM_OK;
}

void prom_destroy(prom_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto st : ctx->streams)
    if (st) (void)hipStreamSynchronize(st);
  drop_graphs(ctx->tr);
  for (auto& e : ctx->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : ctx->tev) (void)hipEventDestroy(e);
  for (auto& e : ctx->pin_ev) (void)hipEventDestroy(e);
  for (int i = 0; i < prom::kMaxSlots; ++i) {
    if (ctx->fork_ev[i]) (void)hipEventDestroy(ctx->fork_ev[i]);
    if (ctx->join_ev[i]) (void)hipEventDestroy(ctx->join_ev[i]);
  }
  if (ctx->pin) (void)hipHostFree(ctx->pin);
  if (ctx->upin) (void)hipHostFree(ctx->upin);
  for (auto& st : ctx->streams)
    if (st) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
    }
  delete ctx;  // DevBuf destructors free device memory
}

const char* prom_last_error(const prom_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int32_t prom_synchronize(prom_ctx* ctx) {
  return guarded(ctx, [&] {
    for (auto st : ctx->streams) PROM_HIP(hipStreamSynchronize(st));
  });
}

// ------------------------------------------------------------------------------ tables
// Bucket directory of a table's nodes: n_dir = 4 n equal buckets over [x0, x[n-1]], dir[j] = number of
// nodes <= x0 + j h.  The tau kernel starts its np.interp bracket search from buckets j, j+1 of a
// target and verifies the bracket, so rounding in j only costs steps, never correctness.
static void build_directory(prom_ctx* ctx, prom::AtomTable& t, const double* x, int64_t n) {
  const int64_t nd = std::max<int64_t>(1, std::min<int64_t>(4 * n, (int64_t)1 << 26));
  const double x0 = x[0], span = x[n - 1] - x[0];
  std::vector<int32_t> d(nd + 1);
  const double h = span > 0.0 ? span / (double)nd : 1.0;
  for (int64_t j = 0; j <= nd; ++j) {
    const double b = x0 + (double)j * h;
    d[j] = (int32_t)(std::upper_bound(x, x + n, b) - x);
  }
  upload(t.dir, d.data(), nd + 1, ctx->stream);
  t.rec.ensure(sizeof(double4) * n);
  ctx->scratch[5].ensure(sizeof(double) * std::max<int64_t>(n, 1));
  ctx->scratch[4].ensure(sizeof(double) * 1024);
  prom::launch_table_recs(ctx->stream, t.x.as<double>(), t.y.as<double>(), n, t.rec.as<double4>(),
                          ctx->scratch[5].as<double>());
  t.amax = prom::reduce_max(ctx->stream, ctx->scratch[5].as<double>(), n, ctx->scratch[4].as<double>());
  t.hx.assign(x, x + n);
  t.n_dir = (int32_t)nd;
  t.dir_x0 = x0;
  t.dir_inv_h = span > 0.0 ? 1.0 / h : 0.0;
}

int32_t prom_table_upload(prom_ctx* ctx, int64_t n, const double* x, const double* log_sigma,
                          double offset, int32_t* table_id) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(n >= 1 && x && log_sigma && table_id, "prom_table_upload: bad arguments");
    PROM_REQUIRE(n < ((int64_t)1 << 31), "prom_table_upload: more than 2^31 - 1 nodes");
    for (int64_t i = 1; i < n; ++i) PROM_REQUIRE(!(x[i] < x[i - 1]), "prom_table_upload: x must be non-decreasing");
    prom::AtomTable t;
    upload(t.x, x, n, ctx->stream);
    upload(t.y, log_sigma, n, ctx->stream);
    t.n = n;
    t.offset = offset;
    double m = -INFINITY;
    for (int64_t i = 0; i < n; ++i) m = std::max(m, log_sigma[i]);
    t.ymax = m;
    build_directory(ctx, t, x, n);
    PROM_HIP(hipStreamSynchronize(ctx->stream));
    t.gen = ++ctx->table_gen;
    *table_id = store_table(ctx->tables, std::move(t));
  });
}

static void voigt_common(prom_ctx* ctx, int64_t n, const double* x, int32_t n_lines, const double* lw,
                         const double* lg, const double* lc, DevBuf& dx) {
  PROM_REQUIRE(n >= 0 && (n == 0 || x) && n_lines >= 0 && (n_lines == 0 || (lw && lg && lc)),
               "voigt: bad arguments");
  upload(dx, x, n, ctx->stream);
  upload(ctx->scratch[1], lw, n_lines, ctx->stream);
  upload(ctx->scratch[2], lg, n_lines, ctx->stream);
  upload(ctx->scratch[3], lc, n_lines, ctx->stream);
}

int32_t prom_table_build_voigt(prom_ctx* ctx, int64_t n, const double* x, int32_t n_lines,
                               const double* line_wavelength, const double* line_gamma,
                               const double* line_coef, double sigma_v, double c_light,
                               double offset, int32_t* table_id, double* log_sigma_out) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(n >= 1 && table_id, "prom_table_build_voigt: bad arguments");
    PROM_REQUIRE(n < ((int64_t)1 << 31), "prom_table_build_voigt: more than 2^31 - 1 nodes");
    for (int64_t i = 1; i < n; ++i) PROM_REQUIRE(!(x[i] < x[i - 1]), "prom_table_build_voigt: x must be non-decreasing");
    prom::AtomTable t;
    voigt_common(ctx, n, x, n_lines, line_wavelength, line_gamma, line_coef, t.x);
    t.y.ensure(sizeof(double) * n);
    prom::launch_voigt(ctx->stream, t.x.as<double>(), n, ctx->scratch[1].as<double>(),
                       ctx->scratch[2].as<double>(), ctx->scratch[3].as<double>(), n_lines, sigma_v, c_light,
                       offset, 1, t.y.as<double>());
    ctx->scratch[4].ensure(sizeof(double) * 1024);
    t.ymax = prom::reduce_max(ctx->stream, t.y.as<double>(), n, ctx->scratch[4].as<double>());
    t.n = n;
    t.offset = offset;
    build_directory(ctx, t, x, n);
    PROM_HIP(hipStreamSynchronize(ctx->stream));
    if (log_sigma_out) {
      download(log_sigma_out, t.y, n, ctx->stream);
      PROM_HIP(hipStreamSynchronize(ctx->stream));
    }
    t.gen = ++ctx->table_gen;
    *table_id = store_table(ctx->tables, std::move(t));
  });
}

int32_t prom_voigt_sigma(prom_ctx* ctx, int64_t n, const double* x, int32_t n_lines,
                         const double* line_wavelength, const double* line_gamma,
                         const double* line_coef, double sigma_v, double c_light, double* sigma_out) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(sigma_out || n == 0, "prom_voigt_sigma: bad arguments");
    voigt_common(ctx, n, x, n_lines, line_wavelength, line_gamma, line_coef, ctx->scratch[0]);
    ctx->scratch[4].ensure(sizeof(double) * std::max<int64_t>(n, 1));
    prom::launch_voigt(ctx->stream, ctx->scratch[0].as<double>(), n, ctx->scratch[1].as<double>(),
                       ctx->scratch[2].as<double>(), ctx->scratch[3].as<double>(), n_lines, sigma_v, c_light,
                       0.0, 0, ctx->scratch[4].as<double>());
    download(sigma_out, ctx->scratch[4], n, ctx->stream);
    PROM_HIP(hipStreamSynchronize(ctx->stream));
  });
}

int32_t prom_table_lookup(prom_ctx* ctx, int32_t table_id, int64_t n_targets, const double* targets,
                          double* out) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(table_ok(ctx->tables, table_id), "prom_table_lookup: unknown table");
    PROM_REQUIRE(n_targets >= 0 && (n_targets == 0 || (targets && out)), "prom_table_lookup: bad arguments");
    const prom::AtomTable& t = ctx->tables[table_id];
    upload(ctx->scratch[0], targets, n_targets, ctx->stream);
    ctx->scratch[1].ensure(sizeof(double) * std::max<int64_t>(n_targets, 1));
    prom::launch_table_lookup(ctx->stream, t.x.as<double>(), t.y.as<double>(), t.n, t.offset,
                              ctx->scratch[0].as<double>(), n_targets, ctx->scratch[1].as<double>());
    download(out, ctx->scratch[1], n_targets, ctx->stream);
    PROM_HIP(hipStreamSynchronize(ctx->stream));
  });
}

// A freed table's memory goes back to the device; a transit problem that reads it is invalidated.
static void free_table(prom_ctx* ctx, bool molecular, int32_t id) {
  for (auto st : ctx->streams) PROM_HIP(hipStreamSynchronize(st));   // runs in flight may read it
  prom::TransitDev& tr = ctx->tr;
  bool used = !molecular && tr.star && tr.star_table_id == id;
  for (const auto& t : tr.terms)
    if ((t.is_molecule != 0) == molecular && t.table == id) used = true;
  if (used) {
    drop_graphs(tr);
    tr.ready = false;
    tr.ran = false;
  }
  if (molecular) ctx->mtables[id] = prom::MolTable{};
  else ctx->tables[id] = prom::AtomTable{};
}

int32_t prom_table_free(prom_ctx* ctx, int32_t table_id) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(table_ok(ctx->tables, table_id), "prom_table_free: unknown table");
    free_table(ctx, false, table_id);
  });
}

int32_t prom_molecular_free(prom_ctx* ctx, int32_t table_id) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(table_ok(ctx->mtables, table_id), "prom_molecular_free: unknown table");
    free_table(ctx, true, table_id);
  });
}

int32_t prom_table_count(prom_ctx* ctx, int32_t* n_atomic, int32_t* n_molecular, int64_t* device_bytes) {
  return guarded(ctx, [&] {
    int32_t a = 0, m = 0;
    int64_t b = 0;
    for (const auto& t : ctx->tables)
      if (t.live) {
        ++a;
        b += (int64_t)(t.x.cap + t.y.cap + t.dir.cap + t.rec.cap);
      }
    for (const auto& t : ctx->mtables)
      if (t.live) {
        ++m;
        b += (int64_t)(t.P.cap + t.T.cap + t.W.cap + t.V.cap);
      }
    if (n_atomic) *n_atomic = a;
    if (n_molecular) *n_molecular = m;
    if (device_bytes) *device_bytes = b;
  });
}

// ------------------------------------------------------------------------------ molecular
int32_t prom_molecular_upload(prom_ctx* ctx, int32_t n_p, const double* P, int32_t n_t, const double* T,
                              int64_t n_w, const double* wavelength, const double* log_sigma,
                              double offset, int32_t* table_id) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(n_p >= 2 && n_t >= 2 && n_w >= 2 && P && T && wavelength && log_sigma && table_id,
                 "prom_molecular_upload: bad arguments (each axis needs >= 2 nodes)");
    prom::MolTable t;
    upload(t.P, P, n_p, ctx->stream);
    upload(t.T, T, n_t, ctx->stream);
    upload(t.W, wavelength, n_w, ctx->stream);
    const int64_t nv = (int64_t)n_p * n_t * n_w;
    upload(t.V, log_sigma, nv, ctx->stream);
    t.n_p = n_p;
    t.n_t = n_t;
    t.n_w = n_w;
    t.offset = offset;
    double m = -INFINITY;
    for (int64_t i = 0; i < nv; ++i) m = std::max(m, log_sigma[i]);
    t.vmax = m;
    PROM_HIP(hipStreamSynchronize(ctx->stream));
    *table_id = store_table(ctx->mtables, std::move(t));
  });
}

int32_t prom_molecular_sigma(prom_ctx* ctx, int32_t table_id, int64_t n_chords, int32_t n_x,
                             const double* P, double T, int64_t n_wav, const double* wavelength,
                             double* sigma_out) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(table_ok(ctx->mtables, table_id), "prom_molecular_sigma: unknown table");
    PROM_REQUIRE(n_chords >= 0 && n_x >= 0 && n_wav >= 0, "prom_molecular_sigma: bad sizes");
    const int64_t tot = n_chords * n_x * n_wav;
    upload(ctx->scratch[0], P, n_chords * n_x, ctx->stream);
    upload(ctx->scratch[1], wavelength, n_chords * n_wav, ctx->stream);
    ctx->scratch[2].ensure(sizeof(double) * std::max<int64_t>(tot, 1));
    prom::launch_molecular_sigma(ctx->stream, ctx->mtables[table_id], n_chords, n_x, ctx->scratch[0].as<double>(),
                                 T, n_wav, ctx->scratch[1].as<double>(), ctx->scratch[2].as<double>());
    download(sigma_out, ctx->scratch[2], tot, ctx->stream);
    PROM_HIP(hipStreamSynchronize(ctx->stream));
  });
}

// ------------------------------------------------------------------------------ density
int32_t prom_number_density(prom_ctx* ctx, const prom_density_model* model, int32_t n_x, const double* x,
                            int64_t n_chords, const double* y, const double* z, const double* body_x,
                            const double* body_y, double* n_out) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(model && valid_kind(model->kind) && model->kind != PROM_DENSITY_TABULATED &&
                     model->kind != PROM_DENSITY_GRIDDED,
                 "prom_number_density: unknown, tabulated or gridded density kind (gridded: prom_gridded_density)");
    PROM_REQUIRE(n_x >= 0 && n_chords >= 0, "prom_number_density: bad sizes");
    upload(ctx->scratch[0], x, n_x, ctx->stream);
    upload(ctx->scratch[1], y, n_chords, ctx->stream);
    upload(ctx->scratch[2], z, n_chords, ctx->stream);
    upload(ctx->scratch[3], body_x, n_chords, ctx->stream);
    upload(ctx->scratch[4], body_y, n_chords, ctx->stream);
    ctx->scratch[5].ensure(sizeof(double) * std::max<int64_t>(n_chords * n_x, 1));
    prom::launch_density(ctx->stream, to_dev(*model), ctx->scratch[0].as<double>(), n_x,
                         ctx->scratch[1].as<double>(), ctx->scratch[2].as<double>(), ctx->scratch[3].as<double>(),
                         ctx->scratch[4].as<double>(), n_chords, ctx->scratch[5].as<double>());
    download(n_out, ctx->scratch[5], n_chords * n_x, ctx->stream);
    PROM_HIP(hipStreamSynchronize(ctx->stream));
  });
}

int32_t prom_gridded_density(prom_ctx* ctx, int32_t n_gx, const double* gx, int32_t n_gy, const double* gy,
                             int32_t n_gz, const double* gz, const double* values, int64_t n_points,
                             const double* px, const double* py, const double* pz, double* out) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(n_gx >= 2 && n_gy >= 2 && n_gz >= 2 && gx && gy && gz && values,
                 "prom_gridded_density: need >= 2 nodes per axis");
    PROM_REQUIRE((int64_t)n_gx * n_gy * n_gz < ((int64_t)1 << 31), "prom_gridded_density: grid too large");
    PROM_REQUIRE(n_points >= 0 && (n_points == 0 || (px && py && pz && out)), "prom_gridded_density: bad points");
    for (const auto& ax : {std::make_pair(gx, n_gx), std::make_pair(gy, n_gy), std::make_pair(gz, n_gz)})
      for (int32_t i = 1; i < ax.second; ++i)
        PROM_REQUIRE(ax.first[i] > ax.first[i - 1], "prom_gridded_density: axes must be strictly ascending");
    const int64_t nv = (int64_t)n_gx * n_gy * n_gz;
    std::vector<double> g;
    g.reserve(n_gx + n_gy + n_gz + nv);
    g.insert(g.end(), gx, gx + n_gx);
    g.insert(g.end(), gy, gy + n_gy);
    g.insert(g.end(), gz, gz + n_gz);
    g.insert(g.end(), values, values + nv);
    upload(ctx->scratch[0], g.data(), (int64_t)g.size(), ctx->stream);
    upload(ctx->scratch[1], px, n_points, ctx->stream);
    upload(ctx->scratch[2], py, n_points, ctx->stream);
    upload(ctx->scratch[3], pz, n_points, ctx->stream);
    ctx->scratch[4].ensure(sizeof(double) * std::max<int64_t>(n_points, 1));
    prom::launch_gridded(ctx->stream, ctx->scratch[0].as<double>(), n_gx, n_gy, n_gz, n_points,
                         ctx->scratch[1].as<double>(), ctx->scratch[2].as<double>(), ctx->scratch[3].as<double>(),
                         ctx->scratch[4].as<double>());
    download(out, ctx->scratch[4], n_points, ctx->stream);
    PROM_HIP(hipStreamSynchronize(ctx->stream));
  });
}

int32_t prom_star_disk_flux(prom_ctx* ctx, int32_t star_table, int32_t n_cells, const double* shift,
                            const double* clv, const double* rho, double dphi, double drho, int64_t n_wav,
                            const double* wavelength, double* out) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(table_ok(ctx->tables, star_table), "prom_star_disk_flux: unknown star table");
    PROM_REQUIRE(n_cells >= 0 && n_wav >= 0 && (n_cells == 0 || (shift && clv && rho)) &&
                     (n_wav == 0 || (wavelength && out)),
                 "prom_star_disk_flux: bad arguments");
    const prom::AtomTable& sb = ctx->tables[star_table];
    PROM_REQUIRE(sb.offset == 0.0, "prom_star_disk_flux: the star table must have offset 0 (10**Fstar_function)");
    // interp1d(bounds_error=True) semantics of the reference's Fstar_function: every target lambda / shift
    // inside [x_0, x_{n-1}] (IEEE division is monotone: the extremes decide)
    double smin = INFINITY, smax = -INFINITY, lmin = INFINITY, lmax = -INFINITY;
    for (int32_t c = 0; c < n_cells; ++c) {
      PROM_REQUIRE(shift[c] > 0.0 && std::isfinite(shift[c]), "prom_star_disk_flux: Doppler factors must be positive");
      smin = std::min(smin, shift[c]);
      smax = std::max(smax, shift[c]);
    }
    for (int64_t w = 0; w < n_wav; ++w) {
      PROM_REQUIRE(std::isfinite(wavelength[w]), "prom_star_disk_flux: non-finite wavelength");
      lmin = std::min(lmin, wavelength[w]);
      lmax = std::max(lmax, wavelength[w]);
    }
    if (n_cells > 0 && n_wav > 0) {
      PROM_REQUIRE(lmin / smax >= sb.hx.front(), "prom_star_disk_flux: a target is below the interpolation range");
      PROM_REQUIRE(lmax / smin <= sb.hx.back(), "prom_star_disk_flux: a target is above the interpolation range");
    }
    const prom::SigTabDev tb{sb.x.as<double>(), sb.y.as<double>(), sb.n, sb.offset, nullptr, sb.dir.as<int32_t>(),
                             sb.n_dir, 0, sb.dir_x0, sb.dir_inv_h, 0.0, 0.0, 0.0, sb.hx.front(), sb.hx.back(),
                             sb.rec.as<double4>()};
    const hipStream_t s = ctx->stream;
    upload(ctx->scratch[0], shift, n_cells, s);
    upload(ctx->scratch[1], clv, n_cells, s);
    upload(ctx->scratch[2], rho, n_cells, s);
    upload(ctx->scratch[3], wavelength, n_wav, s);
    ctx->scratch[4].ensure(sizeof(double) * std::max<int64_t>(n_wav, 1));
    prom::launch_star_disk(s, tb, ctx->scratch[0].as<double>(), ctx->scratch[1].as<double>(),
                           ctx->scratch[2].as<double>(), n_cells, dphi, drho, ctx->scratch[3].as<double>(), n_wav,
                           ctx->scratch[4].as<double>());
    download(out, ctx->scratch[4], n_wav, s);
    PROM_HIP(hipStreamSynchronize(s));
  });
}

int32_t prom_timing_begin(prom_ctx* ctx) {
  return guarded(ctx, [&] {
    ctx->timing = true;
    ctx->timed_runs = 0;
    ctx->window_runs = 0;
  });
}

int32_t prom_timing_stride(prom_ctx* ctx, int32_t stride) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(stride >= 1, "prom_timing_stride: stride must be >= 1");
    ctx->timing_stride = stride;
  });
}

int32_t prom_timing_end(prom_ctx* ctx, int32_t max_runs, double* ms, int32_t* n_runs) {
  return guarded(ctx, [&] {
    PROM_REQUIRE(n_runs && (max_runs <= 0 || ms), "prom_timing_end: bad arguments");
    ctx->timing = false;
    const int32_t n = std::min(ctx->timed_runs, std::max(max_runs, 0));
    for (auto st : ctx->streams) PROM_HIP(hipStreamSynchronize(st));
    int clock_khz = 0;
    PROM_HIP(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, ctx->device));
    std::vector<unsigned long long> ts;
    for (int32_t r = 0; r < n; ++r) {
      hipEvent_t* e = &ctx->tev[4 * (size_t)r];
      float v[4];
      // timed runs carry one event pair: the ordering kernel's completion -> the tau kernel's
      // completion (the tau kernel's run time plus its dispatch behind the ordering kernel)
      PROM_HIP(hipEventElapsedTime(&v[2], e[2], e[3]));
      ms[4 * r + 0] = ms[4 * r + 1] = ms[4 * r + 3] = std::nan("");
      ms[4 * r + 2] = v[2];
      // and the tau kernel's own span on the device clock: first workgroup start -> last workgroup end
      const int32_t nb = r < (int32_t)ctx->ts_blocks.size() ? ctx->ts_blocks[r] : 0;
      if (nb > 0 && clock_khz > 0) {
        ts.resize(2 * (size_t)nb);
        PROM_HIP(hipMemcpy(ts.data(), ctx->tsbuf[r].p, sizeof(unsigned long long) * ts.size(), hipMemcpyDeviceToHost));
        unsigned long long lo = ~0ull, hi = 0;
        for (int32_t b = 0; b < nb; ++b) {
          lo = std::min(lo, ts[2 * (size_t)b]);
          hi = std::max(hi, ts[2 * (size_t)b + 1]);
        }
        if (hi >= lo) ms[4 * r + 3] = (double)(hi - lo) / (double)clock_khz;
      }
    }
    *n_runs = ctx->timed_runs;
    ctx->timed_runs = 0;
  });
}

}  // extern "C"
