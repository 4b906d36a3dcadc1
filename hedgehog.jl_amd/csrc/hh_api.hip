// C-ABI of libhedgehog_mc.so (include/hedgehog_mc.h): context, argument checking, staging of
// caller buffers, kernel sequencing.  No arithmetic of the pricing path happens on the host except
// hh_mc_finalize's discount·mean (montecarlo.jl:489-490) on the reduced accumulator vector.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <vector>

#include "hh_assets.h"
#include "hh_kernels.h"
#include "hh_localvol.h"
#include "hh_lsm_basis.h"
#include "hh_qe.h"

#include "hh_ctx.h"

namespace {

const char* const kNoCtx = "hedgehog_mc: no context";

int ncomp_of(int dynamics) { return dynamics == HH_HESTON ? 2 : 1; }

// launch limits (documented in hedgehog_mc.h): threads per launch < 2^32, grid.y <= 65535
constexpr uint64_t kMaxPaths = (1ull << 32) - 256;
constexpr uint32_t kMaxEulerSteps = 4u * 65535u;  // replay_pack_kernel: 4 steps per grid.y
constexpr uint32_t kMaxGridSteps = 65534u;        // LSM / exact grid: one grid.y per row, n_steps + 1 rows

// degrees of freedom of the noncentral chi-squared law of V_T (heston.jl:128): the Bessel order is
// d/2 - 1, which must stay strictly above -1 in fp64 and within what the tables of hh_bessel.h cover
// … and the constants of a transition of length dt (heston.jl:129-130, :170-172) must come out finite:
// kappa·dt beyond ±700 overflows e^{∓κ dt}
static bool bk_law_ok(const hh_model* m, double dt) {
  const double s2 = m->sigma * m->sigma;
  const double d = 4.0 * m->kappa * m->theta / s2;
  if (!(d >= 1e-8 && d <= 1e6)) return false;
  const double em1 = -std::expm1(-m->kappa * dt);
  const double lam_per_v = 4.0 * m->kappa * std::exp(-m->kappa * dt) / (s2 * em1);  // λ / V0
  const double cscale = s2 * em1 / (4.0 * m->kappa);
  const double nuk = 4.0 * m->kappa * std::exp(-0.5 * m->kappa * dt) / s2 / em1;
  return std::isfinite(lam_per_v) && lam_per_v >= 0.0 && std::isfinite(cscale) && cscale > 0.0 &&
         std::isfinite(nuk) && nuk > 0.0 && std::isfinite(m->kappa * (1.0 + std::exp(-m->kappa * dt)) / em1);
}

int validate(hh_ctx* ctx, const hh_model* m, const hh_config* c) {
  if (!m || !c) return fail(ctx, HH_ERR_INVALID, "model/config is NULL");
  if (c->n_paths == 0) return fail(ctx, HH_ERR_INVALID, "n_paths must be >= 1");
  // one 256-thread workgroup per 256 trajectories: HIP rejects a launch of 2^32 threads or more
  if (c->n_paths > kMaxPaths)
    return fail(ctx, HH_ERR_INVALID, "n_paths too large (max 2^32 - 256 per call; shard the ensemble)");
  // grid.y of the REPLAY repack / fill kernels (4 and 16 steps per workgroup) is limited to 65535
  if (c->strategy == HH_EULER_MARUYAMA && c->n_steps > kMaxEulerSteps)
    return fail(ctx, HH_ERR_INVALID, "n_steps too large (max %u)", kMaxEulerSteps);
  if (c->n_partials > HH_MAX_PARTIALS)
    return fail(ctx, HH_ERR_INVALID, "n_partials %u > HH_MAX_PARTIALS", c->n_partials);
  const bool logn = c->dynamics == HH_LOGNORMAL, hest = c->dynamics == HH_HESTON;
  if (!logn && !hest) return fail(ctx, HH_ERR_INVALID, "unknown dynamics %d", c->dynamics);
  // the (dynamics, strategy) pairs that have a sde_problem / marginal_law method in the reference
  // (montecarlo.jl:140-231, 293-320); anything else is a MethodError there
  const bool ok = (logn && (c->strategy == HH_EULER_MARUYAMA || c->strategy == HH_EXACT_LAW)) ||
                  (hest && (c->strategy == HH_EULER_MARUYAMA || c->strategy == HH_BROADIE_KAYA));
  if (!ok)
    return fail(ctx, HH_ERR_UNSUPPORTED, "no simulation method for dynamics %d with strategy %d",
                c->dynamics, c->strategy);
  if (!(m->S0 > 0.0) || !std::isfinite(m->S0)) return fail(ctx, HH_ERR_INVALID, "S0 must be > 0");
  if (!(m->T > 0.0) || !std::isfinite(m->T)) return fail(ctx, HH_ERR_INVALID, "T must be > 0");
  if (m->cp != 1.0 && m->cp != -1.0) return fail(ctx, HH_ERR_INVALID, "cp must be +1 or -1");
  if (hest && !(std::fabs(m->rho) <= 1.0)) return fail(ctx, HH_ERR_INVALID, "|rho| must be <= 1");
  // the scalars the chosen dynamics reads (the reference would carry a NaN through to the price; here it
  // is an argument error, before any launch)
  if (!std::isfinite(m->sigma) || !std::isfinite(m->r_drift) || !std::isfinite(m->discount) ||
      !std::isfinite(m->strike) ||
      (hest && (!std::isfinite(m->V0) || !std::isfinite(m->kappa) || !std::isfinite(m->theta))))
    return fail(ctx, HH_ERR_INVALID, "model scalars must be finite");
  if (c->strategy == HH_EULER_MARUYAMA && c->n_steps == 0)
    return fail(ctx, HH_ERR_INVALID, "n_steps must be >= 1 for EulerMaruyama");
  if (c->strategy == HH_BROADIE_KAYA) {
    // final_sample(law, sample, ::Antithetic) needs mean(law), which LogHestonDistribution does
    // not define (montecarlo.jl:387); dual numbers do not pass rand! (heston.jl:261-276)
    if (c->antithetic)
      return fail(ctx, HH_ERR_UNSUPPORTED, "HestonBroadieKaya has no antithetic form");
    if (c->n_partials)
      return fail(ctx, HH_ERR_UNSUPPORTED, "HestonBroadieKaya does not carry dual partials");
    if (m->sigma == 0.0 || m->kappa == 0.0 || !(m->V0 > 0.0))
      return fail(ctx, HH_ERR_INVALID, "HestonBroadieKaya needs sigma != 0, kappa != 0, V0 > 0");
    // d = 4κθ/σ² degrees of freedom of the noncentral chi-squared law (heston.jl:128), λ >= 0 (:129)
    if ((c->bk_root_form != HH_BK_ROOT_SECANT && c->bk_root_form != HH_BK_ROOT_ORDER2) ||
        (c->bk_bracket_form != HH_BK_BRACKET_MIDPOINT && c->bk_bracket_form != HH_BK_BRACKET_ROOTS) ||
        (c->bk_caps != HH_BK_CAPS_AS_WRITTEN && c->bk_caps != HH_BK_CAPS_ROOTS_DEFAULT))
      return fail(ctx, HH_ERR_INVALID, "bk_root_form, bk_bracket_form, bk_caps: 0 or 1 each (hedgehog_mc.h)");
    if (!bk_law_ok(m, m->T))
      return fail(ctx, HH_ERR_INVALID, "HestonBroadieKaya needs 1e-8 <= d = 4 kappa theta / sigma^2 <= 1e6 "
                                       "(Bessel order d/2 - 1 strictly above -1, tables up to order 5e5) and "
                                       "finite transition constants (|kappa T| < 700)");
  }
  const bool euler = c->strategy == HH_EULER_MARUYAMA;
  if (c->noise_mode == HH_NOISE_REPLAY) {
    if (!c->replay) return fail(ctx, HH_ERR_INVALID, "REPLAY needs a replay buffer");
    if (((uintptr_t)c->replay & 15u) != 0)
      return fail(ctx, HH_ERR_INVALID, "replay buffer must be 16-byte aligned");
    if (c->replay_len) {  // operand shape: what the kernels (or the packer) will index
      uint64_t need = c->n_paths;  // exact law: one normal per trajectory
      if (c->strategy == HH_BROADIE_KAYA) need = 3 * c->n_paths;  // V_T | u | Z
      if (euler)
        need = c->replay_layout == HH_REPLAY_PATH_MAJOR
                   ? c->n_paths * (uint64_t)c->n_steps * (uint64_t)ncomp_of(c->dynamics)
                   : (uint64_t)hh::tiles_for(c->n_paths) * c->n_steps * ncomp_of(c->dynamics) *
                         hh::kTile;
      if (c->replay_len < need)
        return fail(ctx, HH_ERR_INVALID, "replay buffer holds %llu elements, %llu needed",
                    (unsigned long long)c->replay_len, (unsigned long long)need);
    }
  } else if (c->noise_mode == HH_NOISE_GENERATE) {
    if (!c->seeds) return fail(ctx, HH_ERR_INVALID, "GENERATE needs seeds");
    const uint64_t need = euler ? c->n_paths : 1;  // montecarlo.jl:65-66, 331, 456
    if (c->seeds_len && c->seeds_len < need)
      return fail(ctx, HH_ERR_INVALID, "Number of seeds (%llu) must be >= number of trajectories (%llu)",
                  (unsigned long long)c->seeds_len, (unsigned long long)need);
  } else {
    return fail(ctx, HH_ERR_INVALID, "unknown noise_mode %d", c->noise_mode);
  }
  return HH_OK;
}

// the record buffer of the launches that reduce their own records: every word kPoison (hh_sim.h) from the
// allocation on — each launch's reducer leaves it that way again
int ensure_poisoned(hh_ctx* ctx, size_t need) {
  if (need <= ctx->frecords.cap) return HH_OK;
  int rc = ensure(ctx, ctx->frecords, need);
  if (rc) return rc;
  static_assert((hh::kPoison >> 32) == (hh::kPoison & 0xffffffffull), "hipMemsetD32 writes the pattern");
  HH_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)ctx->frecords, (int)(hh::kPoison & 0xffffffffull),
                                ctx->frecords.cap * 2, ctx->stream));
  return HH_OK;
}

// HH_OPT_FUSE_REDUCE = 2 (default), by what was measured (profiles/r05_c_fuse_ab.txt, same process, same box):
// the simulation kernel reduces its own records when they are few (the whole grid is resident at once, the
// reducer finds them all on its first look: -2 % on a 27 µs solve) and when the kernel runs long enough for
// the reducer's wait to disappear behind the other workgroups' work (Euler, 10^6 x 252: -0.3 % in both noise
// modes); a SHORT kernel with thousands of records (the exact law at 10^6-10^7 trajectories, 14-43 µs) is 1-4 %
// faster with reduce_records_kernel behind it, whose 16 workgroups read the records in parallel.
constexpr uint32_t kFuseAutoMaxRecords = 512, kFuseAutoMinSteps = 32;
bool fuse_for(const hh_ctx* ctx, const hh_config* c) {
  if (ctx->fuse_reduce != 2) return ctx->fuse_reduce == 1;
  return hh::sim_records(*c) <= kFuseAutoMaxRecords || (c->strategy == HH_EULER_MARUYAMA && c->n_steps >= kFuseAutoMinSteps);
}

// what a launch that reduces its own records needs of the context beside the poisoned buffer
void fused_controls(const hh_ctx* ctx, hh::DevicePtrs& p) {
  p.finish_state = ctx->finish_state;
  p.finish_spin_ticks = ctx->finish_spin_ticks;
  p.finish_tile_first = ctx->finish_tile_first;
}

// A reducer inside a simulation kernel gave up waiting for a record (hh_sim.h): the record buffer may hold that
// record now, where the next launch would take it for its own.  With the stream idle: every word back to the
// poison, the give-up word cleared.  Returns HH_OK when there was nothing to recover from.
int recover_finish(hh_ctx* ctx) {
  unsigned int state = 0;
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  HH_HIP(ctx, hipMemcpy(&state, ctx->finish_state, sizeof(state), hipMemcpyDeviceToHost));
  if (state == 0u) return HH_OK;
  if (ctx->frecords.cap)
    HH_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)ctx->frecords, (int)(hh::kPoison & 0xffffffffull),
                                  ctx->frecords.cap * 2, ctx->stream));
  HH_HIP(ctx, hipMemsetAsync(ctx->finish_state, 0, 2 * sizeof(unsigned int), ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const long long ticks = ctx->finish_spin_ticks < 0 ? (long long)hh::kFinishSpinTicksDefault : ctx->finish_spin_ticks;
  return fail(ctx, HH_ERR_DEVICE_TIMEOUT,
              "the record reduction inside a simulation kernel gave up: a workgroup's record had not arrived after %lld "
              "ticks of the 100 MHz clock (a queue preempted for that long, or a workgroup that died); the sums of that "
              "solve, and of solves queued behind it, are lost — the context's record buffer has been reset and the "
              "context can be used again", ticks);
}

// hh_mc_finalize refused an accumulator: because a reducer gave up (the named status), or for what it says
int finalize_failed(hh_ctx* ctx, int rc) {
  const int rf = recover_finish(ctx);
  return rf ? rf : fail(ctx, rc, "finalize failed: the accumulator holds no trajectories");
}

size_t replay_elems(uint64_t n_paths, uint32_t n_steps, int dynamics) {
  return (size_t)hh::tiles_for(n_paths) * n_steps * ncomp_of(dynamics) * hh::kTile;
}

// the times of a solve: kernel_ms from ctx->ev0 to ctx->ev1 (the stream has passed ev1), total_ms on the clock
int solve_times(hh_ctx* ctx, const WallClock& clock, double* kernel_ms, double* total_ms) {
  float ms = 0.f;
  HH_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *kernel_ms = ms;
  *total_ms = clock.ms();
  return HH_OK;
}

// mean and sample variance (0 for a single trajectory, clamped at 0) of the payoffs an accumulator vector sums over n
void payoff_moments(const double* acc, double n, double* mean, double* var) {
  *mean = acc[HH_ACC_SUM] / n;
  *var = n > 1.0 ? (acc[HH_ACC_SUMSQ] - n * *mean * *mean) / (n - 1.0) : 0.0;
  if (!(*var > 0.0)) *var = 0.0;
}

}  // namespace

extern "C" {

int hh_abi_version(void) { return HH_ABI_VERSION; }

int hh_ctx_create(hh_ctx** out, int device_id) {
  if (!out) return HH_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return HH_ERR_HIP;  // no CPU fallback
  if (device_id < 0 || device_id >= n) return HH_ERR_INVALID;
  hh_ctx* ctx = new (std::nothrow) hh_ctx();
  if (!ctx) return HH_ERR_NOMEM;
  ctx->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_switch, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_stage, hipEventDisableTiming) != hipSuccess ||
      hipMalloc((void**)&ctx->accum, HH_ACC_LEN * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&ctx->finish_state, 2 * sizeof(unsigned int)) != hipSuccess ||
      hipMemset(ctx->finish_state, 0, 2 * sizeof(unsigned int)) != hipSuccess ||
      hipHostMalloc((void**)&ctx->accum_host, (HH_ACC_LEN + 8) * sizeof(double), hipHostMallocDefault) !=
          hipSuccess) {
    hh_ctx_destroy(ctx);
    return HH_ERR_HIP;
  }
  ctx->stream = ctx->own_stream;
  *out = ctx;
  return HH_OK;
}

void hh_ctx_destroy(hh_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  // a borrowed stream may be gone already: wait for the device (hipFree below synchronises anyway)
  if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
  (void)hipDeviceSynchronize();
  for (auto& e : ctx->seed_cache)
    if (e.dev) (void)hipFree(e.dev);
  if (ctx->accum) (void)hipFree(ctx->accum);
  if (ctx->finish_state) (void)hipFree(ctx->finish_state);
  if (ctx->accum_host) (void)hipHostFree(ctx->accum_host);
  for (auto& pr : ctx->tev)
    for (auto& e : pr)
      if (e) (void)hipEventDestroy(e);
  if (ctx->ev_switch) (void)hipEventDestroy(ctx->ev_switch);
  if (ctx->ev_stage) (void)hipEventDestroy(ctx->ev_stage);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

// Work already queued on the stream being left still uses the ctx's scratch buffers (records, staged
// seeds / increments): the stream taken up next waits for it (an event, no host synchronisation).
static int switch_stream(hh_ctx* ctx, hipStream_t next) {
  if (next == ctx->stream) return HH_OK;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev_switch, ctx->stream));
  HH_HIP(ctx, hipStreamWaitEvent(next, ctx->ev_switch, 0));
  ctx->stream = next;
  return HH_OK;
}

int hh_ctx_set_stream(hh_ctx* ctx, void* hip_stream) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  return switch_stream(ctx, (hipStream_t)hip_stream);  // NULL is the device's default (null) stream
}

int hh_ctx_reset_stream(hh_ctx* ctx) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  return switch_stream(ctx, ctx->own_stream);
}

const char* hh_last_error(const hh_ctx* ctx) { return ctx ? ctx->err : kNoCtx; }

int hh_ctx_set_option(hh_ctx* ctx, int32_t option, int64_t value) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  switch (option) {
    case HH_OPT_LSM_FORM:
      if (value != HH_LSM_FORM_PER_DATE && value != HH_LSM_FORM_PERSISTENT && value != HH_LSM_FORM_AUTO)
        return fail(ctx, HH_ERR_INVALID, "HH_OPT_LSM_FORM: 0 (launch per date), 1 (one launch) or 2 (auto)");
      ctx->lsm_form = (int)value;
      return HH_OK;
    case HH_OPT_BK_TERM_CACHE:
      if (value < 8 || value > 1024)
        return fail(ctx, HH_ERR_INVALID, "HH_OPT_BK_TERM_CACHE: 8 .. 1024 series terms per trajectory");
      ctx->bk_term_cache = (int)value;
      return HH_OK;
    case HH_OPT_LSM_SPIN_TICKS:
      if (value < -1) return fail(ctx, HH_ERR_INVALID, "HH_OPT_LSM_SPIN_TICKS: ticks of the 100 MHz clock, 0 = give up at once, -1 = default");
      ctx->lsm_spin_ticks = value;
      return HH_OK;
    case HH_OPT_GRID_FORM:
      if (value != HH_GRID_FORM_PER_DATE && value != HH_GRID_FORM_BATCHED)
        return fail(ctx, HH_ERR_INVALID, "HH_OPT_GRID_FORM: 0 (one chain per date) or 1 (dates batched)");
      ctx->grid_form = (int)value;
      return HH_OK;
    case HH_OPT_GRID_ORDER:
      if (value != 0 && value != 1)
        return fail(ctx, HH_ERR_INVALID, "HH_OPT_GRID_ORDER: 0 (a chain's pairs in their natural order) or 1 (sorted by their Bessel arguments)");
      ctx->grid_order = (int)value;
      return HH_OK;
    case HH_OPT_FINISH_SPIN_TICKS:
      if (value < -1) return fail(ctx, HH_ERR_INVALID, "HH_OPT_FINISH_SPIN_TICKS: ticks of the 100 MHz clock, 0 = give up at once, -1 = default");
      ctx->finish_spin_ticks = value;
      return HH_OK;
    case HH_OPT_FINISH_TILE_FIRST:
      if (value != 0 && value != 1) return fail(ctx, HH_ERR_INVALID, "HH_OPT_FINISH_TILE_FIRST: 0 (the last tile's workgroup adds the records) or 1 (the first one's)");
      ctx->finish_tile_first = (int)value;
      return HH_OK;
    case HH_OPT_FUSE_REDUCE:
      if (value < 0 || value > 2)
        return fail(ctx, HH_ERR_INVALID, "HH_OPT_FUSE_REDUCE: 0 (a second kernel reduces the records), 1 (the simulation kernel does) or 2 (by size)");
      ctx->fuse_reduce = (int)value;
      return HH_OK;
    default:
      return fail(ctx, HH_ERR_INVALID, "unknown option %d", option);
  }
}

int hh_ctx_synchronize(hh_ctx* ctx) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HH_OK;
}

size_t hh_replay_elems(uint64_t n_paths, uint32_t n_steps, int32_t dynamics) {
  return replay_elems(n_paths, n_steps, dynamics);
}

int hh_replay_pack(hh_ctx* ctx, int32_t dynamics, uint64_t n_paths, uint32_t n_steps,
                   const double* src, int32_t src_on_device, double* dst) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!src || !dst || n_paths == 0 || n_steps == 0 || n_paths > kMaxPaths || n_steps > kMaxEulerSteps)
    return fail(ctx, HH_ERR_INVALID, "hh_replay_pack: bad arguments");
  HH_HIP(ctx, hipSetDevice(ctx->device));
  const int nc = ncomp_of(dynamics);
  const double* src_dev = src;
  if (!src_on_device) {
    const size_t n = (size_t)n_paths * n_steps * nc;
    const int rc = stage_host(ctx, ctx->replay_src, n, src, n, &src_dev);
    if (rc) return rc;
  }
  HH_HIP(ctx, hh::launch_replay_pack(nc, n_paths, n_steps, src_dev, dst, ctx->stream));
  return release_host_operands(ctx);
}

int hh_wiener_fill(hh_ctx* ctx, int32_t dynamics, double rho, double T, uint32_t n_steps,
                   uint64_t n_paths, const uint64_t* seeds, int32_t seeds_on_device, double* dst) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!seeds || !dst || n_paths == 0 || n_steps == 0 || !(T > 0.0) || !(std::fabs(rho) <= 1.0) ||
      n_paths > kMaxPaths || n_steps > kMaxEulerSteps)
    return fail(ctx, HH_ERR_INVALID, "hh_wiener_fill: bad arguments");
  HH_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t* seeds_dev = seeds;
  if (!seeds_on_device) {
    const int rc = stage_host(ctx, ctx->seeds, (size_t)n_paths, seeds, (size_t)n_paths, &seeds_dev);
    if (rc) return rc;
  }
  const double dt = T / (double)n_steps;
  HH_HIP(ctx, hh::launch_wiener_fill(dynamics, rho, std::sqrt(dt), n_steps, n_paths, seeds_dev, dst,
                                     ctx->stream));
  return release_host_operands(ctx);
}

// ---- quasi-Monte Carlo (include/hedgehog_mc.h, "Quasi-Monte Carlo"; hh_sobol.hip) -------------------------------------------

int hh_sobol_directions(uint32_t dim, uint32_t v[32]) {
  if (!v || dim >= HH_SOBOL_MAX_DIMS) return HH_ERR_INVALID;
  hh::sobol_expand(dim, v);
  return HH_OK;
}

// the direction words in the context's device memory: expanded once per process, uploaded once per context
static int sobol_directions_dev(hh_ctx* ctx) {
  if (ctx->sobol_dirs_ready) return HH_OK;
  const std::vector<uint32_t>& all = hh::sobol_all_directions();
  const uint32_t* dev = nullptr;
  const int rc = stage_host(ctx, ctx->sobol_dirs, all.size(), all.data(), all.size(), &dev);
  if (rc) return rc;
  ctx->sobol_dirs_ready = true;
  return HH_OK;
}

// a point range every Sobol' entry point accepts: 1 .. 2^32 − 256 points (one launch), all below point 2^32
static bool sobol_range_ok(uint64_t n_points, uint64_t point_offset) {
  return n_points >= 1 && n_points <= kMaxPaths && point_offset < (1ull << 32) && point_offset + n_points <= (1ull << 32);
}

// the high words of n_dims dimensions for the tiles of [point_offset, point_offset + n_points) under one shift
static int sobol_high_dev(hh_ctx* ctx, uint32_t n_dims, uint64_t n_points, uint64_t point_offset, uint64_t shift_seed,
                          uint32_t randomization, int32_t shifted) {
  int rc = sobol_directions_dev(ctx);
  if (rc) return rc;
  if ((rc = ensure(ctx, ctx->sobol_high, (size_t)hh::tiles_for(n_points) * n_dims * 2u))) return rc;
  HH_HIP(ctx, hh::launch_sobol_high(ctx->sobol_dirs, n_dims, n_points, (uint32_t)point_offset, shift_seed, randomization,
                                    shifted != 0, ctx->sobol_high, ctx->stream));
  return HH_OK;
}

int hh_sobol_points(hh_ctx* ctx, uint32_t n_dims, uint64_t n_points, uint64_t point_offset, uint64_t shift_seed,
                    uint32_t randomization, int32_t shifted, uint32_t* dst_dev) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!dst_dev || n_dims == 0 || !sobol_range_ok(n_points, point_offset))
    return fail(ctx, HH_ERR_INVALID, "hh_sobol_points: bad arguments");
  if (n_dims > HH_SOBOL_MAX_DIMS)
    return fail(ctx, HH_ERR_UNSUPPORTED, "hh_sobol_points: %u dimensions, at most %d", n_dims, HH_SOBOL_MAX_DIMS);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  const int rc = sobol_high_dev(ctx, n_dims, n_points, point_offset, shift_seed, randomization, shifted);
  if (rc) return rc;
  HH_HIP(ctx, hh::launch_sobol_points(ctx->sobol_dirs, ctx->sobol_high, n_dims, n_points, (uint32_t)point_offset, dst_dev,
                                      ctx->stream));
  return release_host_operands(ctx);
}

int hh_sobol_fill(hh_ctx* ctx, int32_t dynamics, double rho, double T, uint32_t n_steps, uint64_t n_points,
                  uint64_t point_offset, uint64_t shift_seed, uint32_t randomization, int32_t shifted,
                  int32_t construction, double* dst) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!dst || n_steps == 0 || !(T > 0.0) || !std::isfinite(T) || !(std::fabs(rho) <= 1.0) ||
      !sobol_range_ok(n_points, point_offset) ||
      (construction != HH_SOBOL_INCREMENTAL && construction != HH_SOBOL_BRIDGE))
    return fail(ctx, HH_ERR_INVALID, "hh_sobol_fill: bad arguments");
  const int nc = ncomp_of(dynamics);
  if ((uint64_t)nc * n_steps > HH_SOBOL_MAX_DIMS)
    return fail(ctx, HH_ERR_UNSUPPORTED, "hh_sobol_fill: %d x %u coordinates per point, at most %d", nc, n_steps,
                HH_SOBOL_MAX_DIMS);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  int rc = sobol_high_dev(ctx, (uint32_t)nc * n_steps, n_points, point_offset, shift_seed, randomization, shifted);
  if (rc) return rc;
  const bool bridge = construction == HH_SOBOL_BRIDGE;
  if (bridge && ctx->sobol_ops_steps != n_steps) {  // tabulated per n_steps; the last table's upload has been waited for
    ctx->sobol_ops_steps = 0;
    ctx->sobol_ops_host = hh::sobol_bridge_ops(n_steps, &ctx->sobol_slots);
    const hh::SobolOp* dev = nullptr;
    const size_t n = ctx->sobol_ops_host.size();
    if ((rc = stage_host(ctx, ctx->sobol_ops, n, ctx->sobol_ops_host.data(), n, &dev))) return rc;
    ctx->sobol_ops_steps = n_steps;
  }
  HH_HIP(ctx, hh::launch_sobol_fill(dynamics, rho, std::sqrt(T / (double)n_steps), n_steps, n_points, (uint32_t)point_offset,
                                    ctx->sobol_dirs, ctx->sobol_high, bridge ? (const hh::SobolOp*)ctx->sobol_ops : nullptr,
                                    bridge ? (uint32_t)ctx->sobol_ops_host.size() : 0u, ctx->sobol_slots, dst, ctx->stream));
  return release_host_operands(ctx);
}

// Shared body of hh_mc_accumulate / hh_mc_accumulate_basket: stage caller buffers, run the
// simulation kernel (which also reduces the payoff of m->strike / m->cp into ctx->records) and
// leave the terminal samples in device memory when asked.
// The noise a simulation reads, in device memory: p.seeds (GENERATE) or p.replay (REPLAY), staged from the
// caller's host buffers where needed.  tile_major_only: path-major Euler increments are repacked even where the
// one-model kernel could stream them as they are (the several-model kernel reads the tile-major layout only).
static int stage_noise(hh_ctx* ctx, const hh_config* c, hh::DevicePtrs& p, bool tile_major_only) {
  int rc = HH_OK;
  const bool bk = c->strategy == HH_BROADIE_KAYA;
  // seeds: per-trajectory for Euler (montecarlo.jl:331), seeds[1] only for the exact laws (:456)
  if (c->noise_mode == HH_NOISE_GENERATE) {
    const size_t need = (c->strategy == HH_EULER_MARUYAMA) ? (size_t)c->n_paths : 1;
    if (c->seeds_on_device)
      p.seeds = c->seeds;
    else if ((rc = stage_host(ctx, ctx->seeds, need, c->seeds, need, &p.seeds)))
      return rc;
  } else if (bk) {
    // the trajectory's three draws [V_T | u | Z], n_paths each (heston.jl:246-259 order)
    const size_t n3 = (size_t)3 * c->n_paths;
    if (c->replay_on_device)
      p.replay = c->replay;
    else if ((rc = stage_host(ctx, ctx->replay, n3, c->replay, n3, &p.replay)))
      return rc;
  } else {
    const uint32_t steps = (c->strategy == HH_EULER_MARUYAMA) ? c->n_steps : 1;
    const int dyn = (c->strategy == HH_EULER_MARUYAMA) ? c->dynamics : HH_LOGNORMAL;
    const size_t tile_elems = replay_elems(c->n_paths, steps, dyn);
    if (c->replay_layout == HH_REPLAY_PATH_MAJOR && c->strategy == HH_EULER_MARUYAMA && !tile_major_only &&
        hh::replay_direct_path_major(steps, ncomp_of(dyn))) {
      // the reference's layout, streamed as it stands (euler_pm_kernel): no repack pass
      const size_t n = (size_t)c->n_paths * steps * ncomp_of(dyn);
      if (c->replay_on_device)
        p.replay = c->replay;
      else if ((rc = stage_host(ctx, ctx->replay_src, n, c->replay, n, &p.replay)))
        return rc;
      p.replay_path_major = true;
    } else if (c->replay_layout == HH_REPLAY_PATH_MAJOR) {
      rc = ensure(ctx, ctx->replay, tile_elems);
      if (rc) return rc;
      rc = hh_replay_pack(ctx, dyn, c->n_paths, steps, c->replay, c->replay_on_device, ctx->replay);
      if (rc) return rc;
      p.replay = ctx->replay;
    } else if (c->replay_layout == HH_REPLAY_TILE_MAJOR) {
      if (c->replay_on_device) {
        p.replay = c->replay;
      } else {
        // exact law: one standard normal per trajectory, n_paths doubles (no tile padding needed:
        // the kernel guards the tail); Euler: the padded tile-major buffer of hh_replay_elems()
        const size_t host_elems =
            (c->strategy == HH_EULER_MARUYAMA) ? tile_elems : (size_t)c->n_paths;
        rc = stage_host(ctx, ctx->replay, tile_elems, c->replay, host_elems, &p.replay);
        if (rc) return rc;
      }
    } else {
      return fail(ctx, HH_ERR_INVALID, "unknown replay_layout %d", c->replay_layout);
    }
  }

  return HH_OK;
}

// accum_dev != NULL (and the ctx's HH_OPT_FUSE_REDUCE): the simulation kernel reduces its own records into
// accum_dev — *reduced says whether it did.  The Broadie–Kaya chain always adds its own records (its tail kernel):
// into accum_dev, or into ctx->accum when the caller has no use for the sums.  The timing slot opened here is
// closed by end_timing() once the caller has enqueued its last kernel.
static int run_simulation(hh_ctx* ctx, const hh_model* m, const hh_config* c, double* terminal,
                          bool need_terminal_dev, double** terminal_dev_out, double* accum_dev = nullptr,
                          bool* reduced = nullptr) {
  int rc = HH_OK;
  const uint32_t n_tiles = hh::tiles_for(c->n_paths);
  const bool bk = c->strategy == HH_BROADIE_KAYA;
  rc = ensure(ctx, ctx->records, (size_t)(bk ? hh::bk_record_count(c->n_paths) : n_tiles) * hh::kRecStride);
  if (rc) return rc;

  hh::DevicePtrs p{};
  p.records = ctx->records;
  const bool fuse = accum_dev && !bk && fuse_for(ctx, c);
  if (fuse) {  // records in the buffer that holds the poison pattern between launches (hh_sim.h)
    if ((rc = ensure_poisoned(ctx, (size_t)n_tiles * hh::kRecStride))) return rc;
    p.records = ctx->frecords;
    p.accum = accum_dev;
    fused_controls(ctx, p);
  }
  if (reduced) *reduced = fuse || bk;
  if (bk) {
    rc = ensure_bk_scratch(ctx, hh::bk_scratch_bytes(c->n_paths, ctx->bk_term_cache));
    if (rc) return rc;
    p.accum = accum_dev ? accum_dev : ctx->accum;
    p.bk_scratch = ctx->bk_scratch;
    p.bk_table_key = &ctx->bk_table_key;
    p.bk_term_cache = ctx->bk_term_cache;
    ctx->bk_last_n = c->n_paths;
    ctx->bk_last_cache = ctx->bk_term_cache;
  }

  if ((rc = stage_noise(ctx, c, p, false))) return rc;

  const size_t n_term = (size_t)c->n_paths * (c->antithetic ? 2 : 1);
  if (terminal && c->terminal_on_device) {
    p.terminal = terminal;
  } else if (terminal || need_terminal_dev) {
    rc = ensure(ctx, ctx->terminal, n_term);
    if (rc) return rc;
    p.terminal = ctx->terminal;
  }
  const int n_active = c->n_partials ? hh::count_active_partials(*m, *c) : 0;
  if (need_terminal_dev && n_active) {
    rc = ensure(ctx, ctx->terminal_d, n_term * (size_t)hh::pad_partials((uint32_t)n_active));
    if (rc) return rc;
    p.terminal_d = ctx->terminal_d;
  }
  if (terminal_dev_out) *terminal_dev_out = p.terminal;

  if (ctx->timing) HH_HIP(ctx, hipEventRecord(ctx->tev[ctx->t_count % hh_ctx::kTimingSlots][0], ctx->stream));
  if (c->strategy == HH_BROADIE_KAYA)
    HH_HIP(ctx, hh::launch_bk(*m, *c, p, ctx->stream));
  else
    HH_HIP(ctx, hh::launch_simulation(*m, *c, p, ctx->stream));
  return HH_OK;
}

// the call's last kernel has been enqueued: close the timing slot run_simulation opened
static int end_timing(hh_ctx* ctx) {
  if (ctx->timing) {
    HH_HIP(ctx, hipEventRecord(ctx->tev[ctx->t_count % hh_ctx::kTimingSlots][1], ctx->stream));
    ++ctx->t_count;
  }
  return HH_OK;
}

static int copy_back_terminal(hh_ctx* ctx, const hh_config* c, double* terminal) {
  if (terminal && !c->terminal_on_device) {
    const size_t n_term = (size_t)c->n_paths * (c->antithetic ? 2 : 1);
    HH_HIP(ctx, hipMemcpyAsync(terminal, ctx->terminal, n_term * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
    HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return HH_OK;
}

int hh_mc_accumulate(hh_ctx* ctx, const hh_model* m, const hh_config* c, double* accum_dev,
                     double* terminal) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  int rc = validate(ctx, m, c);
  if (rc) return rc;
  if (!accum_dev) return fail(ctx, HH_ERR_INVALID, "accum_dev is NULL");
  HH_HIP(ctx, hipSetDevice(ctx->device));
  bool reduced = false;
  rc = run_simulation(ctx, m, c, terminal, false, nullptr, accum_dev, &reduced);
  if (rc) return rc;
  if (!reduced)
    HH_HIP(ctx, hh::launch_reduce_records(ctx->records, hh::sim_records(*c), (double)c->n_paths, accum_dev, ctx->stream, 1, m, c));
  if ((rc = end_timing(ctx))) return rc;
  if ((rc = release_host_operands(ctx))) return rc;
  return copy_back_terminal(ctx, c, terminal);
}

// sizes of the passes n_models are run in: at most kMaxModelsPerPass models per launch, never one alone
static int next_pass(int remaining) {
  if (remaining <= hh::kMaxModelsPerPass) return remaining;
  return remaining == hh::kMaxModelsPerPass + 1 ? hh::kMaxModelsPerPass - 1 : hh::kMaxModelsPerPass;
}

int hh_mc_accumulate_multi(hh_ctx* ctx, const hh_model* models, uint32_t n_models, const hh_config* c,
                           double* accum_dev, double* const* terminals) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!models || n_models == 0 || n_models > HH_MAX_MODELS)
    return fail(ctx, HH_ERR_INVALID, "hh_mc_accumulate_multi: 1 .. %d models", HH_MAX_MODELS);
  if (!accum_dev) return fail(ctx, HH_ERR_INVALID, "accum_dev is NULL");
  int rc;
  for (uint32_t k = 0; k < n_models; ++k)
    if ((rc = validate(ctx, &models[k], c))) return rc;
  if (c->n_partials)
    return fail(ctx, HH_ERR_UNSUPPORTED, "several models in one pass carry no dual partials (n_partials must be 0)");
  if (n_models == 1) return hh_mc_accumulate(ctx, models, c, accum_dev, terminals ? terminals[0] : nullptr);
  HH_HIP(ctx, hipSetDevice(ctx->device));  // before anything is allocated: the caller's thread may be on another device
  if (c->strategy == HH_BROADIE_KAYA) {
    // One chain per set of models that the variance process cannot tell apart (hh::bk_same_chain: a bumped spot, rate,
    // ρ, strike — the finite-difference delta / gamma / rho of greeks_problem.jl:279-329, 360-422): the first of a set
    // runs the chain, the others are finished from the ∫V it left (bk_refinish_kernel, ~10 µs each), with the records —
    // hence the sums — of a chain of their own.  A bumped κ, θ, σ, V0 or T is another chain.
    const uint32_t count = hh::bk_record_count(c->n_paths);
    if ((rc = ensure(ctx, ctx->records, 2 * (size_t)count * hh::kRecStride))) return rc;  // BEFORE a chain runs
    std::vector<int> leader(n_models, -1);
    for (uint32_t k = 0; k < n_models; ++k)
      for (uint32_t j = 0; j < k; ++j)
        if (leader[j] < 0 && hh::bk_same_chain(models[j], models[k])) {
          leader[k] = (int)j;
          break;
        }
    for (uint32_t k = 0; k < n_models; ++k) {
      if (leader[k] >= 0) continue;
      if ((rc = hh_mc_accumulate(ctx, &models[k], c, accum_dev + (size_t)k * HH_ACC_LEN, terminals ? terminals[k] : nullptr)))
        return rc;
      for (uint32_t f = k + 1; f < n_models; ++f) {
        if (leader[f] != (int)k) continue;
        double* terminal = terminals ? terminals[f] : nullptr;
        hh::DevicePtrs p{};
        p.records = ctx->records + (size_t)count * hh::kRecStride;
        p.bk_scratch = ctx->bk_scratch;
        p.bk_term_cache = ctx->bk_term_cache;
        // (the draws, the ballots and ∫V are where the chain left them: no seeds, no noise here)
        if (terminal && c->terminal_on_device) {
          p.terminal = terminal;
        } else if (terminal) {
          if ((rc = ensure(ctx, ctx->terminal, (size_t)c->n_paths))) return rc;
          p.terminal = ctx->terminal;
        }
        if (ctx->timing) HH_HIP(ctx, hipEventRecord(ctx->tev[ctx->t_count % hh_ctx::kTimingSlots][0], ctx->stream));
        HH_HIP(ctx, hh::launch_bk_refinish(models[f], *c, p, ctx->records, ctx->stream));
        HH_HIP(ctx, hh::launch_reduce_records(p.records, count, (double)c->n_paths, accum_dev + (size_t)f * HH_ACC_LEN,
                                              ctx->stream, 1, &models[f], c, false,
                                              hh::bk_live_records(ctx->bk_scratch, c->n_paths)));
        if ((rc = end_timing(ctx))) return rc;
        if ((rc = copy_back_terminal(ctx, c, terminal))) return rc;
      }
    }
    return HH_OK;
  }
  const uint32_t n_tiles = hh::tiles_for(c->n_paths);
  const size_t rec_elems = (size_t)n_tiles * hh::kRecStride;
  const bool fuse = fuse_for(ctx, c);
  if (fuse) rc = ensure_poisoned(ctx, (size_t)n_models * rec_elems);
  else rc = ensure(ctx, ctx->records, (size_t)n_models * rec_elems);
  if (rc) return rc;
  hh::DevicePtrs base{};
  if (fuse) fused_controls(ctx, base);
  if ((rc = stage_noise(ctx, c, base, /*tile_major_only=*/true))) return rc;
  // terminal samples: a model's own device buffer, or a slice of the ctx's staging buffer for a host buffer
  const size_t n_term = (size_t)c->n_paths * (c->antithetic ? 2 : 1);
  bool any_host_terminal = false;
  if (terminals && !c->terminal_on_device) {
    for (uint32_t k = 0; k < n_models; ++k) any_host_terminal = any_host_terminal || terminals[k] != nullptr;
    if (any_host_terminal && (rc = ensure(ctx, ctx->terminal, (size_t)n_models * n_term))) return rc;
  }
  std::vector<hh::DevicePtrs> p(n_models, base);
  for (uint32_t k = 0; k < n_models; ++k) {
    p[k].records = (fuse ? ctx->frecords : ctx->records) + (size_t)k * rec_elems;
    p[k].accum = fuse ? accum_dev + (size_t)k * HH_ACC_LEN : nullptr;
    double* t = terminals ? terminals[k] : nullptr;
    p[k].terminal = !t ? nullptr : c->terminal_on_device ? t : ctx->terminal + (size_t)k * n_term;
  }
  if (ctx->timing) HH_HIP(ctx, hipEventRecord(ctx->tev[ctx->t_count % hh_ctx::kTimingSlots][0], ctx->stream));
  for (uint32_t k0 = 0; k0 < n_models;) {
    const int take = next_pass((int)(n_models - k0));
    HH_HIP(ctx, hh::launch_simulation_multi(models + k0, take, *c, p.data() + k0, ctx->stream));
    if (!fuse)
      for (int k = 0; k < take; ++k)
        HH_HIP(ctx, hh::launch_reduce_records(p[k0 + k].records, hh::sim_records(*c), (double)c->n_paths,
                                              accum_dev + (size_t)(k0 + k) * HH_ACC_LEN, ctx->stream, 1, &models[k0 + k], c));
    k0 += (uint32_t)take;
  }
  if ((rc = end_timing(ctx))) return rc;
  if ((rc = release_host_operands(ctx))) return rc;
  if (any_host_terminal) {
    for (uint32_t k = 0; k < n_models; ++k)
      if (terminals[k])
        HH_HIP(ctx, hipMemcpyAsync(terminals[k], p[k].terminal, n_term * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return HH_OK;
}

int hh_mc_solve_multi(hh_ctx* ctx, const hh_model* models, uint32_t n_models, const hh_config* c, hh_result* out,
                      double* const* terminals) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!out || !models || n_models == 0 || n_models > HH_MAX_MODELS)
    return fail(ctx, HH_ERR_INVALID, "hh_mc_solve_multi: 1 .. %d models and their results", HH_MAX_MODELS);
  const WallClock clock;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n_acc = (size_t)n_models * HH_ACC_LEN;
  int rc = ensure(ctx, ctx->basket_accum, n_acc);
  if (rc) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if ((rc = hh_mc_accumulate_multi(ctx, models, n_models, c, ctx->basket_accum, terminals))) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  double host[HH_MAX_MODELS * HH_ACC_LEN];
  HH_HIP(ctx, hipMemcpyAsync(host, ctx->basket_accum, n_acc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double kernel_ms, total_ms;
  if ((rc = solve_times(ctx, clock, &kernel_ms, &total_ms))) return rc;
  rc = finalize_results(models, 1, c, host, n_models, kernel_ms, total_ms, out);
  return rc ? finalize_failed(ctx, rc) : HH_OK;
}

int hh_mc_accumulate_basket(hh_ctx* ctx, const hh_model* m, const hh_config* c,
                            const double* strikes, const double* cps, uint32_t n_payoffs,
                            double* accum_dev, double* terminal) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  int rc = validate(ctx, m, c);
  if (rc) return rc;
  if (!accum_dev || !strikes || !cps || n_payoffs == 0 || n_payoffs > 65535)
    return fail(ctx, HH_ERR_INVALID, "hh_mc_accumulate_basket: bad arguments");
  for (uint32_t k = 0; k < n_payoffs; ++k)
    if (cps[k] != 1.0 && cps[k] != -1.0) return fail(ctx, HH_ERR_INVALID, "cp must be +1 or -1");
  if (m->dstrike)
    return fail(ctx, HH_ERR_UNSUPPORTED, "strike partials are not carried through a basket");
  HH_HIP(ctx, hipSetDevice(ctx->device));
  double* term_dev = nullptr;
  rc = run_simulation(ctx, m, c, terminal, true, &term_dev);
  if (rc) return rc;

  hh::BasketArgs b{};
  b.n_paths = c->n_paths;
  b.n_chunks = hh::basket_chunks(c->n_paths);
  b.antithetic = c->antithetic;
  std::vector<double> payoffs(strikes, strikes + n_payoffs);  // strikes | cps
  payoffs.insert(payoffs.end(), cps, cps + n_payoffs);
  const double* payoffs_dev = nullptr;
  rc = stage_host(ctx, ctx->payoffs, payoffs.size(), payoffs.data(), payoffs.size(), &payoffs_dev);
  if (rc) return rc;
  rc = ensure(ctx, ctx->basket_records, (size_t)n_payoffs * b.n_chunks * hh::kRecStride);
  if (rc) return rc;
  b.terminal = term_dev;
  const int n_active = c->n_partials ? hh::count_active_partials(*m, *c) : 0;
  b.terminal_d = n_active ? ctx->terminal_d : nullptr;
  b.strikes = payoffs_dev;
  b.cps = payoffs_dev + n_payoffs;
  b.records = ctx->basket_records;
  HH_HIP(ctx, hh::launch_basket_payoffs(b, n_payoffs, (uint32_t)n_active, ctx->stream));
  HH_HIP(ctx, hh::launch_reduce_records(ctx->basket_records, b.n_chunks, (double)c->n_paths,
                                        accum_dev, ctx->stream, n_payoffs, m, c, true));
  if (c->strategy == HH_BROADIE_KAYA)  // the simulation's fall-back / series counters (the chain left its sums in
    HH_HIP(ctx, hh::launch_copy_bk_counters(ctx->accum, accum_dev, n_payoffs, ctx->stream));  // ctx->accum), for every payoff
  if ((rc = end_timing(ctx))) return rc;
  if ((rc = release_host_operands(ctx))) return rc;
  return copy_back_terminal(ctx, c, terminal);
}

int hh_mc_solve_basket(hh_ctx* ctx, const hh_model* m, const hh_config* c, const double* strikes,
                       const double* cps, uint32_t n_payoffs, hh_result* out, double* terminal) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!out) return fail(ctx, HH_ERR_INVALID, "result is NULL");
  const WallClock clock;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n_acc = (size_t)n_payoffs * HH_ACC_LEN;
  int rc = ensure(ctx, ctx->basket_accum, n_acc);
  if (rc) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  rc = hh_mc_accumulate_basket(ctx, m, c, strikes, cps, n_payoffs, ctx->basket_accum, terminal);
  if (rc) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  std::vector<double> host(n_acc);
  HH_HIP(ctx, hipMemcpyAsync(host.data(), ctx->basket_accum, n_acc * sizeof(double),
                             hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double kernel_ms, total_ms;
  if ((rc = solve_times(ctx, clock, &kernel_ms, &total_ms))) return rc;
  rc = finalize_results(m, 0, c, host.data(), n_payoffs, kernel_ms, total_ms, out);
  return rc ? finalize_failed(ctx, rc) : HH_OK;
}

int hh_mc_finalize(const hh_model* m, const hh_config* c, const double* acc, hh_result* out) {
  if (!m || !c || !acc || !out) return HH_ERR_INVALID;
  const double n = acc[HH_ACC_NPATHS];
  if (!(n >= 1.0)) return HH_ERR_INVALID;
  double mean, var;
  payoff_moments(acc, n, &mean, &var);
  out->sum_payoff = acc[HH_ACC_SUM];
  out->sumsq_payoff = acc[HH_ACC_SUMSQ];
  out->price = m->discount * mean;  // montecarlo.jl:489-490
  out->std_error = m->discount * std::sqrt(var / n);
  for (uint32_t k = 0; k < HH_MAX_PARTIALS; ++k) {
    double d = 0.0;
    if (k < c->n_partials) {
      const double dD = m->ddiscount ? m->ddiscount[k] : 0.0;
      d = dD * mean + m->discount * (acc[HH_ACC_DSUM + k] / n);
    }
    out->dprice[k] = d;
  }
  out->n_paths_done = (uint64_t)n;
  out->bk_newton_fail = (uint64_t)acc[HH_ACC_BK_NEWTON_FAIL];
  out->bk_bisect_fallback = (uint64_t)acc[HH_ACC_BK_BISECT];
  out->bk_maxguess_fallback = (uint64_t)acc[HH_ACC_BK_MAXGUESS];
  out->bk_cf_terms = (uint64_t)acc[HH_ACC_BK_CF_TERMS];
  return HH_OK;
}

int hh_mc_solve(hh_ctx* ctx, const hh_model* m, const hh_config* c, hh_result* out,
                double* terminal) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!out) return fail(ctx, HH_ERR_INVALID, "result is NULL");
  const WallClock clock;
  std::memset(out, 0, sizeof(*out));
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int rc = hh_mc_accumulate(ctx, m, c, ctx->accum, terminal);
  if (rc) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HH_HIP(ctx, hipMemcpyAsync(ctx->accum_host, ctx->accum, HH_ACC_LEN * sizeof(double),
                             hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  rc = hh_mc_finalize(m, c, ctx->accum_host, out);
  if (rc) return finalize_failed(ctx, rc);
  return solve_times(ctx, clock, &out->kernel_ms, &out->total_ms);
}

int hh_ctx_check_last(hh_ctx* ctx) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  return recover_finish(ctx);
}

int hh_bk_decisions(hh_ctx* ctx, uint64_t n_paths, uint32_t* decisions, uint32_t* series_len) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!ctx->bk_scratch || ctx->bk_last_n == 0 || n_paths != ctx->bk_last_n)
    return fail(ctx, HH_ERR_INVALID, "hh_bk_decisions: the last Broadie-Kaya solve of this context had %llu trajectories",
                (unsigned long long)ctx->bk_last_n);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t *dec = nullptr, *len = nullptr;
  hh::bk_diag_ptrs(ctx->bk_scratch, n_paths, ctx->bk_last_cache, &dec, &len);
  if (decisions)
    HH_HIP(ctx, hipMemcpyAsync(decisions, dec, n_paths * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (series_len)
    HH_HIP(ctx, hipMemcpyAsync(series_len, len, n_paths * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HH_OK;
}

// the quadrature cuts each of its 256 panels into at most hh::kCarrMadanMaxSubpanels (hh_fourier.hip)
#define HH_CM_BOUND_MSG "%s: bound/alpha must be <= 196608 (1024 sub-panels of half-width 0.75 alpha per lane)"
static_assert(hh::kCarrMadanMaxSubpanels * 192 == 196608, "HH_CM_BOUND_MSG names the limit");

int hh_carr_madan(hh_ctx* ctx, const hh_model* m, int32_t dynamics, int32_t compat_sqrt_alpha,
                  double alpha, double bound, double* price_out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!m || !price_out) return fail(ctx, HH_ERR_INVALID, "hh_carr_madan: NULL argument");
  if (dynamics != HH_LOGNORMAL && dynamics != HH_HESTON)
    return fail(ctx, HH_ERR_INVALID, "unknown dynamics %d", dynamics);
  if (!(m->S0 > 0.0) || !(m->strike > 0.0) || !(m->T > 0.0) || !(alpha > 0.0) || !(bound > 0.0) ||
      (m->cp != 1.0 && m->cp != -1.0) || (dynamics == HH_HESTON && m->sigma == 0.0))
    return fail(ctx, HH_ERR_INVALID, "hh_carr_madan: bad scalars");
  if (!hh::carr_madan_subpanels(alpha, bound)) return fail(ctx, HH_ERR_INVALID, HH_CM_BOUND_MSG, "hh_carr_madan");
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hh::launch_carr_madan(*m, dynamics, compat_sqrt_alpha, alpha, bound, ctx->accum,
                                    ctx->stream));
  HH_HIP(ctx, hipMemcpyAsync(ctx->accum_host, ctx->accum, sizeof(double), hipMemcpyDeviceToHost,
                             ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const double call = ctx->accum_host[0];
  // parity_transform (payoffs.jl:172-193): put = call − S + K·D
  *price_out = m->cp > 0.0 ? call : call - m->S0 + m->strike * m->discount;
  return HH_OK;
}

// The payoffs of a Carr–Madan basket (`who`: the entry point, for the messages) checked, packed as log K | T | r_drift |
// discount into host[0 .. 4n) and uploaded into ctx->payoffs, which is made to hold 4n + out_len doubles.
static int cm_upload_payoffs(hh_ctx* ctx, const char* who, const double* strikes, const double* cps, const double* Ts,
                             const double* r_drifts, const double* discounts, size_t n, size_t out_len,
                             std::vector<double>& host) {
  for (size_t k = 0; k < n; ++k) {
    if (!(strikes[k] > 0.0) || !(Ts[k] > 0.0) || (cps[k] != 1.0 && cps[k] != -1.0) ||
        !std::isfinite(r_drifts[k]) || !(discounts[k] > 0.0))
      return fail(ctx, HH_ERR_INVALID, "%s: payoff %zu: strike, T, discount > 0, cp = +-1", who, k);
    host[k] = std::log(strikes[k]);
    host[n + k] = Ts[k];
    host[2 * n + k] = r_drifts[k];
    host[3 * n + k] = discounts[k];
  }
  HH_HIP(ctx, hipSetDevice(ctx->device));
  int rc = ensure(ctx, ctx->payoffs, 4 * n + out_len);
  if (rc) return rc;
  HH_HIP(ctx, hipMemcpyAsync(ctx->payoffs, host.data(), 4 * n * sizeof(double), hipMemcpyHostToDevice,
                             ctx->stream));
  return HH_OK;
}

// One Carr–Madan basket entry point: who it is, what it refuses about the model and the rule, and what it launches.
struct CmBasket {
  const char* who;
  std::function<bool()> bad_scalars;  // the model's and the rule's scalars the entry point refuses …
  const char* bad_scalars_text;       // … and what it says then, after "<who>: "
  std::function<int()> law_check;     // the law's own parameters
  bool law_check_first;               // the forms that take a dynamics code name an unknown one before they count the payoffs
  std::function<int(const double* per_payoff_dev, uint32_t n_payoffs, double* out_dev)> launch;
};
struct CmPayoffs {
  const double *strikes, *cps, *Ts, *r_drifts, *discounts;
  uint32_t n;
};

// Everything of such a call up to the results on the host: the checks in the entry points' order, the upload, the launch
// and the copy back of `width` doubles per payoff into host[4n ..).
static int cm_basket_run(hh_ctx* ctx, const CmBasket& f, bool null_arg, double alpha, double bound, const CmPayoffs& q,
                         size_t width, std::vector<double>& host) {
  if (null_arg || !q.strikes || !q.cps || !q.Ts || !q.r_drifts || !q.discounts)
    return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", f.who);
  int rc;
  if (f.law_check_first && (rc = f.law_check())) return rc;
  if (q.n == 0 || q.n > (1u << 20)) return fail(ctx, HH_ERR_INVALID, "%s: 1 .. 2^20 payoffs per call", f.who);
  if (f.bad_scalars()) return fail(ctx, HH_ERR_INVALID, "%s: %s", f.who, f.bad_scalars_text);
  if (!f.law_check_first && (rc = f.law_check())) return rc;
  if (!hh::carr_madan_subpanels(alpha, bound)) return fail(ctx, HH_ERR_INVALID, HH_CM_BOUND_MSG, f.who);
  const size_t n = q.n;
  host.resize(4 * n + width * n);  // log K | T | r_drift | discount | out [n][width]
  if ((rc = cm_upload_payoffs(ctx, f.who, q.strikes, q.cps, q.Ts, q.r_drifts, q.discounts, n, width * n, host))) return rc;
  double* out_dev = ctx->payoffs + 4 * n;
  HH_HIP(ctx, f.launch(ctx->payoffs, q.n, out_dev));
  HH_HIP(ctx, hipMemcpyAsync(host.data() + 4 * n, out_dev, width * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HH_OK;
}

// parity_transform (payoffs.jl:172-193): put = call − S + K·D
static double cm_parity(double call, double cp, double S0, double strike, double discount) {
  return cp > 0.0 ? call : call - S0 + strike * discount;
}

// hh_carr_madan_basket, _jump, _bates and _vg: the call prices of the launch, puts by parity
static int carr_madan_basket_call(hh_ctx* ctx, const CmBasket& f, bool null_arg, const hh_model* m, double alpha, double bound,
                                  const CmPayoffs& q, double* prices_out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  std::vector<double> host;
  const int rc = cm_basket_run(ctx, f, null_arg || !m || !prices_out, alpha, bound, q, 1, host);
  if (rc) return rc;
  for (size_t k = 0, n = q.n; k < n; ++k)
    prices_out[k] = cm_parity(host[4 * n + k], q.cps[k], m->S0, q.strikes[k], q.discounts[k]);
  return HH_OK;
}

static int check_cm_dynamics(hh_ctx* ctx, int32_t dynamics) {
  if (dynamics != HH_LOGNORMAL && dynamics != HH_HESTON) return fail(ctx, HH_ERR_INVALID, "unknown dynamics %d", dynamics);
  return HH_OK;
}

int hh_carr_madan_basket(hh_ctx* ctx, const hh_model* m, int32_t dynamics, int32_t compat_sqrt_alpha,
                         double alpha, double bound, const double* strikes, const double* cps,
                         const double* Ts, const double* r_drifts, const double* discounts,
                         uint32_t n_payoffs, double* prices_out) {
  return carr_madan_basket_call(
      ctx,
      {"hh_carr_madan_basket",
       [&] { return !(m->S0 > 0.0) || !(alpha > 0.0) || !(bound > 0.0) || (dynamics == HH_HESTON && m->sigma == 0.0); },
       "bad scalars", [&] { return check_cm_dynamics(ctx, dynamics); }, true,
       [&](const double* per_payoff, uint32_t n, double* out) {
         return hh::launch_carr_madan_basket(*m, dynamics, compat_sqrt_alpha, alpha, bound, per_payoff, n, out, ctx->stream);
       }},
      false, m, alpha, bound, {strikes, cps, Ts, r_drifts, discounts, n_payoffs}, prices_out);
}

int hh_carr_madan_basket_grad(hh_ctx* ctx, const hh_model* m, int32_t dynamics,
                              int32_t compat_sqrt_alpha, double alpha, double bound,
                              const double* strikes, const double* cps, const double* Ts,
                              const double* r_drifts, const double* discounts, uint32_t n_payoffs,
                              double* prices_out, double* grad_out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  const CmBasket f = {
      "hh_carr_madan_basket_grad",
      [&] {
        return !(m->S0 > 0.0) || !(alpha > 0.0) || !(bound > 0.0) ||
               (dynamics == HH_HESTON && (m->sigma == 0.0 || m->theta == 0.0));
      },
      "bad scalars (Heston: sigma, theta != 0)", [&] { return check_cm_dynamics(ctx, dynamics); }, true,
      [&](const double* per_payoff, uint32_t n, double* out) {
        return hh::launch_carr_madan_grad(*m, dynamics, compat_sqrt_alpha, alpha, bound, per_payoff, n, out, ctx->stream);
      }};
  std::vector<double> host;
  const int rc = cm_basket_run(ctx, f, !m || !prices_out || !grad_out, alpha, bound,
                               {strikes, cps, Ts, r_drifts, discounts, n_payoffs}, HH_CM_GRAD_LEN, host);
  if (rc) return rc;
  for (size_t k = 0, n = n_payoffs; k < n; ++k) {
    const double* o = host.data() + 4 * n + HH_CM_GRAD_LEN * k;  // call, then d/d(S0 V0 κ θ σ ρ r_drift)
    double* g = grad_out + HH_CM_GRAD_LEN * k;
    for (int i = 0; i < 7; ++i) g[i] = o[1 + i];
    g[HH_CM_GRAD_DISCOUNT] = o[0] / discounts[k];  // the price is linear in the discount factor
    if (cps[k] < 0.0) {                            // the put's parity terms: −S0 + K·D
      g[HH_CM_GRAD_S0] -= 1.0;
      g[HH_CM_GRAD_DISCOUNT] += strikes[k];
    }
    prices_out[k] = cm_parity(o[0], cps[k], m->S0, strikes[k], discounts[k]);
  }
  return HH_OK;
}

size_t hh_lsm_grid_elems(uint64_t n_paths, uint32_t n_steps, int32_t antithetic) {
  return (size_t)(n_steps + 1) * n_paths * (antithetic ? 2 : 1);
}

// the buffers of a backward induction over ntot trajectories
static int ensure_lsm_buffers(hh_ctx* ctx, uint64_t ntot, uint32_t n_steps, int32_t degree) {
  int rc;
  if ((rc = ensure(ctx, ctx->lsm_val, (size_t)ntot))) return rc;
  if ((rc = ensure(ctx, ctx->lsm_tau, (size_t)ntot))) return rc;
  if ((rc = ensure(ctx, ctx->lsm_scratch, hh::lsm_scratch_doubles(ntot, n_steps, degree)))) return rc;
  return ensure(ctx, ctx->records, (size_t)hh::lsm_chunks(ntot) * hh::kRecStride);
}

// queue the copies back of an induction's row counters (regressed, skipped) into counters[0 .. 2) and, where the
// caller asked for them, of its stopping times and values
static int copy_back_lsm(hh_ctx* ctx, uint64_t ntot, uint32_t n_steps, int32_t degree, double* counters,
                         int32_t* stop_time, double* stop_value) {
  const hh::LsmScratch at(ntot, n_steps, degree);
  HH_HIP(ctx, hipMemcpyAsync(counters, ctx->lsm_scratch + at.counters, 2 * sizeof(double),
                             hipMemcpyDeviceToHost, ctx->stream));
  if (stop_time)
    HH_HIP(ctx, hipMemcpyAsync(stop_time, ctx->lsm_tau, ntot * sizeof(int32_t),
                               hipMemcpyDeviceToHost, ctx->stream));
  if (stop_value)
    HH_HIP(ctx, hipMemcpyAsync(stop_value, ctx->lsm_val, ntot * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
  return HH_OK;
}

// Backward induction on a spot grid already in device memory (rows = dates, ntot trajectories):
// launches, reduction and the copies back.  The caller recorded ctx->ev0 before producing the grid.
static int lsm_on_grid(hh_ctx* ctx, const double* grid_dev, uint64_t ntot, uint32_t n_steps,
                       const hh_model* m, int32_t degree, double step_discount, hh_lsm_result* out,
                       int32_t* stop_time, double* stop_value, const WallClock& clock) {
  const uint32_t ch = hh::lsm_chunks(ntot);
  const hh::LsmScratch at(ntot, n_steps, degree);
  int rc;
  if ((rc = ensure_lsm_buffers(ctx, ntot, n_steps, degree))) return rc;
  // enqueue the induction, the final reduction and every copy back, then synchronise ONCE; the
  // one-launch form leaves a word behind when its workgroups could not all be resident together
  // (another kernel held CUs): nothing was written then, and the launch-per-date form runs instead
  int form_used = hh::kLsmFormPerDate;
  // the small results land in PINNED memory behind the accumulator (a copy to the stack is staged
  // through the runtime's own buffer and costs ~10 µs apiece)
  double* counters = ctx->accum_host + HH_ACC_LEN;
  unsigned int& gave_up = *reinterpret_cast<unsigned int*>(ctx->accum_host + HH_ACC_LEN + 2);
  counters[0] = counters[1] = 0.0;
  int32_t fallbacks = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    const int form = attempt == 0 ? ctx->lsm_form : hh::kLsmFormPerDate;
    HH_HIP(ctx, hh::launch_lsm(grid_dev, ntot, n_steps, m->strike, m->cp, step_discount, degree,
                               ctx->lsm_tau, ctx->lsm_val, ctx->lsm_scratch, ctx->records,
                               ctx->stream, form, &form_used,
                               ctx->lsm_spin_ticks < 0 ? 100000000ull : (unsigned long long)ctx->lsm_spin_ticks));
    HH_HIP(ctx, hh::launch_reduce_records(ctx->records, ch, (double)ntot, ctx->accum, ctx->stream));
    HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    gave_up = 0;
    if (form_used == hh::kLsmFormPersistent)
      HH_HIP(ctx, hipMemcpyAsync(&gave_up, hh::lsm_persistent_status(ctx->lsm_scratch, at),
                                 sizeof(gave_up), hipMemcpyDeviceToHost, ctx->stream));
    HH_HIP(ctx, hipMemcpyAsync(ctx->accum_host, ctx->accum, HH_ACC_LEN * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = copy_back_lsm(ctx, ntot, n_steps, degree, counters, stop_time, stop_value))) return rc;
    HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!gave_up) break;
    ++ctx->lsm_persistent_fallbacks;
    ++fallbacks;
  }
  // the reduction wrote (double)ntot into slot HH_ACC_NPATHS
  if ((rc = hh_lsm_finalize(ctx->accum_host, out))) return finalize_failed(ctx, rc);
  out->rows_regressed = (uint32_t)counters[0];
  out->rows_skipped = (uint32_t)counters[1];
  out->form = form_used;
  out->persistent_fallbacks = fallbacks;
  return solve_times(ctx, clock, &out->kernel_ms, &out->total_ms);
}

static int lsm_check_scalars(hh_ctx* ctx, const hh_model* m, const hh_config* c, int32_t degree,
                             double step_discount) {
  if (c->n_paths == 0 || c->n_steps == 0 || degree < 1 || degree > 8)
    return fail(ctx, HH_ERR_INVALID, "LSM: n_paths, n_steps >= 1, 1 <= degree <= 8");
  if (c->n_paths > kMaxPaths / 2 || c->n_steps > kMaxGridSteps)
    return fail(ctx, HH_ERR_INVALID, "LSM: at most 2^31 - 128 trajectories (x2 antithetic) and %u steps",
                kMaxGridSteps);
  if (!(m->S0 > 0.0) || !(m->T > 0.0) || (m->cp != 1.0 && m->cp != -1.0) ||
      !(step_discount > 0.0) || !std::isfinite(step_discount))
    return fail(ctx, HH_ERR_INVALID, "LSM: bad model scalars");
  return HH_OK;
}

// seeds of the trajectories in device memory (staged if the caller's are on the host)
static int stage_path_seeds(hh_ctx* ctx, const hh_config* c, const uint64_t** out) {
  if (!c->seeds) return fail(ctx, HH_ERR_INVALID, "GENERATE needs seeds");
  if (c->seeds_len && c->seeds_len < c->n_paths)
    return fail(ctx, HH_ERR_INVALID, "Number of seeds (%llu) must be >= number of trajectories (%llu)",
                (unsigned long long)c->seeds_len, (unsigned long long)c->n_paths);
  *out = c->seeds;
  if (c->seeds_on_device) return HH_OK;
  return stage_host(ctx, ctx->seeds, (size_t)c->n_paths, c->seeds, (size_t)c->n_paths, out);
}

// The n_steps Broadie–Kaya transitions of length T/n_steps into ctx->lsm_grid (spot rows) and
// ctx->heston_var (variance rows); per-transition accumulator vectors (BK counters) into
// ctx->basket_accum[n_steps][HH_ACC_LEN].
static int run_heston_grid(hh_ctx* ctx, const hh_model* m, const hh_config* c) {
  if (c->dynamics != HH_HESTON || c->strategy != HH_BROADIE_KAYA)
    return fail(ctx, HH_ERR_UNSUPPORTED, "exact Heston grid needs HestonDynamics + HestonBroadieKaya");
  if (c->noise_mode != HH_NOISE_GENERATE || c->n_partials != 0 || c->antithetic)
    return fail(ctx, HH_ERR_UNSUPPORTED,
                "exact Heston grid: GENERATE noise, no dual partials, no antithetic form");
  if (c->n_paths == 0 || c->n_steps == 0 || c->n_paths > kMaxPaths || c->n_steps > kMaxGridSteps)
    return fail(ctx, HH_ERR_INVALID, "exact Heston grid: 1 <= n_paths <= 2^32 - 256, 1 <= n_steps <= %u",
                kMaxGridSteps);
  if (!(m->S0 > 0.0) || !(m->T > 0.0) || !std::isfinite(m->S0) || !std::isfinite(m->T) ||
      !(std::fabs(m->rho) <= 1.0) || m->sigma == 0.0 || m->kappa == 0.0 || !(m->V0 > 0.0) ||
      !std::isfinite(m->sigma) || !std::isfinite(m->kappa) || !std::isfinite(m->theta) ||
      !std::isfinite(m->V0) || !std::isfinite(m->r_drift) ||
      !bk_law_ok(m, m->T / (double)c->n_steps))
    return fail(ctx, HH_ERR_INVALID,
                "exact Heston grid: S0, T, V0 > 0, |rho| <= 1, 1e-8 <= 4 kappa theta / sigma^2 <= 1e6, all finite (|kappa dt| < 700)");
  const uint64_t n = c->n_paths;
  const size_t grid_elems = (size_t)(c->n_steps + 1) * n;
  // dates per kernel chain: given the variance rows, the CF inversions of different dates are
  // independent, so a batch of dates runs as ONE chain over its (date, trajectory) pairs
  uint32_t per_chain = ctx->grid_form == HH_GRID_FORM_BATCHED ? hh::bk_grid_dates_per_chain(n, c->n_steps) : 1u;
  int rc;
  if ((rc = ensure(ctx, ctx->lsm_grid, grid_elems))) return rc;
  if ((rc = ensure(ctx, ctx->heston_var, grid_elems))) return rc;
  // a chain's scratch is 48 bytes per (date, trajectory) pair beside the fixed term cache: on a device
  // that cannot spare it (shared with another allocator) the dates go into shorter chains, down to one
  // chain per date — same bits either way
  uint64_t n_chain = n * per_chain;
  while ((rc = ensure_bk_scratch(ctx, hh::bk_scratch_bytes(n_chain, ctx->bk_term_cache))) == HH_ERR_NOMEM &&
         per_chain > 1) {
    per_chain = (per_chain + 1) / 2;
    n_chain = n * per_chain;
  }
  if (rc) return rc;
  if ((rc = ensure(ctx, ctx->records, (size_t)hh::bk_record_count(n_chain) * hh::kRecStride))) return rc;
  if ((rc = ensure(ctx, ctx->basket_accum, (size_t)c->n_steps * HH_ACC_LEN))) return rc;
  hh::DevicePtrs p{};
  p.records = ctx->records;
  p.bk_scratch = ctx->bk_scratch;
  p.bk_table_key = &ctx->bk_table_key;
  p.bk_term_cache = ctx->bk_term_cache;
  if (per_chain > 1 && ctx->grid_order) {  // the batched chains run their pairs in the order of their Bessel arguments
    if ((rc = ensure(ctx, ctx->bk_sort, hh::bk_grid_sort_bytes(n_chain)))) return rc;
    p.bk_sort = ctx->bk_sort;
  }
  if ((rc = stage_path_seeds(ctx, c, &p.seeds))) return rc;
  HH_HIP(ctx, hh::launch_fill_rows(ctx->lsm_grid, ctx->heston_var, n, m->S0, m->V0, ctx->stream));
  hh_model step_model = *m;
  step_model.T = m->T / (double)c->n_steps;  // dt of solve(NoiseProblem; dt = T / steps)
  step_model.cp = 1.0;
  hh_config step_cfg = *c;
  step_cfg.path_offset = 0;
  if (per_chain > 1) {
    HH_HIP(ctx, hipMemsetAsync(ctx->basket_accum, 0, (size_t)c->n_steps * HH_ACC_LEN * sizeof(double),
                               ctx->stream));
    for (uint32_t k = 0; k < c->n_steps; k += per_chain) {
      const uint32_t nd = std::min(per_chain, c->n_steps - k);
      p.accum = ctx->basket_accum + (size_t)k * HH_ACC_LEN;  // the counters of the batch's pairs, kept in the slot of its first date
      HH_HIP(ctx, hh::launch_bk_grid(step_model, step_cfg, p, ctx->stream, ctx->lsm_grid + (size_t)k * n,
                                     ctx->heston_var + (size_t)k * n, k, nd, /*upload_tables=*/k == 0));
    }
    return HH_OK;
  }
  for (uint32_t k = 0; k < c->n_steps; ++k) {
    const hh::BkTransition tr{ctx->lsm_grid + (size_t)k * n, ctx->heston_var + (size_t)k * n,
                              ctx->lsm_grid + (size_t)(k + 1) * n,
                              ctx->heston_var + (size_t)(k + 1) * n, k};
    p.accum = ctx->basket_accum + (size_t)k * HH_ACC_LEN;
    HH_HIP(ctx, hh::launch_bk(step_model, step_cfg, p, ctx->stream, &tr, /*upload_tables=*/k == 0));
  }
  return HH_OK;
}

// BK counters of all transitions, summed
static int heston_grid_counters(hh_ctx* ctx, uint32_t n_steps, uint64_t* newton_fail,
                                uint64_t* bisect, uint64_t* maxguess, uint64_t* cf_terms) {
  std::vector<double> acc((size_t)n_steps * HH_ACC_LEN);
  HH_HIP(ctx, hipMemcpyAsync(acc.data(), ctx->basket_accum, acc.size() * sizeof(double),
                             hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double f = 0, b = 0, g = 0, t = 0;
  for (uint32_t k = 0; k < n_steps; ++k) {
    const double* a = acc.data() + (size_t)k * HH_ACC_LEN;
    f += a[HH_ACC_BK_NEWTON_FAIL]; b += a[HH_ACC_BK_BISECT];
    g += a[HH_ACC_BK_MAXGUESS]; t += a[HH_ACC_BK_CF_TERMS];
  }
  *newton_fail = (uint64_t)f; *bisect = (uint64_t)b; *maxguess = (uint64_t)g; *cf_terms = (uint64_t)t;
  return HH_OK;
}

// The end of a grid entry point, once ctx->ev1 is recorded behind the grid: the spot and variance rows into the
// caller's buffers (device or host memory), then *out — with the summed Broadie–Kaya counters of the transitions
// for the exact Heston grid (bk_counters).
static int grid_results(hh_ctx* ctx, const hh_config* c, double* spot_grid, double* var_grid,
                        int32_t grids_on_device, bool bk_counters, hh_result* out, const WallClock& clock) {
  const size_t bytes = hh_lsm_grid_elems(c->n_paths, c->n_steps, c->antithetic) * sizeof(double);
  const hipMemcpyKind kind = grids_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (spot_grid) HH_HIP(ctx, hipMemcpyAsync(spot_grid, ctx->lsm_grid, bytes, kind, ctx->stream));
  if (var_grid) HH_HIP(ctx, hipMemcpyAsync(var_grid, ctx->heston_var, bytes, kind, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!out) return HH_OK;
  std::memset(out, 0, sizeof(*out));
  int rc;
  if (bk_counters && (rc = heston_grid_counters(ctx, c->n_steps, &out->bk_newton_fail, &out->bk_bisect_fallback,
                                                &out->bk_maxguess_fallback, &out->bk_cf_terms)))
    return rc;
  out->n_paths_done = c->n_paths;
  return solve_times(ctx, clock, &out->kernel_ms, &out->total_ms);
}

// the spot grid an LSM solve regressed on, into the caller's host buffer (when given)
static int copy_back_spot_grid(hh_ctx* ctx, const hh_config* c, double* spot_grid) {
  if (!spot_grid) return HH_OK;
  HH_HIP(ctx, hipMemcpyAsync(spot_grid, ctx->lsm_grid,
                             hh_lsm_grid_elems(c->n_paths, c->n_steps, c->antithetic) * sizeof(double),
                             hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HH_OK;
}

// The paths of an LSM solve into ctx->lsm_grid, after the checks.  The reference's LSM regresses on the first state
// component of simulate_paths' solution (least_squares_montecarlo.jl:53,76).  Path sources: the GBM noise process of
// (LognormalDynamics, BlackScholesExact) (montecarlo.jl:140-159), whose state IS the spot, and the per-date exact
// Heston transitions of (HestonDynamics, HestonBroadieKaya) (montecarlo.jl:209-231), whose spot rows exp(log S) are
// used here (the reference hands its regression the log-state).  start (when given) is recorded in
// front of the grid.
static int lsm_paths(hh_ctx* ctx, const hh_model* m, const hh_config* c, int32_t degree, double step_discount,
                     hipEvent_t start) {
  const bool gbm = c->dynamics == HH_LOGNORMAL && c->strategy == HH_EXACT_LAW;
  const bool heston = c->dynamics == HH_HESTON && c->strategy == HH_BROADIE_KAYA;
  if (!gbm && !heston)
    return fail(ctx, HH_ERR_UNSUPPORTED,
                "LSM needs LognormalDynamics + BlackScholesExact or HestonDynamics + "
                "HestonBroadieKaya paths");
  if (c->noise_mode != HH_NOISE_GENERATE || c->n_partials != 0)
    return fail(ctx, HH_ERR_UNSUPPORTED, "LSM: GENERATE noise, no dual partials");
  int rc = lsm_check_scalars(ctx, m, c, degree, step_discount);
  if (rc) return rc;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  if (start) HH_HIP(ctx, hipEventRecord(start, ctx->stream));
  if (heston) return run_heston_grid(ctx, m, c);
  if ((rc = ensure(ctx, ctx->lsm_grid, hh_lsm_grid_elems(c->n_paths, c->n_steps, c->antithetic)))) return rc;
  const uint64_t* seeds_dev = nullptr;
  if ((rc = stage_path_seeds(ctx, c, &seeds_dev))) return rc;
  HH_HIP(ctx, hh::launch_gbm_grid(seeds_dev, c->n_paths, c->n_steps, m->S0, m->r_drift, m->sigma,
                                  m->T, c->antithetic, ctx->lsm_grid, ctx->stream));
  return HH_OK;
}

int hh_heston_exact_grid(hh_ctx* ctx, const hh_model* m, const hh_config* c, double* spot_grid,
                         double* var_grid, int32_t grids_on_device, hh_result* out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!m || !c) return fail(ctx, HH_ERR_INVALID, "hh_heston_exact_grid: NULL argument");
  const WallClock clock;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int rc = run_heston_grid(ctx, m, c);
  if (rc) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  return grid_results(ctx, c, spot_grid, var_grid, grids_on_device, /*bk_counters=*/true, out, clock);
}

int hh_lsm_solve(hh_ctx* ctx, const hh_model* m, const hh_config* c, int32_t degree,
                 double step_discount, hh_lsm_result* out, int32_t* stop_time, double* stop_value,
                 double* spot_grid) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!m || !c || !out) return fail(ctx, HH_ERR_INVALID, "hh_lsm_solve: NULL argument");
  const WallClock clock;
  int rc = lsm_paths(ctx, m, c, degree, step_discount, ctx->ev0);
  if (rc) return rc;
  const uint64_t ntot = c->n_paths * (c->antithetic ? 2 : 1);
  rc = lsm_on_grid(ctx, ctx->lsm_grid, ntot, c->n_steps, m, degree, step_discount, out, stop_time,
                   stop_value, clock);
  if (rc) return rc;
  return copy_back_spot_grid(ctx, c, spot_grid);
}

// ---- Euler–Maruyama path grids (GENERATE) -------------------------------------------------------------

// The Euler states of every date into ctx->lsm_grid (spot or log-spot rows, hh_path_state) and, want_var, the
// Heston variance rows into ctx->heston_var.  The grid is [n_steps+1][n_paths·(1+antithetic)] (hh_lsm_grid_elems).
static int run_euler_grid(hh_ctx* ctx, const hh_model* m, const hh_config* c, int32_t path_state, bool want_var) {
  if (path_state != HH_PATH_SPOT && path_state != HH_PATH_LOG)
    return fail(ctx, HH_ERR_INVALID, "path_state must be HH_PATH_SPOT (0) or HH_PATH_LOG (1)");
  const bool hest = c->dynamics == HH_HESTON;
  if (c->strategy != HH_EULER_MARUYAMA || (c->dynamics != HH_LOGNORMAL && !hest))
    return fail(ctx, HH_ERR_UNSUPPORTED, "Euler grid needs LognormalDynamics or HestonDynamics + EulerMaruyama");
  if (c->noise_mode != HH_NOISE_GENERATE || c->n_partials != 0)
    return fail(ctx, HH_ERR_UNSUPPORTED, "Euler grid: GENERATE noise, no dual partials");
  if (want_var && !hest)
    return fail(ctx, HH_ERR_UNSUPPORTED, "Euler grid: variance rows belong to HestonDynamics");
  if (c->n_paths == 0 || c->n_steps == 0 || c->n_paths > kMaxPaths / 2 || c->n_steps > kMaxGridSteps)
    return fail(ctx, HH_ERR_INVALID, "Euler grid: 1 <= n_paths <= 2^31 - 128, 1 <= n_steps <= %u", kMaxGridSteps);
  if (!(m->S0 > 0.0) || !(m->T > 0.0) || !std::isfinite(m->S0) || !std::isfinite(m->T) ||
      !std::isfinite(m->sigma) || !std::isfinite(m->r_drift) ||
      (hest && (!(std::fabs(m->rho) <= 1.0) || !std::isfinite(m->V0) || !std::isfinite(m->kappa) ||
                !std::isfinite(m->theta))))
    return fail(ctx, HH_ERR_INVALID, "Euler grid: S0, T > 0, |rho| <= 1, model scalars finite");
  const size_t elems = hh_lsm_grid_elems(c->n_paths, c->n_steps, c->antithetic);
  int rc;
  if ((rc = ensure(ctx, ctx->lsm_grid, elems))) return rc;
  if (want_var && (rc = ensure(ctx, ctx->heston_var, elems))) return rc;
  const uint64_t* seeds_dev = nullptr;
  if ((rc = stage_path_seeds(ctx, c, &seeds_dev))) return rc;
  HH_HIP(ctx, hh::launch_euler_grid(*m, *c, seeds_dev, path_state == HH_PATH_LOG, ctx->lsm_grid,
                                    want_var ? ctx->heston_var : nullptr, ctx->stream));
  return HH_OK;
}

int hh_euler_grid(hh_ctx* ctx, const hh_model* m, const hh_config* c, int32_t path_state, double* spot_grid,
                  double* var_grid, int32_t grids_on_device, hh_result* out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!m || !c) return fail(ctx, HH_ERR_INVALID, "hh_euler_grid: NULL argument");
  const WallClock clock;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int rc = run_euler_grid(ctx, m, c, path_state, var_grid != nullptr);
  if (rc) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  return grid_results(ctx, c, spot_grid, var_grid, grids_on_device, /*bk_counters=*/false, out, clock);
}

int hh_lsm_solve_euler(hh_ctx* ctx, const hh_model* m, const hh_config* c, int32_t path_state, int32_t degree,
                       double step_discount, hh_lsm_result* out, int32_t* stop_time, double* stop_value,
                       double* spot_grid) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!m || !c || !out) return fail(ctx, HH_ERR_INVALID, "hh_lsm_solve_euler: NULL argument");
  const WallClock clock;
  int rc = lsm_check_scalars(ctx, m, c, degree, step_discount);
  if (rc) return rc;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if ((rc = run_euler_grid(ctx, m, c, path_state, false))) return rc;
  const uint64_t ntot = c->n_paths * (c->antithetic ? 2 : 1);
  rc = lsm_on_grid(ctx, ctx->lsm_grid, ntot, c->n_steps, m, degree, step_discount, out, stop_time, stop_value, clock);
  if (rc) return rc;
  return copy_back_spot_grid(ctx, c, spot_grid);
}

// ---- path-dependent payoffs on Euler–Maruyama paths (GENERATE) ---------------------------------------------

// the call's next kernels go into a timing slot of their own (closed by end_timing)
static int begin_timing(hh_ctx* ctx) {
  if (ctx->timing) HH_HIP(ctx, hipEventRecord(ctx->tev[ctx->t_count % hh_ctx::kTimingSlots][0], ctx->stream));
  return HH_OK;
}

// rows of the statistics under `extremes` (enum hh_path_extremes, validated)
static int path_stat_rows(int32_t extremes) { return extremes == HH_EXTREMES_BRIDGE ? HH_PATH_STATS_BRIDGE : HH_PATH_STATS; }

// The jump parameters of a Merton entry point (`who`); span: what one Poisson draw covers (T, or T/n_steps).
static int check_jump(hh_ctx* ctx, const char* who, const hh_jump* jump, double span) {
  if (!(jump->lambda >= 0.0) || !std::isfinite(jump->lambda))
    return fail(ctx, HH_ERR_INVALID, "%s: jump lambda must be finite and >= 0", who);
  if (!(jump->sigma_j >= 0.0) || !std::isfinite(jump->sigma_j))
    return fail(ctx, HH_ERR_INVALID, "%s: jump sigma_j must be finite and >= 0", who);
  if (!std::isfinite(jump->mu_j)) return fail(ctx, HH_ERR_INVALID, "%s: jump mu_j must be finite", who);
  if (!std::isfinite(hh::merton_compensator(*jump)))
    return fail(ctx, HH_ERR_INVALID, "%s: exp(mu_j + sigma_j^2/2) must be finite", who);
  if (!(jump->lambda * span <= HH_JUMP_MAX_MEAN))
    return fail(ctx, HH_ERR_INVALID, "%s: the Poisson mean of one draw, lambda * %g = %g, is above HH_JUMP_MAX_MEAN = %g", who,
                span, jump->lambda * span, (double)HH_JUMP_MAX_MEAN);
  return HH_OK;
}

// The parameters of a Variance Gamma entry point (`who`) with the model's σ; p: the moment of S_T the entry point needs
// finite — 1 for the martingale compensator ω, 1 + α under the damped transform.
static int check_vg(hh_ctx* ctx, const char* who, const hh_model* m, const hh_vg* vg, double p) {
  if (!(vg->nu > 0.0) || !std::isfinite(vg->nu)) return fail(ctx, HH_ERR_INVALID, "%s: vg nu must be finite and > 0", who);
  if (!std::isfinite(vg->theta)) return fail(ctx, HH_ERR_INVALID, "%s: vg theta must be finite", who);
  if (!(m->sigma >= 0.0)) return fail(ctx, HH_ERR_INVALID, "%s: sigma must be >= 0", who);
  if (!(hh::vg_moment_arg(m->sigma, *vg, 1.0) > 0.0))
    return fail(ctx, HH_ERR_INVALID, "%s: 1 - theta nu - sigma^2 nu / 2 = %g must be > 0 (E S_T is infinite otherwise)", who,
                hh::vg_moment_arg(m->sigma, *vg, 1.0));
  if (p != 1.0 && !(hh::vg_moment_arg(m->sigma, *vg, p) > 0.0))
    return fail(ctx, HH_ERR_INVALID,
                "%s: 1 - theta nu (1 + alpha) - sigma^2 nu (1 + alpha)^2 / 2 = %g must be > 0 (the damped transform needs the "
                "(1 + alpha)-th moment)", who, hh::vg_moment_arg(m->sigma, *vg, p));
  return HH_OK;
}

// The assets and the index of a multi-asset entry point (`who`): everything that does not depend on the model or the
// configuration, the positive definiteness of the correlation matrix included.
static int check_assets(hh_ctx* ctx, const char* who, const hh_assets* as) {
  if (as->n_assets < 1u || as->n_assets > (uint32_t)HH_MAX_ASSETS)
    return fail(ctx, HH_ERR_INVALID, "%s: n_assets (%u) must lie in 1 .. %d", who, as->n_assets, HH_MAX_ASSETS);
  if (as->index_kind < HH_INDEX_WEIGHTED_SUM || as->index_kind > HH_INDEX_WORST_OF)
    return fail(ctx, HH_ERR_INVALID, "%s: unknown index_kind %d", who, as->index_kind);
  const bool extreme = as->index_kind == HH_INDEX_BEST_OF || as->index_kind == HH_INDEX_WORST_OF;
  bool any_weight = false;
  for (uint32_t i = 0; i < as->n_assets; ++i) {
    if (!(as->spots[i] > 0.0) || !std::isfinite(as->spots[i]))
      return fail(ctx, HH_ERR_INVALID, "%s: asset %u: the spot must be finite and > 0", who, i);
    if (!(as->sigmas[i] >= 0.0) || !std::isfinite(as->sigmas[i]))
      return fail(ctx, HH_ERR_INVALID, "%s: asset %u: sigma must be finite and >= 0", who, i);
    if (!std::isfinite(as->weights[i])) return fail(ctx, HH_ERR_INVALID, "%s: asset %u: the weight must be finite", who, i);
    if (extreme && !(as->weights[i] > 0.0))
      return fail(ctx, HH_ERR_INVALID, "%s: asset %u: a best-of / worst-of weight must be > 0", who, i);
    any_weight = any_weight || as->weights[i] != 0.0;
  }
  if (as->index_kind == HH_INDEX_WEIGHTED_SUM && !any_weight)
    return fail(ctx, HH_ERR_INVALID, "%s: every weight of the weighted sum is zero", who);
  if (const char* defect = hh::corr_defect(*as)) return fail(ctx, HH_ERR_INVALID, "%s: %s", who, defect);
  double L[hh::kAssetsTri];
  if (!hh::cholesky(as->corr, as->n_assets, L))
    return fail(ctx, HH_ERR_INVALID, "%s: the correlation matrix is not positive definite", who);
  return HH_OK;
}

// The scalars of a quadratic-exponential entry point (`who`), after the checks every path entry point makes.
static int check_qe(hh_ctx* ctx, const char* who, const hh_model* m, const hh_config* c, const hh_qe* qe) {
  if (!(m->kappa > 0.0) || !(m->theta > 0.0) || !(m->sigma > 0.0) || !(m->V0 >= 0.0))
    return fail(ctx, HH_ERR_INVALID, "%s: kappa, theta, sigma must be > 0 and V0 >= 0", who);
  // ψ <= σ²/(2κθ) in every state (its maximum over v >= 0): bounded, 1 − p = 2/(ψ + 1) stays far from rounding to 0
  if (!((m->sigma * m->sigma) / (2.0 * m->kappa * m->theta) <= HH_QE_MAX_PSI))
    return fail(ctx, HH_ERR_INVALID, "%s: sigma^2 / (2 kappa theta) = %g is above HH_QE_MAX_PSI = %g", who,
                (m->sigma * m->sigma) / (2.0 * m->kappa * m->theta), (double)HH_QE_MAX_PSI);
  if (!(qe->psi_c == 0.0 || (qe->psi_c >= 1.0 && qe->psi_c <= 2.0)))
    return fail(ctx, HH_ERR_INVALID, "%s: psi_c must be 0 (the default 1.5) or lie in [1, 2]", who);
  const hh::QeArgs q = hh::qe_launch_args(*m, *c, *qe);
  const double all[] = {q.E, q.c1, q.c2, q.th_ome, q.rdt, q.K0, q.K1, q.K2, q.K3, q.A, q.k13};
  for (double t : all)
    if (!std::isfinite(t)) return fail(ctx, HH_ERR_INVALID, "%s: the step's constants are not finite", who);
  if (!(q.th_ome > 0.0) || !(q.c2 > 0.0))
    return fail(ctx, HH_ERR_INVALID, "%s: kappa * dt is so small that 1 - exp(-kappa * dt) or the step's variance rounds to 0", who);
  if (qe->martingale && q.A > 0.0)
    return fail(ctx, HH_ERR_UNSUPPORTED,
                "%s: the martingale correction needs A = K2 + K4/2 <= 0 (every rho <= 0 gives that), A = %g: run without it",
                who, q.A);
  return HH_OK;
}

// The surface of a local-volatility entry point (`who`): everything that does not depend on the model or the configuration.
static int check_localvol(hh_ctx* ctx, const char* who, const hh_localvol* lv) {
  if (!lv->times || !lv->vols) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument (the surface's times or vols)", who);
  if (lv->n_times < 1u || lv->n_x < 2u)
    return fail(ctx, HH_ERR_INVALID, "%s: the surface needs n_times >= 1 and n_x >= 2 (%u, %u)", who, lv->n_times, lv->n_x);
  if ((uint64_t)lv->n_times * lv->n_x > (uint64_t)HH_LV_MAX_NODES)
    return fail(ctx, HH_ERR_INVALID, "%s: n_times * n_x = %llu is above HH_LV_MAX_NODES = %d", who,
                (unsigned long long)lv->n_times * lv->n_x, HH_LV_MAX_NODES);
  if (!std::isfinite(lv->x_lo)) return fail(ctx, HH_ERR_INVALID, "%s: x_lo must be finite", who);
  if (!(lv->h > 0.0) || !std::isfinite(lv->h) || !std::isfinite(1.0 / lv->h))
    return fail(ctx, HH_ERR_INVALID, "%s: h must be finite and > 0", who);
  for (uint32_t j = 0; j < lv->n_times; ++j) {
    if (!(lv->times[j] >= 0.0) || !std::isfinite(lv->times[j]))
      return fail(ctx, HH_ERR_INVALID, "%s: times[%u] must be finite and >= 0", who, j);
    if (j && !(lv->times[j] > lv->times[j - 1]))
      return fail(ctx, HH_ERR_INVALID, "%s: times must be strictly increasing (times[%u])", who, j);
  }
  const size_t n_nodes = (size_t)lv->n_times * lv->n_x;
  for (size_t q = 0; q < n_nodes; ++q)
    if (!(lv->vols[q] > 0.0) || !std::isfinite(lv->vols[q]))
      return fail(ctx, HH_ERR_INVALID, "%s: vols[%u][%u] must be finite and > 0", who, (unsigned)(q / lv->n_x),
                  (unsigned)(q % lv->n_x));
  return HH_OK;
}

// The table, then w_k and j_k of every step (hh_localvol.h: localvol_row on t_k = (double)k·dt, dt as make_args forms
// it), staged as one block; *out: what the kernel reads.
static int stage_localvol(hh_ctx* ctx, const hh_localvol* lv, double T, uint32_t n_steps, hh::LocalVolArgs* out) {
  const size_t n_nodes = (size_t)lv->n_times * lv->n_x;
  std::vector<double> host(hh::localvol_stage_doubles(lv->n_times, lv->n_x, n_steps), 0.0);
  std::memcpy(host.data(), lv->vols, n_nodes * sizeof(double));
  double* const w = host.data() + n_nodes;
  uint32_t* const rows = reinterpret_cast<uint32_t*>(w + n_steps);
  const double dt = T / (double)n_steps;
  for (uint32_t k = 0; k < n_steps; ++k) {
    const hh::LocalVolRow r = hh::localvol_row(lv->times, lv->n_times, (double)k * dt);
    w[k] = r.w;
    rows[k] = r.j;
  }
  const double* dev = nullptr;
  const int rc = stage_host(ctx, ctx->localvol, host.size(), host.data(), host.size(), &dev);
  if (rc) return rc;
  out->vols = dev;
  out->step_w = dev + n_nodes;
  out->step_row = reinterpret_cast<const uint32_t*>(dev + n_nodes + n_steps);
  out->x_lo = lv->x_lo;
  out->inv_h = 1.0 / lv->h;
  out->n_times = lv->n_times;
  out->n_x = lv->n_x;
  return HH_OK;
}

// The path-statistics family: which kernel an entry point runs and what travels with it — one constructor per kernel.
struct PathFamily {
  enum Kernel { kEuler, kJump, kQe, kBates, kAssets, kLocalVol, kCoupled, kVg } kernel;
  enum CoupledForm { kCoupledForm };  // names the constructor of the coupled form
  const char* who;                           // the entry point, as its messages name it
  int32_t last_kind;                         // the last payoff kind it admits (the solve forms)
  int32_t extremes = HH_EXTREMES_MONITORED;  // enum hh_path_extremes: the bridge form is path_stats_kernel's alone
  const hh_jump* jump = nullptr;
  const hh_qe* qe = nullptr;
  const hh_assets* assets = nullptr;
  const hh_localvol* localvol = nullptr;
  const hh_vg* vg = nullptr;
  double* var_T = nullptr;  // host, nullable: the variance at expiry of every member (the QE step)
  bool missing = false;     // a struct the kernel needs came as NULL: the entry point's "NULL argument"
  bool date_rows = false;   // the kernel's date-row sibling: the grid into ctx->lsm_grid, no statistics (hh_mc_path_grid)
  bool state_rows = false;  // with date_rows: the state-row sibling instead — (x, v) per date (hh_mc_path_states; kEuler
                            // under Heston dynamics, kQe, kBates)
  bool tangent = false;     // path_tangent_kernel: the statistics with their tangents, cfg->n_partials directions (kEuler)
  // path_stats_kernel: lognormal or Heston dynamics by Euler–Maruyama
  PathFamily(const char* w, int32_t last, int32_t ext) : kernel(kEuler), who(w), last_kind(last), extremes(ext) {}
  // jump_stats_kernel, the Merton form: lognormal dynamics
  PathFamily(const char* w, int32_t last, const hh_jump* j) : kernel(kJump), who(w), last_kind(last), jump(j), missing(!j) {}
  // qe_stats_kernel: the quadratic-exponential Heston step
  PathFamily(const char* w, int32_t last, const hh_qe* q, double* v)
      : kernel(kQe), who(w), last_kind(last), qe(q), var_T(v), missing(!q) {}
  // bates_stats_kernel: that step with jumps, its constants formed on r_c = r_drift − λκ̄
  PathFamily(const char* w, int32_t last, const hh_qe* q, const hh_jump* j, double* v)
      : kernel(kBates), who(w), last_kind(last), jump(j), qe(q), var_T(v), missing(!q || !j) {}
  // assets_stats_kernel: the index of several correlated lognormal assets; of the model only T, r_drift, discount are read
  PathFamily(const char* w, int32_t last, const hh_assets* a) : kernel(kAssets), who(w), last_kind(last), assets(a), missing(!a) {}
  // localvol_stats_kernel: lognormal dynamics by Euler–Maruyama with the σ of every step read from the surface; both
  // extremes forms; model->sigma is not read
  PathFamily(const char* w, int32_t last, const hh_localvol* lv, int32_t ext)
      : kernel(kLocalVol), who(w), last_kind(last), extremes(ext), localvol(lv), missing(!lv) {}
  // coupled_stats_kernel: path_stats_kernel's monitored trajectories on cfg->n_steps steps, each with its partner on
  // half as many steps and the summed increments (multilevel Monte Carlo)
  PathFamily(const char* w, int32_t last, CoupledForm) : kernel(kCoupled), who(w), last_kind(last) {}
  // vg_stats_kernel: the Variance Gamma increments, exact in law on any dates — lognormal dynamics, HH_EXACT_LAW
  PathFamily(const char* w, int32_t last, const hh_vg* g) : kernel(kVg), who(w), last_kind(last), vg(g), missing(!g) {}
  // the rows and columns of the statistics: the coupled form's are the antithetic layout's
  hh::PathStatsLayout layout(const hh_config* c) const {
    return hh::PathStatsLayout(c->n_paths, c->antithetic != 0 || kernel == kCoupled, path_stat_rows(extremes));
  }
  // this member in its date-row form
  PathFamily rows() const {
    PathFamily f = *this;
    f.date_rows = true;
    return f;
  }
  // this member (a walk that holds a variance) in its state-row form
  PathFamily states() const {
    PathFamily f = rows();
    f.state_rows = true;
    return f;
  }
  // this member (kEuler) with the tangents of the statistics
  PathFamily tangents() const {
    PathFamily f = *this;
    f.tangent = true;
    return f;
  }
};

// the rows of the tangent form: the carried slots are those of the call's seeds (hh_mc_solve's map)
static hh::PathTangentLayout tangent_layout(const hh_model* m, const hh_config* c) {
  return hh::PathTangentLayout(c->n_paths, c->antithetic != 0, hh::partial_map(*m, *c).n_active);
}

// the dates of a call lie on every `every`-th step (`word`: what the entry point calls it)
static int check_every(hh_ctx* ctx, const char* who, const char* word, uint32_t every, uint32_t n_steps) {
  if (every == 0 || n_steps % every != 0)
    return fail(ctx, HH_ERR_INVALID, "%s: %s (%u) must be >= 1 and divide n_steps (%u)", who, word, every, n_steps);
  return HH_OK;
}

// The checks of every entry point, then the statistics of every trajectory into ctx->path_stats (one timing slot) and,
// where f.var_T, the variances at expiry into ctx->heston_var.  f.date_rows: monitor_every is the entry point's
// exercise_every, and the rows of every such step go into ctx->lsm_grid ([n_steps/monitor_every + 1][n_total]) instead —
// of the several-asset walk its state rows, [n_steps/monitor_every + 1][n_assets][n_total], under f.state_rows the rows
// (x, v), [n_steps/monitor_every + 1][2][n_total].
static int run_path_stats(hh_ctx* ctx, const PathFamily& f, const hh_model* m, const hh_config* c, uint32_t monitor_every,
                          int32_t include_start) {
  const char* who = f.who;
  hh_model m_lv;  // local volatility: model->sigma is not read — nor checked
  if (f.localvol) {
    m_lv = *m;
    m_lv.sigma = 0.0;
    m = &m_lv;
  }
  const bool hest = c->dynamics == HH_HESTON, logn = c->dynamics == HH_LOGNORMAL, em = c->strategy == HH_EULER_MARUYAMA;
  // the dynamics and strategy a kernel simulates, and how its entry points say so
  static const char kLognEm[] = "LognormalDynamics + EulerMaruyama";
  static const char kAnyEm[] = "LognormalDynamics or HestonDynamics + EulerMaruyama";
  bool ok = false;
  const char* needs = kAnyEm;
  switch (f.kernel) {
    case PathFamily::kEuler:
    case PathFamily::kCoupled: ok = em && (logn || hest); break;
    case PathFamily::kJump:  // dynamics that are neither are told what the plain entry points tell them
      ok = em && logn;
      if (hest || !em) needs = kLognEm;
      break;
    case PathFamily::kAssets:
    case PathFamily::kLocalVol:
      ok = em && logn;
      needs = kLognEm;
      break;
    case PathFamily::kQe:
    case PathFamily::kBates:
      ok = hest && c->strategy == HH_QE;
      needs = "HestonDynamics + the quadratic-exponential strategy (HH_QE)";
      break;
    case PathFamily::kVg:
      ok = logn && c->strategy == HH_EXACT_LAW;
      needs = "LognormalDynamics + the exact law (HH_EXACT_LAW)";
      break;
  }
  if (!ok) return fail(ctx, HH_ERR_UNSUPPORTED, "%s needs %s", who, needs);
  if (f.tangent && c->noise_mode == HH_NOISE_REPLAY)
    return fail(ctx, HH_ERR_UNSUPPORTED, "%s: GENERATE noise: the pathwise tangent has no REPLAY form", who);
  if (f.tangent && (c->n_partials == 0 || c->n_partials > HH_MAX_PARTIALS))
    return fail(ctx, HH_ERR_INVALID, "%s: n_partials (%u) must be 1 .. %d", who, c->n_partials, HH_MAX_PARTIALS);
  if (c->noise_mode == HH_NOISE_REPLAY || (c->n_partials != 0 && !f.tangent))
    return fail(ctx, HH_ERR_UNSUPPORTED, "%s: GENERATE noise, no dual partials", who);
  const bool coupled = f.kernel == PathFamily::kCoupled;
  if (coupled && c->antithetic)
    return fail(ctx, HH_ERR_UNSUPPORTED, "%s: no antithetic pairs (the second column of a trajectory is its coarse partner)", who);
  if (c->noise_mode != HH_NOISE_GENERATE) return fail(ctx, HH_ERR_INVALID, "unknown noise_mode %d", c->noise_mode);
  if (f.extremes != HH_EXTREMES_MONITORED && f.extremes != HH_EXTREMES_BRIDGE)
    return fail(ctx, HH_ERR_INVALID, "%s: unknown extremes %d", who, f.extremes);
  if (c->n_paths == 0 || c->n_steps == 0 || c->n_paths > kMaxPaths / 2 || c->n_steps > kMaxEulerSteps)
    return fail(ctx, HH_ERR_INVALID, "%s: 1 <= n_paths <= 2^31 - 128, 1 <= n_steps <= %u", who, kMaxEulerSteps);
  int rc;
  if ((rc = check_every(ctx, who, f.date_rows ? "exercise_every" : "monitor_every", monitor_every, c->n_steps))) return rc;
  if (f.date_rows && c->n_steps / monitor_every > kMaxGridSteps)
    return fail(ctx, HH_ERR_INVALID, "%s: n_steps / exercise_every = %u dates is above %u", who, c->n_steps / monitor_every,
                kMaxGridSteps);
  if (coupled && ((c->n_steps & 1u) || (monitor_every & 1u)))
    return fail(ctx, HH_ERR_INVALID, "%s: n_steps (%u, the fine grid) and monitor_every (%u) must be even: the coarse grid "
                "has half the steps and the same dates", who, c->n_steps, monitor_every);
  if (f.assets) {
    if (!(m->T > 0.0) || !std::isfinite(m->T) || !std::isfinite(m->r_drift) || !std::isfinite(m->discount))
      return fail(ctx, HH_ERR_INVALID, "%s: T > 0, r_drift and discount finite", who);
  } else if (!(m->S0 > 0.0) || !(m->T > 0.0) || !std::isfinite(m->S0) || !std::isfinite(m->T) ||
             !std::isfinite(m->sigma) || !std::isfinite(m->r_drift) || !std::isfinite(m->discount) ||
             (hest && (!(std::fabs(m->rho) <= 1.0) || !std::isfinite(m->V0) || !std::isfinite(m->kappa) ||
                       !std::isfinite(m->theta))))
    return fail(ctx, HH_ERR_INVALID, "%s: S0, T > 0, |rho| <= 1, model scalars finite", who);
  if (f.assets && (rc = check_assets(ctx, who, f.assets))) return rc;
  if (f.localvol && (rc = check_localvol(ctx, who, f.localvol))) return rc;
  if (f.jump && (rc = check_jump(ctx, who, f.jump, m->T / (double)c->n_steps))) return rc;
  if (f.vg && (rc = check_vg(ctx, who, m, f.vg, 1.0))) return rc;
  hh_model m_c = *m;  // Bates: the step's constants, and their checks, on the compensated rate
  if (f.jump && f.qe) m_c.r_drift = m->r_drift - hh::merton_compensator(*f.jump);
  if (f.qe && (rc = check_qe(ctx, who, &m_c, c, f.qe))) return rc;
  const hh::PathStatsLayout at = f.layout(c);
  const bool rows = f.date_rows;
  if (rows && f.assets)  // the several-asset walk's rows are its d log-states per date (hh_assets_path_rows)
    rc = ensure(ctx, ctx->lsm_grid, hh_assets_rows_elems(c->n_paths, c->n_steps / monitor_every, f.assets->n_assets, c->antithetic));
  else if (rows && f.state_rows)
    rc = ensure(ctx, ctx->lsm_grid, hh_assets_rows_elems(c->n_paths, c->n_steps / monitor_every, 2, c->antithetic));
  else if (rows) rc = ensure(ctx, ctx->lsm_grid, hh_lsm_grid_elems(c->n_paths, c->n_steps / monitor_every, c->antithetic));
  else if (f.tangent) rc = ensure(ctx, ctx->path_stats, tangent_layout(m, c).total);
  else rc = ensure(ctx, ctx->path_stats, at.total);
  if (rc) return rc;
  double* const dst = rows ? ctx->lsm_grid.p : ctx->path_stats.p;
  if (f.qe && f.var_T && (rc = ensure(ctx, ctx->heston_var, (size_t)at.n_total))) return rc;
  const uint64_t* seeds_dev = nullptr;
  if ((rc = stage_path_seeds(ctx, c, &seeds_dev))) return rc;
  hh::LocalVolArgs lv_args{};
  if (f.localvol && (rc = stage_localvol(ctx, f.localvol, m->T, c->n_steps, &lv_args))) return rc;
  if ((rc = begin_timing(ctx))) return rc;
  const bool start = include_start != 0;
  double* const var_dev = f.var_T ? ctx->heston_var.p : nullptr;
  switch (f.kernel) {
    case PathFamily::kEuler:
      if (f.tangent) {
        HH_HIP(ctx, hh::launch_path_tangent(*m, *c, seeds_dev, monitor_every, start, dst, ctx->stream));
        break;
      }
      HH_HIP(ctx, hh::launch_path_stats(*m, *c, seeds_dev, monitor_every, start, f.extremes == HH_EXTREMES_BRIDGE, dst,
                                        ctx->stream, rows, f.state_rows));
      break;
    case PathFamily::kJump:
      HH_HIP(ctx, hh::launch_jump_stats(*m, *c, *f.jump, seeds_dev, monitor_every, start, dst, ctx->stream, rows));
      break;
    case PathFamily::kQe:
      HH_HIP(ctx, hh::launch_qe_stats(*m, *c, *f.qe, seeds_dev, monitor_every, start, dst, var_dev, ctx->stream, rows,
                                      f.state_rows));
      break;
    case PathFamily::kBates:
      HH_HIP(ctx, hh::launch_bates_stats(*m, *c, *f.qe, *f.jump, seeds_dev, monitor_every, start, dst, var_dev, ctx->stream,
                                         rows, f.state_rows));
      break;
    case PathFamily::kAssets:
      if (rows) HH_HIP(ctx, hh::launch_assets_rows(*m, *c, *f.assets, seeds_dev, monitor_every, dst, ctx->stream));
      else HH_HIP(ctx, hh::launch_assets_stats(*m, *c, *f.assets, seeds_dev, monitor_every, start, ctx->path_stats, ctx->stream));
      break;
    case PathFamily::kLocalVol:
      HH_HIP(ctx, hh::launch_localvol_stats(*m, *c, lv_args, seeds_dev, monitor_every, start, f.extremes == HH_EXTREMES_BRIDGE,
                                            dst, ctx->stream, rows));
      break;
    case PathFamily::kCoupled:
      HH_HIP(ctx, hh::launch_coupled_stats(*m, *c, seeds_dev, monitor_every, start, ctx->path_stats, ctx->stream));
      break;
    case PathFamily::kVg:
      HH_HIP(ctx, hh::launch_vg_stats(*m, *c, *f.vg, seeds_dev, monitor_every, start, dst, ctx->stream, rows));
      break;
  }
  return end_timing(ctx);
}

// the statistics-only entry points: hh_mc_path_stats and its _ex, _qe, _bates and _assets forms
static int path_stats_call(hh_ctx* ctx, const PathFamily& f, const hh_model* m, const hh_config* c, uint32_t monitor_every,
                           int32_t include_start, double* stats, int32_t stats_on_device, hh_result* out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!m || !c || !stats || f.missing) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", f.who);
  const WallClock clock;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int rc = run_path_stats(ctx, f, m, c, monitor_every, include_start);
  if (rc) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  const hh::PathStatsLayout at = f.layout(c);
  HH_HIP(ctx, hipMemcpyAsync(stats, ctx->path_stats, at.total * sizeof(double),
                             stats_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  if (f.var_T)
    HH_HIP(ctx, hipMemcpyAsync(f.var_T, ctx->heston_var, at.n_total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = release_host_operands(ctx))) return rc;
  if (!out) return HH_OK;
  std::memset(out, 0, sizeof(*out));
  out->n_paths_done = c->n_paths;
  return solve_times(ctx, clock, &out->kernel_ms, &out->total_ms);
}

int hh_mc_path_stats(hh_ctx* ctx, const hh_model* m, const hh_config* c, uint32_t monitor_every, int32_t include_start,
                     double* stats, int32_t stats_on_device, hh_result* out) {
  return path_stats_call(ctx, {"hh_mc_path_stats", 0, HH_EXTREMES_MONITORED}, m, c, monitor_every, include_start,
                         stats, stats_on_device, out);
}

int hh_mc_path_stats_ex(hh_ctx* ctx, const hh_model* m, const hh_config* c, uint32_t monitor_every, int32_t include_start,
                        int32_t extremes, double* stats, int32_t stats_on_device, hh_result* out) {
  return path_stats_call(ctx, {"hh_mc_path_stats_ex", 0, extremes}, m, c, monitor_every, include_start, stats,
                         stats_on_device, out);
}

// the solve entry points: hh_mc_solve_path (kinds up to HH_PAYOFF_DIGITAL_ASSET) and its _ex, _jump, _qe, _bates and
// _assets forms (the lookbacks too) — the payoffs on the statistics, under kPathAssets those of the index
// the payoffs of a solve entry point, checked before anything runs
static int check_path_payoffs(hh_ctx* ctx, const PathFamily& f, const hh_path_payoff* payoffs, uint32_t n_payoffs) {
  const char* who = f.who;
  const hh_assets* assets = f.assets;
  if (n_payoffs == 0 || n_payoffs > HH_MAX_PATH_PAYOFFS)
    return fail(ctx, HH_ERR_INVALID, "%s: 1 .. %d payoffs", who, HH_MAX_PATH_PAYOFFS);
  for (uint32_t k = 0; k < n_payoffs; ++k) {
    const hh_path_payoff& q = payoffs[k];
    if (q.kind < HH_PAYOFF_VANILLA || q.kind > f.last_kind)
      return fail(ctx, HH_ERR_INVALID, "%s: payoff %u: unknown kind %d", who, k, q.kind);
    if (q.kind == HH_PAYOFF_BARRIER && (q.barrier_type < HH_BARRIER_UP_OUT || q.barrier_type > HH_BARRIER_DOWN_IN))
      return fail(ctx, HH_ERR_INVALID, "%s: payoff %u: unknown barrier type %d", who, k, q.barrier_type);
    if (q.cp != 1.0 && q.cp != -1.0) return fail(ctx, HH_ERR_INVALID, "%s: payoff %u: cp must be +1 or -1", who, k);
    if (!std::isfinite(q.strike) || !std::isfinite(q.rebate) || !std::isfinite(q.cash) || std::isnan(q.barrier))
      return fail(ctx, HH_ERR_INVALID, "%s: payoff %u: strike, rebate, cash finite; barrier not NaN", who, k);
    if (assets && q.kind == HH_PAYOFF_ASIAN_GEOM && assets->index_kind == HH_INDEX_WEIGHTED_SUM)
      for (uint32_t i = 0; i < assets->n_assets && i < (uint32_t)HH_MAX_ASSETS; ++i)  // n_assets is checked further down
        if (assets->weights[i] < 0.0)
          return fail(ctx, HH_ERR_INVALID,
                      "%s: payoff %u: a geometric Asian on a weighted sum with a negative weight: the sum of logarithms "
                      "is not defined where the index is <= 0", who, k);
  }
  return HH_OK;
}

// The coupled form (level_payoff_kernel) leaves 2·n_payoffs accumulators — those of Y = p_f − p_c, for `out`, then those of
// p_f, for out_fine (nullable).
static int solve_path_call(hh_ctx* ctx, const PathFamily& f, const hh_model* m, const hh_config* c, uint32_t monitor_every,
                           int32_t include_start, const hh_path_payoff* payoffs, uint32_t n_payoffs, hh_result* out,
                           double* path_values, double* stats, hh_result* out_fine = nullptr) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  const char* who = f.who;
  if (!m || !c || !payoffs || !out || f.missing) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", who);
  int rc = check_path_payoffs(ctx, f, payoffs, n_payoffs);
  if (rc) return rc;
  const WallClock clock;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if ((rc = run_path_stats(ctx, f, m, c, monitor_every, include_start))) return rc;

  const hh::PathStatsLayout at = f.layout(c);
  hh::PathPayoffArgs b{};
  b.stats = ctx->path_stats;
  b.n_paths = c->n_paths;
  b.n_chunks = hh::basket_chunks(c->n_paths);
  b.antithetic = c->antithetic;
  b.extremes = f.extremes;
  b.n_mon = (double)(c->n_steps / monitor_every + (include_start ? 1u : 0u));
  if ((rc = stage_host(ctx, ctx->path_payoffs, (size_t)n_payoffs, payoffs, (size_t)n_payoffs, &b.payoffs))) return rc;
  const bool coupled = f.kernel == PathFamily::kCoupled;
  const uint32_t n_groups = coupled ? 2u * n_payoffs : n_payoffs;
  const size_t n_acc = (size_t)n_groups * HH_ACC_LEN;
  if ((rc = ensure(ctx, ctx->basket_records, (size_t)n_groups * b.n_chunks * hh::kRecStride))) return rc;
  if ((rc = ensure(ctx, ctx->basket_accum, n_acc))) return rc;
  if (path_values && (rc = ensure(ctx, ctx->path_values, (size_t)n_payoffs * at.n_total))) return rc;
  b.values = path_values ? ctx->path_values.p : nullptr;
  b.records = ctx->basket_records;
  if ((rc = begin_timing(ctx))) return rc;
  if (coupled) HH_HIP(ctx, hh::launch_level_payoffs(b, n_payoffs, ctx->stream));
  else HH_HIP(ctx, hh::launch_path_payoffs(b, n_payoffs, ctx->stream));
  HH_HIP(ctx, hh::launch_reduce_records(ctx->basket_records, b.n_chunks, (double)c->n_paths, ctx->basket_accum,
                                        ctx->stream, n_groups));
  if ((rc = end_timing(ctx))) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  std::vector<double> host(n_acc);
  HH_HIP(ctx, hipMemcpyAsync(host.data(), ctx->basket_accum, n_acc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (path_values)
    HH_HIP(ctx, hipMemcpyAsync(path_values, ctx->path_values, (size_t)n_payoffs * at.n_total * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
  if (stats)
    HH_HIP(ctx, hipMemcpyAsync(stats, ctx->path_stats, at.total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (f.var_T)
    HH_HIP(ctx, hipMemcpyAsync(f.var_T, ctx->heston_var, at.n_total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = release_host_operands(ctx))) return rc;
  double kernel_ms, total_ms;
  if ((rc = solve_times(ctx, clock, &kernel_ms, &total_ms))) return rc;
  rc = finalize_results(m, 0, c, host.data(), n_payoffs, kernel_ms, total_ms, out);
  if (!rc && coupled && out_fine)
    rc = finalize_results(m, 0, c, host.data() + (size_t)n_payoffs * HH_ACC_LEN, n_payoffs, kernel_ms, total_ms, out_fine);
  return rc ? fail(ctx, rc, "finalize failed: the accumulator holds no trajectories") : HH_OK;
}

int hh_mc_solve_path(hh_ctx* ctx, const hh_model* m, const hh_config* c, uint32_t monitor_every, int32_t include_start,
                     const hh_path_payoff* payoffs, uint32_t n_payoffs, hh_result* out, double* path_values,
                     double* stats) {
  return solve_path_call(ctx, {"hh_mc_solve_path", HH_PAYOFF_DIGITAL_ASSET, HH_EXTREMES_MONITORED}, m, c,
                         monitor_every, include_start, payoffs, n_payoffs, out, path_values, stats);
}

int hh_mc_solve_path_ex(hh_ctx* ctx, const hh_model* m, const hh_config* c, uint32_t monitor_every, int32_t include_start,
                        int32_t extremes, const hh_path_payoff* payoffs, uint32_t n_payoffs, hh_result* out,
                        double* path_values, double* stats) {
  return solve_path_call(ctx, {"hh_mc_solve_path_ex", HH_PAYOFF_LOOKBACK_FIXED, extremes}, m, c, monitor_every,
                         include_start, payoffs, n_payoffs, out, path_values, stats);
}

// ---- pathwise derivatives (hedgehog_mc.h, "Pathwise derivatives of path-dependent payoffs") ----

size_t hh_path_tangent_rows(uint32_t n_active) {
  return (size_t)HH_PATH_STATS + HH_TANGENT_DATE_ROWS + (size_t)HH_TANGENT_ROWS_PER_SLOT * n_active;
}

int hh_mc_path_stats_tangent(hh_ctx* ctx, const hh_model* m, const hh_config* c, uint32_t monitor_every,
                             int32_t include_start, double* rows, int32_t rows_on_device, int32_t* basis_out,
                             hh_result* out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  const PathFamily f = PathFamily("hh_mc_path_stats_tangent", 0, HH_EXTREMES_MONITORED).tangents();
  if (!m || !c || !rows) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", f.who);
  const WallClock clock;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int rc = run_path_stats(ctx, f, m, c, monitor_every, include_start);
  if (rc) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  const hh::PartialMap pm = hh::partial_map(*m, *c);
  const hh::PathTangentLayout at = tangent_layout(m, c);
  HH_HIP(ctx, hipMemcpyAsync(rows, ctx->path_stats, at.total * sizeof(double),
                             rows_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = release_host_operands(ctx))) return rc;
  if (basis_out)
    for (int j = 0; j < hh::kMaxBasis; ++j) basis_out[j] = j < pm.n_active ? pm.basis[j] : -1;
  if (!out) return HH_OK;
  std::memset(out, 0, sizeof(*out));
  out->n_paths_done = c->n_paths;
  return solve_times(ctx, clock, &out->kernel_ms, &out->total_ms);
}

int hh_mc_solve_path_tangent(hh_ctx* ctx, const hh_model* m, const hh_config* c, uint32_t monitor_every,
                             int32_t include_start, const hh_path_payoff* payoffs, uint32_t n_payoffs, hh_result* out,
                             double* rows) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  const PathFamily f = PathFamily("hh_mc_solve_path_tangent", HH_PAYOFF_LOOKBACK_FIXED, HH_EXTREMES_MONITORED).tangents();
  const char* who = f.who;
  if (!m || !c || !payoffs || !out) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", who);
  int rc = check_path_payoffs(ctx, f, payoffs, n_payoffs);
  if (rc) return rc;
  for (uint32_t k = 0; k < n_payoffs; ++k)
    if (payoffs[k].kind == HH_PAYOFF_BARRIER || payoffs[k].kind == HH_PAYOFF_DIGITAL_CASH ||
        payoffs[k].kind == HH_PAYOFF_DIGITAL_ASSET)
      return fail(ctx, HH_ERR_UNSUPPORTED,
                  "%s: payoff %u (kind %d) is discontinuous: its pathwise derivative omits the jump term — use "
                  "FiniteDifference", who, k, payoffs[k].kind);
  const WallClock clock;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if ((rc = run_path_stats(ctx, f, m, c, monitor_every, include_start))) return rc;

  const hh::PartialMap pm = hh::partial_map(*m, *c);
  const hh::PathTangentLayout at = tangent_layout(m, c);
  hh::PathTangentArgs b{};
  b.rows = ctx->path_stats;
  b.n_paths = c->n_paths;
  b.n_chunks = hh::basket_chunks(c->n_paths);
  b.antithetic = c->antithetic;
  const uint32_t n_dates = c->n_steps / monitor_every;  // the dates after the start: steps every, 2·every, …, n_steps
  b.n_mon = (double)(n_dates + (include_start ? 1u : 0u));
  b.sum_k = (double)monitor_every * (0.5 * (double)n_dates * ((double)n_dates + 1.0));
  b.n_steps = (double)c->n_steps;
  b.dt = m->T / (double)c->n_steps;
  b.n_partials = (int)c->n_partials;
  b.n_active = pm.n_active;
  for (uint32_t k = 0; k < c->n_partials; ++k) {
    for (int j = 0; j < pm.n_active; ++j) b.w[k][j] = pm.w[k][j];
    b.xd0[k] = m->dS0 ? m->dS0[k] / m->S0 : 0.0;
    b.dr[k] = m->dr_drift ? m->dr_drift[k] : 0.0;
    b.dK[k] = pm.dK[k];
  }
  if ((rc = stage_host(ctx, ctx->path_payoffs, (size_t)n_payoffs, payoffs, (size_t)n_payoffs, &b.payoffs))) return rc;
  const size_t n_acc = (size_t)n_payoffs * HH_ACC_LEN;
  if ((rc = ensure(ctx, ctx->basket_records, (size_t)n_payoffs * b.n_chunks * hh::kRecStride))) return rc;
  if ((rc = ensure(ctx, ctx->basket_accum, n_acc))) return rc;
  b.records = ctx->basket_records;
  if ((rc = begin_timing(ctx))) return rc;
  HH_HIP(ctx, hh::launch_path_payoff_tangent(b, n_payoffs, ctx->stream));
  HH_HIP(ctx, hh::launch_reduce_records(ctx->basket_records, b.n_chunks, (double)c->n_paths, ctx->basket_accum,
                                        ctx->stream, n_payoffs));
  if ((rc = end_timing(ctx))) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  std::vector<double> host(n_acc);
  HH_HIP(ctx, hipMemcpyAsync(host.data(), ctx->basket_accum, n_acc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (rows)
    HH_HIP(ctx, hipMemcpyAsync(rows, ctx->path_stats, at.total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = release_host_operands(ctx))) return rc;
  double kernel_ms, total_ms;
  if ((rc = solve_times(ctx, clock, &kernel_ms, &total_ms))) return rc;
  rc = finalize_results(m, 0, c, host.data(), n_payoffs, kernel_ms, total_ms, out);
  return rc ? fail(ctx, rc, "finalize failed: the accumulator holds no trajectories") : HH_OK;
}

// ---- date rows of the family, and LSM on them (hedgehog_mc.h, "Date rows of the log-spot path family") ----

// The family member a source names, in its date-row form, handed to `run`: each kind through the constructor its
// path_stats entry point uses, so run_path_stats makes that entry point's checks in that entry point's words.
// states: the state-row form instead, of the three sources whose walk holds a variance.
static int with_source_family(hh_ctx* ctx, const char* who, const hh_path_source* src,
                              const std::function<int(const PathFamily&)>& run, bool states = false) {
  if (!src) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", who);
  if (states) switch (src->kind) {
    case HH_SOURCE_EULER: return run(PathFamily(who, 0, HH_EXTREMES_MONITORED).states());
    case HH_SOURCE_QE: return run(PathFamily(who, 0, src->qe, nullptr).states());
    case HH_SOURCE_BATES: return run(PathFamily(who, 0, src->qe, src->jump, nullptr).states());
    case HH_SOURCE_JUMP:
    case HH_SOURCE_LOCALVOL:
    case HH_SOURCE_VG:
      return fail(ctx, HH_ERR_UNSUPPORTED, "%s: source kind %d: the walk has no variance (state rows are those of "
                  "HH_SOURCE_EULER under Heston dynamics, HH_SOURCE_QE and HH_SOURCE_BATES)", who, src->kind);
    default: return fail(ctx, HH_ERR_INVALID, "%s: unknown source kind %d", who, src->kind);
  }
  switch (src->kind) {
    case HH_SOURCE_EULER: return run(PathFamily(who, 0, HH_EXTREMES_MONITORED).rows());
    case HH_SOURCE_JUMP: return run(PathFamily(who, 0, src->jump).rows());
    case HH_SOURCE_QE: return run(PathFamily(who, 0, src->qe, nullptr).rows());
    case HH_SOURCE_BATES: return run(PathFamily(who, 0, src->qe, src->jump, nullptr).rows());
    case HH_SOURCE_LOCALVOL: return run(PathFamily(who, 0, src->localvol, HH_EXTREMES_MONITORED).rows());
    case HH_SOURCE_VG: return run(PathFamily(who, 0, src->vg).rows());
  }
  return fail(ctx, HH_ERR_INVALID, "%s: unknown source kind %d", who, src->kind);
}

// cfg with its steps counted in exercise dates (exercise_every has passed check_every): what the grid's consumers
// (grid_results, the induction and its scalar checks) are told
static hh_config dates_config(const hh_config* c, uint32_t exercise_every) {
  hh_config g = *c;
  g.n_steps = c->n_steps / exercise_every;
  return g;
}

int hh_mc_path_grid(hh_ctx* ctx, const hh_path_source* source, const hh_model* m, const hh_config* c,
                    uint32_t exercise_every, double* spot_grid, int32_t grid_on_device, hh_result* out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  return with_source_family(ctx, "hh_mc_path_grid", source, [&](const PathFamily& f) -> int {
    if (!m || !c || f.missing) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", f.who);
    const WallClock clock;
    HH_HIP(ctx, hipSetDevice(ctx->device));
    HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    int rc = run_path_stats(ctx, f, m, c, exercise_every, 1);
    if (rc) return rc;
    HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    const hh_config g = dates_config(c, exercise_every);
    if ((rc = grid_results(ctx, &g, spot_grid, nullptr, grid_on_device, /*bk_counters=*/false, out, clock))) return rc;
    return release_host_operands(ctx);
  });
}

int hh_lsm_solve_path(hh_ctx* ctx, const hh_path_source* source, const hh_model* m, const hh_config* c,
                      uint32_t exercise_every, int32_t degree, double date_discount, hh_lsm_result* out,
                      int32_t* stop_time, double* stop_value, double* spot_grid) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  return with_source_family(ctx, "hh_lsm_solve_path", source, [&](const PathFamily& f) -> int {
    if (!m || !c || !out || f.missing) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", f.who);
    const WallClock clock;
    // the schedule first, then the induction's scalars on its dates, then everything the source's entry point checks
    int rc = check_every(ctx, f.who, "exercise_every", exercise_every, c->n_steps);
    if (rc) return rc;
    const hh_config g = dates_config(c, exercise_every);
    if ((rc = lsm_check_scalars(ctx, m, &g, degree, date_discount))) return rc;
    HH_HIP(ctx, hipSetDevice(ctx->device));
    HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if ((rc = run_path_stats(ctx, f, m, c, exercise_every, 1))) return rc;
    const uint64_t ntot = c->n_paths * (c->antithetic ? 2 : 1);
    rc = lsm_on_grid(ctx, ctx->lsm_grid, ntot, g.n_steps, m, degree, date_discount, out, stop_time, stop_value, clock);
    if (rc) return rc;
    if ((rc = release_host_operands(ctx))) return rc;
    return copy_back_spot_grid(ctx, &g, spot_grid);
  });
}

// ---- state rows of the several-asset walk, and LSM on several state rows (hedgehog_mc.h, "American exercise on several
// state rows"; kernels: hh_assets.hip, hh_lsm_multi.hip) ----

size_t hh_assets_rows_elems(uint64_t n_paths, uint32_t n_dates, uint32_t n_assets, int32_t antithetic) {
  return (size_t)(n_dates + 1) * n_assets * n_paths * (antithetic ? 2 : 1);
}

int hh_assets_path_rows(hh_ctx* ctx, const hh_model* m, const hh_assets* assets, const hh_config* c, uint32_t exercise_every,
                        double* rows, int32_t rows_on_device, hh_result* out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  const PathFamily f = PathFamily("hh_assets_path_rows", 0, assets).rows();
  if (!m || !c || !rows || f.missing) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", f.who);
  const WallClock clock;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int rc = run_path_stats(ctx, f, m, c, exercise_every, 1);
  if (rc) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  const size_t bytes = hh_assets_rows_elems(c->n_paths, c->n_steps / exercise_every, assets->n_assets, c->antithetic) * sizeof(double);
  HH_HIP(ctx, hipMemcpyAsync(rows, ctx->lsm_grid, bytes, rows_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                             ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = release_host_operands(ctx))) return rc;
  if (!out) return HH_OK;
  std::memset(out, 0, sizeof(*out));
  out->n_paths_done = c->n_paths;
  return solve_times(ctx, clock, &out->kernel_ms, &out->total_ms);
}

// the descriptor and the basis of an induction on state rows, after lsm_check_scalars
static int check_lsm_states(hh_ctx* ctx, const char* who, const hh_lsm_states* d, int32_t degree) {
  if (d->kind != HH_LSM_STATES_LOG_ASSETS && d->kind != HH_LSM_STATES_LOG_SPOT_VARIANCE)
    return fail(ctx, HH_ERR_INVALID, "%s: unknown descriptor kind %d", who, d->kind);
  if (d->kind == HH_LSM_STATES_LOG_SPOT_VARIANCE) {  // index_kind and weights are not read
    if (d->n_states != 2u)
      return fail(ctx, HH_ERR_INVALID, "%s: n_states (%u) must be 2 under HH_LSM_STATES_LOG_SPOT_VARIANCE", who, d->n_states);
    if (!std::isfinite(d->strike)) return fail(ctx, HH_ERR_INVALID, "%s: the strike must be finite", who);
  } else {
    if (d->n_states < 1u || d->n_states > (uint32_t)HH_MAX_ASSETS)
      return fail(ctx, HH_ERR_INVALID, "%s: n_states (%u) must lie in 1 .. %d", who, d->n_states, HH_MAX_ASSETS);
    if (d->index_kind < HH_INDEX_WEIGHTED_SUM || d->index_kind > HH_INDEX_WORST_OF)
      return fail(ctx, HH_ERR_INVALID, "%s: unknown index_kind %d", who, d->index_kind);
    if (!std::isfinite(d->strike)) return fail(ctx, HH_ERR_INVALID, "%s: the strike must be finite", who);
    for (uint32_t i = 0; i < d->n_states; ++i)
      if (!std::isfinite(d->weights[i])) return fail(ctx, HH_ERR_INVALID, "%s: asset %u: the weight must be finite", who, i);
  }
  if (hh::lsm_basis_count((int)d->n_states, degree) == 0)
    return fail(ctx, HH_ERR_UNSUPPORTED, "%s: %u state rows at degree %d need more than %d basis functions", who, d->n_states,
                degree, HH_LSM_MAX_BASIS);
  return HH_OK;
}

// The induction on state rows already in device memory: launches, reduction and the copies back.  The caller recorded
// ctx->ev0 and has checked everything.
static int lsm_on_states(hh_ctx* ctx, const hh_lsm_states* d, const double* rows_dev, uint64_t ntot, uint32_t n_dates,
                         int32_t degree, double date_discount, hh_lsm_result* out, int32_t* stop_time, double* stop_value,
                         double* coef, const WallClock& clock, double* policy = nullptr) {
  const hh::LsmMultiScratch at(ntot, n_dates);
  const uint32_t ch = hh::lsm_chunks(ntot);
  int rc;
  if ((rc = ensure(ctx, ctx->lsm_val, (size_t)ntot))) return rc;
  if ((rc = ensure(ctx, ctx->lsm_tau, (size_t)ntot))) return rc;
  if ((rc = ensure(ctx, ctx->lsm_scratch, at.total))) return rc;
  if ((rc = ensure(ctx, ctx->records, (size_t)ch * hh::kRecStride))) return rc;
  double* counters = ctx->accum_host + HH_ACC_LEN;  // pinned, behind the accumulator (lsm_on_grid)
  counters[0] = counters[1] = 0.0;
  HH_HIP(ctx, hh::launch_lsm_multi(*d, rows_dev, ntot, n_dates, degree, date_discount, ctx->lsm_tau, ctx->lsm_val,
                                   ctx->lsm_scratch, ctx->records, ctx->stream));
  HH_HIP(ctx, hh::launch_reduce_records(ctx->records, ch, (double)ntot, ctx->accum, ctx->stream));
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HH_HIP(ctx, hipMemcpyAsync(ctx->accum_host, ctx->accum, HH_ACC_LEN * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipMemcpyAsync(counters, ctx->lsm_scratch + at.counters, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (stop_time)
    HH_HIP(ctx, hipMemcpyAsync(stop_time, ctx->lsm_tau, ntot * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (stop_value)
    HH_HIP(ctx, hipMemcpyAsync(stop_value, ctx->lsm_val, ntot * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (coef) {  // [date][kLsmMultiPad] on the device, [date][B] for the caller
    const size_t B = (size_t)hh::lsm_basis_count((int)d->n_states, degree);
    HH_HIP(ctx, hipMemcpy2DAsync(coef, B * sizeof(double), ctx->lsm_scratch + at.coef, hh::kLsmMultiPad * sizeof(double),
                                 B * sizeof(double), n_dates, hipMemcpyDeviceToHost, ctx->stream));
  }
  // the policy (hh_lsm_fit_states): one more copy — the statistics the induction standardised by, and the coefficients
  const size_t rows = (size_t)n_dates + 1;
  std::vector<double> rowstat, coef_pad;
  if (policy) {
    rowstat.resize(rows * hh::kLsmMultiStats);
    coef_pad.resize(rows * hh::kLsmMultiPad);
    HH_HIP(ctx, hipMemcpyAsync(rowstat.data(), ctx->lsm_scratch + at.rowstat, rowstat.size() * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
    HH_HIP(ctx, hipMemcpyAsync(coef_pad.data(), ctx->lsm_scratch + at.coef, coef_pad.size() * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
  }
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (policy) {  // [date][μ_i, isd_i, coef_j]; a date that was not regressed (0, n_dates): μ = 0, isd = 1, coef = 0
    const size_t m = d->n_states, B = (size_t)hh::lsm_basis_count((int)m, degree), stride = 2 * m + B;
    for (size_t t = 0; t < rows; ++t) {
      const bool regressed = t >= 1 && t < n_dates;
      const double* rs = rowstat.data() + t * hh::kLsmMultiStats;
      for (size_t i = 0; i < m; ++i) {
        policy[t * stride + i] = regressed ? rs[1 + i] : 0.0;
        policy[t * stride + m + i] = regressed ? rs[1 + HH_MAX_ASSETS + i] : 1.0;
      }
      for (size_t j = 0; j < B; ++j) policy[t * stride + 2 * m + j] = regressed ? coef_pad[t * hh::kLsmMultiPad + j] : 0.0;
    }
  }
  if ((rc = hh_lsm_finalize(ctx->accum_host, out))) return finalize_failed(ctx, rc);
  out->rows_regressed = (uint32_t)counters[0];
  out->rows_skipped = (uint32_t)counters[1];
  out->form = hh::kLsmFormPerDate;
  return solve_times(ctx, clock, &out->kernel_ms, &out->total_ms);
}

// the induction's scalars in lsm_check_scalars' words: a model that carries cp alone, a config that carries the sizes
static int check_lsm_states_scalars(hh_ctx* ctx, double cp, uint64_t n_paths, uint32_t n_dates, int32_t degree,
                                    double date_discount) {
  hh_model mm{};
  mm.S0 = 1.0;
  mm.T = 1.0;
  mm.cp = cp;
  hh_config g{};
  g.n_paths = n_paths;
  g.n_steps = n_dates;
  return lsm_check_scalars(ctx, &mm, &g, degree, date_discount);
}

int hh_lsm_solve_states(hh_ctx* ctx, const hh_lsm_states* desc, const double* rows_dev, uint64_t n_total, uint32_t n_dates,
                        int32_t degree, double date_discount, hh_lsm_result* out, int32_t* stop_time, double* stop_value,
                        double* coef) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  static const char who[] = "hh_lsm_solve_states";
  if (!desc || !rows_dev || !out) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", who);
  const WallClock clock;
  int rc = check_lsm_states_scalars(ctx, desc->cp, n_total, n_dates, degree, date_discount);
  if (rc) return rc;
  if ((rc = check_lsm_states(ctx, who, desc, degree))) return rc;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  return lsm_on_states(ctx, desc, rows_dev, n_total, n_dates, degree, date_discount, out, stop_time, stop_value, coef, clock);
}

int hh_lsm_solve_assets(hh_ctx* ctx, const hh_model* m, const hh_assets* assets, const hh_config* c, uint32_t exercise_every,
                        int32_t degree, double date_discount, hh_lsm_result* out, int32_t* stop_time, double* stop_value,
                        double* rows) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  const PathFamily f = PathFamily("hh_lsm_solve_assets", 0, assets).rows();
  if (!m || !c || !out || f.missing) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", f.who);
  const WallClock clock;
  // the schedule first, then the induction's scalars on its dates, then everything the walk's entry point checks
  int rc = check_every(ctx, f.who, "exercise_every", exercise_every, c->n_steps);
  if (rc) return rc;
  const uint32_t n_dates = c->n_steps / exercise_every;
  if ((rc = check_lsm_states_scalars(ctx, m->cp, c->n_paths, n_dates, degree, date_discount))) return rc;
  hh_lsm_states d{};
  d.kind = HH_LSM_STATES_LOG_ASSETS;
  d.n_states = assets->n_assets;
  d.index_kind = assets->index_kind;
  d.cp = m->cp;
  d.strike = m->strike;
  for (uint32_t i = 0; i < assets->n_assets && i < (uint32_t)HH_MAX_ASSETS; ++i) d.weights[i] = assets->weights[i];
  if ((rc = check_lsm_states(ctx, f.who, &d, degree))) return rc;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if ((rc = run_path_stats(ctx, f, m, c, exercise_every, 1))) return rc;
  const uint64_t ntot = c->n_paths * (c->antithetic ? 2 : 1);
  rc = lsm_on_states(ctx, &d, ctx->lsm_grid, ntot, n_dates, degree, date_discount, out, stop_time, stop_value, nullptr, clock);
  if (rc) return rc;
  if ((rc = release_host_operands(ctx))) return rc;
  if (rows) {
    HH_HIP(ctx, hipMemcpyAsync(rows, ctx->lsm_grid, hh_assets_rows_elems(c->n_paths, n_dates, assets->n_assets, c->antithetic) * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
    HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return HH_OK;
}

// ---- state rows of the stochastic-volatility walks, and LSM on (S, V) (hedgehog_mc.h, "American exercise under
// stochastic volatility"; kernels: each walk's *_stats_kernel<…, StateRows<ANTI>>, hh_lsm_multi.hip) ----

// the Euler source walks lognormal dynamics too, and that walk holds no variance
static int check_walk_has_variance(hh_ctx* ctx, const PathFamily& f, const hh_config* c) {
  if (f.kernel == PathFamily::kEuler && c->dynamics == HH_LOGNORMAL)
    return fail(ctx, HH_ERR_UNSUPPORTED, "%s: LognormalDynamics on HH_SOURCE_EULER: the walk has no variance (state rows "
                "need HestonDynamics there)", f.who);
  return HH_OK;
}

int hh_mc_path_states(hh_ctx* ctx, const hh_path_source* source, const hh_model* m, const hh_config* c,
                      uint32_t exercise_every, double* rows, int32_t rows_on_device, hh_result* out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  return with_source_family(ctx, "hh_mc_path_states", source, [&](const PathFamily& f) -> int {
    if (!m || !c || !rows || f.missing) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", f.who);
    int rc = check_walk_has_variance(ctx, f, c);
    if (rc) return rc;
    const WallClock clock;
    HH_HIP(ctx, hipSetDevice(ctx->device));
    HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if ((rc = run_path_stats(ctx, f, m, c, exercise_every, 1))) return rc;
    HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    const size_t bytes = hh_assets_rows_elems(c->n_paths, c->n_steps / exercise_every, 2, c->antithetic) * sizeof(double);
    HH_HIP(ctx, hipMemcpyAsync(rows, ctx->lsm_grid, bytes, rows_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                               ctx->stream));
    HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = release_host_operands(ctx))) return rc;
    if (!out) return HH_OK;
    std::memset(out, 0, sizeof(*out));
    out->n_paths_done = c->n_paths;
    return solve_times(ctx, clock, &out->kernel_ms, &out->total_ms);
  }, /*states=*/true);
}

// hh_lsm_solve_path_states and, with a policy, hh_lsm_fit_path_states (`who`; need_policy: its policy may not be NULL)
static int lsm_path_states_call(hh_ctx* ctx, const char* who, const hh_path_source* source, const hh_model* m,
                                const hh_config* c, uint32_t exercise_every, int32_t degree, double date_discount,
                                hh_lsm_result* out, int32_t* stop_time, double* stop_value, double* coef, double* rows,
                                double* policy, bool need_policy) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  return with_source_family(ctx, who, source, [&](const PathFamily& f) -> int {
    if (!m || !c || !out || f.missing || (need_policy && !policy)) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", f.who);
    const WallClock clock;
    // the schedule first, then the induction's scalars on its dates, then everything the source's entry point checks
    int rc = check_every(ctx, f.who, "exercise_every", exercise_every, c->n_steps);
    if (rc) return rc;
    const uint32_t n_dates = c->n_steps / exercise_every;
    if ((rc = check_lsm_states_scalars(ctx, m->cp, c->n_paths, n_dates, degree, date_discount))) return rc;
    hh_lsm_states d{};
    d.kind = HH_LSM_STATES_LOG_SPOT_VARIANCE;
    d.n_states = 2;
    d.cp = m->cp;
    d.strike = m->strike;
    if ((rc = check_lsm_states(ctx, f.who, &d, degree))) return rc;
    if ((rc = check_walk_has_variance(ctx, f, c))) return rc;
    HH_HIP(ctx, hipSetDevice(ctx->device));
    HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if ((rc = run_path_stats(ctx, f, m, c, exercise_every, 1))) return rc;
    const uint64_t ntot = c->n_paths * (c->antithetic ? 2 : 1);
    rc = lsm_on_states(ctx, &d, ctx->lsm_grid, ntot, n_dates, degree, date_discount, out, stop_time, stop_value, coef, clock,
                       policy);
    if (rc) return rc;
    if ((rc = release_host_operands(ctx))) return rc;
    if (rows) {
      HH_HIP(ctx, hipMemcpyAsync(rows, ctx->lsm_grid, hh_assets_rows_elems(c->n_paths, n_dates, 2, c->antithetic) * sizeof(double),
                                 hipMemcpyDeviceToHost, ctx->stream));
      HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return HH_OK;
  }, /*states=*/true);
}

int hh_lsm_solve_path_states(hh_ctx* ctx, const hh_path_source* source, const hh_model* m, const hh_config* c,
                             uint32_t exercise_every, int32_t degree, double date_discount, hh_lsm_result* out,
                             int32_t* stop_time, double* stop_value, double* coef, double* rows) {
  return lsm_path_states_call(ctx, "hh_lsm_solve_path_states", source, m, c, exercise_every, degree, date_discount, out,
                              stop_time, stop_value, coef, rows, nullptr, false);
}

// ---- dual bounds: the policy as an array, its value on other rows, the nested upper bound (hedgehog_mc.h, "Dual bounds for
// American exercise"; kernels: policy_value_kernel of hh_lsm_multi.hip, hh_bounds.hip) ----

size_t hh_lsm_policy_elems(uint32_t n_dates, uint32_t m, int32_t degree) {
  const int B = m <= (uint32_t)HH_MAX_ASSETS ? hh::lsm_basis_count((int)m, degree) : 0;
  return B ? ((size_t)n_dates + 1) * (2 * (size_t)m + (size_t)B) : 0;
}

int hh_lsm_fit_states(hh_ctx* ctx, const hh_lsm_states* desc, const double* rows_dev, uint64_t n_total, uint32_t n_dates,
                      int32_t degree, double date_discount, hh_lsm_result* out, int32_t* stop_time, double* stop_value,
                      double* policy) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  static const char who[] = "hh_lsm_fit_states";
  if (!desc || !rows_dev || !out || !policy) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", who);
  const WallClock clock;
  int rc = check_lsm_states_scalars(ctx, desc->cp, n_total, n_dates, degree, date_discount);
  if (rc) return rc;
  if ((rc = check_lsm_states(ctx, who, desc, degree))) return rc;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  return lsm_on_states(ctx, desc, rows_dev, n_total, n_dates, degree, date_discount, out, stop_time, stop_value, nullptr, clock,
                       policy);
}

int hh_lsm_fit_path_states(hh_ctx* ctx, const hh_path_source* source, const hh_model* m, const hh_config* c,
                           uint32_t exercise_every, int32_t degree, double date_discount, hh_lsm_result* out, double* policy) {
  return lsm_path_states_call(ctx, "hh_lsm_fit_path_states", source, m, c, exercise_every, degree, date_discount, out, nullptr,
                              nullptr, nullptr, nullptr, policy, true);
}

// every entry of a caller's policy is finite (after check_lsm_states: the basis exists)
static int check_policy(hh_ctx* ctx, const char* who, const double* policy, uint32_t n_dates, uint32_t m, int32_t degree) {
  const size_t n = hh_lsm_policy_elems(n_dates, m, degree), stride = n / ((size_t)n_dates + 1);
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(policy[k]))
      return fail(ctx, HH_ERR_INVALID, "%s: policy entry %zu of date %zu is not finite", who, k % stride, k / stride);
  return HH_OK;
}

// the descriptor of the (log S, V) rows under the model's payoff
static hh_lsm_states spot_variance_states(const hh_model* m) {
  hh_lsm_states d{};
  d.kind = HH_LSM_STATES_LOG_SPOT_VARIANCE;
  d.n_states = 2;
  d.cp = m->cp;
  d.strike = m->strike;
  return d;
}

// The policy and, behind it, D^k for k = 0 .. n_dates into ctx->lsm_policy; *disc_dev: where the powers start.
static int stage_policy(hh_ctx* ctx, const double* policy, size_t n_policy, uint32_t n_dates, double date_discount,
                        const double** policy_dev, const double** disc_dev) {
  std::vector<double> host(policy, policy + n_policy);
  for (uint32_t k = 0; k <= n_dates; ++k) host.push_back(std::pow(date_discount, (double)k));
  int rc = ensure(ctx, ctx->lsm_policy, host.size());
  if (rc) return rc;
  HH_HIP(ctx, hipMemcpyAsync(ctx->lsm_policy, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `host` goes with this frame
  *policy_dev = ctx->lsm_policy;
  if (disc_dev) *disc_dev = ctx->lsm_policy + n_policy;
  return HH_OK;
}

// A checked policy run forward on state rows in device memory: launches, reduction and the copies back.  The caller
// recorded ctx->ev0.
static int policy_on_states(hh_ctx* ctx, const hh_lsm_states* d, const double* policy, int32_t degree, const double* rows_dev,
                            uint64_t ntot, uint32_t n_dates, double date_discount, hh_lsm_result* out, int32_t* stop_time,
                            double* stop_value, const WallClock& clock) {
  const uint32_t ch = hh::lsm_chunks(ntot);
  int rc;
  if ((rc = ensure(ctx, ctx->lsm_val, (size_t)ntot))) return rc;
  if ((rc = ensure(ctx, ctx->lsm_tau, (size_t)ntot))) return rc;
  if ((rc = ensure(ctx, ctx->records, (size_t)ch * hh::kRecStride))) return rc;
  const double* policy_dev = nullptr;
  if ((rc = stage_policy(ctx, policy, hh_lsm_policy_elems(n_dates, d->n_states, degree), n_dates, date_discount, &policy_dev,
                         nullptr)))
    return rc;
  if ((rc = begin_timing(ctx))) return rc;
  HH_HIP(ctx, hh::launch_policy_value(*d, rows_dev, ntot, n_dates, degree, date_discount, policy_dev, ctx->lsm_tau, ctx->lsm_val,
                                      ctx->records, ctx->stream));
  if ((rc = end_timing(ctx))) return rc;
  HH_HIP(ctx, hh::launch_reduce_records(ctx->records, ch, (double)ntot, ctx->accum, ctx->stream));
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HH_HIP(ctx, hipMemcpyAsync(ctx->accum_host, ctx->accum, HH_ACC_LEN * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (stop_time)
    HH_HIP(ctx, hipMemcpyAsync(stop_time, ctx->lsm_tau, ntot * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (stop_value)
    HH_HIP(ctx, hipMemcpyAsync(stop_value, ctx->lsm_val, ntot * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = hh_lsm_finalize(ctx->accum_host, out))) return finalize_failed(ctx, rc);
  out->form = hh::kLsmFormPerDate;
  return solve_times(ctx, clock, &out->kernel_ms, &out->total_ms);
}

int hh_lsm_policy_value(hh_ctx* ctx, const hh_lsm_states* desc, const double* policy, int32_t degree, const double* rows_dev,
                        uint64_t n_total, uint32_t n_dates, double date_discount, hh_lsm_result* out, int32_t* stop_time,
                        double* stop_value) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  static const char who[] = "hh_lsm_policy_value";
  if (!desc || !policy || !rows_dev || !out) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", who);
  const WallClock clock;
  int rc = check_lsm_states_scalars(ctx, desc->cp, n_total, n_dates, degree, date_discount);
  if (rc) return rc;
  if ((rc = check_lsm_states(ctx, who, desc, degree))) return rc;
  if ((rc = check_policy(ctx, who, policy, n_dates, desc->n_states, degree))) return rc;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  return policy_on_states(ctx, desc, policy, degree, rows_dev, n_total, n_dates, date_discount, out, stop_time, stop_value,
                          clock);
}

int hh_lsm_policy_value_path(hh_ctx* ctx, const hh_path_source* source, const hh_model* m, const hh_config* c,
                             uint32_t exercise_every, const double* policy, int32_t degree, double date_discount,
                             hh_lsm_result* out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  return with_source_family(ctx, "hh_lsm_policy_value_path", source, [&](const PathFamily& f) -> int {
    if (!m || !c || !policy || !out || f.missing) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", f.who);
    const WallClock clock;
    // hh_lsm_solve_path_states' order: the schedule, the induction's scalars, the policy, then what the walk's entry point checks
    int rc = check_every(ctx, f.who, "exercise_every", exercise_every, c->n_steps);
    if (rc) return rc;
    const uint32_t n_dates = c->n_steps / exercise_every;
    if ((rc = check_lsm_states_scalars(ctx, m->cp, c->n_paths, n_dates, degree, date_discount))) return rc;
    const hh_lsm_states d = spot_variance_states(m);
    if ((rc = check_lsm_states(ctx, f.who, &d, degree))) return rc;
    if ((rc = check_policy(ctx, f.who, policy, n_dates, 2, degree))) return rc;
    if ((rc = check_walk_has_variance(ctx, f, c))) return rc;
    HH_HIP(ctx, hipSetDevice(ctx->device));
    HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if ((rc = run_path_stats(ctx, f, m, c, exercise_every, 1))) return rc;
    const uint64_t ntot = c->n_paths * (c->antithetic ? 2 : 1);
    rc = policy_on_states(ctx, &d, policy, degree, ctx->lsm_grid, ntot, n_dates, date_discount, out, nullptr, nullptr, clock);
    if (rc) return rc;
    return release_host_operands(ctx);
  }, /*states=*/true);
}

int hh_lsm_upper_bound(hh_ctx* ctx, const hh_model* m, const hh_config* c, uint32_t exercise_every, const double* policy,
                       int32_t degree, double date_discount, uint32_t n_inner, uint64_t inner_seed, hh_bounds_result* out,
                       double* cont, double* cont_se, double* pathwise_max) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  const PathFamily f = PathFamily("hh_lsm_upper_bound", 0, HH_EXTREMES_MONITORED).states();
  const char* who = f.who;
  if (!m || !c || !policy || !out) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", who);
  const WallClock clock;
  int rc = check_every(ctx, who, "exercise_every", exercise_every, c->n_steps);
  if (rc) return rc;
  const uint32_t n_dates = c->n_steps / exercise_every;
  if ((rc = check_lsm_states_scalars(ctx, m->cp, c->n_paths, n_dates, degree, date_discount))) return rc;
  const hh_lsm_states d = spot_variance_states(m);
  if ((rc = check_lsm_states(ctx, who, &d, degree))) return rc;
  if (n_inner == 0 || n_inner % 64u)
    return fail(ctx, HH_ERR_INVALID, "%s: n_inner (%u) must be a multiple of 64 and >= 64 (a wave walks 64 inner paths at a time)",
                who, n_inner);
  if ((rc = check_policy(ctx, who, policy, n_dates, 2, degree))) return rc;
  if ((uint64_t)n_dates * c->n_paths > 0x80000000ull)
    return fail(ctx, HH_ERR_INVALID, "%s: n_dates·n_outer = %llu pairs are above 2^31", who,
                (unsigned long long)n_dates * (unsigned long long)c->n_paths);
  if (c->dynamics != HH_HESTON || c->strategy != HH_EULER_MARUYAMA)
    return fail(ctx, HH_ERR_UNSUPPORTED, "%s needs HestonDynamics + EulerMaruyama: the nested walks restart the Heston Euler step "
                "(no QE, Bates, several-asset or one-variable form)", who);
  if (c->antithetic)
    return fail(ctx, HH_ERR_UNSUPPORTED, "%s: no antithetic outer paths (the martingale is built per outer column)", who);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if ((rc = run_path_stats(ctx, f, m, c, exercise_every, 1))) return rc;  // REPLAY noise, n_partials and the scalars: its words
  const uint64_t n_outer = c->n_paths;
  const size_t n_cont = (size_t)n_dates * n_outer;
  const uint32_t ch = hh::lsm_chunks(n_outer);
  if ((rc = ensure(ctx, ctx->bounds_cont, 2 * n_cont))) return rc;
  if ((rc = ensure(ctx, ctx->lsm_val, (size_t)n_outer))) return rc;
  if ((rc = ensure(ctx, ctx->lsm_tau, (size_t)n_outer))) return rc;
  if ((rc = ensure(ctx, ctx->records, (size_t)ch * hh::kRecStride))) return rc;
  hh::BoundsLaunch b{};
  b.rows = ctx->lsm_grid;
  b.n_dates = n_dates;
  b.n_inner = n_inner;
  b.degree = degree;
  b.inner_seed = inner_seed;
  if ((rc = stage_policy(ctx, policy, hh_lsm_policy_elems(n_dates, 2, degree), n_dates, date_discount, &b.policy, &b.disc_pow)))
    return rc;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  struct EventGuard {
    hipEvent_t* e;
    ~EventGuard() { for (int k = 0; k < 3; ++k) if (e[k]) (void)hipEventDestroy(e[k]); }
  } guard{ev};
  for (int k = 0; k < 3; ++k) HH_HIP(ctx, hipEventCreate(&ev[k]));
  double* const cont_dev = ctx->bounds_cont;
  double* const se_dev = ctx->bounds_cont + n_cont;
  if ((rc = begin_timing(ctx))) return rc;
  HH_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
  HH_HIP(ctx, hh::launch_nested_continuation(*m, *c, b, cont_dev, se_dev, ctx->stream));
  HH_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
  if ((rc = end_timing(ctx))) return rc;
  HH_HIP(ctx, hh::launch_dual_outer(*m, *c, b, cont_dev, ctx->lsm_val, ctx->stream));
  HH_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
  // the mean of pathwise_max and its standard error by the inductions' final kernel at τ = 0, and the record reduction
  HH_HIP(ctx, hipMemsetAsync(ctx->lsm_tau, 0, n_outer * sizeof(int32_t), ctx->stream));
  HH_HIP(ctx, hh::launch_lsm_final(ctx->lsm_tau, ctx->lsm_val, n_outer, 0.0, ctx->records, ctx->stream));
  HH_HIP(ctx, hh::launch_reduce_records(ctx->records, ch, (double)n_outer, ctx->accum, ctx->stream));
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HH_HIP(ctx, hipMemcpyAsync(ctx->accum_host, ctx->accum, HH_ACC_LEN * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (cont) HH_HIP(ctx, hipMemcpyAsync(cont, cont_dev, n_cont * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (cont_se) HH_HIP(ctx, hipMemcpyAsync(cont_se, se_dev, n_cont * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (pathwise_max)
    HH_HIP(ctx, hipMemcpyAsync(pathwise_max, ctx->lsm_val, n_outer * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = release_host_operands(ctx))) return rc;
  hh_lsm_result mean{};
  if ((rc = hh_lsm_finalize(ctx->accum_host, &mean))) return finalize_failed(ctx, rc);
  std::memset(out, 0, sizeof(*out));
  out->upper = mean.price;
  out->upper_se = mean.std_error;
  out->n_outer = n_outer;
  out->n_inner = n_inner;
  float ms = 0.f;
  HH_HIP(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
  out->nested_ms = ms;
  HH_HIP(ctx, hipEventElapsedTime(&ms, ev[1], ev[2]));
  out->outer_ms = ms;
  out->total_ms = clock.ms();
  return HH_OK;
}

// ---- multilevel Monte Carlo (hedgehog_mc.h, "Multilevel Monte Carlo"; kernels: hh_path.hip) ----

int hh_mc_path_stats_coupled(hh_ctx* ctx, const hh_model* m, const hh_config* c, uint32_t monitor_every,
                             int32_t include_start, double* stats, int32_t stats_on_device, hh_result* out) {
  return path_stats_call(ctx, {"hh_mc_path_stats_coupled", 0, PathFamily::kCoupledForm}, m, c, monitor_every, include_start,
                         stats, stats_on_device, out);
}

int hh_mc_solve_path_coupled(hh_ctx* ctx, const hh_model* m, const hh_config* c, uint32_t monitor_every,
                             int32_t include_start, const hh_path_payoff* payoffs, uint32_t n_payoffs, hh_result* out_diff,
                             hh_result* out_fine, double* path_values, double* stats) {
  return solve_path_call(ctx, {"hh_mc_solve_path_coupled", HH_PAYOFF_LOOKBACK_FIXED, PathFamily::kCoupledForm}, m, c,
                         monitor_every, include_start, payoffs, n_payoffs, out_diff, path_values, stats, out_fine);
}

// ---- Merton jump diffusion (hedgehog_mc.h, "Merton (1976) jump diffusion"; kernels: hh_jump.hip, hh_fourier.hip) ----

int hh_mc_solve_path_jump(hh_ctx* ctx, const hh_model* m, const hh_jump* jump, const hh_config* c, uint32_t monitor_every,
                          int32_t include_start, const hh_path_payoff* payoffs, uint32_t n_payoffs, hh_result* out,
                          double* path_values, double* stats) {
  return solve_path_call(ctx, {"hh_mc_solve_path_jump", HH_PAYOFF_LOOKBACK_FIXED, jump}, m, c, monitor_every, include_start,
                         payoffs, n_payoffs, out, path_values, stats);
}

// One solve on a terminal law drawn in one kernel (hh_mc_solve_jump, hh_mc_solve_vg): who it is, the strategies it
// refuses, the law's check, the records of its launch and the launch.
struct TerminalLaw {
  const char* who;
  bool (*bad_strategy)(const hh_config&);
  std::function<int()> law_check;
  uint32_t (*n_records)(uint64_t n_paths);
  std::function<int(const hh::DevicePtrs&)> launch;
};

static int terminal_law_call(hh_ctx* ctx, const TerminalLaw& f, bool null_law, const hh_model* m, const hh_config* c,
                             hh_result* out, double* terminal) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  const char* who = f.who;
  if (!m || null_law || !c || !out) return fail(ctx, HH_ERR_INVALID, "%s: NULL argument", who);
  if (c->dynamics == HH_HESTON || f.bad_strategy(*c))
    return fail(ctx, HH_ERR_UNSUPPORTED, "%s needs LognormalDynamics + the exact law (HH_EXACT_LAW)", who);
  if (c->noise_mode == HH_NOISE_REPLAY || c->n_partials != 0)
    return fail(ctx, HH_ERR_UNSUPPORTED, "%s: GENERATE noise, no dual partials", who);
  int rc = validate(ctx, m, c);
  if (rc) return rc;
  if ((rc = f.law_check())) return rc;
  const WallClock clock;
  std::memset(out, 0, sizeof(*out));
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  const uint32_t n_rec = f.n_records(c->n_paths);
  if ((rc = ensure(ctx, ctx->records, (size_t)n_rec * hh::kRecStride))) return rc;
  hh::DevicePtrs p{};
  p.records = ctx->records;
  if ((rc = stage_noise(ctx, c, p, false))) return rc;  // seeds[0]
  if (terminal && c->terminal_on_device) {
    p.terminal = terminal;
  } else if (terminal) {
    if ((rc = ensure(ctx, ctx->terminal, (size_t)c->n_paths * (c->antithetic ? 2 : 1)))) return rc;
    p.terminal = ctx->terminal;
  }
  if ((rc = begin_timing(ctx))) return rc;
  HH_HIP(ctx, f.launch(p));
  HH_HIP(ctx, hh::launch_reduce_records(ctx->records, n_rec, (double)c->n_paths, ctx->accum, ctx->stream, 1, m, c));
  if ((rc = end_timing(ctx))) return rc;
  HH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HH_HIP(ctx, hipMemcpyAsync(ctx->accum_host, ctx->accum, HH_ACC_LEN * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = release_host_operands(ctx))) return rc;
  if ((rc = copy_back_terminal(ctx, c, terminal))) return rc;
  rc = hh_mc_finalize(m, c, ctx->accum_host, out);
  if (rc) return fail(ctx, rc, "finalize failed: the accumulator holds no trajectories");
  return solve_times(ctx, clock, &out->kernel_ms, &out->total_ms);
}

int hh_mc_solve_jump(hh_ctx* ctx, const hh_model* m, const hh_jump* jump, const hh_config* c, hh_result* out,
                     double* terminal) {
  return terminal_law_call(
      ctx,
      {"hh_mc_solve_jump",  // HH_QE is left to validate
       [](const hh_config& c) { return c.strategy == HH_EULER_MARUYAMA || c.strategy == HH_BROADIE_KAYA; },
       [&] { return check_jump(ctx, "hh_mc_solve_jump", jump, m->T); }, hh::merton_records,
       [&](const hh::DevicePtrs& p) { return hh::launch_merton_exact(*m, *c, *jump, p, ctx->stream); }},
      !jump, m, c, out, terminal);
}

// The scalars hh_carr_madan_jump and hh_carr_madan_vg refuse: their model is S0 and sigma
static bool cm_bad_lognormal_scalars(const hh_model& m, double alpha, double bound) {
  return !(m.S0 > 0.0) || !std::isfinite(m.S0) || !std::isfinite(m.sigma) || !(alpha > 0.0) || !(bound > 0.0);
}

int hh_carr_madan_jump(hh_ctx* ctx, const hh_model* m, const hh_jump* jump, double alpha, double bound,
                       const double* strikes, const double* cps, const double* Ts, const double* r_drifts,
                       const double* discounts, uint32_t n_payoffs, double* prices_out) {
  return carr_madan_basket_call(
      ctx,
      {"hh_carr_madan_jump", [&] { return cm_bad_lognormal_scalars(*m, alpha, bound); }, "bad scalars",
       [&] { return check_jump(ctx, "hh_carr_madan_jump", jump, 0.0); }, false,  // no draw here: the mean of one is not limited
       [&](const double* per_payoff, uint32_t n, double* out) {
         return hh::launch_carr_madan_jump(*m, *jump, alpha, bound, per_payoff, n, out, ctx->stream);
       }},
      !jump, m, alpha, bound, {strikes, cps, Ts, r_drifts, discounts, n_payoffs}, prices_out);
}

// ---- Variance Gamma (hedgehog_mc.h, "Variance Gamma"; kernels: hh_vg.hip, hh_fourier.hip) ----

int hh_mc_path_stats_vg(hh_ctx* ctx, const hh_model* m, const hh_vg* vg, const hh_config* c, uint32_t monitor_every,
                        int32_t include_start, double* stats, int32_t stats_on_device, hh_result* out) {
  return path_stats_call(ctx, {"hh_mc_path_stats_vg", 0, vg}, m, c, monitor_every, include_start, stats, stats_on_device, out);
}

int hh_mc_solve_path_vg(hh_ctx* ctx, const hh_model* m, const hh_vg* vg, const hh_config* c, uint32_t monitor_every,
                        int32_t include_start, const hh_path_payoff* payoffs, uint32_t n_payoffs, hh_result* out,
                        double* path_values, double* stats) {
  return solve_path_call(ctx, {"hh_mc_solve_path_vg", HH_PAYOFF_LOOKBACK_FIXED, vg}, m, c, monitor_every, include_start,
                         payoffs, n_payoffs, out, path_values, stats);
}

int hh_mc_solve_vg(hh_ctx* ctx, const hh_model* m, const hh_vg* vg, const hh_config* c, hh_result* out, double* terminal) {
  return terminal_law_call(
      ctx,
      {"hh_mc_solve_vg", [](const hh_config& c) { return c.strategy != HH_EXACT_LAW; },
       [&] { return check_vg(ctx, "hh_mc_solve_vg", m, vg, 1.0); }, hh::vg_records,
       [&](const hh::DevicePtrs& p) { return hh::launch_vg_exact(*m, *c, *vg, p, ctx->stream); }},
      !vg, m, c, out, terminal);
}

int hh_carr_madan_vg(hh_ctx* ctx, const hh_model* m, const hh_vg* vg, double alpha, double bound, const double* strikes,
                     const double* cps, const double* Ts, const double* r_drifts, const double* discounts,
                     uint32_t n_payoffs, double* prices_out) {
  return carr_madan_basket_call(
      ctx,
      {"hh_carr_madan_vg", [&] { return cm_bad_lognormal_scalars(*m, alpha, bound); }, "bad scalars",
       [&] { return check_vg(ctx, "hh_carr_madan_vg", m, vg, 1.0 + alpha); }, false,
       [&](const double* per_payoff, uint32_t n, double* out) {
         return hh::launch_carr_madan_vg(*m, *vg, alpha, bound, per_payoff, n, out, ctx->stream);
       }},
      !vg, m, alpha, bound, {strikes, cps, Ts, r_drifts, discounts, n_payoffs}, prices_out);
}

// ---- Heston paths by the quadratic-exponential scheme (hedgehog_mc.h; kernel: hh_qe.hip) ----------------------

int hh_mc_path_stats_qe(hh_ctx* ctx, const hh_model* m, const hh_qe* qe, const hh_config* c, uint32_t monitor_every,
                        int32_t include_start, double* stats, int32_t stats_on_device, double* var_T, hh_result* out) {
  return path_stats_call(ctx, {"hh_mc_path_stats_qe", 0, qe, var_T}, m, c, monitor_every, include_start, stats,
                         stats_on_device, out);
}

int hh_mc_solve_path_qe(hh_ctx* ctx, const hh_model* m, const hh_qe* qe, const hh_config* c, uint32_t monitor_every,
                        int32_t include_start, const hh_path_payoff* payoffs, uint32_t n_payoffs, hh_result* out,
                        double* path_values, double* stats, double* var_T) {
  return solve_path_call(ctx, {"hh_mc_solve_path_qe", HH_PAYOFF_LOOKBACK_FIXED, qe, var_T}, m, c, monitor_every, include_start,
                         payoffs, n_payoffs, out, path_values, stats);
}

// ---- several correlated lognormal assets (hedgehog_mc.h; kernel: hh_assets.hip) --------------------------------------

int hh_mc_path_stats_assets(hh_ctx* ctx, const hh_model* m, const hh_assets* assets, const hh_config* c,
                            uint32_t monitor_every, int32_t include_start, double* stats, int32_t stats_on_device,
                            hh_result* out) {
  return path_stats_call(ctx, {"hh_mc_path_stats_assets", 0, assets}, m, c, monitor_every, include_start, stats,
                         stats_on_device, out);
}

int hh_mc_solve_path_assets(hh_ctx* ctx, const hh_model* m, const hh_assets* assets, const hh_config* c,
                            uint32_t monitor_every, int32_t include_start, const hh_path_payoff* payoffs,
                            uint32_t n_payoffs, hh_result* out, double* path_values, double* stats) {
  return solve_path_call(ctx, {"hh_mc_solve_path_assets", HH_PAYOFF_LOOKBACK_FIXED, assets}, m, c, monitor_every, include_start,
                         payoffs, n_payoffs, out, path_values, stats);
}

// ---- local volatility on a tabulated surface (hedgehog_mc.h; kernel: hh_localvol.hip) -------------------------------

int hh_mc_path_stats_lv(hh_ctx* ctx, const hh_model* m, const hh_localvol* lv, const hh_config* c, uint32_t monitor_every,
                        int32_t include_start, int32_t extremes, double* stats, int32_t stats_on_device, hh_result* out) {
  return path_stats_call(ctx, {"hh_mc_path_stats_lv", 0, lv, extremes}, m, c, monitor_every, include_start, stats,
                         stats_on_device, out);
}

int hh_mc_solve_path_lv(hh_ctx* ctx, const hh_model* m, const hh_localvol* lv, const hh_config* c, uint32_t monitor_every,
                        int32_t include_start, int32_t extremes, const hh_path_payoff* payoffs, uint32_t n_payoffs,
                        hh_result* out, double* path_values, double* stats) {
  return solve_path_call(ctx, {"hh_mc_solve_path_lv", HH_PAYOFF_LOOKBACK_FIXED, lv, extremes}, m, c, monitor_every,
                         include_start, payoffs, n_payoffs, out, path_values, stats);
}

// ---- Bates: the quadratic-exponential step with Merton jumps (hedgehog_mc.h; kernels: hh_bates.hip, hh_fourier.hip) ----

int hh_mc_path_stats_bates(hh_ctx* ctx, const hh_model* m, const hh_qe* qe, const hh_jump* jump, const hh_config* c,
                           uint32_t monitor_every, int32_t include_start, double* stats, int32_t stats_on_device,
                           double* var_T, hh_result* out) {
  return path_stats_call(ctx, {"hh_mc_path_stats_bates", 0, qe, jump, var_T}, m, c, monitor_every, include_start, stats,
                         stats_on_device, out);
}

int hh_mc_solve_path_bates(hh_ctx* ctx, const hh_model* m, const hh_qe* qe, const hh_jump* jump, const hh_config* c,
                           uint32_t monitor_every, int32_t include_start, const hh_path_payoff* payoffs,
                           uint32_t n_payoffs, hh_result* out, double* path_values, double* stats, double* var_T) {
  return solve_path_call(ctx, {"hh_mc_solve_path_bates", HH_PAYOFF_LOOKBACK_FIXED, qe, jump, var_T}, m, c, monitor_every, include_start,
                         payoffs, n_payoffs, out, path_values, stats);
}

int hh_carr_madan_bates(hh_ctx* ctx, const hh_model* m, const hh_jump* jump, double alpha, double bound,
                        const double* strikes, const double* cps, const double* Ts, const double* r_drifts,
                        const double* discounts, uint32_t n_payoffs, double* prices_out) {
  return carr_madan_basket_call(
      ctx,
      {"hh_carr_madan_bates",  // hh_carr_madan_basket's scalars, under HH_HESTON
       [&] { return !(m->S0 > 0.0) || !(alpha > 0.0) || !(bound > 0.0) || m->sigma == 0.0; }, "bad scalars",
       [&] { return check_jump(ctx, "hh_carr_madan_bates", jump, 0.0); }, false,
       [&](const double* per_payoff, uint32_t n, double* out) {
         return hh::launch_carr_madan_bates(*m, *jump, alpha, bound, per_payoff, n, out, ctx->stream);
       }},
      !jump, m, alpha, bound, {strikes, cps, Ts, r_drifts, discounts, n_payoffs}, prices_out);
}

// ---- LSM on an ensemble sharded over several devices ------------------------------------------------

size_t hh_lsm_shard_xchg_elems(uint32_t n_steps, int32_t degree) {
  return (size_t)(n_steps + 1) * (size_t)(2 * (degree < 1 ? 1 : degree) + 1);
}

static int shard_phase(hh_ctx* ctx, int phase, uint32_t t, const double* in_dev, double* out_dev) {
  const auto& sh = ctx->shard;
  HH_HIP(ctx, hh::launch_lsm_phase(phase, t, ctx->lsm_grid, sh.ntot, sh.n_steps, sh.m.strike, sh.m.cp,
                                   sh.step_discount, sh.degree, ctx->lsm_tau, ctx->lsm_val,
                                   ctx->lsm_scratch, ctx->records, in_dev, out_dev, ctx->stream));
  return HH_OK;
}

int hh_lsm_shard_begin(hh_ctx* ctx, const hh_model* m, const hh_config* c, int32_t degree,
                       double step_discount, double* xchg_dev) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  ctx->shard.active = false;
  if (!m || !c || !xchg_dev) return fail(ctx, HH_ERR_INVALID, "hh_lsm_shard_begin: NULL argument");
  int rc = lsm_paths(ctx, m, c, degree, step_discount, nullptr);
  if (rc) return rc;
  const uint64_t ntot = c->n_paths * (c->antithetic ? 2 : 1);
  if ((rc = ensure_lsm_buffers(ctx, ntot, c->n_steps, degree))) return rc;
  ctx->shard.m = *m;
  ctx->shard.ntot = ntot;
  ctx->shard.n_steps = c->n_steps;
  ctx->shard.degree = degree;
  ctx->shard.step_discount = step_discount;
  if ((rc = shard_phase(ctx, hh::kLsmPhaseStats, 0, nullptr, xchg_dev))) return rc;
  ctx->shard.active = true;
  return release_host_operands(ctx);
}

int hh_lsm_shard_phase(hh_ctx* ctx, int32_t phase, uint32_t t, const double* in_dev, double* out_dev) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!ctx->shard.active) return fail(ctx, HH_ERR_INVALID, "no sharded LSM in progress");
  if (phase != HH_LSM_PHASE_POW && phase != HH_LSM_PHASE_INIT && phase != HH_LSM_PHASE_STEP)
    return fail(ctx, HH_ERR_INVALID, "unknown LSM phase %d", phase);
  if (!in_dev) return fail(ctx, HH_ERR_INVALID, "hh_lsm_shard_phase: in_dev is NULL");
  const bool emits = phase != HH_LSM_PHASE_STEP ? (phase == HH_LSM_PHASE_POW || ctx->shard.n_steps >= 2)
                                                : t >= 2;
  if (emits && !out_dev) return fail(ctx, HH_ERR_INVALID, "hh_lsm_shard_phase: out_dev is NULL");
  if (phase == HH_LSM_PHASE_STEP && (t < 1 || t >= ctx->shard.n_steps))
    return fail(ctx, HH_ERR_INVALID, "LSM step index %u outside 1..n_steps-1", t);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  return shard_phase(ctx, phase, t, in_dev, out_dev);
}

int hh_lsm_shard_finish(hh_ctx* ctx, double* accum_dev, int32_t* stop_time, double* stop_value,
                        double* spot_grid, uint32_t* rows_regressed, uint32_t* rows_skipped) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!ctx->shard.active) return fail(ctx, HH_ERR_INVALID, "no sharded LSM in progress");
  if (!accum_dev) return fail(ctx, HH_ERR_INVALID, "accum_dev is NULL");
  HH_HIP(ctx, hipSetDevice(ctx->device));
  const auto& sh = ctx->shard;
  int rc = shard_phase(ctx, hh::kLsmPhaseFinal, 0, nullptr, nullptr);
  if (rc) return rc;
  HH_HIP(ctx, hh::launch_reduce_records(ctx->records, hh::lsm_chunks(sh.ntot), (double)sh.ntot,
                                        accum_dev, ctx->stream));
  double counters[2] = {0, 0};
  if ((rc = copy_back_lsm(ctx, sh.ntot, sh.n_steps, sh.degree, counters, stop_time, stop_value))) return rc;
  if (spot_grid)
    HH_HIP(ctx, hipMemcpyAsync(spot_grid, ctx->lsm_grid,
                               (size_t)(sh.n_steps + 1) * sh.ntot * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (rows_regressed) *rows_regressed = (uint32_t)counters[0];
  if (rows_skipped) *rows_skipped = (uint32_t)counters[1];
  ctx->shard.active = false;
  return HH_OK;
}

int hh_lsm_debug_read(hh_ctx* ctx, uint64_t n_paths_total, uint32_t n_steps, int32_t degree,
                      double* out8) {
  if (!ctx || !out8) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  const hh::LsmScratch at(n_paths_total, n_steps, degree);
  if (!ctx->lsm_scratch || ctx->lsm_scratch.cap < at.total)
    return fail(ctx, HH_ERR_INVALID, "hh_lsm_debug_read: no LSM solve of that shape has run");
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  HH_HIP(ctx, hipMemcpy(out8, ctx->lsm_scratch + at.stamps, hh::kLsmStampSlots * sizeof(double), hipMemcpyDeviceToHost));
  return HH_OK;
}

int hh_lsm_finalize(const double* acc, hh_lsm_result* out) {
  if (!acc || !out) return HH_ERR_INVALID;
  const double n = acc[HH_ACC_NPATHS];
  if (!(n >= 1.0)) return HH_ERR_INVALID;
  double mean, var;
  payoff_moments(acc, n, &mean, &var);
  std::memset(out, 0, sizeof(*out));
  out->price = mean;  // price = mean(discount^t * val) (least_squares_montecarlo.jl:133-134)
  out->std_error = std::sqrt(var / n);
  out->n_paths_total = (uint64_t)n;
  return HH_OK;
}

int hh_lsm_solve_grid(hh_ctx* ctx, const hh_model* m, const double* spot_grid_dev, uint64_t n_paths,
                      uint32_t n_steps, int32_t degree, double step_discount, hh_lsm_result* out,
                      int32_t* stop_time, double* stop_value) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!m || !spot_grid_dev || !out)
    return fail(ctx, HH_ERR_INVALID, "hh_lsm_solve_grid: NULL argument");
  const WallClock clock;
  hh_config c{};
  c.n_paths = n_paths;
  c.n_steps = n_steps;
  int rc = lsm_check_scalars(ctx, m, &c, degree, step_discount);
  if (rc) return rc;
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  return lsm_on_grid(ctx, spot_grid_dev, n_paths, n_steps, m, degree, step_discount, out, stop_time,
                     stop_value, clock);
}

int hh_ctx_enable_timing(hh_ctx* ctx, int32_t on) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  if (on && !ctx->tev[0][0]) {
    for (auto& pr : ctx->tev)
      for (auto& e : pr) HH_HIP(ctx, hipEventCreate(&e));
  }
  ctx->timing = on != 0;
  ctx->t_count = 0;
  return HH_OK;
}

int hh_ctx_read_timings(hh_ctx* ctx, double* ms, int32_t cap, int32_t* n_out) {
  if (!ctx || !ms || !n_out || cap < 0) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int n = ctx->t_count < hh_ctx::kTimingSlots ? ctx->t_count : hh_ctx::kTimingSlots;
  if (n > cap) n = cap;
  for (int i = 0; i < n; ++i) {
    float t = 0.f;
    HH_HIP(ctx, hipEventElapsedTime(&t, ctx->tev[i][0], ctx->tev[i][1]));
    ms[i] = t;
  }
  *n_out = n;
  ctx->t_count = 0;
  return HH_OK;
}

uint64_t hh_seeds_fingerprint(const uint64_t* seeds, uint64_t n) {
  // four independent multiply-xorshift lanes over the whole vector (about a millisecond per 10^6 seeds on one
  // core), folded with the length: every element and its position enter
  uint64_t h[4] = {0x9E3779B97F4A7C15ull ^ n, 0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ull, 0x27D4EB2F165667C5ull};
  uint64_t i = 0;
  for (; i + 4 <= n; i += 4)
    for (int l = 0; l < 4; ++l) {
      uint64_t x = (seeds[i + l] + h[l]) * 0xFF51AFD7ED558CCDull;
      h[l] = (x ^ (x >> 29)) + 0x9E3779B97F4A7C15ull;
    }
  for (; i < n; ++i) {
    uint64_t x = (seeds[i] + h[i & 3]) * 0xFF51AFD7ED558CCDull;
    h[i & 3] = (x ^ (x >> 29)) + 0x9E3779B97F4A7C15ull;
  }
  uint64_t f = n;
  for (int l = 0; l < 4; ++l) {
    f = (f ^ h[l]) * 0xC4CEB9FE1A85EC53ull;
    f ^= f >> 32;
  }
  return f ? f : 1;  // 0 is "not given" in hh_seeds_cache
}

int hh_seeds_cache(hh_ctx* ctx, const uint64_t* seeds, uint64_t n, uint64_t fingerprint, const uint64_t** dev_out) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (!seeds || n == 0 || !dev_out) return fail(ctx, HH_ERR_INVALID, "hh_seeds_cache: seeds, n >= 1 and dev_out");
  *dev_out = nullptr;
  if (fingerprint == 0) fingerprint = hh_seeds_fingerprint(seeds, n);
  const uint64_t head = seeds[0], tail = seeds[n - 1];
  hh_ctx::SeedEntry* victim = &ctx->seed_cache[0];
  for (auto& e : ctx->seed_cache) {
    if (e.dev && e.n == n && e.fingerprint == fingerprint && e.head == head && e.tail == tail) {
      e.stamp = ++ctx->seed_clock;
      ++ctx->seed_hits;
      *dev_out = e.dev;
      return HH_OK;
    }
    // the least recently used one goes — never the entry the call before this one returned (its stamp is the clock's):
    // a second thread of this context may be between ITS lookup and the solve that reads the pointer
    const bool newest = e.dev && e.stamp == ctx->seed_clock, victim_newest = victim->dev && victim->stamp == ctx->seed_clock;
    if (!e.dev ? victim->dev != nullptr : (victim->dev && !newest && (victim_newest || e.stamp < victim->stamp))) victim = &e;
  }
  HH_HIP(ctx, hipSetDevice(ctx->device));
  if (victim->dev) {  // hipFree waits for the device: nothing in flight reads the copy any more
    HH_HIP(ctx, hipFree(victim->dev));
    *victim = hh_ctx::SeedEntry{};
    ++ctx->seed_evictions;
  }
  uint64_t* d = nullptr;
  hipError_t e = hipMalloc((void**)&d, n * sizeof(uint64_t));
  if (e != hipSuccess) return fail(ctx, HH_ERR_NOMEM, "hipMalloc(%llu bytes) failed: %s", (unsigned long long)(n * 8), hipGetErrorString(e));
  // synchronous: the caller's vector may change, or go, as soon as this returns
  if ((e = hipMemcpy(d, seeds, n * sizeof(uint64_t), hipMemcpyHostToDevice)) != hipSuccess) {
    (void)hipFree(d);
    return fail(ctx, HH_ERR_HIP, "hipMemcpy of the seeds failed: %s", hipGetErrorString(e));
  }
  victim->dev = d;
  victim->n = n;
  victim->fingerprint = fingerprint;
  victim->head = head;
  victim->tail = tail;
  victim->stamp = ++ctx->seed_clock;
  ++ctx->seed_uploads;
  *dev_out = d;
  return HH_OK;
}

int hh_seeds_cache_stats(hh_ctx* ctx, uint64_t* hits, uint64_t* uploads, uint64_t* evictions) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  if (hits) *hits = ctx->seed_hits;
  if (uploads) *uploads = ctx->seed_uploads;
  if (evictions) *evictions = ctx->seed_evictions;
  return HH_OK;
}

int hh_device_malloc(hh_ctx* ctx, size_t bytes, void** out_dev) {
  if (!ctx || !out_dev) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  hipError_t e = hipMalloc(out_dev, bytes);
  if (e != hipSuccess)
    return fail(ctx, HH_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  return HH_OK;
}

int hh_device_free(hh_ctx* ctx, void* dev) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipFree(dev));
  return HH_OK;
}

int hh_memcpy_h2d(hh_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HH_OK;
}

int hh_memcpy_d2h(hh_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes) {
  if (!ctx) return HH_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock__(ctx->mu);
  HH_HIP(ctx, hipSetDevice(ctx->device));
  HH_HIP(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HH_OK;
}

}  // extern "C"
