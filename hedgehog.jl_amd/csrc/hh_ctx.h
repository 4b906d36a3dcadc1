// The context object behind the C-ABI's opaque hh_ctx, and the helpers every host translation unit
// (hh_api.hip, hh_mgpu.hip) shares.  Internal; the public surface is include/hedgehog_mc.h.
#pragma once
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "hh_kernels.h"

// A device buffer of the context that grows on demand (ensure) and reads as its pointer.  The context's destructor
// frees it: hh_ctx_destroy deletes the context with its device current and the device idle.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // in elements
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;  // one owner
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  operator T*() const { return p; }
};

struct hh_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_switch = nullptr;
  // recorded behind the last copy FROM a caller's host buffer; staged_host: such a copy is queued and the entry
  // point has to wait for it (release_host_operands) before it returns — the caller owns its buffers again then
  hipEvent_t ev_stage = nullptr;
  bool staged_host = false;
  DevBuf<double> records;  // capacities in elements
  DevBuf<uint64_t> seeds;
  DevBuf<double> replay;      // tile-major staging
  DevBuf<double> replay_src;  // path-major staging
  DevBuf<double> terminal;
  DevBuf<double> terminal_d;  // [P][n_total] terminal partials (basket Greeks)
  DevBuf<double> payoffs;     // [2][n_payoffs]: strikes, cps
  DevBuf<double> basket_records;
  DevBuf<double> basket_accum;
  DevBuf<unsigned char> bk_scratch;
  hh::BkTableKey bk_table_key{};  // Bessel tables resident in bk_scratch (dropped by ensure_bk_scratch)
  DevBuf<double> lsm_grid;    // [n_steps+1][ntot]
  DevBuf<double> heston_var;  // [n_steps+1][n_paths] variance rows of the exact Heston grid
  DevBuf<double> path_stats;           // hh::PathStatsLayout: [5 or 7 rows][n_total]
  DevBuf<double> path_values;          // [n_payoffs][n_total] payoffs per member (hh_mc_solve_path, when asked for)
  DevBuf<hh_path_payoff> path_payoffs; // [n_payoffs]
  DevBuf<double> localvol;             // a local-vol call's table, per-step weights and rows (hh_localvol.h)
  // quasi-Monte Carlo (hh_sobol_points, hh_sobol_fill)
  DevBuf<uint32_t> sobol_dirs;            // [HH_SOBOL_MAX_DIMS][32] direction words, uploaded at the context's first Sobol' call
  bool sobol_dirs_ready = false;
  DevBuf<uint32_t> sobol_high;            // [tiles][n_dims][2]: a call's high words (launch_sobol_high)
  DevBuf<hh::SobolOp> sobol_ops;          // the bridge's schedule for sobol_ops_steps steps (0: none yet)
  std::vector<hh::SobolOp> sobol_ops_host;
  uint32_t sobol_ops_steps = 0, sobol_slots = 0;
  DevBuf<double> lsm_val;
  DevBuf<int32_t> lsm_tau;
  DevBuf<double> lsm_scratch;
  DevBuf<double> lsm_policy;   // a policy [n_dates + 1][2m + B], then D^k, k = 0 .. n_dates (hh_lsm_policy_value, hh_lsm_upper_bound)
  DevBuf<double> bounds_cont;  // [2][n_dates][n_outer]: the nested continuation values, then their standard errors
  // sharded LSM in progress (hh_lsm_shard_begin .. hh_lsm_shard_finish)
  struct {
    bool active = false;
    hh_model m{};
    uint64_t ntot = 0;
    uint32_t n_steps = 0;
    int32_t degree = 0;
    double step_discount = 1.0;
  } shard;
  int lsm_form = hh::kLsmFormAuto;  // hh_ctx_set_option(HH_OPT_LSM_FORM)
  int bk_term_cache = 0;            // hh_ctx_set_option(HH_OPT_BK_TERM_CACHE); 0 = the default
  uint64_t bk_last_n = 0;           // trajectories of the last Broadie–Kaya solve (hh_bk_decisions)
  int bk_last_cache = 0;            // … and the term cache it ran with
  int grid_form = HH_GRID_FORM_BATCHED;  // hh_ctx_set_option(HH_OPT_GRID_FORM)
  int grid_order = 1;                    // hh_ctx_set_option(HH_OPT_GRID_ORDER): 1 = a chain's pairs sorted by their Bessel arguments
  DevBuf<unsigned char> bk_sort;         // scratch of the ordered form (hh::bk_grid_sort_bytes)
  uint64_t lsm_persistent_fallbacks = 0;  // persistent launches that gave up and were redone per date
  long long lsm_spin_ticks = -1;          // hh_ctx_set_option(HH_OPT_LSM_SPIN_TICKS); < 0 = the default (1 s)
  DevBuf<double> frecords;         // records of the launches that reduce them themselves: kPoison between launches (hh_sim.h)
  int fuse_reduce = 2;             // hh_ctx_set_option(HH_OPT_FUSE_REDUCE): 0 a second kernel, 1 in the simulation kernel, 2 by size
  unsigned int* finish_state = nullptr;  // device word: a reducer inside a simulation kernel gave up (hh_sim.h); cleared by recover_finish
  long long finish_spin_ticks = -1;      // hh_ctx_set_option(HH_OPT_FINISH_SPIN_TICKS); < 0 = the default (5 s)
  int finish_tile_first = 0;             // hh_ctx_set_option(HH_OPT_FINISH_TILE_FIRST)
  // seed vectors kept in device memory (hh_seeds_cache): content-addressed, least recently used one out
  struct SeedEntry {
    uint64_t* dev = nullptr;
    uint64_t n = 0, fingerprint = 0, head = 0, tail = 0, stamp = 0;
  };
  static constexpr int kSeedEntries = HH_SEED_CACHE_ENTRIES;
  SeedEntry seed_cache[kSeedEntries];
  uint64_t seed_clock = 0, seed_hits = 0, seed_uploads = 0, seed_evictions = 0;
  double* accum = nullptr;       // device, HH_ACC_LEN
  double* accum_host = nullptr;  // pinned, HH_ACC_LEN + 8 (LSM: row counters and the give-up word behind the accumulator)
  // optional per-launch timing of the simulation kernel (hh_ctx_enable_timing)
  static constexpr int kTimingSlots = 256;
  bool timing = false;
  hipEvent_t tev[kTimingSlots][2] = {};
  int t_count = 0;  // pairs recorded since the last read (capped at kTimingSlots)
  char err[512] = {0};
  std::recursive_mutex mu;  // entry points serialise on it: a ctx may be shared between threads
};

namespace {

[[maybe_unused]] int fail(hh_ctx* ctx, int code, const char* fmt, ...) {
  if (ctx) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

#define HH_HIP(ctx, expr)                                                                   \
  do {                                                                                      \
    hipError_t e__ = (hipError_t)(expr);                                                    \
    if (e__ != hipSuccess)                                                                  \
      return fail(ctx, HH_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),  \
                  __FILE__, __LINE__);                                                      \
  } while (0)

template <class T>
int ensure(hh_ctx* ctx, DevBuf<T>& buf, size_t need) {
  if (need <= buf.cap) return HH_OK;
  if (buf.p) HH_HIP(ctx, hipFree(buf.p));
  buf.p = nullptr;
  buf.cap = 0;
  hipError_t e = hipMalloc((void**)&buf.p, need * sizeof(T));
  if (e != hipSuccess)
    return fail(ctx, HH_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", need * sizeof(T),
                hipGetErrorString(e));
  buf.cap = need;
  return HH_OK;
}

// a copy from a caller's host buffer has just been queued on the ctx stream
[[maybe_unused]] inline int note_host_copy(hh_ctx* ctx) {
  HH_HIP(ctx, hipEventRecord(ctx->ev_stage, ctx->stream));
  ctx->staged_host = true;
  return HH_OK;
}
// n elements of a caller's host buffer into the ctx buffer buf, which is made to hold need >= n elements first (the
// padded tile-major increments are copied short); *dev: where the kernels read them
template <class T>
int stage_host(hh_ctx* ctx, DevBuf<T>& buf, size_t need, const T* src, size_t n, const T** dev) {
  int rc = ensure(ctx, buf, need);
  if (rc) return rc;
  HH_HIP(ctx, hipMemcpyAsync(buf, src, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = note_host_copy(ctx))) return rc;
  *dev = buf;
  return HH_OK;
}
// Before an ASYNCHRONOUS entry point returns: every copy it queued from the caller's host memory has read its
// source (pageable memory is staged by the runtime before hipMemcpyAsync returns, PINNED memory is read by the
// DMA engine whenever the stream gets there) — only the copies are waited for, the kernels behind them run on.
[[maybe_unused]] inline int release_host_operands(hh_ctx* ctx) {
  if (!ctx->staged_host) return HH_OK;
  ctx->staged_host = false;
  HH_HIP(ctx, hipEventSynchronize(ctx->ev_stage));
  return HH_OK;
}

// The Broadie–Kaya scratch also holds the Bessel tables bk_table_key describes: a re-allocation may
// come back at the SAME address (hipFree + hipMalloc of a larger block), so the key is dropped with
// the old block and the tables are uploaded again.
[[maybe_unused]] inline int ensure_bk_scratch(hh_ctx* ctx, size_t need) {
  const size_t before = ctx->bk_scratch.cap;
  const int rc = ensure(ctx, ctx->bk_scratch, need);
  if (ctx->bk_scratch.cap != before) ctx->bk_table_key = hh::BkTableKey{};
  return rc;
}

// the wall time of an entry point (hh_result / hh_lsm_result::total_ms), from where it is declared
struct WallClock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// out[0 .. k) from k accumulator vectors of HH_ACC_LEN doubles: result i is of models[i * model_stride] (1: a model
// per result, 0: one model for every payoff of a basket), zeroed, finalized and stamped with the solve's times.
// hh_mc_finalize's status when it refuses one: the caller says why.
[[maybe_unused]] int finalize_results(const hh_model* models, size_t model_stride, const hh_config* c,
                                      const double* acc, uint32_t k, double kernel_ms, double total_ms,
                                      hh_result* out) {
  for (uint32_t i = 0; i < k; ++i) {
    std::memset(&out[i], 0, sizeof(hh_result));
    const int rc = hh_mc_finalize(&models[i * model_stride], c, acc + (size_t)i * HH_ACC_LEN, &out[i]);
    if (rc) return rc;
    out[i].kernel_ms = kernel_ms;
    out[i].total_ms = total_ms;
  }
  return HH_OK;
}

}  // namespace
