/*
 * hedgehog_mc.h — C-ABI of libhedgehog_mc.so, the MI355X (gfx950) Monte Carlo engine that stands in
 * for the hot path of Hedgehog.jl's
 *
 *     solve(prob::PricingProblem{VanillaOption{…,European,C,Spot},I}, method::MonteCarlo)
 *                                             (reference: src/pricing_methods/montecarlo.jl:478-493)
 *
 * and for the ForwardDiff-dual Greeks that run through it (src/greeks/greeks_problem.jl:249-262,
 * 559-568).  The reference has no FFI seam of its own: its extension point is Julia multiple
 * dispatch on `solve`.  The entry points below are what a Julia `ccall` — or the
 * Python host mirror in this repository — binds to replace that method body.
 *
 * Conventions
 *   - plain C types only; every function returns an int status (0 = HH_OK, negative = error) and
 *     never throws or aborts across the boundary; text via hh_last_error().
 *   - all arithmetic is IEEE fp64 (the reference computes in Float64 throughout).
 *   - the caller owns every buffer it passes, for the duration of the call only — also with the
 *     ASYNCHRONOUS entry points: whatever they read from HOST memory (seeds, increments, strikes) has
 *     been read when they return (the call waits for its staging copies, not for its kernels; pinned
 *     host memory included); DEVICE operands of an asynchronous call are the exception, see below.
 *     The library owns whatever it allocates inside hh_ctx and releases it in hh_ctx_destroy().
 *   - a hh_ctx is bound to ONE device and ONE HIP stream; its entry points serialise on an
 *     internal mutex, so sharing one between threads is safe but gains nothing — use one ctx per
 *     host thread / per GPU.  Multi-GPU = either ONE call on a hh_mgpu (one ctx per device, the
 *     shards enqueued concurrently and the all-reduce inside the library: hh_mgpu_solve), or one process (or
 *     thread) per GPU, each with its own ctx, exchanging only the HH_ACC_LEN-double accumulator
 *     vector (hh_mc_accumulate + the caller's all-reduce + hh_mc_finalize).
 *   - DEVICE buffers the caller passes (seeds / replay / terminal `_on_device`, grids) are read and
 *     written on the ctx's stream, which does not wait for any other stream: data produced on another
 *     stream (PyTorch's, say) must be complete before the call — synchronize it, or lend that stream
 *     to the ctx with hh_ctx_set_stream — and results of the ASYNCHRONOUS entry points
 *     (hh_mc_accumulate, hh_wiener_fill, hh_sobol_fill, hh_sobol_points, hh_replay_pack, the hh_lsm_shard_* phases) are
 *     ready only after
 *     hh_ctx_synchronize.  The synchronous ones (hh_mc_solve, hh_lsm_solve, …) return with their
 *     device outputs complete.
 *   - there is NO CPU fallback in this library: without a HIP device every compute entry point
 *     fails with HH_ERR_HIP.
 */
#ifndef HEDGEHOG_MC_H
#define HEDGEHOG_MC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HH_ABI_VERSION 6
#define HH_MAX_PARTIALS 8   /* max. number of dual-number partials carried through one solve    */
#define HH_TILE_PATHS 256   /* paths per tile of the tile-major REPLAY layout (see below)        */
#define HH_ACC_LEN 16       /* doubles in the accumulator vector exchanged between GPUs          */
#define HH_MAX_MODELS 16    /* models one hh_mc_solve_multi call prices on the same draws          */

/* accumulator vector slots (all are plain sums, so one SUM all-reduce combines shards) */
#define HH_ACC_SUM 0        /* Σ payoff (undiscounted; antithetic: Σ of pair averages)           */
#define HH_ACC_SUMSQ 1      /* Σ payoff²                                                         */
#define HH_ACC_DSUM 2       /* [2, 2+HH_MAX_PARTIALS): Σ ∂payoff/∂θ_k                             */
#define HH_ACC_NPATHS 10    /* number of trajectories accumulated                                */
#define HH_ACC_BK_NEWTON_FAIL 11
#define HH_ACC_BK_BISECT 12
#define HH_ACC_BK_MAXGUESS 13
#define HH_ACC_BK_CF_TERMS 14 /* Σ characteristic-function series terms evaluated (Broadie–Kaya) */

enum hh_status {
  HH_OK = 0,
  HH_ERR_INVALID = -1,     /* bad argument (NULL, sizes, ranges)                                  */
  HH_ERR_UNSUPPORTED = -2, /* combination the reference itself cannot run (e.g. BK + antithetic)  */
  HH_ERR_HIP = -3,         /* HIP runtime error, or no HIP device                                 */
  HH_ERR_NOMEM = -4,
  HH_ERR_RCCL = -5,        /* RCCL missing or failed where the caller REQUIRED it (HH_MGPU_RCCL)  */
  HH_ERR_DEVICE_TIMEOUT = -6 /* the record reduction inside a simulation kernel gave up waiting for a
                                workgroup's record (HH_OPT_FINISH_SPIN_TICKS): that solve's sums are lost,
                                the context has been reset and is usable again (hh_ctx_check_last)    */
};

/* montecarlo.jl:8-22 */
enum hh_dynamics { HH_LOGNORMAL = 0, HH_HESTON = 1 };
/* montecarlo.jl:86-115: EulerMaruyama / BlackScholesExact / HestonBroadieKaya */
enum hh_strategy { HH_EULER_MARUYAMA = 0, HH_EXACT_LAW = 1, HH_BROADIE_KAYA = 2,
                   HH_QE = 3 /* the quadratic-exponential Heston step: hh_mc_path_stats_qe, hh_mc_solve_path_qe only */ };
enum hh_noise_mode { HH_NOISE_GENERATE = 0, HH_NOISE_REPLAY = 1 };
enum hh_replay_layout { HH_REPLAY_TILE_MAJOR = 0, HH_REPLAY_PATH_MAJOR = 1 };

/* readings of find_zero(func, x0, Order2(); atol, maxeval) / find_zero(func, (0, max_guess); xtol, maxeval) */
enum hh_bk_root_form { HH_BK_ROOT_SECANT = 0,    /* the secant iteration from (x0 + dx, x0)                        */
                       HH_BK_ROOT_ORDER2 = 1 };  /* Roots' Order2: a Steffensen step, a secant step while f is large */
enum hh_bk_bracket_form { HH_BK_BRACKET_MIDPOINT = 0, /* arithmetic bisection to width <= atol                      */
                          HH_BK_BRACKET_ROOTS = 1 };  /* Roots' Bisection: midpoints of the BIT PATTERNS, to the last bit */
enum hh_bk_caps { HH_BK_CAPS_AS_WRITTEN = 0,     /* `maxeval` caps evaluations / iterations as the author meant    */
                  HH_BK_CAPS_ROOTS_DEFAULT = 1 };/* `maxeval` is no keyword of Roots 2 and is ignored: 40 steps / none */

typedef struct hh_ctx hh_ctx; /* opaque: device, stream, scratch */

/*
 * Model scalars after the host has resolved dates and curves exactly as the reference does:
 *   T        = yearfrac(referenceDate, expiry)                      (montecarlo.jl:173,197)
 *   r_drift  = zero_rate(rate, 0.0) for Euler (montecarlo.jl:176,200),
 *              zero_rate(rate, expiry) for the exact laws (montecarlo.jl:299,318)
 *   discount = df(rate, expiry)                                     (montecarlo.jl:489)
 *   cp       = +1 call / -1 put                                     (payoffs.jl:76-87)
 * Lognormal: sigma is the flat vol; V0, kappa, theta, rho are ignored.
 * d* are the dual-number seeds: each is NULL or points to n_partials doubles, direction k of
 * parameter θ being dθ[k].  (Spot enters as x0 = log S0, the library applies dx0 = dS0/S0.)
 * Cost: the library carries per trajectory one derivative per PARAMETER with a non-zero seed among
 * V0, kappa, theta, sigma (at most 4, whatever n_partials is) and assembles the n_partials
 * directions from them; seeds on S0, r_drift, discount and strike cost nothing per trajectory.
 */
typedef struct hh_model {
  double S0, V0, kappa, theta, sigma, rho;
  double r_drift, discount, T, strike, cp;
  const double *dS0, *dV0, *dkappa, *dtheta, *dsigma, *dr_drift, *ddiscount, *dstrike;
} hh_model;

typedef struct hh_config {
  int32_t dynamics;          /* enum hh_dynamics                                                  */
  int32_t strategy;          /* enum hh_strategy                                                  */
  int32_t antithetic;        /* 0 NoVarianceReduction, 1 Antithetic (montecarlo.jl:29-43)         */
  int32_t em_split;          /* Euler diffusion evaluated at K=u+dt·f(u) (1) or at u (0)          */
  int32_t compat_sqrt_alpha; /* exact lognormal mean uses (r-σ²/2)·√T as montecarlo.jl:302 (1)
                                or the correct ·T (0); identical at T = 1                         */
  int32_t noise_mode;        /* enum hh_noise_mode                                                */
  int32_t replay_layout;     /* enum hh_replay_layout (REPLAY only)                               */
  int32_t seeds_on_device;   /* seeds / replay / terminal point to device memory of ctx's device  */
  int32_t replay_on_device;
  int32_t terminal_on_device;
  uint32_t n_steps;          /* SimulationConfig.steps (montecarlo.jl:60); exact laws ignore it   */
  uint32_t n_partials;       /* 0..HH_MAX_PARTIALS                                                */
  uint64_t n_paths;          /* SimulationConfig.trajectories of THIS shard: 1 .. 2^32 - 256 per
                                call (one 256-thread workgroup per 256 trajectories, < 2^32
                                threads per launch); larger ensembles are sharded by path_offset.
                                n_steps: Euler at most 262 140; LSM / exact grid at most 65 534   */
  uint64_t path_offset;      /* global index of this shard's first trajectory (exact laws draw by
                                global index from ONE key, montecarlo.jl:456, so results do not
                                depend on the sharding)                                           */
  const uint64_t* seeds;     /* Euler: ≥ n_paths per-trajectory seeds (montecarlo.jl:331);
                                exact laws: seeds[0] only (montecarlo.jl:456)                     */
  const double* replay;      /* REPLAY: Wiener increments, see hh_replay_elems()                  */
  /* Broadie–Kaya controls, defaults of sample_from_cf.jl:27,50,75,105-113 when 0 */
  double bk_n_sigma;         /* n = 5                                                             */
  double bk_cf_tol;          /* cf_tol = 1e-3                                                     */
  double bk_atol;            /* atol = 1e-4                                                       */
  double bk_moment_h;        /* h = 1e-2                                                          */
  int32_t bk_newton_maxiter; /* 10                                                                */
  int32_t bk_bisect_maxiter; /* 100                                                               */
  /* How the two `find_zero` calls of inverse_cdf (sample_from_cf.jl:118,128) are READ — Roots.jl is not part of the
     reference's tree, and three things about those calls cannot be told from its text (the enums above name them,
     DESIGN.md says why; julia/parity_replay.jl's `bk_root_probe` + tools/check_reference_replay.py decide them on a
     Julia host).
     All 0 = what this library prices with.  Any other value sends the whole ensemble through the whole-trajectory
     kernel (a parity seam, ~10x slower), with the same draws.                                              */
  int32_t bk_root_form;      /* enum hh_bk_root_form                                              */
  int32_t bk_bracket_form;   /* enum hh_bk_bracket_form                                           */
  int32_t bk_caps;           /* enum hh_bk_caps                                                   */
  int32_t reserved0;         /* 0                                                                 */
  /* Optional operand-shape checks (0 = not checked): the number of ELEMENTS behind `seeds` and
     `replay`.  When given, a buffer shorter than what the kernels will index is rejected with
     HH_ERR_INVALID on the host instead of faulting on the device.                               */
  uint64_t seeds_len;
  uint64_t replay_len;
} hh_config;

typedef struct hh_result {
  double price;               /* discount · mean(payoff)            (montecarlo.jl:489-490)       */
  double std_error;           /* build extension; the reference computes none                     */
  double sum_payoff, sumsq_payoff;
  double dprice[HH_MAX_PARTIALS]; /* partials of price, direction k                              */
  uint64_t n_paths_done;
  uint64_t bk_newton_fail, bk_bisect_fallback, bk_maxguess_fallback, bk_cf_terms;
  double kernel_ms;           /* HIP-event time of everything the call enqueued: staging copies
                                 of host seeds / increments, simulation, record reduction; the
                                 FIRST call of a size also grows the ctx's scratch buffers
                                 (hipMalloc / hipFree synchronise) inside this bracket — use
                                 hh_ctx_enable_timing for the simulation kernel alone             */
  double total_ms;            /* host wall time of the call                                       */
} hh_result;

int hh_abi_version(void);

/* Context. device_id is a HIP device ordinal of this process. */
int hh_ctx_create(hh_ctx** out, int device_id);
void hh_ctx_destroy(hh_ctx* ctx);
/* Borrow an external hipStream_t (e.g. PyTorch's current stream).  NULL is a valid handle: the
 * device's default (null) stream — which is what PyTorch uses unless told otherwise.
 * hh_ctx_reset_stream goes back to the ctx's own non-blocking stream.  A switch orders the new
 * stream behind whatever the ctx still has queued on the old one (the asynchronous entry points
 * share the ctx's scratch buffers); the borrowed stream must stay alive until then. */
int hh_ctx_set_stream(hh_ctx* ctx, void* hip_stream);
int hh_ctx_reset_stream(hh_ctx* ctx);
const char* hh_last_error(const hh_ctx* ctx); /* NUL-terminated, owned by ctx (or static if NULL) */
/* Build options of a context (none changes a result).  HH_OPT_LSM_FORM: how hh_lsm_solve /
 * hh_lsm_solve_grid run the backward induction.
 *   HH_LSM_FORM_PERSISTENT  ONE launch that keeps every trajectory's stopping state in registers,
 *                           reads each row of the grid once and exchanges the per-date sums between
 *                           its workgroups in the kernel; applies to ensembles of up to 2^21
 *                           trajectories (256 chunks); a COOPERATIVE launch — refused by the runtime, and
 *                           replaced by the other form, when its workgroups cannot all be resident;
 *   HH_LSM_FORM_PER_DATE    one launch per exercise date;
 *   HH_LSM_FORM_AUTO        (default) the persistent form whenever it applies (since round 3 it is the
 *                           faster one at every size: 2·10^6 x 100 dates 1.6 vs 2.9 ms, 2.6·10^5 x 100
 *                           0.59 vs 0.71 ms, 4·10^3 x 100 0.45 vs 0.50 ms), a launch per date beyond
 *                           2^21 trajectories.
 * All forms give bit-identical prices and stopping decisions.
 *
 * HH_OPT_BK_TERM_CACHE: how many CDF-series terms Re ϕ(h·j) the Broadie–Kaya kernels keep per column
 * (8 … 1024, default 256).  A column belongs to a resident workgroup slot of the kernel, not to a
 * trajectory, so the cache is 8 bytes x terms x 393 216 columns (0.81 GB at 256 terms) whatever the
 * ensemble size; beside it a solve keeps 48 bytes per trajectory.  Series that fit are evaluated once
 * and inverted on the cached terms; a trajectory whose series is longer re-evaluates the terms beyond
 * the cache in every CDF call (as the reference does with all of them), in a separate, slower kernel.
 * With the reference's controls the series has 10–15 terms (60 at short maturities, 100–250 for
 * d = 4κθ/σ² ≪ 1 or cf_tol ≪ 1e-3).
 *
 * HH_OPT_GRID_FORM: how hh_heston_exact_grid (and LSM on those paths) runs the dates of a grid:
 *   HH_GRID_FORM_BATCHED   (default) the variances of all dates first, then ONE kernel chain over every
 *                          (date, trajectory) pair — given the variances the CF inversions of different
 *                          dates are independent — then the spot rows; a chain takes at most 2^22 pairs
 *                          (48 bytes each; longer grids run as several chains);
 *   HH_GRID_FORM_PER_DATE  one kernel chain per date.
 * Both forms give bit-identical grids.
 *
 * HH_OPT_LSM_SPIN_TICKS: bound of every wait inside the persistent LSM launch, in ticks of the 100 MHz
 * constant clock (default -1 = 10^8 = one second).  The launch is cooperative (hipLaunchCooperativeKernel:
 * a grid that cannot be resident as a whole is refused at launch and the launch-per-date form runs), so
 * the bound is only the last guard; 0 makes every workgroup give up at once, which is how the tests
 * force the give-up-and-redo path (hh_lsm_result.persistent_fallbacks counts it; same result).
 *
 * HH_OPT_GRID_ORDER: 1 (default) a batched chain of hh_heston_exact_grid (HH_GRID_FORM_BATCHED) runs its (date,
 * trajectory) pairs sorted by a coarse key of V0·V_T — the size of their Bessel argument — so that the lanes of a
 * wave share a regime of the Bessel function and series of similar length (short transitions spread both widely:
 * 0.53 active lanes per instruction unsorted; the same draws sorted run the chain 32 % faster); 0: in their
 * natural order.  The same grid either way, bit for bit.
 *
 * HH_OPT_FUSE_REDUCE: who adds the workgroups' partial sums of a single-payoff solve (mean(payoffs),
 * montecarlo.jl:490): 0 a second kernel (reduce_records_kernel), 1 the simulation kernel itself (the last
 * tile's workgroup, once every record has arrived), 2 (default) by what was measured — the simulation kernel
 * up to 512 records (a launch saved is 2 % of a small solve) and for Euler runs of 32 steps or more (the
 * reducer's wait disappears behind the other workgroups: -0.3 % at 10^6 x 252), the second kernel for short
 * kernels with thousands of records (the exact law at 10^6 - 10^7 trajectories: 1-4 % faster that way).  The
 * same additions in the same order every way: bit-identical results.
 *
 * HH_OPT_FINISH_SPIN_TICKS: how long the workgroup that adds the records INSIDE a simulation kernel
 * (HH_OPT_FUSE_REDUCE) waits for a record that has not arrived, in ticks of the 100 MHz constant clock (default
 * -1 = 5·10^8 = five seconds).  Every workgroup needs only a slot of its own to finish, so the bound is the last
 * guard against a workgroup that died or a queue preempted for that long.  When it is passed the solve's sums are
 * NaN, and — because the missing record may still land in the buffer the next launch reads — every solve queued
 * behind it on this context gives NaN too, until the host has reset the buffer: hh_mc_solve and its kin do that
 * themselves and return HH_ERR_DEVICE_TIMEOUT; callers of the asynchronous entry points ask with
 * hh_ctx_check_last.  0 makes the reducer give up on the first record it does not find, which — with
 * HH_OPT_FINISH_TILE_FIRST = 1: the FIRST tile's workgroup adds the records instead of the last one's, so nearly
 * none is there when it looks — is how the tests force that path. */
enum hh_option { HH_OPT_LSM_FORM = 1, HH_OPT_BK_TERM_CACHE = 2, HH_OPT_GRID_FORM = 3, HH_OPT_LSM_SPIN_TICKS = 4,
                 HH_OPT_FUSE_REDUCE = 5, HH_OPT_GRID_ORDER = 6, HH_OPT_FINISH_SPIN_TICKS = 7,
                 HH_OPT_FINISH_TILE_FIRST = 8 };
enum hh_grid_form { HH_GRID_FORM_PER_DATE = 0, HH_GRID_FORM_BATCHED = 1 };
enum hh_lsm_form { HH_LSM_FORM_PER_DATE = 0, HH_LSM_FORM_PERSISTENT = 1, HH_LSM_FORM_AUTO = 2 };
int hh_ctx_set_option(hh_ctx* ctx, int32_t option, int64_t value);
/*
 * For callers of the ASYNCHRONOUS entry points (hh_mc_accumulate and its kin, whose sums stay on the device): waits
 * for the context's stream, then HH_OK — or HH_ERR_DEVICE_TIMEOUT when a record reduction inside a simulation kernel
 * gave up since the last check (HH_OPT_FINISH_SPIN_TICKS): the accumulators written since then hold NaN, the
 * context's record buffer has been reset, the context is usable again.  Call it where the sums are read back (a NaN
 * in slot HH_ACC_NPATHS says why), or once per batch of solves.
 */
int hh_ctx_check_last(hh_ctx* ctx);

/*
 * Replaces the body of solve(prob, ::MonteCarlo) (montecarlo.jl:478-493): simulate, payoff,
 * discount·mean.  Synchronous.  `terminal` (nullable) receives the samples at expiry that the
 * reference keeps in MonteCarloSolution.ensemble (pricing_solutions.jl:22-27): n_paths doubles,
 * followed by n_paths mirrored samples when antithetic.
 */
int hh_mc_solve(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, hh_result* out,
                double* terminal);

/*
 * Split form for path-sharded multi-GPU runs: enqueue simulation + reduction on the ctx stream and
 * leave the HH_ACC_LEN accumulator doubles in DEVICE memory `accum_dev`, so the caller can all-reduce
 * them (RCCL) and then finalize on the host.  No wait for the kernels; host seeds / increments in cfg
 * have been read when the call returns (it waits for their staging copies only).
 */
int hh_mc_accumulate(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, double* accum_dev,
                     double* terminal);
/* Pure host arithmetic: accumulator vector (HOST memory) -> price, std_error, dprice. */
int hh_mc_finalize(const hh_model* model, const hh_config* cfg, const double* accum_host,
                   hh_result* out);

/*
 * SEVERAL MODELS ON THE SAME DRAWS, in one pass — what the reference's bumped Greeks are made of:
 * compute_fd_derivative (greeks_problem.jl:279-303) solves 2 problems that differ in one number, the
 * second-order stencils (:396-422) 3 or 4, each a full solve(prob, method) with the seeds of the SAME
 * SimulationConfig (common random numbers).  Here the n_models problems — same payoff type, same cfg: dynamics,
 * strategy, trajectories, steps, seeds or increments, variance reduction — are simulated TOGETHER: a lane
 * carries one state per model and steps them all on each draw, so the normals (GENERATE) or the 16 bytes of
 * increments (REPLAY) are paid once per path-step, not once per model and path-step.  Result k is what
 * hh_mc_solve(ctx, &models[k], cfg, …) returns, bit for bit (same arithmetic per model, same summation order).
 *   models     n_models hh_model (1 .. HH_MAX_MODELS); anything may differ between them (spot, variance
 *              parameters, ρ, rate, discount, expiry time T, strike, call/put); d* seeds are ignored
 *   cfg        as for hh_mc_solve; n_partials must be 0 (HH_ERR_UNSUPPORTED otherwise)
 *   out        n_models results;   accum_dev  n_models x HH_ACC_LEN doubles, model-major (all-reducible as ONE
 *              vector over path shards, then hh_mc_finalize(&models[k], cfg, accum + k·HH_ACC_LEN, &out[k]))
 *   terminals  NULL, or n_models pointers (each nullable): model k's samples at expiry, as `terminal` of hh_mc_solve
 * Up to 4 models share a pass (more run as ⌈n/4⌉ passes); Euler–Maruyama and the exact lognormal law share
 * their draws.  Broadie–Kaya shares a whole CHAIN between models that differ in nothing its variance process
 * sees (κ, θ, σ, V0, T equal: a bumped spot, rate, ρ or strike — the finite-difference delta, gamma, rho): the
 * first such model runs the chain, the others are finished from the ∫V it sampled (~10 µs each at 10^6
 * trajectories; a central delta 0.355 ms for the reference's two solves of 0.336); a bumped κ, θ, σ, V0 or T is
 * a chain of its own.
 * Path-major REPLAY increments are repacked to the tile-major layout first.
 */
int hh_mc_solve_multi(hh_ctx* ctx, const hh_model* models, uint32_t n_models, const hh_config* cfg,
                      hh_result* out, double* const* terminals);
int hh_mc_accumulate_multi(hh_ctx* ctx, const hh_model* models, uint32_t n_models, const hh_config* cfg,
                           double* accum_dev, double* const* terminals);

/*
 * Diagnostics of the last HH_BROADIE_KAYA solve of this context (hh_mc_solve / _accumulate with the same
 * n_paths; the scratch it reads is overwritten by the next Broadie–Kaya call): per trajectory, WHAT the
 * root search of inverse_cdf (sample_from_cf.jl:105-135) did —
 *   decisions[i]   bits 0-7   CDF evaluations of the secant iteration (find_zero(…, Order2(); maxevals))
 *                  bits 8-9   0 the secant's root was accepted, 1 bisection finished it (:127-133),
 *                             2 no sign change: max_guess (:124-126)
 *                  bits 16-23 bisection iterations;   bit 31  series longer than the term cache
 *   series_len[i]  terms of the CDF series, set by |ϕ(h j)|/j < π·cf_tol/2 (sample_from_cf.jl:88)
 * Two implementations that agree on both have run the same sequence of operations on that trajectory;
 * the parity tests compare samples per trajectory where they agree and count where they do not.
 * Either output may be NULL.
 */
int hh_bk_decisions(hh_ctx* ctx, uint64_t n_paths, uint32_t* decisions, uint32_t* series_len);

/*
 * Multi-GPU solve in ONE call from ONE host thread — what solve(prob, method) (montecarlo.jl:478-493,
 * the one EnsembleProblem of :329-333,351) becomes when the trajectories are sharded over the GPUs of
 * a node.  A hh_mgpu owns one hh_ctx (own stream, own scratch) per listed device.
 * hh_mgpu_solve cuts the ensemble into contiguous ranges [g·per, min(N, (g+1)·per)), per = ⌈N/G⌉
 * (rounded up to a multiple of HH_TILE_PATHS for tile-major REPLAY data, whose tiles cannot be cut),
 * slices seeds / increments / terminal samples by the same ranges (exact laws: path_offset), enqueues
 * every shard's kernels without waiting, and combines the HH_ACC_LEN-double accumulator vectors
 *   HH_MGPU_REDUCE_RCCL  by ONE ncclAllReduce(ncclSum, ncclDouble) inside ncclGroupStart/End on the
 *                        shards' own streams (communicators from ncclCommInitAll at creation; RCCL is
 *                        bound at run time — librccl.so.1, or the path in $HEDGEHOG_MC_RCCL — so the
 *                        library itself has no link-time dependency on it), or
 *   HH_MGPU_REDUCE_HOST  by a deterministic ordered sum on the host, g = 0 … G−1 (also what is used
 *                        when RCCL is absent, fails to initialise — e.g. a device listed twice — or
 *                        fails in the call: the solve is still completed, hh_mgpu_last_error() says why).
 * Draws depend on (seed, counter) only, so a G-device result differs from the one-device result by
 * the order of that last sum alone (≤ 1e-13 relative); with one device there is no sum and the result
 * is hh_mc_solve's bit for bit.
 *   flags of hh_mgpu_create: HH_MGPU_AUTO  RCCL when n_devices > 1 and it initialises, else host sum;
 *                            HH_MGPU_HOST_SUM  never touch RCCL;
 *                            HH_MGPU_RCCL  RCCL or fail (HH_ERR_RCCL), used even for one device.
 * Enqueueing: the host-side cost of one shard (checks, events, launches) is tens of microseconds, so
 * the devices are served CONCURRENTLY — device 0 by the calling thread, every other device by a
 * library-owned thread bound to it (created on first use, joined in hh_mgpu_destroy; it polls for
 * ~150 µs after a job and sleeps otherwise, and never calls back into the host language).
 * hh_mgpu_set_option(HH_MGPU_OPT_ENQUEUE, HH_MGPU_ENQUEUE_SERIAL) enqueues one shard after the other
 * from the calling thread instead; results are identical.  hh_mgpu_enqueue_stats reports what the last
 * solve's enqueue phase cost on the host: per shard (measured in the thread that enqueued it) and as a
 * whole (wall time until every shard was enqueued).
 * A collective that FAILS in the call (ncclAllReduce refusing rank g after ranks < g were enqueued) may
 * leave kernels on the earlier ranks' streams that wait for peers which never come.  The library never
 * synchronises such a stream: it aborts the communicators (ncclCommAbort — a library without it is not used), retires every shard stream
 * for a fresh one that continues behind the shard's last kernel, and — HH_MGPU_AUTO — completes this
 * and every later solve with the host's ordered sum (hh_mgpu_reduce_mode() then says HOST); with
 * HH_MGPU_RCCL the call returns HH_ERR_RCCL once the caller's buffers are no longer read, and so does
 * every later call on that context.
 * hh_mgpu_solve takes HOST buffers in cfg (seeds, replay) and for `terminal` (n_paths doubles, then the
 * n_paths mirrored samples when antithetic — the layout of hh_mc_solve); *_on_device must be 0.  The
 * REPLAY buffer as a whole must be 16-byte aligned, as for hh_mc_solve; a shard's slice need not be
 * (odd row lengths cut at odd trajectories are staged by the library).
 * hh_mgpu_solve_shards takes one hh_config per device exactly as hh_mc_accumulate would on that device
 * (device-resident seeds / increments allowed; n_paths = 0 leaves a device idle) and optional per-shard
 * terminal pointers — for callers that keep their inputs in HBM.  hh_mgpu_ctx(mg, i) is the i-th
 * device's context (hh_device_malloc, hh_wiener_fill, hh_ctx_enable_timing … on that device); it stays
 * owned by mg.  out->kernel_ms is the LONGEST shard's HIP-event time, total_ms the host wall time.
 * After any error return nothing that reads the caller's buffers is still running (a collective that lost its
 * peers may still sit on a retired stream until ncclCommAbort has released it: hh_mgpu_destroy then leaves that
 * device's streams and buffers alone rather than wait for it).  Should a shard be impossible to move off the
 * stream the failed collective was enqueued on — a stream lent with hh_ctx_set_stream, or no new stream to be
 * had — the context is stuck: the call and every later one return HH_ERR_RCCL, whatever the flags.
 */
typedef struct hh_mgpu hh_mgpu;
enum hh_mgpu_flags { HH_MGPU_AUTO = 0, HH_MGPU_HOST_SUM = 1, HH_MGPU_RCCL = 2 };
enum hh_mgpu_reduce { HH_MGPU_REDUCE_HOST = 0, HH_MGPU_REDUCE_RCCL = 1 };
int hh_mgpu_create(hh_mgpu** out, const int* device_ids, int n_devices, int flags);
void hh_mgpu_destroy(hh_mgpu* mg);
const char* hh_mgpu_last_error(const hh_mgpu* mg);
int hh_mgpu_n_devices(const hh_mgpu* mg);
int hh_mgpu_reduce_mode(const hh_mgpu* mg);       /* enum hh_mgpu_reduce in use                    */
/* What a caller may print next to "reduce: rccl".  hh_mgpu_selftest sends a vector of ones from every device
 * through the exchange a solve uses (the grouped ncclAllReduce on the shards' streams, or the host's ordered
 * sum) and returns the count that came back — the ranks that really took part — and the mode it ran in.
 * hh_mgpu_rccl_info names the library the collective entry points were bound from (dladdr of ncclAllReduce;
 * empty when none), its ncclGetVersion (0 when unknown) and whether $HEDGEHOG_MC_RCCL chose it; HH_ERR_RCCL
 * when no usable RCCL is bound (ncclCommAbort is required: see above). */
int hh_mgpu_selftest(hh_mgpu* mg, int32_t* ranks_out, int32_t* reduce_mode_out /* nullable */);
int hh_mgpu_rccl_info(const hh_mgpu* mg, char* path_out, size_t cap, int32_t* version_out, int32_t* from_env_out);
enum hh_mgpu_option { HH_MGPU_OPT_ENQUEUE = 1 };
enum hh_mgpu_enqueue { HH_MGPU_ENQUEUE_SERIAL = 0, HH_MGPU_ENQUEUE_THREADS = 1 /* default */ };
int hh_mgpu_set_option(hh_mgpu* mg, int32_t option, int64_t value);
/* host microseconds of the last solve's enqueue phase: shard_us[n_devices] (nullable), *phase_us (nullable) */
int hh_mgpu_enqueue_stats(hh_mgpu* mg, double* shard_us, double* phase_us);
hh_ctx* hh_mgpu_ctx(hh_mgpu* mg, int i);          /* NULL when i is out of range                   */
/* shard g of an ensemble of n_paths over n_devices, as hh_mgpu_solve cuts it (tile_aligned = 1 for
 * tile-major REPLAY increments) */
void hh_mgpu_shard_range(uint64_t n_paths, int n_devices, int g, int tile_aligned, uint64_t* start,
                         uint64_t* stop);
int hh_mgpu_solve(hh_mgpu* mg, const hh_model* model, const hh_config* cfg, hh_result* out,
                  double* terminal);
int hh_mgpu_solve_shards(hh_mgpu* mg, const hh_model* model, const hh_config* shard_cfgs /* n_devices */,
                         hh_result* out, double* const* terminals /* nullable; n_devices, each nullable */);
int hh_mgpu_solve_basket(hh_mgpu* mg, const hh_model* model, const hh_config* cfg, const double* strikes,
                         const double* cps, uint32_t n_payoffs, hh_result* out /* n_payoffs */);
/* hh_mc_solve_multi with the trajectories sharded over the devices of mg: every device steps all n_models
 * models on its range's draws, ONE all-reduce of the n_models x HH_ACC_LEN accumulator block.  Host buffers
 * in cfg, as for hh_mgpu_solve; no terminal samples. */
int hh_mgpu_solve_multi(hh_mgpu* mg, const hh_model* models, uint32_t n_models, const hh_config* cfg,
                        hh_result* out /* n_models */);


/*
 * Several payoffs on ONE simulation — solve(::BasketPricingProblem, method) for payoffs that share
 * an expiry (src/calibration/basket.jl:35-38 prices them as independent solves; with the fixed
 * seeds of SimulationConfig they see the same trajectories, so the results coincide).  Payoff k is
 * max(cps[k]·(S_T − strikes[k]), 0); model->strike / model->cp are ignored.  The accumulator block
 * is n_payoffs × HH_ACC_LEN doubles, payoff-major (all-reducible as one vector); dual partials of
 * the model parameters are carried for every payoff (strike partials are not).  Works for every
 * simulation strategy, Broadie–Kaya included.
 */
int hh_mc_accumulate_basket(hh_ctx* ctx, const hh_model* model, const hh_config* cfg,
                            const double* strikes, const double* cps, uint32_t n_payoffs,
                            double* accum_dev, double* terminal);
int hh_mc_solve_basket(hh_ctx* ctx, const hh_model* model, const hh_config* cfg,
                       const double* strikes, const double* cps, uint32_t n_payoffs,
                       hh_result* out /* n_payoffs */, double* terminal);

/*
 * Carr–Madan Fourier price of a European vanilla on the device — solve(prob, ::CarrMadan)
 * (src/pricing_methods/carr_madan.jl:47-92) with the Heston marginal law (heston.jl:307-319) or the
 * lognormal one (sample_from_cf.jl:14-16; compat_sqrt_alpha as in hh_config).  It is the analytic
 * value the reference's MC tests compare against; model->r_drift = zero_rate(rate, expiry),
 * model->T = yearfrac(rate.reference_date, expiry), model->discount = df(rate, expiry).
 * alpha = damping factor, bound = integration bound (CarrMadan(α, bound, dynamics)).
 * The quadrature is fixed: 256 panels over (-bound, bound), each cut into the fewest equal sub-panels of
 * half-width <= 0.75 alpha (one for alpha = 1, bound <= 192), 16-point Gauss–Legendre on each; that keeps the
 * transform's pole at v = i alpha resolved to rounding.  bound/alpha > 196608 (more than 1024 sub-panels) is
 * HH_ERR_INVALID, for all three entry points.  Heston: the (alpha+1)-th moment of S_T must be finite (for every T:
 * kappa - rho sigma (alpha+1) > 0 and its square >= sigma^2 alpha (alpha+1)); this is not checked.
 */
int hh_carr_madan(hh_ctx* ctx, const hh_model* model, int32_t dynamics, int32_t compat_sqrt_alpha,
                  double alpha, double bound, double* price_out);
/*
 * The same for a basket in ONE launch (one workgroup per payoff) — solve(::BasketPricingProblem,
 * ::CarrMadan), i.e. src/calibration/basket.jl:35-38 over carr_madan.jl:47-92: what the calibration
 * objective evaluates at every iterate (src/calibration/calibration.jl:75-88).  The payoffs share the
 * model's parameters (S0 and V0, kappa, theta, sigma, rho — or the lognormal sigma); per payoff k:
 * strikes[k], cps[k] (+1 call / -1 put), Ts[k] = yearfrac(rate.reference_date, expiry_k),
 * r_drifts[k] = zero_rate(rate, expiry_k), discounts[k] = df(rate, expiry_k).  model->strike, cp, T,
 * r_drift and discount are ignored.  1 .. 2^20 payoffs per call.
 */
int hh_carr_madan_basket(hh_ctx* ctx, const hh_model* model, int32_t dynamics,
                         int32_t compat_sqrt_alpha, double alpha, double bound, const double* strikes,
                         const double* cps, const double* Ts, const double* r_drifts,
                         const double* discounts, uint32_t n_payoffs, double* prices_out);
/*
 * Prices AND their gradient in one launch — what a ForwardDiff-differentiated calibration objective
 * (calibration.jl:75-88 with AutoForwardDiff) pushes through carr_madan.jl:47-92 and heston.jl:307-319
 * as Dual numbers.  grad_out[k][HH_CM_GRAD_LEN] = ∂price_k / ∂(S0, V0, kappa, theta, sigma, rho,
 * r_drift_k, discount_k) in that order (enum hh_cm_grad); the caller's Dual price is
 * price + Σ_j grad[j]·(partials of parameter j), r_drift_k and discount_k being whatever its rate curve
 * makes of its parameters.  Lognormal dynamics: sigma = the volatility; V0, kappa, theta, rho slots 0.
 */
enum hh_cm_grad { HH_CM_GRAD_S0 = 0, HH_CM_GRAD_V0, HH_CM_GRAD_KAPPA, HH_CM_GRAD_THETA, HH_CM_GRAD_SIGMA,
                  HH_CM_GRAD_RHO, HH_CM_GRAD_R_DRIFT, HH_CM_GRAD_DISCOUNT, HH_CM_GRAD_LEN };
int hh_carr_madan_basket_grad(hh_ctx* ctx, const hh_model* model, int32_t dynamics,
                              int32_t compat_sqrt_alpha, double alpha, double bound,
                              const double* strikes, const double* cps, const double* Ts,
                              const double* r_drifts, const double* discounts, uint32_t n_payoffs,
                              double* prices_out, double* grad_out);

/*
 * Cox–Ross–Rubinstein binomial trees — solve(prob, ::CoxRossRubinsteinMethod) for a European or American
 * VanillaOption on BlackScholesInputs (src/pricing_methods/cox_ross_rubinstein.jl:99-141), and a basket of them
 * (basket.jl:35-38) in ONE launch, one tree per payoff, all with the same number of steps.  Per tree k:
 *   forwards[k]  = spot / df(rate, expiry)
 *   strikes[k], cps[k] (+1 call / -1 put)
 *   ups[k]       = u = exp(σ·√ΔT), ΔT = yearfrac(referenceDate, expiry) / steps  (p = 1/(1+u) is formed here)
 *   discounts[k] = exp(−zero_rate(rate, expiry)·ΔT), the per-step discount, the same at every step
 *   styles[k]    = enum hh_crr_style
 * HH_CRR_AMERICAN_SPOT trees exercise on sf_i·F·u^k: spot_factors holds n_spot_rows rows of `steps` doubles,
 * sf_i = exp(−zero_rate(rate, tᵢ)·(steps − i)·ΔT) at element i (cox_ross_rubinstein.jl:75-81), and tree k reads
 * row spot_row_of_tree[k] — a surface uploads one row per expiry.  spot_factors, spot_row_of_tree and
 * n_spot_rows (1 .. n_trees) are read only when some tree has that style (NULL / 0 otherwise).
 * 1 <= steps <= HH_CRR_MAX_STEPS, 1 .. 2^20 trees per call; prices_out[n_trees].  Synchronous.  The node
 * factors u^k follow the fixed IEEE sequence of csrc/hh_crr.hip, so prices are reproducible bit for bit, and the
 * kernel form depends on `steps` alone: a tree prices the same alone or in a basket.  Scalars are not checked —
 * every loop is bounded by `steps`, NaN / infinite inputs give NaN / infinite prices.
 */
#define HH_CRR_MAX_STEPS 32768         /* most steps per tree                                        */
#define HH_CRR_FORM_A_MAX_STEPS 2047   /* up to here one wave prices a tree, beyond it a workgroup     */
enum hh_crr_style { HH_CRR_EUROPEAN = 0, HH_CRR_AMERICAN_FORWARD = 1, HH_CRR_AMERICAN_SPOT = 2 };
int hh_crr_solve(hh_ctx* ctx, int32_t steps, uint32_t n_trees, const double* forwards, const double* strikes,
                 const double* cps, const double* ups, const double* discounts, const int32_t* styles,
                 const double* spot_factors, uint32_t n_spot_rows, const uint32_t* spot_row_of_tree,
                 double* prices_out);

/*
 * Crank–Nicolson finite differences — the Black–Scholes equation in x = ln S on a uniform grid, for a European or
 * American VanillaOption on BlackScholesInputs, and a basket of them in ONE launch, one grid per option, all with the
 * same (space_steps M, time_steps N, rannacher_steps R).  The reference has no such method (its roadmap names it).
 * Per option k:
 *   spots[k], strikes[k], cps[k] (+1 call / -1 put)
 *   sigmas[k]      = get_vol(sigma, expiry, strike),  rates[k] = zero_rate(rate, expiry)
 *   expiries[k]    = T = yearfrac(referenceDate, expiry)
 *   half_widths[k] = W, half the grid's width in log-spot (the Python layer: n_std·σ√T + |ln(K/S0)| + |r − σ²/2|·T)
 *   styles[k]      = enum hh_fd_style
 * Grid: h = W / (M/2), x_j = ln S0 + (j − M/2)·h for j = 0 … M (the spot is node M/2), S_j = exp(x_j), payoff
 * g_j = max(cp·(S_j − K), 0).  Operator, a = σ²/2, b = r − σ²/2:  lo = a/h² − b/(2h),  di = −2a/h² − r,
 * up = a/h² + b/(2h).  Backwards from expiry, Δt = T/N: each of the first R steps is two implicit-Euler half steps
 * (k = Δt/2, θ = 1), every other step one Crank–Nicolson step (k = Δt, θ = ½); a step solves
 *   (1 − θk·di)·V_j − θk·lo·V_{j−1} − θk·up·V_{j+1} = V_j + (1 − θ)k·(lo·V_{j−1} + di·V_j + up·V_{j+1}),  j = 1 … M − 1,
 * with the Dirichlet ends at the new τ (τ accumulated by adding k): call V_0 = 0, V_M = S_M − K·e^{−rτ} in both
 * styles; put V_M = 0 and V_0 = K·e^{−rτ} − S_0 (European) or K − S_0 (American).  American exercise is
 * Brennan–Schwartz, a direct solve: a put eliminates the super-diagonal from the top row downwards and substitutes
 * upwards with V_j = max(·, g_j); a call mirrors it; European is the same solve without the max.  Outputs, c = M/2,
 * d1 = (V_{c+1} − V_{c−1})/(2h), d2 = (V_{c+1} − 2V_c + V_{c−1})/h²:  price V_c, delta d1/S0, gamma (d2 − d1)/S0².
 * M even, 4 <= M <= HH_FD_MAX_SPACE; 1 <= N <= HH_FD_MAX_TIME; 0 <= R <= N; 1 .. 2^20 options per call.
 * prices_out[n_options]; deltas_out and gammas_out may be NULL.  Synchronous.  HH_ERR_INVALID — nothing is written —
 * for a NULL required pointer, M / N / R / n_options out of range, an unknown style, or an option whose operator
 * fails `lo > 0 && up > 0` (too coarse a grid for its drift, or a NaN).  Other scalars are not checked: every loop
 * is bounded by M or N.  The kernel form depends on M alone (csrc/hh_fd.hip): an option prices to the same bits
 * alone, in a basket, and at any position in one.
 */
#define HH_FD_MAX_SPACE 4096          /* most space intervals M                                      */
#define HH_FD_MAX_TIME 65536          /* most time steps N                                           */
#define HH_FD_FORM_A_MAX_SPACE 1024   /* up to here one wave prices an option, beyond it four waves  */
enum hh_fd_style { HH_FD_EUROPEAN = 0, HH_FD_AMERICAN = 1 };
int hh_fd_solve(hh_ctx* ctx, int32_t space_steps, int32_t time_steps, int32_t rannacher_steps, uint32_t n_options,
                const double* spots, const double* strikes, const double* cps, const double* sigmas,
                const double* rates, const double* expiries, const double* half_widths, const int32_t* styles,
                double* prices_out, double* deltas_out, double* gammas_out);

/*
 * Longstaff–Schwartz American pricing on the full path grid:
 *   solve(::PricingProblem{VanillaOption{…,American,…}}, ::LSM)
 *                              (src/pricing_methods/least_squares_montecarlo.jl:99-165)
 * cfg: dynamics = HH_LOGNORMAL, strategy = HH_EXACT_LAW (the BlackScholesExact GBM-process paths the
 * reference's LSM is used with, montecarlo.jl:140-159; trajectory i keyed by seeds[i],
 * montecarlo.jl:331; antithetic = flipped σ, :270-284), n_steps, n_paths, antithetic, seeds.
 * step_discount = df(rate, referenceDate + T/nsteps) (:107); degree = LSM.degree (1..8).
 * Optional host outputs (nullable): stop_time / stop_value = the reference's stopping_info
 * ((n_paths·(1+antithetic)) entries), spot_grid = the (n_steps+1) x n_total path matrix in
 * step-major order (the transpose of extract_spot_grid's matrix, :47-85).
 */
typedef struct hh_lsm_result {
  double price, std_error;
  uint64_t n_paths_total;
  uint32_t rows_regressed, rows_skipped; /* time rows with / without an in-the-money path */
  double kernel_ms, total_ms;
  int32_t form;      /* HH_LSM_FORM_PER_DATE / _PERSISTENT: how the backward induction ran */
  int32_t persistent_fallbacks; /* 1: the one-launch form gave up waiting (nothing written) and the
                                   launch-per-date form produced this result instead */
} hh_lsm_result;
size_t hh_lsm_grid_elems(uint64_t n_paths, uint32_t n_steps, int32_t antithetic);
int hh_lsm_solve(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, int32_t degree,
                 double step_discount, hh_lsm_result* out, int32_t* stop_time, double* stop_value,
                 double* spot_grid);
/*
 * The same backward induction on a spot grid the caller already holds in DEVICE memory
 * (grid[(n_steps+1)][n_paths], row k = date k·T/n_steps): the regression / stopping part of
 * least_squares_montecarlo.jl:107-134 alone, for any path source.  Uses model->strike, cp only.
 */
int hh_lsm_solve_grid(hh_ctx* ctx, const hh_model* model, const double* spot_grid_dev,
                      uint64_t n_paths, uint32_t n_steps, int32_t degree, double step_discount,
                      hh_lsm_result* out, int32_t* stop_time, double* stop_value);

/*
 * Euler–Maruyama paths at every date, and LSM on them (opt-in).
 *   simulate_paths(sde_problem(prob, dynamics, EulerMaruyama()), …)   (montecarlo.jl:161-207, 342-375)
 * cfg: dynamics = HH_LOGNORMAL or HH_HESTON, strategy = HH_EULER_MARUYAMA, noise_mode = HH_NOISE_GENERATE,
 * n_partials = 0; em_split and antithetic as for hh_mc_solve.  Seeds: one per trajectory (seeds_len, when set,
 * >= n_paths), trajectory i keyed by seeds[i] (montecarlo.jl:331) and drawn exactly as hh_mc_solve draws it, so
 * row n_steps of the HH_PATH_SPOT grid is hh_mc_solve's terminal output bit for bit.  Antithetic: the mirrored
 * path (-dW) of trajectory i in column n_paths + i.  path_offset is not read — as in every Euler solve, trajectory i
 * takes seeds[i] whatever the offset; a shard passes its own slice of the seeds.
 *
 * Path state.  The state of these problems is [log S, V] (LogGBMProblem, LogHestonProblem); the reference's
 * extract_spot_grid takes its first component (least_squares_montecarlo.jl:47-85), so as run the reference
 * regresses on log S and applies the payoff to log S.  The caller names the reading:
 *   HH_PATH_SPOT  rows exp(log S) — this library's reading, as for the Broadie–Kaya paths (hh_lsm_solve)
 *   HH_PATH_LOG   rows log S — handed to the regression and to the payoff as they are: the reference as run
 * hh_lsm_solve keeps refusing Euler configurations (HH_ERR_UNSUPPORTED): only these entry points reach them.
 *
 * hh_euler_grid: spot_grid (rows in the path state) and var_grid (Heston only: V0 in row 0, then the variance
 * state after each step) are nullable, hh_lsm_grid_elems(n_paths, n_steps, antithetic) doubles each, step-major;
 * host memory, or device memory when grids_on_device.  out (nullable): n_paths_done, kernel_ms, total_ms.
 * hh_lsm_solve_euler: the grid in device memory, then the backward induction of hh_lsm_solve_grid on it (the
 * same forms, fall-backs and HH_OPT_LSM_FORM); the outputs as for hh_lsm_solve.
 * REPLAY noise, dual partials, other strategies and var_grid on lognormal dynamics: HH_ERR_UNSUPPORTED.
 * Not provided: a sharded / multi-GPU Euler LSM (no hh_lsm_shard_begin counterpart).
 */
enum hh_path_state { HH_PATH_SPOT = 0, HH_PATH_LOG = 1 };
int hh_euler_grid(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, int32_t path_state,
                  double* spot_grid, double* var_grid, int32_t grids_on_device, hh_result* out);
int hh_lsm_solve_euler(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, int32_t path_state,
                       int32_t degree, double step_discount, hh_lsm_result* out, int32_t* stop_time,
                       double* stop_value, double* spot_grid);

/*
 * Path-dependent payoffs on Euler–Maruyama paths: arithmetic / geometric Asian, discretely monitored barrier,
 * cash-or-nothing / asset-or-nothing digital.  The reference has none of them (its roadmap lists them as "Structured
 * Payoffs"); the conventions below are this library's.
 *
 * A solve is two kernels.  The first simulates the trajectories hh_euler_grid and hh_mc_solve simulate — the same
 * draws, correlation and step, every state bit for bit — and keeps HH_PATH_STATS numbers of each instead of a grid
 * (enum hh_path_stat), over the MONITORING DATES: the steps m, 2m, …, n_steps with m = monitor_every, which must
 * divide n_steps, and step 0 (S0, log S0) as well when include_start:
 *   HH_STAT_SUM_S  Σ S          HH_STAT_SUM_X  Σ log S          (the first date's term, then one rounded addition
 *   HH_STAT_MAX_S  max S        HH_STAT_MIN_S  min S             per later date, in date order)
 *   HH_STAT_S_T    S at step n_steps — hh_mc_solve's terminal sample
 * with S = exp(log S) as hh_euler_grid's HH_PATH_SPOT rows hold it.  stats[stat][column], HH_PATH_STATS x n_total
 * doubles, n_total = n_paths·(1 + antithetic): column i is trajectory i, column n_paths + i its mirror (-dW).
 * The second kernel evaluates every payoff of the call on those numbers.  With n_mon the number of monitoring dates
 * and van = max(cp·(S_T − strike), 0):
 *   HH_PAYOFF_VANILLA        van
 *   HH_PAYOFF_ASIAN_ARITH    max(cp·(SUM_S / n_mon − strike), 0)
 *   HH_PAYOFF_ASIAN_GEOM     max(cp·(exp(SUM_X / n_mon) − strike), 0)
 *   HH_PAYOFF_BARRIER        hit = MAX_S >= barrier (up) or MIN_S <= barrier (down), a touch counts;
 *                            knock-out: hit ? rebate : van;   knock-in: hit ? van : rebate;   the rebate is paid at expiry
 *   HH_PAYOFF_DIGITAL_CASH   cp·(S_T − strike) > 0 ? cash : 0
 *   HH_PAYOFF_DIGITAL_ASSET  cp·(S_T − strike) > 0 ? S_T : 0
 * Antithetic: a payoff's sample is the pair average (p + p̃)/2 (montecarlo.jl:431).  A payoff's sums do not depend
 * on what else is in the call: result k is that of a call with payoff k alone, bit for bit.
 *
 * cfg: strategy = HH_EULER_MARUYAMA, dynamics = HH_LOGNORMAL or HH_HESTON, noise_mode = HH_NOISE_GENERATE,
 * n_partials = 0; antithetic, em_split and the seeds (host, device, hh_seeds_cache) as for hh_euler_grid.
 * model->strike and model->cp are not read; model->discount multiplies every mean.
 *   hh_mc_path_stats  stats: host memory, or device memory when stats_on_device.  out (nullable): n_paths_done,
 *                     kernel_ms, total_ms.
 *   hh_mc_solve_path  out[k]: price, std_error, the sums, n_paths_done and the call's times of payoff k (dprice zero);
 *                     path_values (nullable, host): row k = payoff k's sample on each of the n_total members, before
 *                     the pair average; stats (nullable, host): as above.
 * Synchronous.  hh_ctx_enable_timing: two slots per hh_mc_solve_path — the statistics kernel, then the payoff kernel
 * with its record reduction — and one per hh_mc_path_stats.
 * HH_ERR_UNSUPPORTED: REPLAY noise, dual partials, every other strategy.  HH_ERR_INVALID: monitor_every = 0 or not a
 * divisor of n_steps, n_payoffs = 0 or above HH_MAX_PATH_PAYOFFS, an unknown kind or barrier type, a strike, rebate
 * or cash that is not finite (a barrier may be ±inf: never / always hit), cp other than ±1, NULL arguments.
 * Not provided: an accumulate (asynchronous) form and a multi-GPU form, REPLAY noise, dual partials (bump the inputs
 * instead: the solves of a finite difference share their seeds), a Julia binding.
 *
 * CONTINUOUS MONITORING AND LOOKBACKS: hh_mc_path_stats_ex, hh_mc_solve_path_ex.  The two calls above with one more
 * argument, `extremes` (enum hh_path_extremes), which says what MAX and MIN of a trajectory are:
 *   HH_EXTREMES_MONITORED  HH_STAT_MAX_S / HH_STAT_MIN_S: the spot on the monitoring dates, as above.  The same
 *                          kernels, five rows: for kinds 0 .. 5 the call IS hh_mc_solve_path, bit for bit.
 *   HH_EXTREMES_BRIDGE     HH_STAT_CMAX_S / HH_STAT_CMIN_S: the maximum and minimum over [0, T] of the scheme's own
 *                          continuous interpolation.  The statistics are HH_PATH_STATS_BRIDGE = 7 rows of n_total: the
 *                          five above, bit for bit, then these two.
 * Both modes admit two more kinds, which read MAX / MIN of the mode as HH_PAYOFF_BARRIER does (a touch counts):
 *   HH_PAYOFF_LOOKBACK_FLOAT  call: S_T − MIN;                   put: MAX − S_T;               strike is not read
 *   HH_PAYOFF_LOOKBACK_FIXED  call: max(MAX − strike, 0);        put: max(strike − MIN, 0)
 * Kinds 0 .. 2, 4 and 5 read neither: under HH_EXTREMES_BRIDGE they are what they are under HH_EXTREMES_MONITORED.
 * The bridge.  An Euler–Maruyama step k takes log S from x_k to x_{k+1} with a diffusion coefficient g_k that is frozen
 * over the step — sigma (lognormal); sqrt of the clipped variance at the drift-updated state (Heston, em_split) or at
 * the step's initial state (em_split = 0) — so between the two states the scheme's interpolation is a Brownian bridge
 * of variance q = g_k²·dt, and the maximum and the minimum of a bridge have closed-form laws that one uniform each
 * inverts.  With Δ = x_{k+1} − x_k and L_i = −2 ln U_i:
 *   M_k = ½·(x_k + x_{k+1} + sqrt(Δ² + q·L_1))          m_k = ½·(x_k + x_{k+1} − sqrt(Δ² + q·L_2))
 * U_1, U_2: one more Philox4x32-10 block per step under the trajectory's seed as key, counter (k, 0, 0, 3) — the 3 is a
 * domain of its own, no Euler increment shares a block with it — U_1 from output words 0, 1 and U_2 from words 2, 3,
 * each ((w >> 12) + ½)·2⁻⁵² of the 64-bit word w = (hi << 32) | lo.  The mirror (−dW) of an antithetic pair has the
 * negated bridge: its maximum takes L_2 and its minimum L_1, on its own states and its own g̃_k; nothing more is drawn.
 * The running extremes start at log S0 — time 0 always counts, whatever include_start says about the sums — and take
 * cmax = max(cmax, M_k, x_{k+1}), cmin = min(cmin, m_k, x_{k+1}) at EVERY step: monitor_every governs the sums and the
 * discrete rows only.  HH_STAT_CMAX_S = exp(cmax), HH_STAT_CMIN_S = exp(cmin).  g_k = 0 (a clipped variance) gives the
 * larger / smaller endpoint.  Under lognormal dynamics the extremes are exact in law (the step is); under Heston they
 * are exact for the scheme's interpolation, not for the model.
 * Each extreme has its exact marginal law, but U_1 and U_2 are independent: the JOINT law of a step's maximum and
 * minimum is not reproduced, so nothing that needs both at once — a double barrier — is offered.
 * Arguments, outputs, errors (with these functions' names in the texts) and timing slots are those of the pair above;
 * an unknown `extremes` is HH_ERR_INVALID, an unknown kind is one outside 0 .. 7.  stats: 5 or 7 rows by the mode.
 * No Julia binding, as for the pair above.
 */
enum hh_path_payoff_kind { HH_PAYOFF_VANILLA = 0, HH_PAYOFF_ASIAN_ARITH = 1, HH_PAYOFF_ASIAN_GEOM = 2,
                           HH_PAYOFF_BARRIER = 3, HH_PAYOFF_DIGITAL_CASH = 4, HH_PAYOFF_DIGITAL_ASSET = 5,
                           HH_PAYOFF_LOOKBACK_FLOAT = 6, HH_PAYOFF_LOOKBACK_FIXED = 7 /* the _ex entry points only */ };
enum hh_barrier_type { HH_BARRIER_UP_OUT = 0, HH_BARRIER_UP_IN = 1, HH_BARRIER_DOWN_OUT = 2, HH_BARRIER_DOWN_IN = 3 };
enum hh_path_stat { HH_STAT_SUM_S = 0, HH_STAT_SUM_X = 1, HH_STAT_MAX_S = 2, HH_STAT_MIN_S = 3, HH_STAT_S_T = 4,
                    HH_STAT_CMAX_S = 5, HH_STAT_CMIN_S = 6 /* HH_EXTREMES_BRIDGE only */ };
enum hh_path_extremes { HH_EXTREMES_MONITORED = 0, HH_EXTREMES_BRIDGE = 1 };
#define HH_PATH_STATS 5
#define HH_PATH_STATS_BRIDGE 7 /* the five, then HH_STAT_CMAX_S = 5, HH_STAT_CMIN_S = 6 */
#define HH_MAX_PATH_PAYOFFS 1024
typedef struct hh_path_payoff {
  int32_t kind, barrier_type;  /* enum hh_path_payoff_kind; enum hh_barrier_type (HH_PAYOFF_BARRIER only) */
  double strike, cp, barrier, rebate, cash;
} hh_path_payoff;
int hh_mc_path_stats(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, uint32_t monitor_every,
                     int32_t include_start, double* stats, int32_t stats_on_device, hh_result* out);
int hh_mc_solve_path(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, uint32_t monitor_every,
                     int32_t include_start, const hh_path_payoff* payoffs, uint32_t n_payoffs, hh_result* out,
                     double* path_values, double* stats);
int hh_mc_path_stats_ex(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, uint32_t monitor_every,
                        int32_t include_start, int32_t extremes, double* stats, int32_t stats_on_device,
                        hh_result* out);
int hh_mc_solve_path_ex(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, uint32_t monitor_every,
                        int32_t include_start, int32_t extremes, const hh_path_payoff* payoffs, uint32_t n_payoffs,
                        hh_result* out, double* path_values, double* stats);

/*
 * Pathwise derivatives of path-dependent payoffs: hh_mc_path_stats_tangent, hh_mc_solve_path_tangent.  The forward-mode
 * (pathwise) derivative of every LIPSCHITZ payoff of the calls above — vanilla, both Asians, both lookbacks, on the
 * monitored extremes — along up to HH_MAX_PARTIALS directions, out of ONE simulation pass: the trajectories, dates and
 * statistics of hh_mc_path_stats, and beside every statistic its tangent.
 *
 * cfg as for hh_mc_path_stats, but n_partials = 1 .. HH_MAX_PARTIALS; the directions are hh_model's d* seed arrays, as
 * for hh_mc_solve.  Of the parameters only those that reach the diffusion are carried per trajectory, with a unit seed
 * each: V0, kappa, theta, sigma under Heston, sigma alone under lognormal dynamics, and of these the ones some direction
 * has a non-zero seed on — the n_active BASIS slots, in that order (hh_mc_path_stats_tangent reports them in basis_out
 * as enum hh_tangent_basis).  Spot, drift rate, strike and discount are finished in closed form and cost nothing per step.
 *
 * Rows.  rows[row][column], hh_path_tangent_rows(n_active) = 5 + 3 + 5·n_active rows of n_total doubles, columns as above:
 *   0 .. 4                            the HH_PATH_STATS statistics, hh_mc_path_stats' bit for bit
 *   HH_TANGENT_K_MAX, HH_TANGENT_K_MIN  the step index, as a double, of the date that holds MAX_S / MIN_S (0 = the start)
 *   HH_TANGENT_SUM_KS                 Σ_dates k_j·S_j, k_j the step index of date j
 *   8 + 5·b + (enum hh_path_tangent_row), for carried slot b, with dx_j = ∂ log S_j / ∂ (parameter of slot b):
 *     HH_TANGENT_DSUM_S  Σ S_j·dx_j      HH_TANGENT_DSUM_X  Σ dx_j      HH_TANGENT_DS_T  S_T·dx_T
 *     HH_TANGENT_DMAX_S, HH_TANGENT_DMIN_S   S·dx of the date that holds the extreme
 * TIE RULE: the tangent and the index of an extreme follow its value — they are replaced exactly when a date's S is
 * STRICTLY greater (less) than the running extreme, so of equal values the FIRST date holds the extreme.  The start's
 * basis tangents are zero.  n_active = 0 (seeds on spot, rate, strike, discount only): the eight rows alone.
 *
 * hh_mc_solve_path_tangent evaluates the payoffs on the five value rows exactly as hh_mc_solve_path(_ex) does — price,
 * std_error and both sums are that call's bit for bit — and their almost-everywhere derivatives.  The tangent of a
 * statistic in direction k is Σ_b seed_k(slot b)·(its row of slot b) plus the passive part from
 * dx_j = dS0_k/S0 + dr_k·(k_j·dt):   dSUM_S += xd0·SUM_S + dr·dt·SUM_KS;   dSUM_X += n_mon·xd0 + dr·dt·Σk_j;
 * dMAX_S += MAX_S·(xd0 + dr·dt·K_MAX), likewise the minimum;   dS_T += S_T·(xd0 + dr·dt·n_steps).  Payoff rules
 * (dK = model->dstrike[k], the strike seed of EVERY payoff of the call; itm = the payoff is > 0):
 *   HH_PAYOFF_VANILLA         1[itm]·cp·(dS_T − dK)
 *   HH_PAYOFF_ASIAN_ARITH     1[itm]·cp·(dSUM_S / n_mon − dK)
 *   HH_PAYOFF_ASIAN_GEOM      1[itm]·cp·(G·dSUM_X / n_mon − dK),  G = exp(SUM_X / n_mon)
 *   HH_PAYOFF_LOOKBACK_FLOAT  call: dS_T − dMIN_S;               put: dMAX_S − dS_T
 *   HH_PAYOFF_LOOKBACK_FIXED  call: 1[itm]·(dMAX_S − dK);        put: 1[itm]·(dK − dMIN_S)
 * Antithetic: the pair average.  out[k].dprice[j] = discount·mean(∂payoff_j) + ddiscount_j·mean(payoff).
 *   hh_mc_path_stats_tangent  rows: host memory, or device memory when rows_on_device, sized for the call's n_active
 *                             (4 is always enough); basis_out (nullable): 4 int32, the carried parameters, −1 beyond
 *                             n_active; out (nullable): n_paths_done, kernel_ms, total_ms.
 *   hh_mc_solve_path_tangent  out[k] as hh_mc_solve_path's with dprice filled; rows (nullable, host): as above.
 * Synchronous, one device.  hh_ctx_enable_timing: the tangent kernel, then the payoff kernel with its record reduction.
 * HH_ERR_UNSUPPORTED: HH_PAYOFF_BARRIER, HH_PAYOFF_DIGITAL_CASH, HH_PAYOFF_DIGITAL_ASSET (the pathwise derivative of a
 * discontinuous payoff omits the jump term: use a finite difference); REPLAY noise; every dynamics/strategy other than
 * lognormal or Heston by HH_EULER_MARUYAMA.  HH_ERR_INVALID: n_partials = 0 or above HH_MAX_PARTIALS, NULL arguments, and
 * everything hh_mc_solve_path rejects.  Not provided: the bridge extremes, the other path families, multilevel, LSM,
 * multi-GPU, REPLAY / Sobol' noise, second order; rho has no seed in hh_model.
 */
enum hh_tangent_date_row { HH_TANGENT_K_MAX = 5, HH_TANGENT_K_MIN = 6, HH_TANGENT_SUM_KS = 7 };
enum hh_path_tangent_row { HH_TANGENT_DSUM_S = 0, HH_TANGENT_DSUM_X = 1, HH_TANGENT_DMAX_S = 2, HH_TANGENT_DMIN_S = 3,
                           HH_TANGENT_DS_T = 4 };
enum hh_tangent_basis { HH_BASIS_V0 = 0, HH_BASIS_KAPPA = 1, HH_BASIS_THETA = 2, HH_BASIS_SIGMA = 3 };
#define HH_TANGENT_DATE_ROWS 3
#define HH_TANGENT_ROWS_PER_SLOT 5
#define HH_TANGENT_MAX_BASIS 4
size_t hh_path_tangent_rows(uint32_t n_active);
int hh_mc_path_stats_tangent(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, uint32_t monitor_every,
                             int32_t include_start, double* rows, int32_t rows_on_device, int32_t* basis_out,
                             hh_result* out);
int hh_mc_solve_path_tangent(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, uint32_t monitor_every,
                             int32_t include_start, const hh_path_payoff* payoffs, uint32_t n_payoffs, hh_result* out,
                             double* rows);

/*
 * Multilevel Monte Carlo (Giles 2008): one level's correction E[P_fine − P_coarse], sampled on a fine and a coarse
 * Euler–Maruyama trajectory driven by the same Brownian increments.  The reference has no multilevel method; the
 * conventions below are this library's.  The host method (MultilevelMonteCarlo) chooses levels and trajectory counts;
 * these two entry points are one level.
 *
 * cfg->n_steps is the FINE step count, even.  Trajectory i takes seeds[i] and carries two states in one lane:
 *   fine    n_steps steps of dt = T/n_steps, drawn, stepped and monitored exactly as hh_mc_path_stats' trajectory i:
 *           per coarse step j, Heston takes the Philox pairs of steps 2j and 2j + 1 (correlated as there), lognormal
 *           dynamics the one block of pair j (sqrt(dt)·z1, then sqrt(dt)·z2);
 *   coarse  n_steps/2 steps of 2·dt on the increment dW_c = dW_a + dW_b of that fine pair — one rounded fp64 addition
 *           per component, for Heston on the already correlated components — with the step constants a plain solve on
 *           n_steps/2 steps forms (its dt is T/(n_steps/2), not 2·(T/n_steps)).
 * monitor_every counts FINE steps and is even: the coarse leg monitors every monitor_every/2 of its steps, so both see
 * the same dates; include_start is the same on both.  The statistics are HH_PATH_STATS rows (monitored extremes only) in
 * the ANTITHETIC layout, n_total = 2·n_paths: column i is the fine trajectory, column n_paths + i its coarse partner.
 *   hh_mc_path_stats_coupled  arguments and outputs of hh_mc_path_stats on that layout.
 *   hh_mc_solve_path_coupled  per trajectory and payoff k (kinds 0 .. 7; the lookbacks read the monitored extremes)
 *                             p_f on the fine rows, p_c on the coarse rows, Y = p_f − p_c (one rounded subtraction).
 *                             out_diff[k]: price = discount·mean Y, std_error, sum_payoff = Σ Y, sumsq_payoff = Σ Y²,
 *                             n_paths_done and the call's times; out_fine[k] (nullable array): the same on p_f.
 *                             path_values (nullable, host): row k = p_f on columns [0, n_paths), p_c on [n_paths,
 *                             2·n_paths); stats (nullable, host): as above.
 * Two identities hold bit for bit:
 *   1. Columns [0, n_paths) of the statistics are hh_mc_path_stats' on the same seeds and n_steps, and out_fine[k] is
 *      result k of hh_mc_solve_path_ex (HH_EXTREMES_MONITORED) — price, std_error and both sums.
 *   2. Columns [n_paths, 2·n_paths) are the statistics of a REPLAY solve on n_steps/2 steps whose increments are the
 *      pairwise sums of hh_wiener_fill's for the fine grid (HH_STAT_SUM_X up to the rounding of log(exp(x))).
 * A payoff's sums do not depend on what else is in the call.  Under lognormal dynamics the log-Euler step is exact in
 * law, so the two legs' S_T differ by rounding alone and every correction is noise: multilevel is for Heston.
 * Synchronous.  hh_ctx_enable_timing: the statistics kernel, then the payoff kernel with its record reduction; one slot
 * for hh_mc_path_stats_coupled.
 * HH_ERR_INVALID: n_steps odd; monitor_every odd, 0 or not a divisor of n_steps; everything hh_mc_solve_path_ex
 * rejects.  HH_ERR_UNSUPPORTED: antithetic, REPLAY noise, dual partials, a strategy other than HH_EULER_MARUYAMA,
 * dynamics other than HH_LOGNORMAL and HH_HESTON.
 * Not provided: local volatility (its per-step table would be staged for two grids), Merton, QE, Bates and multi-asset
 * paths, antithetic pairs, the bridge extremes (the two levels' bridges would have to be coupled), refinement factors
 * other than 2, an accumulate (asynchronous) form, a multi-GPU form, a Julia binding.
 */
int hh_mc_path_stats_coupled(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, uint32_t monitor_every,
                             int32_t include_start, double* stats, int32_t stats_on_device, hh_result* out);
int hh_mc_solve_path_coupled(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, uint32_t monitor_every,
                             int32_t include_start, const hh_path_payoff* payoffs, uint32_t n_payoffs,
                             hh_result* out_diff, hh_result* out_fine, double* path_values, double* stats);

/*
 * Merton (1976) jump diffusion: lognormal dynamics plus a compound Poisson sum of normal jumps in log S, the drift
 * compensated so that e^{-rt}·S stays a martingale.  The reference has no jump model (its roadmap lists "Merton model
 * with Carr–Madan, Merton model with Monte Carlo" as open); the conventions below are this library's.
 *   d log S = (r − σ²/2 − λ·κ̄) dt + σ dW + J dN        J ~ N(μ_J, σ_J²),  N Poisson of intensity λ
 *   κ̄ = exp(μ_J + σ_J²/2) − 1
 * Over a span τ, given n jumps in it, the jump sum is N(n·μ_J, n·σ_J²): one normal serves the whole sum.
 *   ϕ(u) = E exp(iu·log S_T) = exp( iu·(log S0 + (r − σ²/2 − λκ̄)T) − σ²u²T/2 + λT·(exp(iu·μ_J − σ_J²u²/2) − 1) )
 *   call = Σ_n e^{−λT}(λT)ⁿ/n! · (discounted Black call on a lognormal with log-mean log S0 + (r − σ²/2 − λκ̄)T + n·μ_J
 *                                   and log-variance σ²T + n·σ_J²)
 * hh_jump carries λ, μ_J, σ_J; σ = model->sigma, r = model->r_drift.  No existing struct changes.
 *
 * THE JUMP COUNT of a span with Poisson mean m (λ·T, or λ·T/n_steps) from one uniform U, by inversion
 * (csrc/hh_jump.h, poisson_inverse — a host program can call it): with p_0 = exp(−m), formed on the host once per
 * call, c_0 = p_0, p_k = p_{k−1}·m/k and c_k = c_{k−1} + p_k — one rounded fp64 operation each, in this order — N is
 * the smallest n with U <= c_n, and the search stops at n = HH_JUMP_MAX_COUNT whatever U is: in fp64 the cumulative sum
 * can saturate below the largest U = 1 − 2⁻⁵³ (m = 2.5 saturates at 1 − 2⁻⁵²), where a search without the cap would never end.
 * m = 0 gives N = 0 for every U.  U = ((w >> 12) + ½)·2⁻⁵² of a 64-bit word w = (hi << 32) | lo, as everywhere.
 * Every draw is a Philox4x32-10 block whose counter word 3 is 4, a domain no other draw of the library uses.
 *
 * hh_mc_solve_jump — the TERMINAL LAW, cfg->strategy = HH_EXACT_LAW.  Trajectory i of the call has the global index
 * g = cfg->path_offset + i and is keyed by seeds[0], as the exact lognormal law is.
 *   block A  counter (lo32 g, hi32 g, 0, 4): z1, z2 by Box–Muller, as every normal pair of the library
 *   block B  counter (lo32 g, hi32 g, 1, 4): U from output words 0, 1;  N from U with m = λ·T
 *   x_T = fma(σ√T, z1, m_T) + J        m_T = log S0 + ((r − σ²/2) − λκ̄)·T, formed on the host — ·T as it stands: there
 *   J   = fma(σ_J·sqrt((double)N), z2, N·μ_J), added only when N > 0           is no compat_sqrt_alpha reading of it
 * Antithetic: the mirror takes −z1, −z2 and the same N.  terminal (nullable; host, or device when
 * cfg->terminal_on_device): exp(x_T) of the n_paths trajectories, then of their mirrors.  The payoff (model->strike,
 * model->cp), the sums and hh_result are hh_mc_solve's.  1 .. 2^32 − 256 trajectories per call; a lane takes eight of
 * them whatever the call, so a call's sums are reproducible, and [0, n) is [0, k) followed by [k, n) with
 * path_offset = k, sample for sample.  Timing: one slot, as hh_mc_solve.
 *
 * hh_mc_solve_path_jump — the PATH FORM, cfg->strategy = HH_EULER_MARUYAMA: hh_mc_solve_path_ex under
 * HH_EXTREMES_MONITORED with jumps.  Trajectory i is keyed by seeds[i]; its diffusion increments are exactly those of
 * hh_mc_solve_path under lognormal dynamics, and so is the step, with the drift
 * gdrift = (r − σ²/2) − λκ̄ formed on the host in that order: λ = 0 gives hh_mc_solve_path's bits.
 *   block (h, 0, 0, 4) serves steps 2h and 2h+1: U of step 2h from output words 0, 1, U of step 2h+1 from words 2, 3;
 *                      N_k from U with m = λ·dt, dt = T/n_steps
 *   block (k, 1, 0, 4) is drawn only by a trajectory whose N_k > 0: z = the first normal of its pair
 *   after step k:      x ← x + fma(σ_J·sqrt((double)N_k), z, N_k·μ_J), applied only when N_k > 0
 * The mirror takes −dW, the same N_k and −z.  The statistics are the five rows of HH_EXTREMES_MONITORED over the same
 * monitoring dates with the same arithmetic; payoff kinds 0 .. 7 are admitted, the lookbacks read the monitored rows.
 * The log-Euler step is exact for this model, so the states on the dates are exact in law for any n_steps.
 * Arguments, outputs and timing slots are hh_mc_solve_path's.
 *
 * hh_carr_madan_jump — hh_carr_madan_basket (lognormal dynamics, compat_sqrt_alpha = 0) with ϕ above: the same fixed
 * quadrature rule, one workgroup per payoff, the same parity transform for puts.  λ = 0 is hh_carr_madan_basket.
 *
 * All three are synchronous.  Errors, checked on the host before any launch.  HH_ERR_INVALID: jump is NULL; λ or σ_J
 * negative or not finite; μ_J not finite; exp(μ_J + σ_J²/2) not finite; the Poisson mean of one draw — λ·T (terminal
 * law), λ·T/n_steps (path form) — above HH_JUMP_MAX_MEAN; everything hh_mc_solve / hh_mc_solve_path_ex /
 * hh_carr_madan_basket reject.  HH_ERR_UNSUPPORTED: dynamics other than HH_LOGNORMAL, REPLAY noise, n_partials > 0,
 * hh_mc_solve_jump with a strategy other than HH_EXACT_LAW, hh_mc_solve_path_jump with one other than
 * HH_EULER_MARUYAMA.
 * Not provided: multi-GPU and accumulate (asynchronous) forms, the hh_mc_solve_multi form, dual partials (bump the
 * inputs: the solves of a finite difference share their seeds), a gradient of hh_carr_madan_jump, a Julia binding, and
 * continuous (Brownian-bridge) extremes — a bridge between two states is wrong once a jump lies between them.
 */
#define HH_JUMP_MAX_MEAN  64.0   /* largest Poisson mean of one draw: λ·T (terminal law), λ·T/n_steps (path form) */
#define HH_JUMP_MAX_COUNT 255    /* the inversion's search stops here at the latest */
typedef struct hh_jump { double lambda, mu_j, sigma_j; } hh_jump;        /* 24 bytes */
int hh_mc_solve_jump(hh_ctx* ctx, const hh_model* model, const hh_jump* jump, const hh_config* cfg, hh_result* out,
                     double* terminal);
int hh_mc_solve_path_jump(hh_ctx* ctx, const hh_model* model, const hh_jump* jump, const hh_config* cfg,
                          uint32_t monitor_every, int32_t include_start, const hh_path_payoff* payoffs,
                          uint32_t n_payoffs, hh_result* out, double* path_values, double* stats);
int hh_carr_madan_jump(hh_ctx* ctx, const hh_model* model, const hh_jump* jump, double alpha, double bound,
                       const double* strikes, const double* cps, const double* Ts, const double* r_drifts,
                       const double* discounts, uint32_t n_payoffs, double* prices_out);

/*
 * Heston paths by the quadratic-exponential scheme (Andersen 2008, "Simple and efficient simulation of the Heston
 * stochastic volatility model", the QE scheme with central weights γ1 = γ2 = ½).  The Euler step with a clipped
 * variance is badly biased where 2κθ < σ²; this step matches the conditional mean and variance of the variance process
 * exactly and costs about what an Euler step costs.  The reference has no such scheme; the conventions are this
 * library's.  cfg->strategy = HH_QE, cfg->dynamics = HH_HESTON; hh_qe carries ψ_c and the martingale switch.
 *
 * ON THE HOST, once per call, each a single rounded fp64 operation in this order (csrc/hh_qe.h, qe_args), with
 * κ, θ, σ, ρ of the model, r = model->r_drift and dt = T/n_steps:
 *   E   = exp(−(κ·dt))             ome = 1 − E              s2 = σ·σ
 *   c1  = ((s2·E)·ome)/κ           c2  = ((θ·s2)·(ome·ome))/(2·κ)           th_ome = θ·ome        rdt = r·dt
 *   K0  = −((((ρ·κ)·θ)·dt)/σ)      h   = (½·dt)·((κ·ρ)/σ − ½)
 *   K1  = h − ρ/σ                  K2  = h + ρ/σ            K3 = K4 = (½·dt)·(1 − ρ·ρ)
 *   A   = K2 + ½·K4                k13 = K1 + ½·K3          ψ_c = qe->psi_c, 1.5 when that is 0
 * They travel by value beside the model block (QeArgs); no existing struct changes.
 *
 * ONE STEP k takes (x, v) = (log S, variance) to (x′, v′), operation by operation (csrc/hh_qe.h):
 *   m  = th_ome + v·E              s² = v·c1 + c2           ψ = s²/(m·m)
 *   quadratic branch, ψ <= ψ_c:    t = 2/ψ     b² = (t − 1) + sqrt(t)·sqrt(t − 1)      a = m/(1 + b²)
 *                                  v′ = a·((sqrt(b²) + Z_v)·(sqrt(b²) + Z_v))
 *   exponential branch, otherwise: p = (ψ − 1)/(ψ + 1)     q = 1 − p     β = q/m
 *                                  v′ = 0 if U <= p, else log(q/(1 − U))/β
 *   x′ = (x + (((rdt + K0) + K1·v) + K2·v′)) + sqrt(K3·v + K4·v′)·Z_x
 * MARTINGALE CORRECTION (qe->martingale != 0): K0 is replaced, per step and member, by K0* = −ln M − k13·v with
 *   quadratic branch:    d = 1 − (2·A)·a       ln M = ((A·b²)·a)/d − ½·log(d)
 *   exponential branch:  ln M = log(p + (β·q)/(β − A))
 * so that E[exp(x′ − rdt) | x, v] = exp(x) exactly.  It is admitted only when A <= 0 — every ρ <= 0 gives that — where
 * d >= 1 and β − A >= β > 0 in every state; A > 0 with the correction requested is HH_ERR_UNSUPPORTED.
 * Degenerate states: the checks below give th_ome > 0 and c2 > 0, and v >= 0 always (v′ is a square times a > 0, zero,
 * or a logarithm of a number >= 1 over β > 0), so m > 0 and ψ > 0 in every state: no division meets a zero.
 * ψ <= ψ_c <= 2 gives t >= 1, ψ > ψ_c >= 1 gives 0 < p < 1; K3·v + K4·v′ >= 0.  Every device loop is bounded by n_steps.
 *
 * DRAWS: Philox4x32-10 blocks under the trajectory's seed (seeds[i]) as key, counter word 3 = 5, a domain no other draw
 * of the library uses.
 *   block (k, 0, 0, 5)  the Box–Muller pair of step k: (Z_v, Z_x), independent — the correlation lives in the K's
 *   block (k, 1, 0, 5)  U = ((w >> 12) + ½)·2⁻⁵² from output words 0, 1; drawn only by a trajectory that is in the
 *                       exponential branch at step k
 * The mirror of an antithetic pair takes −Z_v, −Z_x and 1 − U (exact: the uniforms are symmetric about ½) on its own
 * states, and reads U when it is itself in the exponential branch.
 *
 * hh_mc_path_stats_qe / hh_mc_solve_path_qe: hh_mc_path_stats / hh_mc_solve_path_ex under HH_EXTREMES_MONITORED with this
 * step in place of the Euler step — the same monitoring dates, the same statistics arithmetic, the same five rows, the
 * same payoff kernel; kinds 0 .. 7 are admitted, the lookbacks read the monitored rows.  var_T (nullable, host):
 * n_total doubles, the variance at expiry of each member, mirrors at n_paths + i.  Synchronous; timing slots as the
 * Euler pair's.  Errors, checked on the host before any launch.  HH_ERR_INVALID: qe is NULL; κ, θ or σ not > 0,
 * V0 < 0, |ρ| > 1, anything not finite; ψ_c outside {0} ∪ [1, 2]; κ·dt so small that 1 − E rounds to 0;
 * σ²/(2κθ) — the maximum of ψ over v >= 0, whatever dt — above HH_QE_MAX_PSI, so that 1 − p = 2/(ψ + 1) and β stay
 * far from rounding to 0; everything
 * hh_mc_solve_path_ex rejects.  HH_ERR_UNSUPPORTED: dynamics other than HH_HESTON, a strategy other than HH_QE, REPLAY
 * noise, n_partials > 0, the correction with A > 0 (run without it).
 * Not provided: bridge extremes (the QE step's interpolation is not a frozen-coefficient bridge), REPLAY noise, dual
 * partials (bump the inputs: the solves share their seeds), accumulate and multi-GPU forms, the hh_mc_solve_multi form,
 * a variance grid (the spot rows and LSM on them: hh_mc_path_grid, hh_lsm_solve_path), weights other than ½, the TG
 * scheme, the correction for A > 0, a Julia binding.
 */
#define HH_QE_MAX_PSI 1e9   /* largest σ²/(2κθ), the maximum of ψ over v >= 0, these entry points admit */
typedef struct hh_qe { double psi_c; int32_t martingale; int32_t reserved; } hh_qe;   /* 16 bytes */
int hh_mc_path_stats_qe(hh_ctx* ctx, const hh_model* model, const hh_qe* qe, const hh_config* cfg,
                        uint32_t monitor_every, int32_t include_start, double* stats, int32_t stats_on_device,
                        double* var_T, hh_result* out);
int hh_mc_solve_path_qe(hh_ctx* ctx, const hh_model* model, const hh_qe* qe, const hh_config* cfg,
                        uint32_t monitor_every, int32_t include_start, const hh_path_payoff* payoffs,
                        uint32_t n_payoffs, hh_result* out, double* path_values, double* stats, double* var_T);

/*
 * Bates (1996): Heston variance with Merton jumps — the model often called SVJ: the stochastic variance of the section
 * above and the compound Poisson jumps of the Merton section in one log spot.
 *   d log S = (r − λκ̄ − v/2) dt + √v dW_S + J dN        J ~ N(μ_J, σ_J²),  N Poisson of intensity λ
 *   dv      = κ(θ − v) dt + σ√v dW_v                     corr(dW_S, dW_v) = ρ
 *   κ̄ = exp(μ_J + σ_J²/2) − 1
 * The jumps are independent of both Brownian motions.  The parameters travel in the existing hh_model, hh_qe and
 * hh_jump, with cfg->dynamics = HH_HESTON and cfg->strategy = HH_QE: no struct changes, no enum gains a value.
 *
 * ON THE HOST, once per call:
 *   lam_kbar = λ·expm1(μ_J + ½σ_J²)       the compensator, the same function the Merton entry points use
 *   r_c      = model->r_drift − lam_kbar
 *   the QE constants of the section above (csrc/hh_qe.h, qe_args) with r_c in place of r: rdt = r_c·dt, dt = T/n_steps,
 *   every other constant as there;  mean = λ·dt and p_0 = exp(−mean) of the jump count (csrc/hh_jump.h, jump_args).
 * λ = 0 gives r_c == r and mean == 0.
 *
 * ONE STEP k, operation by operation:
 *   1. the QE step of the section above on (x, v), on its own draws of domain 5, unchanged: block (k, 0, 0, 5) gives
 *      (Z_v, Z_x), block (k, 1, 0, 5) gives U under the same branch condition;
 *   2. N_k = the jump count (csrc/hh_jump.h, poisson_inverse) of U_J with mean and p_0; U_J from block (k >> 1, 0, 0, 4):
 *      output words 0, 1 for an even k, words 2, 3 for an odd one — one block serves two consecutive steps;
 *   3. only where N_k > 0: z = the first normal of block (k, 1, 0, 4);
 *   4. x ← x + fma(σ_J·sqrt((double)N_k), z, N_k·μ_J), only where N_k > 0 — after the QE step and before the monitoring
 *      date.
 * These are the jump draws of hh_mc_solve_path_jump under the same seed and counters; domains 4 and 5 are disjoint, so
 * the two streams are independent.  The mirror of an antithetic pair takes −Z_v, −Z_x and 1 − U on its own states, the
 * same N_k and −z.  The MARTINGALE CORRECTION is QE's, unchanged: the jumps are compensated through r_c alone, so that
 * with it E[exp(x′ − r·dt) | x, v] = exp(x) exactly (E exp(J·) = exp(λκ̄·dt) exactly, whatever dt).
 * Two identities follow and are tested:
 *   λ = 0 gives hh_mc_solve_path_qe's bits in every output;
 *   a trajectory of these entry points and one of hh_mc_solve_path_jump with the same seed and the same λ·dt have the
 *   same N_k and z at every step.
 * Every device loop is bounded by n_steps, the count search by HH_JUMP_MAX_COUNT.
 *
 * hh_mc_path_stats_bates / hh_mc_solve_path_bates: hh_mc_path_stats_qe / hh_mc_solve_path_qe with `jump` after `qe` —
 * the same dates, the same statistics arithmetic, the same five rows and var_T, payoff kinds 0 .. 7, the same timing
 * slots.  Synchronous.
 *
 * hh_carr_madan_bates — hh_carr_madan_basket under HH_HESTON (compat_sqrt_alpha = 0) with
 *   ϕ_B(u) = ϕ_H(u; r → r_c) · exp(λT·(exp(iu·μ_J − σ_J²u²/2) − 1))
 * Per payoff r_c = r_k − lam_kbar, in that order; the Heston exponent as hh_carr_madan_basket forms it, with r_c in it;
 * (λ·T)·(exp(μ_J·iu − (½σ_J²)·u²) − 1) added to the exponent last.  The same quadrature rule, one workgroup per payoff,
 * the same parity transform for puts.  λ = 0 returns hh_carr_madan_basket's bits (HH_HESTON, compat_sqrt_alpha = 0).
 * Synchronous.
 *
 * Errors, checked on the host before any launch.  HH_ERR_INVALID: qe or jump is NULL; everything the Merton entry points
 * reject in hh_jump, the Poisson mean of one draw being λ·T/n_steps (hh_carr_madan_bates draws nothing: no limit on
 * it); everything the QE entry points reject, the step's constants being formed on r_c; everything hh_mc_solve_path_ex
 * or hh_carr_madan_basket reject.  HH_ERR_UNSUPPORTED: dynamics other than HH_HESTON, a strategy other than HH_QE,
 * REPLAY noise, n_partials > 0, the martingale correction with A > 0.
 * Not provided: a terminal-law form on Broadie–Kaya, bridge extremes, a gradient of hh_carr_madan_bates, a variance grid
 * (the spot rows and LSM on them: hh_mc_path_grid, hh_lsm_solve_path), multi-GPU and accumulate forms, the hh_mc_solve_multi form, dual partials (bump the inputs: the solves share
 * their seeds), a Julia binding.
 */
int hh_mc_path_stats_bates(hh_ctx* ctx, const hh_model* model, const hh_qe* qe, const hh_jump* jump,
                           const hh_config* cfg, uint32_t monitor_every, int32_t include_start, double* stats,
                           int32_t stats_on_device, double* var_T, hh_result* out);
int hh_mc_solve_path_bates(hh_ctx* ctx, const hh_model* model, const hh_qe* qe, const hh_jump* jump,
                           const hh_config* cfg, uint32_t monitor_every, int32_t include_start,
                           const hh_path_payoff* payoffs, uint32_t n_payoffs, hh_result* out, double* path_values,
                           double* stats, double* var_T);
int hh_carr_madan_bates(hh_ctx* ctx, const hh_model* model, const hh_jump* jump, double alpha, double bound,
                        const double* strikes, const double* cps, const double* Ts, const double* r_drifts,
                        const double* discounts, uint32_t n_payoffs, double* prices_out);

/*
 * Several correlated lognormal assets and a scalar INDEX of them: baskets, spreads, geometric baskets, best-of and
 * worst-of (rainbow) options.  The reference prices options on one underlying only; the conventions are this library's.
 *   d log S_i = (r − σ_i²/2) dt + σ_i dW_i          corr(dW_i, dW_j) = C_ij          i, j < d = n_assets <= HH_MAX_ASSETS
 * The statistics kernel keeps the five running numbers of hh_mc_path_stats (enum hh_path_stat) for the index instead
 * of for a spot, so every payoff kind of hh_mc_solve_path_ex prices on the index through the same payoff kernel.  The
 * log-Euler step below is exact in law for this model: the states on the dates are exact for any n_steps.
 * Of hh_model only T, r_drift and discount are read; hh_assets carries the rest.  cfg->dynamics = HH_LOGNORMAL,
 * cfg->strategy = HH_EULER_MARUYAMA.  No existing struct changes, no enum gains a value.
 *
 * ON THE HOST, once per call (csrc/hh_assets.h — a host program can include it), every operation one rounded fp64
 * operation in the order written:
 *   CHOLESKY, Cholesky–Banachiewicz, row by row: for i = 0 .. d−1, for j = 0 .. i:
 *       s = C_ij;  for k = 0 .. j−1 in this order:  s = s − L_ik·L_jk   (a product, then a subtraction)
 *       j < i:  L_ij = s / L_jj          j == i:  L_ii = sqrt(s); s not > 0 or not finite: not positive definite
 *   dt = T/n_steps          sqrt_dt = sqrt(dt)
 *   drift_i = (r_drift − (0.5·σ_i)·σ_i)·dt
 *   A_ij    = (σ_i·L_ij)·sqrt_dt                       j <= i
 *   x0_i    = log(spot_i)                              best-of, worst-of: log(spot_i) + log(w_i)
 * They travel by value in the kernel's argument block.
 *
 * DRAWS: trajectory i is keyed by seeds[i].  At step k (0-based) the asset pair h = 0 .. ⌈d/2⌉−1 takes the Philox4x32-10
 * block of counter (k, h, 0, 6) — word 3 = 6, a domain no other draw of the library uses — whose Box–Muller pair, as every
 * normal pair of the library, is (z_2h, z_2h+1); for odd d the last block's second normal is dropped.
 *
 * ONE STEP, per asset i = 0 .. d−1 in order:
 *   acc = drift_i;   for j = 0 .. i:  acc = fma(A_ij, z_j, acc);   x_i = x_i + acc
 * The mirror of an antithetic pair lives in the same lane and takes −z_j in the same chain; nothing more is drawn.
 *
 * THE INDEX on a monitoring date — the dates are hh_mc_path_stats': steps monitor_every, 2·monitor_every, …, n_steps,
 * and step 0 when include_start — is the pair (I, x) the statistics take as (S, log S):
 *   HH_INDEX_WEIGHTED_SUM   I = w_0·exp(x_0), then I = fma(w_i, exp(x_i), I) in asset order;   x = log(I)
 *   HH_INDEX_GEOMETRIC      x = w_0·x_0, then x = fma(w_i, x_i, x);                            I = exp(x)
 *   HH_INDEX_BEST_OF        x = max_i x_i   (log w_i is in the initial state);                 I = exp(x)
 *   HH_INDEX_WORST_OF       x = min_i x_i                                                      I = exp(x)
 * so the index is Σ w_i S_i, Π S_i^{w_i}, max_i w_i S_i, min_i w_i S_i.  A weighted sum with negative weights (a spread)
 * may be <= 0: its row HH_STAT_SUM_X is then NaN or −inf and no admitted payoff reads it.  The date-0 term comes from the
 * same function on the initial states: with every σ_i = 0 and r_drift = 0 all dates of a trajectory agree bit for bit.
 *
 * hh_mc_path_stats_assets / hh_mc_solve_path_assets: hh_mc_path_stats / hh_mc_solve_path_ex under
 * HH_EXTREMES_MONITORED on the index — the same five rows, the same layout (mirrors at n_paths + i), the same payoff
 * kernel, payoff kinds 0 .. 7, the lookbacks on the monitored rows.  Arguments, outputs and timing slots are
 * hh_mc_solve_path's.  Synchronous.
 *
 * Errors, checked on the host before any launch.  HH_ERR_INVALID: assets is NULL; n_assets outside 1 .. HH_MAX_ASSETS;
 * an unknown index_kind; a spot not finite or not > 0; a sigma not finite or < 0; C_ii != 1; C_ij != C_ji; C_ij not
 * finite or |C_ij| > 1; C not positive definite (above); a weight not finite; all weights zero (weighted sum); a weight
 * <= 0 (best-of, worst-of); HH_PAYOFF_ASIAN_GEOM on a weighted sum with a negative weight; T not > 0, r_drift or
 * discount not finite; everything else hh_mc_solve_path_ex rejects.  HH_ERR_UNSUPPORTED: dynamics other than
 * HH_LOGNORMAL, a strategy other than HH_EULER_MARUYAMA, REPLAY noise, n_partials > 0.
 * Not provided: barriers on single assets, payoffs that read more than one index (one call per index, on the same
 * seeds), dividends and quantos, stochastic volatility per asset, American exercise through these two entry points (it is hh_lsm_solve_assets', further
 * down), continuous (bridge) monitoring,
 * REPLAY noise, dual partials (bump the inputs: the solves share their seeds), accumulate, hh_mc_solve_multi and
 * multi-GPU forms, more than HH_MAX_ASSETS assets, a Julia binding.
 */
#define HH_MAX_ASSETS 8
enum hh_index_kind { HH_INDEX_WEIGHTED_SUM = 0, HH_INDEX_GEOMETRIC = 1, HH_INDEX_BEST_OF = 2, HH_INDEX_WORST_OF = 3 };
typedef struct hh_assets {
  uint32_t n_assets; int32_t index_kind;
  double spots[HH_MAX_ASSETS], sigmas[HH_MAX_ASSETS], weights[HH_MAX_ASSETS];
  double corr[HH_MAX_ASSETS * HH_MAX_ASSETS];   /* corr[i*HH_MAX_ASSETS + j], i, j < n_assets */
} hh_assets;                                    /* 8 + 3·64 + 512 = 712 bytes */
int hh_mc_path_stats_assets(hh_ctx* ctx, const hh_model* model, const hh_assets* assets, const hh_config* cfg,
                            uint32_t monitor_every, int32_t include_start, double* stats, int32_t stats_on_device,
                            hh_result* out);
int hh_mc_solve_path_assets(hh_ctx* ctx, const hh_model* model, const hh_assets* assets, const hh_config* cfg,
                            uint32_t monitor_every, int32_t include_start, const hh_path_payoff* payoffs,
                            uint32_t n_payoffs, hh_result* out, double* path_values, double* stats);

/*
 * Local volatility on a tabulated surface: paths that reprice an observed vanilla surface.
 *   d log S = (r − σ(t, S)²/2) dt + σ(t, S) dW
 * with σ read off a rectangular table in (t, x = log S) — linear interpolation, constant extrapolation, as the
 * reference's RectVolSurface interpolates; how the table is made (Dupire's formula on call prices, say) is the caller's
 * business.  The parameters travel in the existing hh_model and in hh_localvol, with cfg->dynamics = HH_LOGNORMAL and
 * cfg->strategy = HH_EULER_MARUYAMA: model->S0, r_drift, T and the discounting fields are read, model->sigma and the
 * Heston fields are ignored.  No existing struct changes, no enum gains a value.
 *
 * ON THE HOST, once per call (csrc/hh_localvol.h — a host program can include it), every operation one rounded fp64
 * operation in the order written:
 *   dt = T/n_steps          sqrt_dt = sqrt(dt)          inv_h = 1/h
 *   per step k = 0 .. n_steps−1, with t_k = (double)k·dt:
 *     j_k = the largest j with times[j] <= t_k, clamped to [0, max(n_times − 2, 0)]
 *     w_k = (t_k − times[j_k])/(times[j_k+1] − times[j_k]) clamped to [0, 1];  w_k = 0 when n_times == 1
 *   so σ is constant in time before times[0] and after times[n_times−1].  j_k and w_k are the same for every trajectory.
 *
 * DRAWS: the lognormal Euler kernel's own.  Trajectory i is keyed by seeds[i]; the Philox4x32-10 block of counter
 * (h, 0, 0, 0) gives the normals of steps 2h (first) and 2h + 1 (second), dW = sqrt_dt·z; under HH_EXTREMES_BRIDGE the
 * block of counter (k, 0, 0, 3) gives the two bridge draws of step k, as for hh_mc_path_stats_ex.  No other draw.
 *
 * ONE STEP k of a trajectory at log spot x, operation by operation (a = row j_k of vols, b = row j_k + 1):
 *   1. u = (x − x_lo)·inv_h, clamped to [0, n_x − 1]: constant extrapolation in x;
 *   2. i = min((uint32)u, n_x − 2),  f = u − i;
 *   3. c0 = fma(w_k, b_i − a_i, a_i),  c1 = fma(w_k, b_{i+1} − a_{i+1}, a_{i+1})   (time first; n_times == 1: c0 = a_i,
 *      c1 = a_{i+1}, the same bits),  σ = fma(f, c1 − c0, c0)   (then x);
 *   4. g = r_drift − (0.5·σ)·σ;
 *   5. x′ = fma(σ, dW, fma(dt, g, x)): the lognormal Euler step with the σ and g of this step;
 *   6. HH_EXTREMES_BRIDGE: σ is the frozen coefficient of bridge k, q = (σ·σ)·dt, in the extremes of hh_mc_path_stats_ex.
 * The mirror of an antithetic pair takes −dW on its own state and its own σ, and the bridge draws swapped.
 * One identity follows and is tested: a table whose entries all equal σ0 gives hh_mc_path_stats_ex's bits under
 * model->sigma = σ0 in every row, in both extremes forms (fma(·, 0, c) = c exactly).
 * The kernel holds the whole table in LDS (n_times·n_x·8 bytes, hence HH_LV_MAX_NODES); every device loop is bounded by
 * n_steps or the table's size.
 *
 * hh_mc_path_stats_lv / hh_mc_solve_path_lv: hh_mc_path_stats_ex / hh_mc_solve_path_ex with `lv` after `model` — the
 * same dates, the same statistics arithmetic, the five rows (seven under HH_EXTREMES_BRIDGE), payoff kinds 0 .. 7, the
 * same layout (mirrors at n_paths + i) and timing slots.  Synchronous.
 *
 * Errors, checked on the host before any launch.  HH_ERR_INVALID: lv, lv->times or lv->vols is NULL; n_times = 0,
 * n_x < 2 or n_times·n_x > HH_LV_MAX_NODES; a time not finite, negative or not above the one before it; a vol not finite
 * or <= 0; x_lo not finite; h not finite or <= 0; everything hh_mc_solve_path_ex rejects (model->sigma excepted).
 * HH_ERR_UNSUPPORTED: dynamics other than HH_LOGNORMAL, a strategy other than HH_EULER_MARUYAMA, REPLAY noise,
 * n_partials > 0.
 * Not provided: REPLAY noise, dual partials (bump the inputs: the solves share their seeds), accumulate,
 * hh_mc_solve_multi and multi-GPU forms (American exercise: hh_lsm_solve_path), local volatility on the Crank–Nicolson grid, stochastic-local
 * volatility, tables above 64 KiB, non-uniform log-spot grids, a Julia binding.
 */
#define HH_LV_MAX_NODES 8192          /* n_times · n_x doubles = 64 KiB of LDS */
typedef struct hh_localvol {          /* 40 bytes */
  const double* times;   /* host, [n_times], finite, >= 0, strictly increasing */
  const double* vols;    /* host, [n_times][n_x] row-major: sigma at (times[j], x_lo + i*h), each finite and > 0 */
  double x_lo, h;        /* log-spot grid: x_i = x_lo + i*h, h > 0 */
  uint32_t n_times, n_x; /* n_times >= 1, n_x >= 2, n_times*n_x <= HH_LV_MAX_NODES */
} hh_localvol;
int hh_mc_path_stats_lv(hh_ctx* ctx, const hh_model* model, const hh_localvol* lv, const hh_config* cfg,
                        uint32_t monitor_every, int32_t include_start, int32_t extremes, double* stats,
                        int32_t stats_on_device, hh_result* out);
int hh_mc_solve_path_lv(hh_ctx* ctx, const hh_model* model, const hh_localvol* lv, const hh_config* cfg,
                        uint32_t monitor_every, int32_t include_start, int32_t extremes, const hh_path_payoff* payoffs,
                        uint32_t n_payoffs, hh_result* out, double* path_values, double* stats);

/*
 * The same solve for an ensemble SHARDED over several devices (one process and one hh_ctx per
 * device, trajectories split by contiguous ranges as for hh_mc_accumulate).  The backward induction
 * needs sums over ALL trajectories at three points — the in-the-money statistics of every row, the
 * power sums of every row, and the moment sums Σ z^k y of each exercise date — so the solve is cut
 * exactly there: every call leaves a vector of LOCAL sums in device memory, the host all-reduces it
 * (SUM) over the ranks (torch.distributed / RCCL), and hands the GLOBAL vector to the next call:
 *
 *   hh_lsm_shard_begin(cfg of THIS shard)            ->  out [n_steps+1][3]
 *   hh_lsm_shard_phase(HH_LSM_PHASE_POW,  0, in, out):   in [n_steps+1][3]        out [n_steps+1][2D+1]
 *   hh_lsm_shard_phase(HH_LSM_PHASE_INIT, 0, in, out):   in [n_steps+1][2D+1]     out [D+1]  (row n_steps-1)
 *   for t = n_steps-1 .. 1:
 *   hh_lsm_shard_phase(HH_LSM_PHASE_STEP, t, in, out):   in [D+1] of row t        out [D+1] of row t-1
 *                                                                                  (nothing for t = 1)
 *   hh_lsm_shard_finish(accum_dev)                   ->  accum_dev[HH_ACC_LEN]: Σ, Σ² of the discounted
 *                                                        stopped values and the local trajectory count
 *   hh_lsm_finalize(all-reduced accumulator, host)   ->  price, std_error, n_paths_total
 *
 * in / out are device pointers (they may alias); hh_lsm_shard_xchg_elems() doubles hold the largest
 * of them.  With one rank (no all-reduce) the sequence reproduces hh_lsm_solve bit for bit.  The
 * optional host outputs of hh_lsm_shard_finish are this shard's stopping_info / spot rows.
 */
enum hh_lsm_phase { HH_LSM_PHASE_POW = 1, HH_LSM_PHASE_INIT = 2, HH_LSM_PHASE_STEP = 3 };
size_t hh_lsm_shard_xchg_elems(uint32_t n_steps, int32_t degree);
int hh_lsm_shard_begin(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, int32_t degree,
                       double step_discount, double* out_dev);
int hh_lsm_shard_phase(hh_ctx* ctx, int32_t phase, uint32_t t, const double* in_dev, double* out_dev);
int hh_lsm_shard_finish(hh_ctx* ctx, double* accum_dev, int32_t* stop_time, double* stop_value,
                        double* spot_grid, uint32_t* rows_regressed, uint32_t* rows_skipped);
int hh_lsm_finalize(const double* accum_host, hh_lsm_result* out);
/* Retired diagnostic, kept for ABI compatibility: copies the 8 doubles behind the row counters of an LSM
 * solve of that shape.  They held the phase totals of a diagnostic build that is no longer part of the
 * library; nothing writes them now, so their contents are unspecified (zeros after some forms, whatever the
 * reused scratch held after others). */
int hh_lsm_debug_read(hh_ctx* ctx, uint64_t n_paths_total, uint32_t n_steps, int32_t degree,
                      double* out8);

/*
 * hh_lsm_solve (least_squares_montecarlo.jl:99-136) with the trajectories sharded over the devices of
 * mg, in ONE call: the phased induction of hh_lsm_shard_* on every device, the vectors of local sums
 * all-reduced INSIDE the library between consecutive phases (2 + (n_steps − 1) + 1 exchanges of at most
 * (n_steps + 1)·(2·degree + 1) doubles: ncclAllReduce in place on the shards' streams, or — host-sum
 * contexts — copied back, added in the order g = 0 … G−1 and handed out again).  Unlike the European
 * solve this path exchanges IN PLACE between its phases, so the local sums go with a collective that
 * fails in the middle: the communicators are aborted and the streams retired as described above, and
 * the whole induction is run again with the host's ordered sum (HH_MGPU_AUTO) or the call returns
 * HH_ERR_RCCL (HH_MGPU_RCCL).  cfg: the whole ensemble with HOST seeds, as for hh_lsm_solve; every device must get
 * at least one trajectory.  stop_time / stop_value (nullable, host): the reference's stopping_info in
 * the whole-ensemble order of hh_lsm_solve (n_paths entries, then the n_paths mirrored ones).  Same
 * regression sums up to their summation order: identical stopping decisions except where a payoff
 * equals its fitted continuation value to rounding.
 */
int hh_mgpu_lsm_solve(hh_mgpu* mg, const hh_model* model, const hh_config* cfg, int32_t degree,
                      double step_discount, hh_lsm_result* out, int32_t* stop_time, double* stop_value);

/*
 * Per-date EXACT Heston paths: the NoiseProblem that sde_problem(::PricingProblem, ::HestonDynamics,
 * ::HestonBroadieKaya) builds (src/pricing_methods/montecarlo.jl:209-231) on the HestonNoise process
 * (src/distributions/heston.jl:82-91), stepped with dt = T/n_steps by simulate_paths (:342-353):
 * every step draws (log S, V) at t+dt from LogHestonDistribution(S_t, V_t, κ, θ, σ, ρ, r, dt) —
 * one Broadie–Kaya transition per date and trajectory.
 * cfg: dynamics = HH_HESTON, strategy = HH_BROADIE_KAYA, noise_mode = HH_NOISE_GENERATE, n_steps,
 * n_paths, seeds (ONE PER TRAJECTORY here, montecarlo.jl:331 — unlike the one-shot terminal law,
 * which reads seeds[0] only), bk_* controls; no antithetic form, no dual partials.
 * Outputs (nullable; host, or device when grids_on_device): spot_grid[(n_steps+1)][n_paths] =
 * exp(log S) rows (row 0 = S0) and var_grid of the same shape (row 0 = V0);
 * hh_lsm_grid_elems(n_paths, n_steps, 0) doubles each.  out (nullable): the bk_* counters summed
 * over all transitions, n_paths_done, kernel_ms, total_ms; price fields are zero.
 * hh_lsm_solve accepts the same (dynamics, strategy) pair and regresses on the spot rows.
 */
int hh_heston_exact_grid(hh_ctx* ctx, const hh_model* model, const hh_config* cfg, double* spot_grid,
                         double* var_grid, int32_t grids_on_device, hh_result* out);

/*
 * REPLAY increments.  Tile-major layout (what the step kernels stream):
 *     dW[tile][step][comp][HH_TILE_PATHS],  tile = path / 256, comp < ncomp (1 lognormal, 2 Heston),
 * the last tile zero-padded.  hh_replay_elems() = ceil(n_paths/256)·n_steps·ncomp·256 doubles.
 * Path-major layout (what the reference's saved noise gives per trajectory, montecarlo.jl:258,370):
 *     dW[path][step][comp]  (n_paths·n_steps·ncomp doubles), replay_layout = HH_REPLAY_PATH_MAJOR.
 * hh_mc_solve / hh_mc_accumulate STREAM such a buffer directly (no repacked copy) whenever a
 * trajectory's row is a multiple of 16 bytes — n_steps·ncomp even: every Heston shape, lognormal with an
 * even step count; the rows may start on any 16-byte boundary.  A device-resident buffer
 * (replay_on_device) is then read in place WHILE THE KERNEL RUNS: it must stay untouched until the
 * call's stream has completed (hh_mc_solve returns after that; after hh_mc_accumulate, synchronize) and
 * must not alias `terminal`.  A host buffer is copied to the ctx's staging buffer first, as always.  Only
 * the remaining case (lognormal Euler with an odd n_steps, and the one-normal-per-trajectory buffer of the
 * exact law when it is declared path-major) is repacked into the tile-major layout first, by the kernel
 * behind hh_replay_pack(), which callers may also use themselves.
 * For Heston the increments are the CORRELATED ones, cov = dt·[1 ρ; ρ 1] (heston.jl:18-20).
 * Exact lognormal law (HH_EXACT_LAW) in REPLAY mode: `replay` holds ONE standard normal per
 * trajectory, n_paths doubles (x = μ + σ̃·z, montecarlo.jl:302,413); no padding required.
 * Broadie–Kaya (HH_BROADIE_KAYA) in REPLAY mode: `replay` holds the three draws the reference makes
 * per trajectory, in its order (heston.jl:246-259) — V_T = c·rand(NoncentralChisq(d, λ)) (:125-133),
 * the uniform u of sample_from_cf (sample_from_cf.jl:29) and the normal Z of sample_log_S_T
 * (heston.jl:296) — as [V_T | u | Z], 3·n_paths doubles.  Everything downstream of the draws
 * (moments_from_cf, cdf_from_cf, inverse_cdf, log S_T) then runs on the reference's own numbers.
 */
size_t hh_replay_elems(uint64_t n_paths, uint32_t n_steps, int32_t dynamics);
int hh_replay_pack(hh_ctx* ctx, int32_t dynamics, uint64_t n_paths, uint32_t n_steps,
                   const double* src_path_major, int32_t src_on_device, double* dst_tile_major_dev);
/*
 * Fill a tile-major REPLAY buffer on the device with exactly the increments GENERATE mode would
 * draw (Philox4x32-10 keyed by seeds[i], counter = step; Box–Muller; lower-triangular correlation).
 */
int hh_wiener_fill(hh_ctx* ctx, int32_t dynamics, double rho, double T, uint32_t n_steps,
                   uint64_t n_paths, const uint64_t* seeds, int32_t seeds_on_device,
                   double* dst_tile_major_dev);

/*
 * Quasi-Monte Carlo: Sobol' points, and a tile-major REPLAY buffer filled from them (no reference method; every REPLAY
 * consumer — hh_mc_solve and its kin — prices on such a buffer unchanged).
 *
 * THE POINT RULE.  Dimension d < HH_SOBOL_MAX_DIMS has 32 direction words v_d[j] = m_(j+1) << (31 − j), expanded from
 * the Joe–Kuo set new-joe-kuo-6.21201 (csrc/hh_sobol_table.h; dimension 0 is the van der Corput sequence).
 *   x      point i (0 <= i < 2^32) of dimension d is the XOR of v_d[b] over the set bits b of g = i ^ (i >> 1): Gray-code
 *          order, the rows of the unscrambled engines of PyTorch and SciPy, row for row
 *   shift  randomisation r XORs a digital shift into x: for dimension d the word d & 3 of the Philox4x32-10 block with
 *          counter (d >> 2, r, 0, kDomSobol = 7) and key (shift_seed low word, shift_seed high word).  shifted = 0: none
 *   u      (x + 1/2)·2^-32 — exact in fp64, never 0 or 1; the smallest tail is 2^-33 = 1.16e-10
 *   z      the standard normal quantile of u (Wichura's AS 241, csrc/hh_math.h)
 *
 * THE CONSTRUCTION, on n_steps unit-variance steps of ncomp (1 lognormal, 2 Heston) independent factors; coordinate
 * ncomp·j + comp of the point is the normal z_j of factor comp:
 *   HH_SOBOL_INCREMENTAL   d_k = z_k, the step's own normal
 *   HH_SOBOL_BRIDGE        W_0 = 0; bridge index 0 is the terminal value W_n = sqrt(n)·z_0; every later index j takes the
 *                          next interval (l, r) with r − l >= 2 from a queue that starts with (0, n), sets m = (l + r) / 2
 *                          (rounded down),  W_m = fma(wl, W_l, fma(wr, W_r, sd·z_j))  with  wl = (r − m)/(r − l),
 *                          wr = (m − l)/(r − l),  sd = sqrt((m − l)·(r − m)/(r − l))  — each one rounded fp64 division or
 *                          product of the integers as doubles, sqrt correctly rounded — and queues (l, m), then (m, r): any
 *                          n_steps, not only powers of two; the first ncomp coordinates carry the terminal values.
 *                          d_k = W_(k+1) − W_k.
 * and the increments, in hh_wiener_fill's form and with its covariance dt·[1 ρ; ρ 1], dt = T/n_steps, sqrt_dt = sqrt(dt):
 *   dW_k[0] = sqrt_dt·d_k[0];   Heston: dW_k[1] = sqrt_dt·fma(ρ, d_k[0], sqrt(1 − ρ²)·d_k[1]).
 * Every operation named is one rounded fp64 operation, in the order written (fma: one rounding).
 *
 * hh_sobol_directions: the 32 words of dimension dim.  Host arithmetic, no context, no GPU.  HH_ERR_INVALID: v NULL or
 *     dim >= HH_SOBOL_MAX_DIMS.
 * hh_sobol_points: the raw words x (shifted or not) of points point_offset … point_offset + n_points − 1 in the first
 *     n_dims dimensions, dst_dev[dim][point], n_dims·n_points uint32 in device memory.  HH_ERR_INVALID: NULL arguments,
 *     n_dims = 0, n_points = 0 or above 2^32 − 256, point_offset + n_points > 2^32; HH_ERR_UNSUPPORTED:
 *     n_dims > HH_SOBOL_MAX_DIMS.
 * hh_sobol_fill: dW[tile][step][comp][HH_TILE_PATHS] of hh_replay_elems(n_points, n_steps, dynamics) doubles, lane p of
 *     tile t being point point_offset + 256·t + p, the last tile zero-padded.  Shards of one point set compose: a fill of
 *     [a, b) holds the columns of a fill of [0, b) bit for bit.  T = n_steps = 1 with HH_LOGNORMAL leaves one standard
 *     normal per point: what the exact law's REPLAY mode reads.  HH_ERR_INVALID: NULL arguments, |rho| > 1, T <= 0,
 *     n_steps = 0, n_points = 0 or above 2^32 − 256, point_offset + n_points > 2^32, an unknown construction;
 *     HH_ERR_UNSUPPORTED: ncomp·n_steps > HH_SOBOL_MAX_DIMS.
 * Both device entry points are asynchronous, like hh_wiener_fill.
 */
#define HH_SOBOL_MAX_DIMS 4096
enum hh_sobol_construction { HH_SOBOL_INCREMENTAL = 0, HH_SOBOL_BRIDGE = 1 };
int hh_sobol_directions(uint32_t dim, uint32_t v[32]);
int hh_sobol_points(hh_ctx* ctx, uint32_t n_dims, uint64_t n_points, uint64_t point_offset, uint64_t shift_seed,
                    uint32_t randomization, int32_t shifted, uint32_t* dst_dev);
int hh_sobol_fill(hh_ctx* ctx, int32_t dynamics, double rho, double T, uint32_t n_steps, uint64_t n_points,
                  uint64_t point_offset, uint64_t shift_seed, uint32_t randomization, int32_t shifted,
                  int32_t construction, double* dst_tile_major_dev);

/*
 * Measurement hooks (the reference has no tracing; the build supplies its own).  When
 * enabled, every hh_mc_accumulate / hh_mc_solve brackets EVERYTHING IT ENQUEUES — the simulation
 * kernels and, where it is a kernel of its own, the record reduction; not the staging copies in front —
 * with HIP events on the ctx stream (one slot per call; hh_mc_accumulate_multi on Broadie–Kaya: one per
 * model — a chain's, then each finish pass's); hh_crr_solve and hh_fd_solve bracket their one kernel (one slot per
 * call, neither the upload nor the copy back); hh_ctx_read_timings
 * synchronizes the stream and returns the elapsed ms of the slots recorded since the last read
 * (at most 256 are kept).
 */
int hh_ctx_enable_timing(hh_ctx* ctx, int32_t on);
int hh_ctx_read_timings(hh_ctx* ctx, double* ms, int32_t cap, int32_t* n_out);

/*
 * Variance Gamma (Madan, Carr and Chang 1998): a Brownian motion with drift θ and volatility σ run on a gamma clock — a
 * pure-jump Lévy model with infinitely many jumps, no Brownian part of its own, and skew and kurtosis at every expiry.
 * The reference has no such model; the conventions below are this library's.
 *   X_t = θ·G_t + σ·W(G_t)        G a gamma process, G_t ~ Gamma(shape t/ν, scale ν)  (mean t, variance ν·t)
 *   log S_t = log S0 + (r + ω)·t + X_t        ω = log(1 − θν − σ²ν/2)/ν,   requires 1 − θν − σ²ν/2 > 0
 *   ϕ(u) = E exp(iu·log S_T) = exp(iu·(log S0 + (r + ω)T)) · (1 − iuθν + σ²νu²/2)^(−T/ν)      (principal branch)
 *   call = E_G[ discounted Black call on a lognormal with log-mean log S0 + (r + ω)T + θG and log-variance σ²G ]
 * hh_vg carries θ and ν; σ = model->sigma, r = model->r_drift.  No existing struct changes.  The increments of X over
 * disjoint spans are independent and exact in law, so the states on any set of dates carry no discretisation bias.
 *
 * ON THE HOST, once per call (csrc/hh_vg.h, vg_args), each a single rounded fp64 operation in this order, τ being what
 * one gamma draw covers — T (terminal law), dt = T/n_steps (path form):
 *   arg = (1 − (θ·ν)) − ((0.5·(σ·σ))·ν)        ω = log(arg)/ν        drift = (r + ω)·τ
 *   a = τ/ν        boost = a < 1        a′ = boost ? a + 1 : a        d = a′ − 1/3  (1/3 the double 1.0/3.0)
 *   c = 1/sqrt(9·d)        inv_a = 1/a        nu_d = ν·d
 *
 * THE GAMMA VARIATE Gamma(a, ν) by Marsaglia and Tsang (2000) with the shape boost (csrc/hh_vg.h, gamma_mt — a function
 * of a draw source, which a host program can call on draws of its choosing).  Attempt t = 0, 1, … takes a standard
 * normal z, a uniform U and, boosted, a uniform U′, all of its own, then — one rounded operation each, in this order —
 *   x = 1 + c·z        v = (x·x)·x        and only where v > 0:
 *   rhs = (((0.5·z)·z + d) − d·v) + d·log v        val = nu_d·v,  boosted: val·exp(log(U′)·inv_a)
 * and accepts val when log U < rhs.  The loop ends after HH_VG_MAX_ATTEMPTS attempts at the latest with the val of the
 * last attempt that had v > 0 (+0 when none had); an attempt is accepted with probability > 0.95 whatever the shape, so
 * the cap is met with probability below 0.05⁶⁴ — it is there because no device loop may be bounded by data alone.
 * The boosted product may underflow to +0 (a = 0.008: 0.3 % of the variates): the span then adds the drift alone.
 * Every draw is a Philox4x32-10 block whose counter word 3 is 8, a domain no other draw of the library uses; z is the
 * FIRST normal of a block's Box–Muller pair (as every normal pair of the library; the second is not used),
 * U = u01(words 0, 1) and U′ = u01(words 2, 3) of a second block, u01(lo, hi) = ((w >> 12) + ½)·2⁻⁵² of
 * w = (hi << 32) | lo as everywhere.
 *
 * THE INCREMENT over a span, from its variate g and a standard normal z_B independent of it:
 *   inc = (drift + θ·g) + (σ·sqrt(g))·z_B        sqrt correctly rounded; the antithetic mirror takes the same g and −z_B.
 *
 * hh_mc_solve_vg — the TERMINAL LAW, cfg->strategy = HH_EXACT_LAW.  Trajectory i of the call has the global index
 * g = cfg->path_offset + i and is keyed by seeds[0], as the exact lognormal law is.
 *   attempt t:  z from block (lo32 g, hi32 g, 2t, 8);  U, U′ from block (lo32 g, hi32 g, 2t + 1, 8)
 *   z_B:        the first normal of block (lo32 g, hi32 g, 2·HH_VG_MAX_ATTEMPTS, 8)
 *   x_T = log S0 + inc        with τ = T
 * terminal (nullable; host, or device when cfg->terminal_on_device): exp(x_T) of the n_paths trajectories, then of their
 * mirrors.  The payoff (model->strike, model->cp), the sums and hh_result are hh_mc_solve's.  1 .. 2^32 − 256
 * trajectories per call; a lane takes eight of them whatever the call, so a call's sums are reproducible, and [0, n) is
 * [0, k) followed by [k, n) with path_offset = k, sample for sample.  Timing: one slot, as hh_mc_solve.
 *
 * hh_mc_path_stats_vg, hh_mc_solve_path_vg — the PATH FORM, cfg->strategy = HH_EXACT_LAW with cfg->n_steps spans of
 * dt = T/n_steps: hh_mc_path_stats / hh_mc_solve_path_ex under HH_EXTREMES_MONITORED on these paths.  Trajectory i is
 * keyed by seeds[i].  Step k = 0 .. n_steps − 1:
 *   attempt t:  z from block (k, t, 0, 8);  U, U′ from block (k, t, 1, 8)
 *   z_B:        the normal the lognormal hh_mc_path_stats draws for step k — block (k >> 1, 0, 0, 0), its first normal for
 *               an even k, its second for an odd one: one block per two steps, an odd n_steps leaving the last half read
 *   x ← x + inc        with τ = dt, then the monitoring date
 * The statistics are the five rows of HH_EXTREMES_MONITORED over the same monitoring dates with the same arithmetic;
 * payoff kinds 0 .. 7 are admitted, the lookbacks read the monitored rows.  There are no continuous (bridge) extremes:
 * between two dates the path is no diffusion bridge.  Arguments, outputs and timing slots are hh_mc_path_stats' and
 * hh_mc_solve_path's.
 *
 * hh_carr_madan_vg — hh_carr_madan_basket (lognormal dynamics, compat_sqrt_alpha = 0) with ϕ above, the power taken as
 * exp(−(T/ν)·log(base)) on the principal branch: the same fixed quadrature rule, one workgroup per payoff, the same
 * parity transform for puts.  On the contour Im u = −(1+α) the base's real part is at least
 * 1 − θν(1+α) − σ²ν(1+α)²/2, which the entry point requires to be positive (the (1+α)-th moment is then finite): the
 * base never crosses the negative real axis and the principal branch is continuous along the whole contour.
 *
 * All four are synchronous.  Errors, checked on the host before any launch.  HH_ERR_INVALID: vg is NULL; ν <= 0 or not
 * finite; θ not finite; σ < 0; 1 − θν − σ²ν/2 <= 0; for hh_carr_madan_vg 1 − θν(1+α) − σ²ν(1+α)²/2 <= 0; everything
 * hh_mc_solve / hh_mc_solve_path_ex / hh_carr_madan_basket reject.  HH_ERR_UNSUPPORTED: Heston dynamics, REPLAY noise,
 * n_partials > 0, a strategy other than HH_EXACT_LAW.  After any refusal the context stays usable.
 * Not provided: NIG and CGMY, the difference-of-gammas form, bridge or continuous monitoring, REPLAY and quasi-Monte
 * Carlo, dual partials (bump the inputs: the solves of a finite difference share their seeds), multilevel coupling,
 * accumulate, hh_mc_solve_multi and multi-GPU forms (American exercise: hh_lsm_solve_path), a gradient of
 * hh_carr_madan_vg, a Julia binding.
 */
#define HH_VG_MAX_ATTEMPTS 64    /* the rejection loop of one gamma variate stops here at the latest */
typedef struct hh_vg { double theta, nu; } hh_vg;                        /* 16 bytes */
int hh_mc_solve_vg(hh_ctx* ctx, const hh_model* model, const hh_vg* vg, const hh_config* cfg, hh_result* out,
                   double* terminal);
int hh_mc_path_stats_vg(hh_ctx* ctx, const hh_model* model, const hh_vg* vg, const hh_config* cfg, uint32_t monitor_every,
                        int32_t include_start, double* stats, int32_t stats_on_device, hh_result* out);
int hh_mc_solve_path_vg(hh_ctx* ctx, const hh_model* model, const hh_vg* vg, const hh_config* cfg, uint32_t monitor_every,
                        int32_t include_start, const hh_path_payoff* payoffs, uint32_t n_payoffs, hh_result* out,
                        double* path_values, double* stats);
int hh_carr_madan_vg(hh_ctx* ctx, const hh_model* model, const hh_vg* vg, double alpha, double bound,
                     const double* strikes, const double* cps, const double* Ts, const double* r_drifts,
                     const double* discounts, uint32_t n_payoffs, double* prices_out);

/*
 * Date rows of the log-spot path family, and American / Bermudan exercise on them (kernels: each *_stats_kernel of the
 * family instantiated on the second sink, *_stats_kernel<…, DateRows<ANTI>>; hh_path_stats.h).
 *
 * A SOURCE names one of the family's six kernels and carries the structs it reads beside model and cfg:
 *   HH_SOURCE_EULER     hh_mc_path_stats        lognormal or Heston dynamics, HH_EULER_MARUYAMA      no struct
 *   HH_SOURCE_JUMP      hh_mc_solve_path_jump   lognormal dynamics, HH_EULER_MARUYAMA                jump
 *   HH_SOURCE_QE        hh_mc_path_stats_qe     Heston dynamics, HH_QE                               qe
 *   HH_SOURCE_BATES     hh_mc_path_stats_bates  Heston dynamics, HH_QE                               qe, jump
 *   HH_SOURCE_LOCALVOL  hh_mc_path_stats_lv     lognormal dynamics, HH_EULER_MARUYAMA                localvol
 *   HH_SOURCE_VG        hh_mc_path_stats_vg     lognormal dynamics, HH_EXACT_LAW                     vg
 * The trajectories are those of the entry point named, on the same seeds (seeds[i] keys trajectory i; path_offset is not
 * read), under HH_EXTREMES_MONITORED: the same draws, step and host-formed constants — the two kernels of a source run
 * one statement of the walk.  A struct the kind does not list is not read.
 *
 * hh_mc_path_grid — the spots on every exercise_every-th step.  n_dates = n_steps / exercise_every, exercise_every >= 1
 * a divisor of n_steps.  spot_grid (host, or device when grid_on_device) takes hh_lsm_grid_elems(n_paths, n_dates,
 * antithetic) doubles, step-major as hh_euler_grid's:
 *   row 0   S0 in every column
 *   row j   exp(x) after step j·exercise_every, j = 1 .. n_dates — S = exp(x) is formed on those steps alone
 *   column i < n_paths: trajectory i;  column n_paths + i (antithetic): its mirror
 * With the statistics of the source's path_stats call at monitor_every = exercise_every, include_start = 0: S_T is row
 * n_dates, MAX_S / MIN_S the extremes over rows 1 .. n_dates, SUM_S those rows added in date order, bit for bit.  The
 * rows at exercise_every = m are rows 0, m, 2m, … of the grid at exercise_every = 1; HH_SOURCE_EULER at exercise_every
 * = 1 is hh_euler_grid's HH_PATH_SPOT grid.  out (nullable): n_paths_done and the times.  Timing: one slot.
 *
 * hh_lsm_solve_path — that grid into the context, then the backward induction of hh_lsm_solve_grid over its n_dates
 * exercise dates: hh_lsm_solve_euler's path behind another source, so HH_OPT_LSM_FORM, the one-launch form's fall-back
 * and hh_lsm_result are as there.  date_discount is the discount over ONE EXERCISE PERIOD, T·exercise_every/n_steps
 * (hh_lsm_solve_euler's step_discount at exercise_every = 1).  stop_time (nullable, n_total) is hh_lsm_solve_grid's on that
 * grid: it counts EXERCISE DATES — the grid's rows — not simulation steps, date j lying at time j·T/n_dates.
 * stop_value, spot_grid (nullable, host): as hh_lsm_solve_euler's, the grid being the one above.
 * exercise_every = n_steps leaves one date: the European price, date_discount times the mean payoff at expiry.
 *
 * Both are synchronous.  Errors, checked on the host before any launch, in the words of the source's path_stats entry
 * point wherever it makes the same check.  HH_ERR_INVALID: a NULL source, model, cfg (out for hh_lsm_solve_path) or a
 * struct the kind lists; an unknown kind; exercise_every = 0 or not a divisor of n_steps; n_dates > 65534; everything
 * the source's path_stats entry point rejects (scalars, jump, qe, surface, vg); for hh_lsm_solve_path what
 * hh_lsm_solve_euler rejects (degree outside 1 .. 8, cp not ±1, date_discount not finite or <= 0).
 * HH_ERR_UNSUPPORTED: REPLAY noise, n_partials > 0, dynamics or a strategy that are not the kernel's own.
 * hh_lsm_solve_path checks exercise_every first, then the induction's scalars on its n_dates (in hh_lsm_solve_euler's
 * words), then everything the source's entry point checks; where several things are wrong the first of these is reported.
 * Not provided: sharded and multi-GPU forms, the log path state (the regression on log S is hh_lsm_solve_euler's, on
 * every step), the bridge form, the coupled kernel (the several-asset walk has state rows of its own: "American exercise
 * on several state rows").
 * Provided elsewhere: variance rows for QE and Bates, and for Heston Euler — hh_mc_path_states, "American exercise under
 * stochastic volatility".
 */
enum hh_path_source_kind { HH_SOURCE_EULER = 0, HH_SOURCE_JUMP = 1, HH_SOURCE_QE = 2, HH_SOURCE_BATES = 3,
                           HH_SOURCE_LOCALVOL = 4, HH_SOURCE_VG = 5 };
typedef struct hh_path_source {       /* 40 bytes */
  int32_t kind;                       /* enum hh_path_source_kind */
  const hh_jump* jump;
  const hh_qe* qe;
  const hh_localvol* localvol;
  const hh_vg* vg;
} hh_path_source;
int hh_mc_path_grid(hh_ctx* ctx, const hh_path_source* source, const hh_model* model, const hh_config* cfg,
                    uint32_t exercise_every, double* spot_grid, int32_t grid_on_device, hh_result* out);
int hh_lsm_solve_path(hh_ctx* ctx, const hh_path_source* source, const hh_model* model, const hh_config* cfg,
                      uint32_t exercise_every, int32_t degree, double date_discount, hh_lsm_result* out,
                      int32_t* stop_time, double* stop_value, double* spot_grid);

/*
 * American exercise on several state rows: the state rows of the several-asset walk, and Longstaff–Schwartz with a
 * regression basis in several variables on them (kernels: assets_rows_kernel, hh_assets.hip; the induction,
 * hh_lsm_multi.hip; the basis, csrc/hh_lsm_basis.h — a host program can include it).
 *
 * hh_assets_path_rows — the walk of hh_mc_path_stats_assets (the same draws, step and host-formed constants) with no
 * statistics: on every exercise_every-th step the d = n_assets log-states x_i as the walk holds them, log w_i folded in
 * under best-of and worst-of.  n_dates = n_steps / exercise_every.  rows (host, or device when rows_on_device) takes
 * hh_assets_rows_elems(n_paths, n_dates, n_assets, antithetic) = (n_dates + 1)·d·n_total doubles,
 *   rows[(date·d + asset)·n_total + column]      date-major, then asset-major, n_total = n_paths·(1 + antithetic) columns
 *   date 0: x0_i in every column;  date j: the states after step j·exercise_every;  column n_paths + i: the mirror of i
 * Log-states, not spots: the index of "Several correlated lognormal assets" formed on a stored row is the pair (I, x) the
 * statistics kernel forms on that date, bit for bit, for every index kind — the rows do not depend on the kind beyond x0.
 * The non-mirrored half of an antithetic grid equals the plain grid column for column.  out (nullable): n_paths_done and
 * the times.  Timing: one slot.
 *
 * hh_lsm_solve_states — the backward induction on a DEVICE grid rows_dev[n_dates + 1][m][n_total] of m = desc->n_states
 * state rows per date the caller supplies; the counterpart of hh_lsm_solve_grid.  desc says how a column's m states give
 * the exercise value and the m regressors.  HH_LSM_STATES_LOG_ASSETS: the states are log-states of assets,
 *   exercise value  pay = cp·(I − strike), I the index of kind index_kind and weights[] on the m states (above)
 *   regressors      v_i = exp(x_i), in asset order
 * HH_LSM_STATES_LOG_SPOT_VARIANCE (n_states = 2; index_kind and weights are not read): state 0 is a log spot, state 1 a
 * variance ("American exercise under stochastic volatility" below),
 *   exercise value  pay = cp·(exp(x_0) − strike)
 *   regressors      v_0 = exp(x_0), v_1 = x_1 — the variance as stored
 * Per date t = n_dates − 1 down to 1, on the columns IN THE MONEY, pay > 0, alone (the one-variable rule; the others
 * add exact zeros to every sum):
 *   statistics   n, Σv_i, Σv_i²;  μ_i = Σv_i/n, var_i = Σv_i²/n − μ_i·μ_i, isd_i = 1/sqrt(var_i) if var_i > 0 else 1
 *                (n = 0: the date is skipped, no fit);  z_i = (v_i − μ_i)·isd_i
 *   basis        all monomials φ = Π z_i^{e_i} of total degree <= degree in GRADED LEXICOGRAPHIC order: by total degree,
 *                within a degree the exponent tuples (e_0, …, e_{m−1}) in descending lexicographic order — m = 2, degree
 *                2: 1, z_0, z_1, z_0², z_0·z_1, z_1².  B = C(m + degree, degree) <= HH_LSM_MAX_BASIS functions: m = 5 .. 8 at
 *                degree <= 2, m = 4 at <= 3, m = 3 at <= 4, m = 2 and m = 1 at <= 8.  A value is
 *                1·z_0 (e_0 times)·z_1 (e_1 times)·…, one rounded product after the other, by ONE function for the Gram
 *                sums, the moment sums and the fitted value.
 *   Gram sums    G_jk = Σ φ_j·φ_k          moment sums  b_j = Σ φ_j·y,  y = date_discount^(τ − t)·val
 *   solve        G c = b by LDLᵀ without pivoting; a pivot not above 1e-13·G_cc is dropped, its coefficient 0
 *   exercise     where pay > 0 and pay > c_0·φ_0 + fma(c_j, φ_j, ·) in basis order:  τ = t, val = pay
 * from τ = n_dates, val = max(pay, 0) at expiry; price = mean(date_discount^τ·val), by hh_lsm_solve_grid's final kernel
 * into hh_lsm_result (form = HH_LSM_FORM_PER_DATE: there is no other).  Every sum has a fixed tree (hh_lsm_multi.hip
 * states it: chunks of 512·Q columns by hh_lsm_solve_grid's chunk rule, wave butterflies or the matrix instruction's
 * batches of four columns, waves in order, chunks in order), no atomics: the same inputs give the same bits on every
 * run.  stop_time (nullable, host, n_total) counts EXERCISE DATES — the grid's dates; stop_value (nullable, host,
 * n_total); coef (nullable, host, n_dates·B): the fitted coefficients, coef[t·B + j] of date t, zeros where no fit ran
 * (date 0, a date with no column in the money) and for a dropped pivot.
 *
 * hh_lsm_solve_assets — hh_assets_path_rows into the context, then hh_lsm_solve_states on them with
 * {HH_LSM_STATES_LOG_ASSETS, n_assets, index_kind, cp and strike of the model, the assets' weights}.  date_discount is
 * the discount over ONE EXERCISE PERIOD.  rows (nullable, host): the state rows.  exercise_every = n_steps leaves one
 * date: the European price, date_discount times the mean payoff at expiry.
 *
 * All synchronous.  Errors, checked on the host before any launch, in hh_mc_path_stats_assets' and hh_lsm_solve_path's
 * words wherever the check is the same; a refusal uses no timing slot.  HH_ERR_INVALID: a NULL ctx, model, assets, cfg,
 * desc, rows / rows_dev or out (hh_assets_path_rows: rows); exercise_every = 0 or not a divisor of n_steps; n_dates >
 * 65534; an unknown descriptor kind or index kind; n_states outside 1 .. HH_MAX_ASSETS (HH_LSM_STATES_LOG_SPOT_VARIANCE:
 * other than 2); cp not ±1; strike or a weight
 * not finite; degree outside 1 .. 8; date_discount not finite or <= 0; n_total = 0 or above 2^31 − 128; everything
 * hh_mc_path_stats_assets rejects.  HH_ERR_UNSUPPORTED: C(m + degree, degree) > HH_LSM_MAX_BASIS; REPLAY noise,
 * n_partials > 0, dynamics or a strategy that are not the walk's own.  hh_lsm_solve_assets checks exercise_every first,
 * then the induction's scalars, then everything hh_assets_path_rows checks.
 * Not provided: a persistent or cooperative form, sharded and multi-GPU forms, REPLAY or Sobol' noise, dual partials, basis families other than
 * monomials (sorted assets, the payoff as a regressor, Laguerre), more than HH_LSM_MAX_BASIS functions, barriers on
 * single assets, a Julia binding.
 */
#define HH_LSM_MAX_BASIS 45
enum hh_lsm_states_kind { HH_LSM_STATES_LOG_ASSETS = 0, HH_LSM_STATES_LOG_SPOT_VARIANCE = 1 };
typedef struct hh_lsm_states {        /* 88 bytes */
  int32_t kind;                       /* enum hh_lsm_states_kind */
  uint32_t n_states;                  /* m, 1 .. HH_MAX_ASSETS */
  int32_t index_kind;                 /* enum hh_index_kind */
  int32_t reserved;
  double cp, strike;
  double weights[HH_MAX_ASSETS];
} hh_lsm_states;
size_t hh_assets_rows_elems(uint64_t n_paths, uint32_t n_dates, uint32_t n_assets, int32_t antithetic);
int hh_assets_path_rows(hh_ctx* ctx, const hh_model* model, const hh_assets* assets, const hh_config* cfg,
                        uint32_t exercise_every, double* rows, int32_t rows_on_device, hh_result* out);
int hh_lsm_solve_states(hh_ctx* ctx, const hh_lsm_states* desc, const double* rows_dev, uint64_t n_total,
                        uint32_t n_dates, int32_t degree, double date_discount, hh_lsm_result* out, int32_t* stop_time,
                        double* stop_value, double* coef);
int hh_lsm_solve_assets(hh_ctx* ctx, const hh_model* model, const hh_assets* assets, const hh_config* cfg,
                        uint32_t exercise_every, int32_t degree, double date_discount, hh_lsm_result* out,
                        int32_t* stop_time, double* stop_value, double* rows);

/*
 * American exercise under stochastic volatility: the state rows (log spot, variance) of the walks that hold a variance,
 * and Longstaff–Schwartz with a regression on (S, V) on them (kernels: path_stats_kernel<HestonModel, …>, qe_stats_kernel
 * and bates_stats_kernel instantiated on the third sink, StateRows<ANTI>, hh_path_stats.h; the induction, hh_lsm_multi.hip).
 *
 * hh_mc_path_states — the walk the source names ("Date rows of the log-spot path family": the same draws, step and
 * host-formed constants as its path_stats entry point) with no statistics: on every exercise_every-th step the lane's
 * log spot x and variance v.  Admitted sources: HH_SOURCE_EULER under Heston dynamics, HH_SOURCE_QE, HH_SOURCE_BATES.
 * n_dates = n_steps / exercise_every.  rows (host, or device when rows_on_device) takes hh_assets_rows_elems(n_paths,
 * n_dates, 2, antithetic) = (n_dates + 1)·2·n_total doubles, hh_assets_path_rows' layout at d = 2:
 *   rows[(date·2 + state)·n_total + column]      state 0 = x, state 1 = v, n_total = n_paths·(1 + antithetic) columns
 *   date 0: (log S0, V0) in every column;  date j: the state after step j·exercise_every;  column n_paths + i: the mirror
 * RAW STATE: x and v are stored as the walk holds them.  No exp is formed; under HH_SOURCE_EULER v is the full-truncation
 * scheme's unclipped variance, which can be negative (the step clips where it reads it) — hh_euler_grid's var_grid, and at
 * exercise_every = 1 the x rows are hh_euler_grid's HH_PATH_LOG rows, both bit for bit.  Under QE and Bates v >= 0 and the
 * last v row is var_T of the source's path_stats entry point.  The x rows added in date order are HH_STAT_SUM_X of that
 * entry point at monitor_every = exercise_every, include_start = 0; the rows at exercise_every = m are rows 0, m, 2m, …
 * of the rows at exercise_every = 1; the non-mirrored half of an antithetic grid equals the plain grid.  out (nullable):
 * n_paths_done and the times.  Timing: one slot.
 *
 * hh_lsm_solve_path_states — those rows into the context, then hh_lsm_solve_states on them with
 * {HH_LSM_STATES_LOG_SPOT_VARIANCE, 2, cp and strike of the model}: the exercise value cp·(exp(x) − strike), the
 * regressors S = exp(x) and v, the variance as stored.  date_discount is the discount over ONE EXERCISE PERIOD.
 * stop_time, stop_value (nullable, host, n_total), coef (nullable, host, n_dates·C(2 + degree, degree)): as
 * hh_lsm_solve_states'.  rows (nullable, host): the state rows.  exercise_every = n_steps leaves one date: the European
 * price, date_discount times the mean payoff at expiry.
 *
 * Both are synchronous.  Errors, checked on the host before any launch, in the words of the source's path_stats entry
 * point and of hh_lsm_solve_assets wherever the check is the same; a refusal uses no timing slot.  HH_ERR_INVALID: a NULL
 * ctx, source, model, cfg, rows (hh_mc_path_states), out (hh_lsm_solve_path_states) or a struct the kind lists; an
 * unknown source kind; exercise_every = 0 or not a divisor of n_steps; n_dates > 65534; cp not ±1; a strike not finite;
 * degree outside 1 .. 8; date_discount not finite or <= 0; everything the source's path_stats entry point rejects.
 * HH_ERR_UNSUPPORTED: HH_SOURCE_JUMP, HH_SOURCE_LOCALVOL, HH_SOURCE_VG, and lognormal dynamics on HH_SOURCE_EULER — the
 * walk has no variance; REPLAY noise, n_partials > 0, dynamics or a strategy that are not the kernel's own.
 * hh_lsm_solve_path_states checks exercise_every first, then the induction's scalars, then everything hh_mc_path_states
 * checks.
 * Not provided: a log-spot or payoff regressor and Laguerre bases, variance rows of the exact Heston and Broadie–Kaya
 * sources, a persistent form of the induction, REPLAY or Sobol' noise, dual partials, multi-GPU, a Julia binding.
 */
int hh_mc_path_states(hh_ctx* ctx, const hh_path_source* source, const hh_model* model, const hh_config* cfg,
                      uint32_t exercise_every, double* rows, int32_t rows_on_device, hh_result* out);
int hh_lsm_solve_path_states(hh_ctx* ctx, const hh_path_source* source, const hh_model* model, const hh_config* cfg,
                             uint32_t exercise_every, int32_t degree, double date_discount, hh_lsm_result* out,
                             int32_t* stop_time, double* stop_value, double* coef, double* rows);

/*
 * Dual bounds for American exercise: the fitted policy as an array, its value on other paths (a lower bound) and the
 * Andersen–Broadie (2004) upper bound by nested simulation (kernels: policy_value_kernel, hh_lsm_multi.hip;
 * nested_continuation_kernel and dual_outer_kernel, hh_bounds.hip).
 *
 * A POLICY is a date-major host array of hh_lsm_policy_elems(n_dates, m, degree) = (n_dates + 1)·(2m + B) doubles, B =
 * C(m + degree, degree) (0 where hh_lsm_solve_states admits no such basis):
 *   policy[t·(2m + B) + i]            μ_i of date t, i < m
 *   policy[t·(2m + B) + m + i]        isd_i of date t
 *   policy[t·(2m + B) + 2m + j]       coef_j of date t, j < B, the layout of hh_lsm_solve_states' coef
 * Dates where no fit ran (date 0, date n_dates, a date with no column in the money) hold μ = 0, isd = 1, coef = 0.  THE
 * RULE a policy states, at date t = 1 .. n_dates − 1 on a column with exercise value pay and regressors v_i:
 *   z_i = (v_i − μ_i)·isd_i;  fit = c_0·φ_0 + fma(c_j, φ_j, ·) in basis order (φ by csrc/hh_lsm_basis.h's lsm_phi);
 *   exercise where pay > 0 and pay > fit;  at date n_dates: stop with max(pay, 0).
 * Any finite array is a policy, not only a fitted one: all zeros exercises at the first date in the money, c_0 = 1e300 on
 * every date never exercises before expiry.
 *
 * hh_lsm_fit_states — hh_lsm_solve_states' induction, unchanged, and one more copy: μ_i and isd_i of every regressed date
 * beside the coefficients.  out, stop_time, stop_value and the coef part of policy are hh_lsm_solve_states' on the same
 * rows bit for bit.  hh_lsm_fit_path_states — hh_mc_path_states' rows into the context, then that fit under
 * {HH_LSM_STATES_LOG_SPOT_VARIANCE, 2, cp and strike of the model}: hh_lsm_solve_path_states with the policy.
 *
 * hh_lsm_policy_value — THE RULE run forward on the device rows rows_dev[n_dates + 1][m][n_total], one lane per column
 * from date 1: the first date the policy exercises, else expiry.  stop_time, stop_value (nullable, host, n_total) and out
 * (price = mean(date_discount^τ·val), by the inductions' final kernel) as hh_lsm_solve_states'; rows_regressed and
 * rows_skipped are 0.  On the rows a policy was fitted on it reproduces the induction's stop_time, stop_value and price
 * bit for bit; on rows of other seeds the price is a LOWER bound in expectation (the policy does not see them).  No
 * atomics: the same inputs give the same bits.  hh_lsm_policy_value_path — hh_mc_path_states' rows (HH_SOURCE_EULER under
 * Heston dynamics, HH_SOURCE_QE, HH_SOURCE_BATES) on cfg's seeds into the context, then that valuation at m = 2.  Timing:
 * one slot for the valuation (the forward kernel and the final kernel), before it one for the rows of the _path form.
 *
 * hh_lsm_upper_bound — the dual bound.  Outer pass: hh_mc_path_states' rows of HH_SOURCE_EULER under Heston dynamics on
 * cfg_outer's n_outer = n_paths seeds, plain (no antithetic pairs), kept on the device.  Nested pass: for every date t = 0 ..
 * n_dates − 1 and outer column i, n_inner (a multiple of 64) walks restart from the stored (x, v) of (t, i), take steps
 * t·exercise_every .. n_steps − 1 of the same Euler step, follow THE RULE from date t + 1 and keep y = date_discount^(τ − t)
 * ·val;  cont[t·n_outer + i] = Ĉ = Σy/n_inner and cont_se[…] = sqrt(max(Σy² − n_inner·Ĉ², 0)/(n_inner·(n_inner − 1))).
 * INNER KEYS: walk j of (t, i) draws step s from Philox key
 *   key = mix(mix(inner_seed + 0x9E3779B97F4A7C15·(i + 1)) ^ (t·2^32 + j)),
 *   mix(z): z = (z ^ z >> 30)·0xBF58476D1CE4E5B9; z = (z ^ z >> 27)·0x94D049BB133111EB; z ^ z >> 31   (mod 2^64)
 * at counter (s + 2^31, 0, 0, domain 0): an outer walk's counters are (s, 0, 0, 0) with s < 2^31, so no inner draw is an
 * outer draw whatever the seeds.  Outer recursion, per column, D = date_discount, M_0 = 0:
 *   L_t = pay_t where the policy exercises at t (t = n_dates: max(pay_t, 0)), else Ĉ[t];
 *   M_t = M_{t−1} + D^t·L_t − D^{t−1}·Ĉ[t−1];   pathwise_max[i] = max over t = 0 .. n_dates of D^t·max(pay_t, 0) − M_t
 * upper = mean(pathwise_max), upper_se its standard error, by the inductions' final kernel and record reduction.  By
 * Jensen's inequality the inner noise biases upper UPWARD only: it stays an upper bound in expectation for every n_inner.
 * cont, cont_se (n_dates·n_outer), pathwise_max (n_outer): nullable, host.  The same inputs give the same bits.  Timing:
 * one slot for the rows, one for the nested kernel.
 *
 * All synchronous.  Errors, checked on the host before any launch, in hh_lsm_solve_path_states' words wherever the check
 * is the same; a refusal uses no timing slot.  HH_ERR_INVALID: a NULL ctx, desc, rows_dev, source, model, cfg, policy or
 * out; exercise_every = 0 or not a divisor of n_steps; degree, date_discount, cp, strike, the descriptor and the sizes as
 * hh_lsm_solve_states checks them; n_inner = 0 or not a multiple of 64; a policy entry that is not finite; n_dates·n_outer
 * above 2^31.  HH_ERR_UNSUPPORTED: more than HH_LSM_MAX_BASIS basis functions; the sources hh_mc_path_states refuses;
 * for hh_lsm_upper_bound everything but Heston dynamics by Euler–Maruyama, antithetic outer paths, REPLAY noise,
 * n_partials > 0.
 * Not provided: nested walks for QE, Bates, the several-asset walk and the one-variable spot grid; antithetic, sharded or
 * multi-GPU forms; sub-simulation savings (skipping Ĉ where exercise is clearly suboptimal); a Julia binding.
 */
typedef struct hh_bounds_result {     /* 56 bytes */
  double upper, upper_se;
  uint64_t n_outer;
  uint32_t n_inner, reserved;
  double nested_ms, outer_ms;         /* nested_continuation_kernel, dual_outer_kernel */
  double total_ms;
} hh_bounds_result;
size_t hh_lsm_policy_elems(uint32_t n_dates, uint32_t m, int32_t degree);
int hh_lsm_fit_states(hh_ctx* ctx, const hh_lsm_states* desc, const double* rows_dev, uint64_t n_total, uint32_t n_dates,
                      int32_t degree, double date_discount, hh_lsm_result* out, int32_t* stop_time, double* stop_value,
                      double* policy);
int hh_lsm_fit_path_states(hh_ctx* ctx, const hh_path_source* source, const hh_model* model, const hh_config* cfg,
                           uint32_t exercise_every, int32_t degree, double date_discount, hh_lsm_result* out,
                           double* policy);
int hh_lsm_policy_value(hh_ctx* ctx, const hh_lsm_states* desc, const double* policy, int32_t degree,
                        const double* rows_dev, uint64_t n_total, uint32_t n_dates, double date_discount,
                        hh_lsm_result* out, int32_t* stop_time, double* stop_value);
int hh_lsm_policy_value_path(hh_ctx* ctx, const hh_path_source* source, const hh_model* model, const hh_config* cfg,
                             uint32_t exercise_every, const double* policy, int32_t degree, double date_discount,
                             hh_lsm_result* out);
int hh_lsm_upper_bound(hh_ctx* ctx, const hh_model* model, const hh_config* cfg_outer, uint32_t exercise_every,
                       const double* policy, int32_t degree, double date_discount, uint32_t n_inner, uint64_t inner_seed,
                       hh_bounds_result* out, double* cont, double* cont_se, double* pathwise_max);

/*
 * A SimulationConfig's seed vector in the device memory of ctx, uploaded once and kept — repeated solves on one
 * config (finite-difference Greeks, calibration loops) would otherwise move 8 MB per 10^6 trajectories at
 * every call, about a third of a GENERATE solve of that size.  The reference reads seeds[i] at every solve
 * (montecarlo.jl:331), so the cache is CONTENT-addressed: an entry is found by the vector's length and a
 * fingerprint of ALL its elements (hh_seeds_fingerprint, ~1 ms per 10^6 seeds) — a vector changed in place, or
 * another vector at the same address, is simply another key and is uploaded; the same numbers at another
 * address hit.  `fingerprint` = 0 lets the call compute it; a host whose vector cannot change (the Python
 * mirror freezes its copy) computes it once and passes it.  At most HH_SEED_CACHE_ENTRIES vectors are kept per
 * context, the least recently used one goes first, all go with the context.  *dev_out stays valid until a
 * later hh_seeds_cache call of this context MISSES (an eviction frees it): ask right before every solve,
 * pass the pointer as cfg->seeds with seeds_on_device = 1, do not keep it.  The upload is synchronous — the
 * host vector is free to change when the call returns.  The entry the call BEFORE a miss returned is never the one
 * evicted, so two host threads that share a context and each look up, then solve, cannot free each other's vector
 * between the two steps; more than two such threads serialise lookup + solve themselves (a context is one stream:
 * they gain nothing from running side by side).
 */
#define HH_SEED_CACHE_ENTRIES 8
uint64_t hh_seeds_fingerprint(const uint64_t* seeds, uint64_t n);  /* pure host arithmetic; never 0 */
int hh_seeds_cache(hh_ctx* ctx, const uint64_t* seeds_host, uint64_t n, uint64_t fingerprint,
                   const uint64_t** dev_out);
int hh_seeds_cache_stats(hh_ctx* ctx, uint64_t* hits, uint64_t* uploads, uint64_t* evictions); /* each nullable */

/* Device memory helpers for hosts without another allocator (the Julia wrapper). */
int hh_device_malloc(hh_ctx* ctx, size_t bytes, void** out_dev);
int hh_device_free(hh_ctx* ctx, void* dev);
int hh_memcpy_h2d(hh_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int hh_memcpy_d2h(hh_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int hh_ctx_synchronize(hh_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* HEDGEHOG_MC_H */
