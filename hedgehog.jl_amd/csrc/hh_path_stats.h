// The monitored statistics of a trajectory and its mirror (enum hh_path_stat), stated once for the kernels that keep
// them on log spots: path_stats_kernel (hh_path.hip), jump_stats_kernel (hh_jump.hip), qe_stats_kernel (hh_qe.hip),
// bates_stats_kernel (hh_bates.hip), localvol_stats_kernel (hh_localvol.hip) and vg_stats_kernel (hh_vg.hip).  Running is
// the arithmetic of the five rows, Monitor the dates they are taken on, Extremes the two rows of the bridge form; a kernel
// supplies its states, its step and the call after it.  DateRows is the second sink of the same walks: each kernel takes its
// sink as its last template parameter (Monitor by default) and, instantiated on DateRows, leaves the dates themselves
// (hh_mc_path_grid).  assets_stats_kernel (hh_assets.hip) uses Running and writes the dates out itself (its head
// comment says why).  Internal.
#pragma once
#include "hh_sim.h"

namespace hh {
namespace {

// v_max_f64 / v_min_f64 as ONE instruction each: written with fmax / fmin the compiler first canonicalises the
// loop-carried operand (v_max_f64 v, v, v), as in HestonModel::step.  No operand is ever NaN here, but for the one
// case Extremes names, where the instruction's own rule (the other operand) is what is wanted.
__device__ __forceinline__ double vmax(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double vmin(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// the running statistics of one trajectory (enum hh_path_stat)
struct Running {
  double sum_s = 0.0, sum_x = 0.0, max_s = 0.0, min_s = 0.0, s_t = 0.0;
  __device__ __forceinline__ void first(double S, double x) {  // a sum starts with its first term
    sum_s = S;
    sum_x = x;
    max_s = S;
    min_s = S;
    s_t = S;
  }
  __device__ __forceinline__ void next(double S, double x) {  // … and takes one rounded addition per later date
    sum_s = sum_s + S;
    sum_x = sum_x + x;
    max_s = vmax(max_s, S);
    min_s = vmin(min_s, S);
    s_t = S;
  }
  __device__ __forceinline__ void store(double* __restrict__ stats, const PathStatsLayout& at, uint64_t col) const {
    // plain stores, not the grids' nontemporal ones: path_payoff_kernel reads the rows straight back (measured:
    // its 27 µs become 31 µs behind nontemporal stores, the statistics kernel does not change)
    stats[at.row(HH_STAT_SUM_S) + col] = sum_s;
    stats[at.row(HH_STAT_SUM_X) + col] = sum_x;
    stats[at.row(HH_STAT_MAX_S) + col] = max_s;
    stats[at.row(HH_STAT_MIN_S) + col] = min_s;
    stats[at.row(HH_STAT_S_T) + col] = s_t;
  }
};

// The monitoring dates of one lane: its trajectory and (ANTI) the mirror in the same lane, column n_paths + i.  The dates
// are the steps monitor_every, 2·monitor_every, …, n_steps — monitor_every divides n_steps, so the last step is one —
// and step 0 when include_start.  The countdown to the next date and the "a first term is in" flag depend on kernel
// arguments alone: uniform branches.
template <bool ANTI>
struct Monitor {
  // (the members in the reverse of the order the kernels once declared them as locals: promoted to registers in this
  // order, eleven of the thirteen path_stats_kernel forms and every jump, QE and Bates kernel compile to the code they
  // compiled to with those locals)
  static constexpr bool kStats = true;  // keeps the five rows (DateRows: writes the dates out)
  const uint32_t every;
  uint32_t left;
  bool started;
  Running ra, r;
  __device__ __forceinline__ Monitor(uint32_t monitor_every, int include_start)
      : every(monitor_every), left(monitor_every), started(include_start != 0) {}
  // where a sink writes as it goes (DateRows); the statistics go out at the end, through store
  __device__ __forceinline__ void bind(double*, uint64_t, uint64_t) {}
  // step 0, taken when include_start alone: (S0, log S0), from which the mirror starts as well
  __device__ __forceinline__ void start(double S0, double x0) {
    if (!started) return;
    r.first(S0, x0);
    if constexpr (ANTI) ra.first(S0, x0);
  }
  // A step has been taken: x and (ANTI: read then alone) xa are the log spots after it.  S = exp(x) is formed on a date
  // only, as euler_grid_kernel's `put` forms it, and the trajectory's pair goes into its sums before the mirror's is formed.
  __device__ __forceinline__ void date(const double& x, const double& xa) {
    if (--left != 0u) return;
    left = every;
    const double S = exp(x);
    if (started) r.next(S, x);
    else r.first(S, x);
    if constexpr (ANTI) {
      const double Sa = exp(xa);
      if (started) ra.next(Sa, xa);
      else ra.first(Sa, xa);
    }
    started = true;
  }
  // The rows of the trajectory, then of the mirror.  (A kernel that stores more per member — var_T — stores r and ra
  // itself, each member's rows before its extra number: qe_stats_kernel.)
  __device__ __forceinline__ void store(double* __restrict__ stats, const PathStatsLayout& at, uint64_t i,
                                        uint64_t n_paths) const {
    r.store(stats, at, i);
    if constexpr (ANTI) ra.store(stats, at, n_paths + i);
  }
};

// The other sink of the family's walks, with Monitor's start / date / store: every date's exp(x) goes OUT, into the
// step-major grid [n_steps/every + 1][n_total] of hh_lsm_grid_elems, and nothing is kept.  Row 0 is S0 as euler_grid_kernel
// writes it (a plain store, whatever include_start says), row j the state after step j·every, the mirror of trajectory i
// in column n_paths + i.  One lane writes one column: a wave's store is 512 contiguous bytes per date and member.  The
// grid is written once and read once by the induction, far beyond what the caches hold: nontemporal stores, as there.
// The lane carries the address of its column in the next row and adds n_total (size_t) per date; the countdown is
// Monitor's uniform branch.
template <bool ANTI>
struct DateRows {
  static constexpr bool kStats = false;
  const uint32_t every;
  uint32_t left;
  double* next = nullptr;  // column i of the next row
  size_t n_total = 0, mirror = 0;
  __device__ __forceinline__ DateRows(uint32_t exercise_every, int) : every(exercise_every), left(exercise_every) {}
  __device__ __forceinline__ void bind(double* __restrict__ grid, uint64_t i, uint64_t n_paths) {
    next = grid + i;
    n_total = (size_t)(ANTI ? 2 * n_paths : n_paths);
    mirror = (size_t)n_paths;
  }
  __device__ __forceinline__ void start(double S0, double) {
    next[0] = S0;
    if constexpr (ANTI) next[mirror] = S0;
    next += n_total;
  }
  __device__ __forceinline__ void date(const double& x, const double& xa) {
    if (--left != 0u) return;
    left = every;
    __builtin_nontemporal_store(exp(x), next);
    if constexpr (ANTI) __builtin_nontemporal_store(exp(xa), next + mirror);
    next += n_total;
  }
  __device__ __forceinline__ void store(double* __restrict__, const PathStatsLayout&, uint64_t, uint64_t) const {}
};

// The running extremes of the scheme's CONTINUOUS interpolation, in log space (the bridge form of path_stats_kernel and
// localvol_stats_kernel).  Between x0 and x1 an Euler step with frozen diffusion coefficient g is a Brownian bridge of
// variance q = g²·dt, whose maximum and minimum have the laws that one uniform each inverts:
// ½(x0 + x1 ± sqrt((x1 - x0)² + q·L)),  L = -2 ln U.
// The endpoint x1 goes in by itself, so cmax >= every state exactly whatever the formula's rounding.  q = 0 (a clipped
// variance) gives the endpoints' max / min from the same formula; should x1 == x0 as well, sqrt_pos(0) is NaN, which
// v_max_f64 / v_min_f64 drop in favour of their other operand: the endpoint is all there is.
struct Extremes {
  double cmax = 0.0, cmin = 0.0;
  __device__ __forceinline__ void first(double x) { cmax = cmin = x; }  // time 0 always counts
  __device__ __forceinline__ void next(double x0, double x1, double q, double Lmax, double Lmin) {
    const double d = x1 - x0, d2 = d * d, m = x0 + x1;
    const double up = 0.5 * (m + sqrt_pos(fma(q, Lmax, d2)));
    const double dn = 0.5 * (m - sqrt_pos(fma(q, Lmin, d2)));
    cmax = vmax(vmax(cmax, up), x1);
    cmin = vmin(vmin(cmin, dn), x1);
  }
  __device__ __forceinline__ void store(double* __restrict__ stats, const PathStatsLayout& at, uint64_t col) const {
    stats[at.row(HH_STAT_CMAX_S) + col] = exp(cmax);
    stats[at.row(HH_STAT_CMIN_S) + col] = exp(cmin);
  }
};

}  // namespace
}  // namespace hh
