// The monitored statistics of a trajectory and its mirror (enum hh_path_stat), stated once for the kernels that keep
// them on log spots: path_stats_kernel (hh_path.hip), jump_stats_kernel (hh_jump.hip), qe_stats_kernel (hh_qe.hip),
// bates_stats_kernel (hh_bates.hip), localvol_stats_kernel (hh_localvol.hip) and vg_stats_kernel (hh_vg.hip).  Running is
// the arithmetic of the five rows, Monitor the dates they are taken on, Extremes the two rows of the bridge form; a kernel
// supplies its states, its step and the call after it.  DateRows is the second sink of the same walks: each kernel takes its
// sink as its last template parameter (Monitor by default) and, instantiated on DateRows, leaves the dates themselves
// (hh_mc_path_grid); the three walks that hold a variance take StateRows as well and leave (x, v) per date
// (hh_mc_path_states).  assets_stats_kernel (hh_assets.hip) uses Running and writes the dates out itself (its head
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
  static constexpr bool kStates = false;  // reads the log spots alone (StateRows: the variance beside them)
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
  static constexpr bool kStates = false;
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

// The third sink, of the walks that hold a variance beside the log spot (HestonModel's Euler step, the QE step, Bates):
// every date's STATE goes out, x and v as the walk holds them — the raw registers: no exp, and on Euler the variance
// before any clipping (the step clips where it reads) — into the date-major, then state-major rows
// rows[(date·2 + state)·n_total + column] of hh_assets_rows_elems at d = 2, state 0 = x, state 1 = v: the layout of
// assets_rows_kernel, so the several-variable induction reads them as it reads those.  Row 0 is (log S0, V0) by plain
// stores, the later rows nontemporal, the mirror of trajectory i in column n_paths + i: DateRows' access pattern, two
// rows per date — a wave's store is 512 contiguous bytes per date, state and member.  A kernel hands the variances to
// start / date behind `if constexpr (Sink::kStates)`: the other sinks' instantiations do not see them.
template <bool ANTI>
struct StateRows {
  static constexpr bool kStats = false;
  static constexpr bool kStates = true;
  const uint32_t every;
  uint32_t left;
  double* next = nullptr;  // column i of state 0 of the next date
  size_t n_total = 0, mirror = 0;
  __device__ __forceinline__ StateRows(uint32_t exercise_every, int) : every(exercise_every), left(exercise_every) {}
  __device__ __forceinline__ void bind(double* __restrict__ rows, uint64_t i, uint64_t n_paths) {
    next = rows + i;
    n_total = (size_t)(ANTI ? 2 * n_paths : n_paths);
    mirror = (size_t)n_paths;
  }
  __device__ __forceinline__ void start(double x0, double v0) {
    next[0] = x0;
    next[n_total] = v0;
    if constexpr (ANTI) {
      next[mirror] = x0;
      next[n_total + mirror] = v0;
    }
    next += 2 * n_total;
  }
  __device__ __forceinline__ void date(const double& x, const double& xa, const double& v, const double& va) {
    if (--left != 0u) return;
    left = every;
    __builtin_nontemporal_store(x, next);
    __builtin_nontemporal_store(v, next + n_total);
    if constexpr (ANTI) {
      __builtin_nontemporal_store(xa, next + mirror);
      __builtin_nontemporal_store(va, next + n_total + mirror);
    }
    next += 2 * n_total;
  }
  __device__ __forceinline__ void store(double* __restrict__, const PathStatsLayout&, uint64_t, uint64_t) const {}
};

// The statistics of one member WITH their tangents along P carried basis slots (path_tangent_kernel, hh_path.hip;
// PathTangentLayout).  The five values go through Running, in its order: rows 0-4 are Monitor's bit for bit.  Beside them
// the date rows — k_max, k_min: the step index of the date that holds the extreme; sum_ks = Σ k_j·S_j — and per slot
// Σ S·dx, Σ dx, S·dx at the two extremes and at the last date, dx = ∂x/∂(the slot's parameter) on that date.
// TIE RULE: an extreme's tangent and index follow its value: they are replaced exactly when the new S is STRICTLY
// greater (less) than the running extreme, so the first of equal dates holds it.  The comparison is made once, before
// Running::next, whose vmax / vmin still give the value.
template <int P>
struct RunningTangent {
  static constexpr int N = P > 0 ? P : 1;
  Running r;
  double k_max = 0.0, k_min = 0.0, sum_ks = 0.0;
  double dsum_s[N], dsum_x[N], dmax_s[N], dmin_s[N], ds_t[N];
  __device__ __forceinline__ void first(double S, double x, double k, const double (&dx)[N]) {
    r.first(S, x);
    k_max = k;
    k_min = k;
    sum_ks = k * S;
#pragma unroll
    for (int b = 0; b < P; ++b) {
      const double t = S * dx[b];
      dsum_s[b] = t;
      dsum_x[b] = dx[b];
      dmax_s[b] = t;
      dmin_s[b] = t;
      ds_t[b] = t;
    }
  }
  __device__ __forceinline__ void next(double S, double x, double k, const double (&dx)[N]) {
    const bool up = S > r.max_s, dn = S < r.min_s;
    r.next(S, x);
    k_max = up ? k : k_max;
    k_min = dn ? k : k_min;
    sum_ks = fma(k, S, sum_ks);
#pragma unroll
    for (int b = 0; b < P; ++b) {
      const double t = S * dx[b];
      dsum_s[b] = dsum_s[b] + t;
      dsum_x[b] = dsum_x[b] + dx[b];
      dmax_s[b] = up ? t : dmax_s[b];
      dmin_s[b] = dn ? t : dmin_s[b];
      ds_t[b] = t;
    }
  }
  // plain stores, for the reason Running::store gives: path_payoff_tangent_kernel reads the rows straight back
  __device__ __forceinline__ void store(double* __restrict__ rows, const PathTangentLayout& at, uint64_t col) const {
    rows[at.row(HH_STAT_SUM_S) + col] = r.sum_s;
    rows[at.row(HH_STAT_SUM_X) + col] = r.sum_x;
    rows[at.row(HH_STAT_MAX_S) + col] = r.max_s;
    rows[at.row(HH_STAT_MIN_S) + col] = r.min_s;
    rows[at.row(HH_STAT_S_T) + col] = r.s_t;
    rows[at.row(HH_TANGENT_K_MAX) + col] = k_max;
    rows[at.row(HH_TANGENT_K_MIN) + col] = k_min;
    rows[at.row(HH_TANGENT_SUM_KS) + col] = sum_ks;
#pragma unroll
    for (int b = 0; b < P; ++b) {
      rows[at.slot_row(b, HH_TANGENT_DSUM_S) + col] = dsum_s[b];
      rows[at.slot_row(b, HH_TANGENT_DSUM_X) + col] = dsum_x[b];
      rows[at.slot_row(b, HH_TANGENT_DMAX_S) + col] = dmax_s[b];
      rows[at.slot_row(b, HH_TANGENT_DMIN_S) + col] = dmin_s[b];
      rows[at.slot_row(b, HH_TANGENT_DS_T) + col] = ds_t[b];
    }
  }
};

// Monitor with the tangents: its dates, its include_start rule and its "first term starts the sum" rule, on the dual log
// spots of the trajectory and (ANTI) of the mirror.  k counts the steps taken, as a double (exact: n_steps < 2^53).  The
// start's basis tangents are zero: no carried parameter reaches log S0.
template <int P, bool ANTI>
struct TangentMonitor {
  static constexpr int N = P > 0 ? P : 1;
  const uint32_t every;
  uint32_t left;
  bool started;
  double k = 0.0;
  RunningTangent<P> ra, r;
  __device__ __forceinline__ TangentMonitor(uint32_t monitor_every, int include_start)
      : every(monitor_every), left(monitor_every), started(include_start != 0) {}
  __device__ __forceinline__ void start(double S0, double x0) {
    if (!started) return;
    double zero[N];
#pragma unroll
    for (int b = 0; b < N; ++b) zero[b] = 0.0;
    r.first(S0, x0, 0.0, zero);
    if constexpr (ANTI) ra.first(S0, x0, 0.0, zero);
  }
  __device__ __forceinline__ void date(const DualT<P>& x, const DualT<P>& xa) {
    if (--left != 0u) return;
    left = every;
    k += (double)every;
    const double S = exp(x.v);
    if (started) r.next(S, x.v, k, x.d);
    else r.first(S, x.v, k, x.d);
    if constexpr (ANTI) {
      const double Sa = exp(xa.v);
      if (started) ra.next(Sa, xa.v, k, xa.d);
      else ra.first(Sa, xa.v, k, xa.d);
    }
    started = true;
  }
  __device__ __forceinline__ void store(double* __restrict__ rows, const PathTangentLayout& at, uint64_t i,
                                        uint64_t n_paths) const {
    r.store(rows, at, i);
    if constexpr (ANTI) ra.store(rows, at, n_paths + i);
  }
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
