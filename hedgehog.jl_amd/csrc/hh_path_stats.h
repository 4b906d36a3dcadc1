// The running statistics of one trajectory (enum hh_path_stat), shared by the kernels that keep them: path_stats_kernel
// (hh_path.hip) and its jump form (hh_jump.hip).  Internal.
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

}  // namespace
}  // namespace hh
