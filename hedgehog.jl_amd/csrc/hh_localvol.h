// Local volatility on a tabulated surface σ(t, x), x = log S (include/hedgehog_mc.h, "Local volatility on a tabulated
// surface" — every operation is stated there in this order): the per-step row and weight the host forms once per call,
// the bilinear lookup and the log-Euler step with the σ of that step, as functions the device kernel (hh_localvol.hip)
// and a host program share — a host compiler sees nothing of HIP in it, so that tests/c/localvol_host_check.cpp can hold
// them to long-double evaluations and run them under the host sanitizers.  Every operation is one rounded fp64 operation
// (the library is built with -ffp-contract=off).  Internal; the public surface is include/hedgehog_mc.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/hedgehog_mc.h"

#if defined(__HIPCC__)
#define HH_LV_HD __host__ __device__
#else
#define HH_LV_HD
#endif

namespace hh {

// The surface of a launch, passed BY VALUE beside SimArgs (wave-uniform: scalar registers).  The three arrays are one
// device block, the table first (localvol_stage_doubles).
struct LocalVolArgs {
  const double* vols;        // device, [n_times][n_x]: the table the workgroup copies into LDS
  const double* step_w;      // device, [n_steps]: w_k
  const uint32_t* step_row;  // device, [n_steps]: j_k
  double x_lo, inv_h;        // the log-spot grid: x_i = x_lo + i·h;  inv_h = 1/h, formed on the host once
  uint32_t n_times, n_x;
};

// The host's part: row j_k and weight w_k of step k, t_k = (double)k·dt.  j_k is the largest j with times[j] <= t_k,
// clamped to [0, max(n_times − 2, 0)]; w_k = (t_k − times[j])/(times[j+1] − times[j]) clamped to [0, 1], and 0 for a
// one-row table: constant before times[0] and after times[n_times − 1].
struct LocalVolRow {
  uint32_t j;
  double w;
};
inline LocalVolRow localvol_row(const double* times, uint32_t n_times, double t) {
  LocalVolRow r{0u, 0.0};
  if (n_times < 2u) return r;
  while (r.j + 2u < n_times && times[r.j + 1u] <= t) ++r.j;
  double w = (t - times[r.j]) / (times[r.j + 1u] - times[r.j]);
  w = w < 0.0 ? 0.0 : w;
  w = w > 1.0 ? 1.0 : w;
  r.w = w;
  return r;
}

// doubles of the staged block: the table, the weights, then the rows as packed uint32
inline size_t localvol_stage_doubles(uint32_t n_times, uint32_t n_x, uint32_t n_steps) {
  return (size_t)n_times * n_x + (size_t)n_steps + ((size_t)n_steps + 1u) / 2u;
}

// The cell of log spot x: u = (x − x_lo)·(1/h) clamped to [0, n_x − 1] (constant extrapolation), i = min((uint32)u,
// n_x − 2), f = u − i.  x is finite.
struct LocalVolCell {
  uint32_t i;
  double f;
};
HH_LV_HD inline __attribute__((always_inline)) LocalVolCell localvol_cell(double x, double x_lo, double inv_h, uint32_t n_x) {
  double u = (x - x_lo) * inv_h;
  const double top = (double)(n_x - 1u);
  u = u < 0.0 ? 0.0 : u;
  u = u > top ? top : u;
  LocalVolCell c;
  c.i = (uint32_t)u;
  c.i = c.i < n_x - 2u ? c.i : n_x - 2u;
  c.f = u - (double)c.i;
  return c;
}

// σ of the cell: rows a = j_k and b = j_k + 1 blended in time first, then in x.  two_rows = false (a one-row table)
// reads row a alone: fma(0, ·, a_i) = a_i, the same bits.
template <class Row>
HH_LV_HD inline __attribute__((always_inline)) double localvol_sigma(Row a, Row b, bool two_rows, const LocalVolCell& c, double w) {
  double c0 = a[c.i], c1 = a[c.i + 1u];
  if (two_rows) {
    c0 = fma(w, b[c.i] - c0, c0);
    c1 = fma(w, b[c.i + 1u] - c1, c1);
  }
  return fma(c.f, c1 - c0, c0);
}

// GbmModel::step with the σ and g = r − σ²/2 of this step (g as make_args writes gdrift)
HH_LV_HD inline __attribute__((always_inline)) double localvol_step(double x, double sigma, double r, double dt, double dW) {
  const double sig2h = 0.5 * sigma * sigma;
  const double g = r - sig2h;
  return fma(sigma, dW, fma(dt, g, x));
}

}  // namespace hh
