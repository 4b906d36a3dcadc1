// Heston paths by Andersen's quadratic-exponential scheme for gfx950 (wave64, fp64 VALU): include/hedgehog_mc.h,
// "Heston paths by the quadratic-exponential scheme" — the step, the draws and the host-formed constants are stated
// there in full; the step's arithmetic lives in hh_qe.h, shared with a host program.
//
//   qe_stats_kernel<ANTI, MART>  path_stats_kernel's monitored form with the QE step in place of the Euler step: one
//                                trajectory per lane and its mirror in the same lane, the same dates and Running
//                                arithmetic (hh_path_stats.h), the same five rows.  Its output goes through
//                                path_payoff_kernel untouched.  var_T (nullable): the variance at expiry of each member.
//
// The constants travel in QeArgs beside SimArgs<0>, whose layout stays as it is.  Every loop is bounded by n_steps; none
// by data.  The two branches diverge within a wave, and block (k, 1, 0, kDomQe) is drawn only by a lane one of whose
// members is in the exponential branch at step k — a branch, not a select over a block every lane would pay for.
#include "hh_path_stats.h"
#include "hh_qe.h"
#include "hh_sim.h"

namespace hh {
namespace {

struct QeState {
  double x, v;
};

// (x, v) -> (x′, v′) of one member: its own moments mo, its own normals and — exponential branch only — its own U
template <bool MART>
__device__ __forceinline__ void qe_member_step(QeState& s, const QeArgs& q, const QeMoments& mo, bool quad, double zv,
                                               double zx, double U) {
  double vn, k0 = q.K0;
  if (quad) {
    const QeQuad b = qe_quad(mo);
    vn = qe_quad_next(b, zv);
    if constexpr (MART) k0 = qe_k0_star(q, qe_quad_lnM(b, q.A), s.v);
  } else {
    const QeExp e = qe_exp(mo);
    vn = qe_exp_next(e, U);
    if constexpr (MART) k0 = qe_k0_star(q, qe_exp_lnM(e, q.A), s.v);
  }
  s.x = qe_log_spot(q, s.x, s.v, vn, k0, zx);
  s.v = vn;
}

template <bool ANTI, bool MART>
__global__ __launch_bounds__(256) void qe_stats_kernel(const SimArgs<0> a, const QeArgs q, const double S0,
                                                       const uint32_t monitor_every, const int include_start,
                                                       double* __restrict__ stats, double* __restrict__ var_T) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_paths) return;
  const PathStatsLayout at(a.n_paths, ANTI, HH_PATH_STATS);
  const uint32_t n_steps = a.n_steps;
  QeState st{a.x0.v, a.v0.v}, sa{a.x0.v, a.v0.v};
  Running r, ra;
  bool started = include_start != 0;
  if (started) {
    r.first(S0, a.x0.v);
    if constexpr (ANTI) ra.first(S0, a.x0.v);
  }
  uint32_t left = monitor_every;
  const uint64_t key = a.seeds[i];
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  for (uint32_t k = 0; k < n_steps; ++k) {
    double zv, zx;
    normal_pair(key, k, 0u, 0u, kDomQe, zv, zx);
    const QeMoments mo = qe_moments(q, st.v);
    const bool quad = mo.psi <= q.psi_c;
    QeMoments moa = mo;
    bool quada = true;
    if constexpr (ANTI) {
      moa = qe_moments(q, sa.v);
      quada = moa.psi <= q.psi_c;
    }
    double U = 0.5;  // read by a member in the exponential branch only
    if (!quad || !quada) {
      const Philox4 b = philox4x32_10(k, 1u, 0u, kDomQe, k0, k1);
      U = u01_fast(b.c0, b.c1);
    }
    qe_member_step<MART>(st, q, mo, quad, zv, zx, U);
    if constexpr (ANTI) qe_member_step<MART>(sa, q, moa, quada, -zv, -zx, 1.0 - U);  // 1 − U is exact
    if (--left == 0u) {
      left = monitor_every;
      const double S = exp(st.x);
      if (started) r.next(S, st.x);
      else r.first(S, st.x);
      if constexpr (ANTI) {
        const double Sa = exp(sa.x);
        if (started) ra.next(Sa, sa.x);
        else ra.first(Sa, sa.x);
      }
      started = true;
    }
  }
  r.store(stats, at, i);
  if (var_T) var_T[i] = st.v;
  if constexpr (ANTI) {
    ra.store(stats, at, a.n_paths + i);
    if (var_T) var_T[a.n_paths + i] = sa.v;
  }
}

}  // namespace

QeArgs qe_launch_args(const hh_model& m, const hh_config& c, const hh_qe& qe) {
  return qe_args(m.kappa, m.theta, m.sigma, m.rho, m.r_drift, m.T / (double)c.n_steps, qe.psi_c);
}

int launch_qe_stats(const hh_model& m, const hh_config& c, const hh_qe& qe, const uint64_t* seeds_dev,
                    uint32_t monitor_every, bool include_start, double* stats, double* var_T, hipStream_t s) {
  DevicePtrs p{};
  p.seeds = seeds_dev;
  const SimArgs<0> a = make_args0(m, c, p);
  const QeArgs q = qe_launch_args(m, c, qe);
  const dim3 g((unsigned)((c.n_paths + 255) / 256)), blk(256);
  const bool anti = c.antithetic != 0, mart = qe.martingale != 0;
  auto kernel = anti ? (mart ? qe_stats_kernel<true, true> : qe_stats_kernel<true, false>)
                     : (mart ? qe_stats_kernel<false, true> : qe_stats_kernel<false, false>);
  hipLaunchKernelGGL(kernel, g, blk, 0, s, a, q, m.S0, monitor_every, (int)include_start, stats, var_T);
  return (int)hipGetLastError();
}

}  // namespace hh
