// Device-side check of hedgehog.jl_amd/csrc/hh_math.h, the code the GPU runs (hardware reciprocal, SGPR-constant
// fma, frexp / ldexp builtins, v_bitop3 sign flips).  tests/test_gpu_math_device.py holds the output to the bars.
//
//   arg / random_worst_ulp   fm::sqrt_lean against sqrt() as the device computes it: named arguments (bits), and
//                            the largest ulp distance over 10^6 random arguments in [2^-767, 2^1000]
//   sin … nquant             the host program's argument sets, measure and references (tests/c/math_cases.h),
//                            evaluated here: "name samples worst_ulp worst_argument_bits [second_argument_bits]"
//   rcp, div2sqrt,           device-only routines at the accuracy their comments claim, in the same format
//   sqrt_rough, exp_under
//   expfin_mismatch          arguments on which exp_finite and exp differ in a bit
//   special …                bits of exp / exp_finite, normal_quantile and atan2 at special arguments
//   div nq|atan2 …           one argument per line, its result's bits in three lane layouts: sorted by region,
//                            every wave holding all regions, a seeded shuffle
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "hh_math.h"
#include "math_cases.h"

using mc::bits;

__global__ void probe(const double* w, double* lean, double* ref, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  lean[i] = hh::fm::sqrt_lean(w[i]);
  ref[i] = sqrt(w[i]);
}

__global__ void k_sincos(const double* x, double* s, double* c, double* ns, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  hh::fm::sincos(x[i], s[i], c[i]);
  double wc;
  hh::fm::sincos_wide(x[i], ns[i], wc);
}
__global__ void k_wide(const double* x, double* s, double* c, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) hh::fm::sincos_wide(x[i], s[i], c[i]);
}
__global__ void k_exp(const double* x, double* e, double* ef, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  e[i] = hh::fm::exp(x[i]);
  ef[i] = hh::fm::exp_finite(x[i]);
}
__global__ void k_log(const double* x, double* l, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) l[i] = hh::fm::log(x[i]);
}
__global__ void k_atan2(const double* y, const double* x, double* a, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = hh::fm::atan2(y[i], x[i]);
}
__global__ void k_nq(const double* p, double* q, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) q[i] = hh::fm::normal_quantile(p[i]);
}
__global__ void k_rcp(const double* x, double* r, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) r[i] = hh::fm::rcp(x[i]);
}
__global__ void k_sqrt_rough(const double* x, double* r, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) r[i] = hh::fm::sqrt_rough(x[i]);
}
// t = sqrt_lean(w, &h), then a / (2t) from h
__global__ void k_div2sqrt(const double* a, const double* w, double* t, double* q, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double h;
  t[i] = hh::fm::sqrt_lean(w[i], &h);
  q[i] = hh::fm::div_by_2sqrt(a[i], t[i], h);
}

static bool ok = true;

// device buffers for host vectors; every call is checked, and the program stops at the first failure
struct Dev {
  std::vector<double*> ptrs;
  double* put(const std::vector<double>& v) {
    double* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(v.size(), 1) * 8) != hipSuccess) { ok = false; return nullptr; }
    ptrs.push_back(d);
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * 8, hipMemcpyHostToDevice) != hipSuccess) ok = false;
    return d;
  }
  double* out(size_t n) { return put(std::vector<double>(n, 0.0)); }
  void get(std::vector<double>& v, const double* d) {
    if (!v.empty() && hipMemcpy(v.data(), d, v.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) ok = false;
  }
  ~Dev() { for (double* p : ptrs) (void)hipFree(p); }
};
static dim3 blocks(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

static bool launched() {
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) ok = false;
  return ok;
}

static double from_bits(uint64_t b) {
  double x;
  memcpy(&x, &b, 8);
  return x;
}

// the pin of sqrt_lean
static int sqrt_lean_part() {
  Dev D;
  std::vector<double> w = {0.0,    4.9406564584124654e-324, 1e-310, 0x1p-1022, 0x1p-768, 0x1p-767, 0x1.8p-767, 1e-200,
                           0.25,   1.0,  2.0,  3.0,  1e300,  0x1.fffffffffffffp+1023, INFINITY, NAN, -1.0, -0.0, -1e-300};
  const int n_named = (int)w.size();
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 1000000; ++i) {  // mantissa and exponent uniformly over [2^-767, 2^1000)
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    const uint64_t e = 1023 - 767 + (s >> 11) % (767 + 1000);
    w.push_back(from_bits((e << 52) | (s & 0xFFFFFFFFFFFFFull)));
  }
  const int n = (int)w.size();
  double *dw = D.put(w), *dl = D.out(n), *dr = D.out(n);
  if (!ok) return 2;
  hipLaunchKernelGGL(probe, blocks(n), dim3(256), 0, 0, dw, dl, dr, n);
  if (!launched()) return 3;
  std::vector<double> l(n), r(n);
  D.get(l, dl);
  D.get(r, dr);
  if (!ok) return 3;
  for (int i = 0; i < n_named; ++i)
    printf("arg %016llx lean %016llx sqrt %016llx\n", (unsigned long long)bits(w[i]), (unsigned long long)bits(l[i]),
           (unsigned long long)bits(r[i]));
  long long worst = 0;
  for (int i = n_named; i < n; ++i) {
    const long long d = (long long)bits(l[i]) - (long long)bits(r[i]);
    if (llabs(d) > worst) worst = llabs(d);
  }
  printf("random_worst_ulp %lld\n", worst);
  return 0;
}

// the host program's sets and measure, and the special values it checks
static int shared_part() {
  Dev D;
  const mc::Args a = mc::make_args();
  mc::Out o;
  o.resize(a);
  const int n = (int)a.x.size(), nw = (int)a.wx.size(), ne = (int)a.ex.size(), nl = (int)a.lx.size(),
            nl1 = (int)a.lx1.size(), na = (int)a.ay.size(), nq = (int)a.p.size();
  double *x = D.put(a.x), *s = D.out(n), *c = D.out(n), *ns = D.out(n);
  double *wx = D.put(a.wx), *ws = D.out(nw), *wc = D.out(nw);
  double *ex = D.put(a.ex), *e = D.out(ne), *ef = D.out(ne);
  double *lx = D.put(a.lx), *l = D.out(nl), *lx1 = D.put(a.lx1), *l1 = D.out(nl1);
  double *ay = D.put(a.ay), *ax = D.put(a.ax), *at = D.out(na);
  double *p = D.put(a.p), *q = D.out(nq);
  std::vector<double> sx(mc::exp_specials(), mc::exp_specials() + mc::kExpSpecials);
  std::vector<double> sp(mc::nq_specials(), mc::nq_specials() + mc::kNqSpecials);
  // atan2 on the axes and diagonals, both signs of zero
  std::vector<double> sy, sxa;
  for (double yy : {0.0, -0.0, 1.0, -1.0})
    for (double xx : {0.0, -0.0, 1.0, -1.0})
      if (yy != 0.0 || xx != 0.0) { sy.push_back(yy); sxa.push_back(xx); }
  double *dsx = D.put(sx), *dse = D.out(sx.size()), *dsef = D.out(sx.size());
  double *dsp = D.put(sp), *dsq = D.out(sp.size());
  double *dsy = D.put(sy), *dsxa = D.put(sxa), *dsat = D.out(sy.size());
  if (!ok) return 2;
  hipLaunchKernelGGL(k_sincos, blocks(n), dim3(256), 0, 0, x, s, c, ns, n);
  hipLaunchKernelGGL(k_wide, blocks(nw), dim3(256), 0, 0, wx, ws, wc, nw);
  hipLaunchKernelGGL(k_exp, blocks(ne), dim3(256), 0, 0, ex, e, ef, ne);
  hipLaunchKernelGGL(k_log, blocks(nl), dim3(256), 0, 0, lx, l, nl);
  hipLaunchKernelGGL(k_log, blocks(nl1), dim3(256), 0, 0, lx1, l1, nl1);
  hipLaunchKernelGGL(k_atan2, blocks(na), dim3(256), 0, 0, ay, ax, at, na);
  hipLaunchKernelGGL(k_nq, blocks(nq), dim3(256), 0, 0, p, q, nq);
  hipLaunchKernelGGL(k_exp, blocks(sx.size()), dim3(256), 0, 0, dsx, dse, dsef, (int)sx.size());
  hipLaunchKernelGGL(k_nq, blocks(sp.size()), dim3(256), 0, 0, dsp, dsq, (int)sp.size());
  hipLaunchKernelGGL(k_atan2, blocks(sy.size()), dim3(256), 0, 0, dsy, dsxa, dsat, (int)sy.size());
  if (!launched()) return 3;
  D.get(o.s, s); D.get(o.c, c); D.get(o.ns, ns); D.get(o.ws, ws); D.get(o.wc, wc); D.get(o.e, e); D.get(o.ef, ef);
  D.get(o.l, l); D.get(o.l1, l1); D.get(o.at, at); D.get(o.q, q);
  std::vector<double> se(sx.size()), sef(sx.size()), sq(sp.size()), sat(sy.size());
  D.get(se, dse); D.get(sef, dsef); D.get(sq, dsq); D.get(sat, dsat);
  if (!ok) return 3;
  mc::Errors E = mc::measure(a, o);
  if (!mc::exp_specials_ok(se.data(), sef.data())) E.exp.take(1e9, NAN);
  if (!mc::nq_specials_ok(sq.data())) E.nquant.take(1e9, NAN);
  E.print();
  for (size_t i = 0; i < sx.size(); ++i)
    printf("special exp %016llx %016llx %016llx\n", (unsigned long long)bits(sx[i]), (unsigned long long)bits(se[i]),
           (unsigned long long)bits(sef[i]));
  for (size_t i = 0; i < sp.size(); ++i)
    printf("special nq %016llx %016llx\n", (unsigned long long)bits(sp[i]), (unsigned long long)bits(sq[i]));
  for (size_t i = 0; i < sy.size(); ++i)
    printf("special atan2 %016llx %016llx %016llx\n", (unsigned long long)bits(sy[i]), (unsigned long long)bits(sxa[i]),
           (unsigned long long)bits(sat[i]));
  return 0;
}

// routines only the device build has in their own form
static int device_only_part() {
  Dev D;
  std::mt19937_64 rng(2024);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  auto sgn = [&](double v) { return U(rng) < 0.5 ? -v : v; };
  // rcp: normal x with normal 1/x, |x| in [2^-1022, 2^1022]; the ends, powers of two, all-ones mantissas
  std::vector<double> rx = {0x1p-1022, 0x1p1022, -0x1p1022, 0x1.0000000000001p-1022, 0x1.fffffffffffffp1021, 1.0, 3.0,
                            0x1.fffffffffffffp-1, 0x1.0000000000001p0, -1.5, 0x1.fffffffffffffp0};
  for (int i = 0; i < 1000000; ++i) rx.push_back(sgn(std::ldexp(1.0 + U(rng), -1022 + (int)(2044.0 * U(rng)))));
  // div_by_2sqrt: w on sqrt_lean's domain [2^-767, 2^1000] (and zero's neighbour 2^-767 itself), a of any sign
  std::vector<double> dw = {0x1p-767, 1.0, 2.0, 0x1p1000, 0x1.fffffffffffffp999}, da = {1.0, 1.0, -3.0, 0x1p300, -1.0};
  for (int i = 0; i < 1000000; ++i) {
    dw.push_back(std::ldexp(1.0 + U(rng), -767 + (int)(1767.0 * U(rng))));
    da.push_back(sgn(std::ldexp(1.0 + U(rng), -300 + (int)(600.0 * U(rng)))));
  }
  // sqrt_rough: positive normal w
  std::vector<double> qw = {0x1p-1022, 1.0, 2.0, 0x1.fffffffffffffp1023};
  for (int i = 0; i < 1000000; ++i) qw.push_back(std::ldexp(1.0 + U(rng), -1022 + (int)(2045.0 * U(rng))));
  // exp's gradual underflow: x in [-745.2, -708]
  std::vector<double> ux = {-708.0, -708.3964185322641, -708.4, -709.0, -744.44007192138122, -745.0,
                            -745.13321910194110, -745.1332191019412, -745.2};
  for (int i = 0; i < 1000000; ++i) ux.push_back(-708.0 - 37.2 * U(rng));
  const int nr = (int)rx.size(), nd = (int)dw.size(), ns = (int)qw.size(), nu = (int)ux.size();
  double *drx = D.put(rx), *drr = D.out(nr);
  double *dda = D.put(da), *ddw = D.put(dw), *ddt = D.out(nd), *ddq = D.out(nd);
  double *dqw = D.put(qw), *dqr = D.out(ns);
  double *dux = D.put(ux), *due = D.out(nu), *duf = D.out(nu);
  if (!ok) return 2;
  hipLaunchKernelGGL(k_rcp, blocks(nr), dim3(256), 0, 0, drx, drr, nr);
  hipLaunchKernelGGL(k_div2sqrt, blocks(nd), dim3(256), 0, 0, dda, ddw, ddt, ddq, nd);
  hipLaunchKernelGGL(k_sqrt_rough, blocks(ns), dim3(256), 0, 0, dqw, dqr, ns);
  hipLaunchKernelGGL(k_exp, blocks(nu), dim3(256), 0, 0, dux, due, duf, nu);
  if (!launched()) return 3;
  std::vector<double> rr(nr), dt(nd), dq(nd), qr(ns), ue(nu), uf(nu);
  D.get(rr, drr); D.get(dt, ddt); D.get(dq, ddq); D.get(qr, dqr); D.get(ue, due); D.get(uf, duf);
  if (!ok) return 3;
  mc::Worst wr, wd, wq, wu;
  for (int i = 0; i < nr; ++i) wr.take(mc::ulp_err(rr[i], 1.0L / (long double)rx[i]), rx[i]);
  // the quotient by 2t, t the square root the routine returned (its own contract)
  for (int i = 0; i < nd; ++i) wd.take(mc::ulp_err(dq[i], (long double)da[i] / (2.0L * (long double)dt[i])), da[i], dw[i]);
  for (int i = 0; i < ns; ++i) {
    const long double want = sqrtl((long double)qw[i]);
    wq.take((double)(fabsl((long double)qr[i] - want) / want), qw[i]);
  }
  long long mism = 0;
  for (int i = 0; i < nu; ++i) {
    wu.take((double)(fabsl((long double)ue[i] - expl((long double)ux[i])) / 0x1p-1074L), ux[i]);
    mism += bits(ue[i]) != bits(uf[i]);
  }
  printf("rcp %d %.3f %016llx\n", nr, wr.err, (unsigned long long)bits(wr.arg));
  printf("div2sqrt %d %.3f %016llx %016llx\n", nd, wd.err, (unsigned long long)bits(wd.arg),
         (unsigned long long)bits(wd.arg2));
  printf("sqrt_rough %d %.6g %016llx\n", ns, wq.err, (unsigned long long)bits(wq.arg));
  printf("exp_under %d %.3f %016llx\n", nu, wu.err, (unsigned long long)bits(wu.arg));
  printf("expfin_mismatch %lld\n", mism);
  return 0;
}

// normal_quantile and atan2 with their regions sorted, interleaved and shuffled over the lanes
static int divergence_part() {
  Dev D;
  constexpr int kPer = 4096;
  std::mt19937_64 rng(77);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  auto side = [&](double tail) { return U(rng) < 0.5 ? tail : 1.0 - tail; };
  // regions of normal_quantile: body |p - 1/2| <= 0.425; tail with r = sqrt(-log tail) <= 5 (tail >= e^-25);
  // far tail below e^-25 (the upper side no further than 1 - p = 2^-53)
  std::vector<double> p[3], y[3], x[3];
  for (int i = 0; i < kPer; ++i) {
    p[0].push_back(0.075 + 0.85 * U(rng));
    p[1].push_back(side(std::exp(-(2.6 + 22.3 * U(rng)))));
    const double far = std::exp(-(25.2 + 665.0 * U(rng)));
    p[2].push_back(U(rng) < 0.5 ? far : 1.0 - std::max(far, 0x1p-53));
  }
  // regions of atan2: min/max >= 7/16; |y| < 7/16 |x|; |x| < 7/16 |y| — each with both signs of x and y
  for (int i = 0; i < kPer; ++i) {
    const double m = std::exp2(-20.0 + 40.0 * U(rng));
    const double t[3] = {0.4375 + 0.5625 * U(rng), 0.4375 * U(rng), 0.4375 * U(rng)};
    for (int r = 0; r < 3; ++r) {
      const double big = m, small = m * t[r];
      const double yy = r == 2 ? big : small, xx = r == 2 ? small : big;
      y[r].push_back(U(rng) < 0.5 ? -yy : yy);
      x[r].push_back(U(rng) < 0.5 ? -xx : xx);
    }
  }
  const int n = 3 * kPer;
  // layout -> case index at each lane
  std::vector<int> lay[3];
  for (int i = 0; i < n; ++i) lay[0].push_back(i);                              // sorted: region r at r·kPer …
  for (int i = 0; i < n; ++i) lay[1].push_back((i % 3) * kPer + i / 3);         // every wave holds all regions
  lay[2] = lay[0];
  std::shuffle(lay[2].begin(), lay[2].end(), std::mt19937_64(99));
  std::vector<double> pin[3], yin[3], xin[3];
  auto flat = [&](const std::vector<double>* v, int i) { return v[i / kPer][i % kPer]; };
  for (int L = 0; L < 3; ++L)
    for (int i = 0; i < n; ++i) {
      pin[L].push_back(flat(p, lay[L][i]));
      yin[L].push_back(flat(y, lay[L][i]));
      xin[L].push_back(flat(x, lay[L][i]));
    }
  double *dp[3], *dq[3], *dy[3], *dx[3], *da[3];
  for (int L = 0; L < 3; ++L) {
    dp[L] = D.put(pin[L]); dq[L] = D.out(n); dy[L] = D.put(yin[L]); dx[L] = D.put(xin[L]); da[L] = D.out(n);
  }
  if (!ok) return 2;
  for (int L = 0; L < 3; ++L) {
    hipLaunchKernelGGL(k_nq, blocks(n), dim3(256), 0, 0, dp[L], dq[L], n);
    hipLaunchKernelGGL(k_atan2, blocks(n), dim3(256), 0, 0, dy[L], dx[L], da[L], n);
  }
  if (!launched()) return 3;
  std::vector<double> q[3], a[3];
  for (int L = 0; L < 3; ++L) {
    q[L].resize(n); a[L].resize(n);
    D.get(q[L], dq[L]); D.get(a[L], da[L]);
  }
  if (!ok) return 3;
  std::vector<uint64_t> qb[3], ab[3];  // by case
  for (int L = 0; L < 3; ++L) {
    qb[L].resize(n); ab[L].resize(n);
    for (int i = 0; i < n; ++i) {
      qb[L][lay[L][i]] = bits(q[L][i]);
      ab[L][lay[L][i]] = bits(a[L][i]);
    }
  }
  for (int i = 0; i < n; ++i)
    printf("div nq %d %016llx %016llx %016llx %016llx\n", i / kPer, (unsigned long long)bits(flat(p, i)),
           (unsigned long long)qb[0][i], (unsigned long long)qb[1][i], (unsigned long long)qb[2][i]);
  for (int i = 0; i < n; ++i)
    printf("div atan2 %d %016llx %016llx %016llx %016llx %016llx\n", i / kPer, (unsigned long long)bits(flat(y, i)),
           (unsigned long long)bits(flat(x, i)), (unsigned long long)ab[0][i], (unsigned long long)ab[1][i],
           (unsigned long long)ab[2][i]);
  return 0;
}

int main() {
  int rc = sqrt_lean_part();
  if (rc == 0) rc = shared_part();
  if (rc == 0) rc = device_only_part();
  if (rc == 0) rc = divergence_part();
  return rc;
}
