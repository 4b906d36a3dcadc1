// The argument sets, error measure and 80-bit references of the hh_math.h accuracy checks, shared by the host
// program (tests/c/math_check.cpp, g++) and the device program (tests/c/math_device_check.hip), so that both
// measure the same thing on the same arguments.  Host code only: the device program generates here, evaluates on
// the GPU and measures here.
//
// Output, one line per routine: "name samples worst_ulp worst_argument_bits [second_argument_bits]".
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace mc {

inline double ulp_err(double got, long double want) {
  if (want == 0.0L) return got == 0.0 ? 0.0 : 1e9;
  int e;
  std::frexp((double)want, &e);
  const long double ulp = std::ldexp(1.0L, e - 53);
  return (double)(fabsl((long double)got - want) / ulp);
}

// sin / cos: ulp of the result, absolute 2^-73 where the value is below 1e-6 (the CF uses both components at O(1)
// magnitude together)
inline double sc_err(double got, long double want) {
  return fabsl(want) > 1e-6L ? ulp_err(got, want) : (double)(fabsl(got - want) / 1.2e-22L);
}

inline uint64_t bits(double x) {
  uint64_t b;
  std::memcpy(&b, &x, 8);
  return b;
}

// the normal quantile's reference: an 80-bit Newton refinement of Φ(x) = p from x0, Φ by erfcl
inline long double nq_ref(double p, double x0) {
  long double x = x0;
  for (int it = 0; it < 4; ++it) {
    const long double phi = expl(-0.5L * x * x) / sqrtl(2.0L * 3.14159265358979323846264338327950288L);
    // Φ(x) - p; in the upper half from the complements, 1 - p being exact and erfcl free of cancellation there
    const long double res = p < 0.5 ? 0.5L * erfcl(-x / sqrtl(2.0L)) - (long double)p
                                    : (1.0L - (long double)p) - 0.5L * erfcl(x / sqrtl(2.0L));
    x -= res / phi;
  }
  return x;
}

// near p = 1/2 the quantile passes through 0: absolute there
inline double nq_err(double got, long double x) {
  return fabsl(x) > 1e-3L ? ulp_err(got, x) : (double)(fabsl((long double)got - x) / 2.2e-19L);
}

constexpr int kN = 2000000;    // arguments per routine
constexpr int kNq = 400000;    // draws of the normal quantile (the invalid ones are skipped)

struct Args {
  std::vector<double> x;       // sincos, |x| <= 2^20 (and sincos_wide, which must agree there)
  std::vector<double> wx;      // sincos_wide, 2^18 <= |x| <= 2^45
  std::vector<double> ex;      // exp, exp_finite
  std::vector<double> lx, lx1; // log: 2^±600, and around 1
  std::vector<double> ay, ax;  // atan2: random, then the axes and diagonals
  std::vector<double> p;       // normal_quantile
};

inline Args make_args() {
  Args a;
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  for (int i = 0; i < kN; ++i) {
    // angles: dense near 0, up to +-2^20 on a log scale
    const double mag = std::exp2(-30.0 + 50.0 * U(rng));
    a.x.push_back(U(rng) < 0.5 ? -mag : mag);
    // the wide reduction: up to +-2^45, where an angle still determines its sine to ~1e-3
    const double wm = std::exp2(18.0 + 27.0 * U(rng));
    a.wx.push_back(U(rng) < 0.5 ? -wm : wm);
    const double ex = (U(rng) < 0.1 ? 1400.0 : 60.0) * (U(rng) - 0.5) * (U(rng) < 0.3 ? std::exp2(-20.0 * U(rng)) : 1.0);
    a.ex.push_back(ex);
    a.lx.push_back(std::exp2(-600.0 + 1200.0 * U(rng)) * (1.0 + U(rng)));
    a.lx1.push_back(1.0 + (U(rng) - 0.5) * std::exp2(-40.0 * U(rng)));  // around 1
    const double r = std::exp2(-40.0 + 80.0 * U(rng)), ph = 6.283185307179586 * U(rng);
    a.ay.push_back(r * std::sin(ph) * std::exp2(-30.0 * U(rng) * (U(rng) < 0.3)));
    a.ax.push_back(r * std::cos(ph));
  }
  // the normal quantile: body, both tails, far tails
  for (int i = 0; i < kNq; ++i) {
    double p = U(rng);
    if (i % 4 == 1) p = std::exp2(-1000.0 * U(rng));            // far lower tail (third region below 1.4e-11)
    if (i % 4 == 2) p = 1.0 - std::exp2(-52.0 * U(rng));         // upper tail up to 1 - 2^-52
    if (!(p > 0.0 && p < 1.0)) continue;
    a.p.push_back(p);
  }
  // axes and diagonals
  const double pts[][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1},
                           {0.4375, 1}, {0.6875, 1}, {1, 0.4375}, {1e-300, 1}, {1, 1e-300}};
  for (auto& q : pts) {
    a.ay.push_back(q[0]);
    a.ax.push_back(q[1]);
  }
  return a;
}

// results of the routines on Args, in the same order
struct Out {
  std::vector<double> s, c;      // sincos(x)
  std::vector<double> ws, wc;    // sincos_wide(wx)
  std::vector<double> ns;        // sin of sincos_wide(x)
  std::vector<double> e, ef;     // exp(ex), exp_finite(ex)
  std::vector<double> l, l1;     // log(lx), log(lx1)
  std::vector<double> at;        // atan2(ay, ax)
  std::vector<double> q;         // normal_quantile(p)
  void resize(const Args& a) {
    s.resize(a.x.size()); c.resize(a.x.size()); ns.resize(a.x.size());
    ws.resize(a.wx.size()); wc.resize(a.wx.size());
    e.resize(a.ex.size()); ef.resize(a.ex.size());
    l.resize(a.lx.size()); l1.resize(a.lx1.size());
    at.resize(a.ay.size()); q.resize(a.p.size());
  }
};

// the largest error of one routine and the argument(s) it was met at
struct Worst {
  double err = 0.0, arg = 0.0, arg2 = 0.0;
  void take(double e, double x, double y = 0.0) {
    if (!(e <= err)) { err = e; arg = x; arg2 = y; }  // (a NaN error is the worst of all)
  }
};

// The measure of tests/test_math_host.py; special values are checked by the callers (an exp / normal-quantile
// special out of place sets that routine's error to 1e9).
struct Errors {
  Worst sin, cos, log, atan2, exp, wsin, wcos, nquant;
  void print() const {
    auto one = [](const char* name, int n, const Worst& w, bool two) {
      if (two)
        std::printf("%s %d %.3f %016llx %016llx\n", name, n, w.err, (unsigned long long)bits(w.arg),
                    (unsigned long long)bits(w.arg2));
      else
        std::printf("%s %d %.3f %016llx\n", name, n, w.err, (unsigned long long)bits(w.arg));
    };
    one("sin", kN, sin, false); one("cos", kN, cos, false); one("log", kN, log, false);
    one("atan2", kN, atan2, true); one("exp", kN, exp, false); one("wsin", kN, wsin, false);
    one("wcos", kN, wcos, false); one("nquant", kNq, nquant, false);
  }
};

inline Errors measure(const Args& a, const Out& o) {
  Errors E;
  for (size_t i = 0; i < a.x.size(); ++i) {
    const double x = a.x[i];
    const long double ws = sinl((long double)x), wc = cosl((long double)x);
    E.sin.take(sc_err(o.s[i], ws), x);
    E.cos.take(sc_err(o.c[i], wc), x);
    E.wsin.take(sc_err(o.ns[i], ws), x);  // the wide form agrees with the narrow one on the narrow range
  }
  for (size_t i = 0; i < a.wx.size(); ++i) {
    const double wx = a.wx[i];
    E.wsin.take(sc_err(o.ws[i], sinl((long double)wx)), wx);
    E.wcos.take(sc_err(o.wc[i], cosl((long double)wx)), wx);
  }
  for (size_t i = 0; i < a.ex.size(); ++i) {
    const long double we = expl((long double)a.ex[i]);
    if (we > 1e-300L && we < 1e300L) E.exp.take(ulp_err(o.e[i], we), a.ex[i]);
    if (o.ef[i] != o.e[i]) E.exp.take(1e9, a.ex[i]);  // the form without clamp and NaN select: the same bits
  }
  for (size_t i = 0; i < a.lx.size(); ++i) E.log.take(ulp_err(o.l[i], logl((long double)a.lx[i])), a.lx[i]);
  for (size_t i = 0; i < a.lx1.size(); ++i) {
    const double x = a.lx1[i];
    E.log.take(std::fabs(x - 1.0) > 1e-300 ? ulp_err(o.l1[i], logl((long double)x)) : 0.0, x);
  }
  for (size_t i = 0; i < a.ay.size(); ++i)
    E.atan2.take(ulp_err(o.at[i], atan2l((long double)a.ay[i], (long double)a.ax[i])), a.ay[i], a.ax[i]);
  for (size_t i = 0; i < a.p.size(); ++i) E.nquant.take(nq_err(o.q[i], nq_ref(a.p[i], o.q[i])), a.p[i]);
  return E;
}

// saturation and special values of exp, at these arguments
constexpr int kExpSpecials = 6;
inline const double* exp_specials() {
  static const double v[kExpSpecials] = {-2000.0, 2000.0, NAN, -1e6, 0.0, -745.0};
  return v;
}
// e[i] = exp(exp_specials()[i]), ef[i] = exp_finite(...)
inline bool exp_specials_ok(const double* e, const double* ef) {
  const bool fin = ef[0] == 0.0 && std::isinf(ef[1]) && std::isnan(ef[2]) && ef[3] == 0.0;
  const bool ful = e[0] == 0.0 && std::isinf(e[1]) && e[4] == 1.0 && std::isnan(e[2]) && e[5] > 0.0;
  return fin && ful;
}

// the normal quantile at 0, 1, NaN and 1/2
constexpr int kNqSpecials = 4;
inline const double* nq_specials() {
  static const double v[kNqSpecials] = {0.0, 1.0, NAN, 0.5};
  return v;
}
inline bool nq_specials_ok(const double* q) {
  return q[0] < -1e300 && q[1] > 1e300 && std::isnan(q[2]) && q[3] == 0.0;
}

}  // namespace mc
