// Host-side accuracy check of hedgehog.jl_amd/csrc/hh_math.h against 80-bit libm.
// Prints one line per function: name, samples, max error in ulp of the fp64 result, the argument it was met at.
// The arguments, the measure and the references are those of tests/c/math_cases.h, which the device program
// (tests/c/math_device_check.hip) shares.
#include "math_cases.h"

#include "hh_math.h"

int main() {
  const mc::Args a = mc::make_args();
  mc::Out o;
  o.resize(a);
  for (size_t i = 0; i < a.x.size(); ++i) {
    hh::fm::sincos(a.x[i], o.s[i], o.c[i]);
    double wc;
    hh::fm::sincos_wide(a.x[i], o.ns[i], wc);
  }
  for (size_t i = 0; i < a.wx.size(); ++i) hh::fm::sincos_wide(a.wx[i], o.ws[i], o.wc[i]);
  for (size_t i = 0; i < a.ex.size(); ++i) {
    o.e[i] = hh::fm::exp(a.ex[i]);
    o.ef[i] = hh::fm::exp_finite(a.ex[i]);
  }
  for (size_t i = 0; i < a.lx.size(); ++i) o.l[i] = hh::fm::log(a.lx[i]);
  for (size_t i = 0; i < a.lx1.size(); ++i) o.l1[i] = hh::fm::log(a.lx1[i]);
  for (size_t i = 0; i < a.ay.size(); ++i) o.at[i] = hh::fm::atan2(a.ay[i], a.ax[i]);
  for (size_t i = 0; i < a.p.size(); ++i) o.q[i] = hh::fm::normal_quantile(a.p[i]);
  mc::Errors E = mc::measure(a, o);
  double e[mc::kExpSpecials], ef[mc::kExpSpecials], q[mc::kNqSpecials];
  for (int i = 0; i < mc::kExpSpecials; ++i) {
    e[i] = hh::fm::exp(mc::exp_specials()[i]);
    ef[i] = hh::fm::exp_finite(mc::exp_specials()[i]);
  }
  for (int i = 0; i < mc::kNqSpecials; ++i) q[i] = hh::fm::normal_quantile(mc::nq_specials()[i]);
  if (!mc::exp_specials_ok(e, ef)) E.exp.take(1e9, NAN);
  if (!mc::nq_specials_ok(q)) E.nquant.take(1e9, NAN);
  E.print();
  return 0;
}
