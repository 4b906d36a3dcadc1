// Device-side check of the Box–Muller transform of hedgehog.jl_amd/csrc/hh_rng.h — u01_fast, two_u01_fast,
// neg2_log_unit, sqrt_pos, sincospi_02 and normal_pair, which exist for the device only — against long-double
// references on the lattices the kernels produce.  tests/test_gpu_rng_device.py holds the output to the bars.
//
//   u01 lo hi fast two               named words: the bits of u01_fast and two_u01_fast
//   u01_random n mismatches          10^6 random words against u01_from_bits (2·u01_from_bits), bit for bit
//   nlog n worst_ulp arg             -2 ln u on every binade of [2^-53, 1 - 2^-53], lattice (k + 1/2)·2^-52
//   nlog_binade e n worst_ulp        the same per binade [2^e, 2^(e+1))
//   sqrt n worst_ulp arg             sqrt_pos on [2^-52, 73.7]
//   sin|cos n worst_ulp arg          sincospi_02 on the lattice (k + 1/2)·2^-51 of (0, 2)
//   sign_mismatch n                  components whose sign is not their quadrant's
//   pair n worst_rel arg_words       normal_pair: max |z - z_ref| / |z_ref| in units of 2^-52, and its words
//   pairbits c0 c1 c2 c3 z1 z2       hand-built words: the device's bits
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "hh_rng.h"

static uint64_t bits(double x) {
  uint64_t b;
  memcpy(&b, &x, 8);
  return b;
}
static double ulp_err(double got, long double want) {
  if (want == 0.0L) return got == 0.0 ? 0.0 : 1e9;
  int e;
  std::frexp((double)want, &e);
  return (double)(fabsl((long double)got - want) / std::ldexp(1.0L, e - 53));
}
static const long double kPiL = 3.14159265358979323846264338327950288L;

// sin(π t), cos(π t) for a lattice t in (0, 2): q = rint(2t), r = t - q/2 exactly in double, then the long-double
// pair at π r rotated by q
static void sincospi_ref(double t, long double& s, long double& c) {
  const double q = std::rint(2.0 * t);
  const double r = t - 0.5 * q;  // exact: t and q/2 are multiples of 2^-52 below 2
  const long double sr = sinl(kPiL * r), cr = cosl(kPiL * r);
  switch (((int)q) & 3) {
    case 0: s = sr; c = cr; break;
    case 1: s = cr; c = -sr; break;
    case 2: s = -sr; c = -cr; break;
    default: s = -cr; c = sr; break;
  }
}

__global__ void k_u01(const uint32_t* lo, const uint32_t* hi, double* fast, double* two, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fast[i] = hh::u01_fast(lo[i], hi[i]);
  two[i] = hh::two_u01_fast(lo[i], hi[i]);
}
__global__ void k_nlog(const double* u, double* y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = hh::neg2_log_unit(u[i]);
}
__global__ void k_sqrt(const double* a, double* y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = hh::sqrt_pos(a[i]);
}
__global__ void k_scp(const double* t, double* s, double* c, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) hh::sincospi_02(t[i], s[i], c[i]);
}
__global__ void k_pair(const uint32_t* w, double* z1, double* z2, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const hh::Philox4 b{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
  hh::normal_pair(b, z1[i], z2[i]);
}

static bool ok = true;
struct Dev {
  std::vector<void*> ptrs;
  template <class T>
  T* put(const std::vector<T>& v) {
    void* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(v.size(), 1) * sizeof(T)) != hipSuccess) { ok = false; return nullptr; }
    ptrs.push_back(d);
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) ok = false;
    return (T*)d;
  }
  double* out(size_t n) { return put(std::vector<double>(n, 0.0)); }
  void get(std::vector<double>& v, const double* d) {
    if (!v.empty() && hipMemcpy(v.data(), d, v.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) ok = false;
  }
  ~Dev() { for (void* p : ptrs) (void)hipFree(p); }
};
static dim3 blocks(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
static bool launched() {
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) ok = false;
  return ok;
}

int main() {
  Dev D;
  std::mt19937_64 rng(20261016);
  // ---- uniforms
  std::vector<uint32_t> lo = {0u, 0xffffffffu}, hi = {0u, 0xffffffffu};
  for (int b = 0; b < 64; ++b) {
    const uint64_t w = 1ull << b;
    lo.push_back((uint32_t)w);
    hi.push_back((uint32_t)(w >> 32));
  }
  const int n_named = (int)lo.size();
  for (int i = 0; i < 1000000; ++i) {
    const uint64_t w = rng();
    lo.push_back((uint32_t)w);
    hi.push_back((uint32_t)(w >> 32));
  }
  const int nu = (int)lo.size();
  // ---- -2 ln u: every binade [2^e, 2^(e+1)), e = -53 … -1, on the lattice u = (k + 1/2)·2^-52, k in [klo, khi]
  std::vector<double> lu;
  std::vector<int> lbin;
  for (int e = -53; e <= -1; ++e) {
    const uint64_t klo = e >= -52 ? 1ull << (e + 52) : 0ull, khi = (1ull << (e + 53)) - 1;
    auto add = [&](uint64_t k) {
      if (k < klo || k > khi) return;
      lu.push_back(((double)k + 0.5) * 0x1p-52);
      lbin.push_back(e);
    };
    for (uint64_t d = 0; d < 64; ++d) { add(klo + d); add(khi - d); }  // the binade's ends
    // ±64 ulp around the mantissa switch at sqrt(1/2)·2^(e+1)
    const uint64_t ks = (uint64_t)std::llround(0.70710678118654752440L * std::ldexp(1.0L, e + 53) - 0.5L);
    for (int64_t d = -64; d <= 64; ++d) add(ks + d);
    std::uniform_int_distribution<uint64_t> K(klo, khi);
    for (int i = 0; i < (1 << 14); ++i) add(K(rng));
  }
  const int nl = (int)lu.size();
  // ---- sqrt_pos on [2^-52, 73.7] (-2 ln u of the lattice: 2^-52 … 73.67)
  std::vector<double> sa = {0x1p-52, 73.7, 73.66867657, 1.0, 2.0, 4.0, 0x1.fffffffffffffp0, 0x1.0000000000001p0};
  std::uniform_real_distribution<double> U(0.0, 1.0);
  for (int i = 0; i < 1000000; ++i) sa.push_back(std::exp2(-52.0 + (52.0 + std::log2(73.7)) * U(rng)));
  const int ns = (int)sa.size();
  // ---- sincospi_02 on t = (k + 1/2)·2^-51, k in [0, 2^52)
  std::vector<double> tt;
  auto addt = [&](int64_t k) {
    if (k >= 0 && k < (int64_t)(1ll << 52)) tt.push_back(((double)k + 0.5) * 0x1p-51);
  };
  for (int j = 1; j <= 7; ++j)
    for (int64_t d = -64; d < 64; ++d) addt((int64_t)j * (1ll << 49) + d);  // ±64 lattice points around t = j/4
  for (int64_t k = 0; k < 2048; ++k) {  // within 2^-40 of 0, 1 and 2
    addt(k);
    addt((1ll << 51) - 1 - k);
    addt((1ll << 51) + k);
    addt((1ll << 52) - 1 - k);
  }
  for (int i = 0; i < 1000000; ++i) addt((int64_t)(rng() >> 12));
  const int nt = (int)tt.size();
  // ---- normal_pair at hand-built words: u1 at its ends, binade ends and the sqrt(1/2) switch; the angle at the
  // seams of sincospi_02; then random words
  std::vector<uint64_t> w1 = {0ull, ~0ull, 1ull << 12, 2ull << 12, (1ull << 63), (1ull << 63) - 1,
                              (uint64_t)0xB504F333F9DE6000ull, (uint64_t)0xB504F333F9DE7000ull, (1ull << 62) | 0xabcull};
  std::vector<uint64_t> w2 = {0ull, ~0ull};
  for (int j = 1; j <= 7; ++j)
    for (int64_t d = -2; d <= 1; ++d) w2.push_back((((uint64_t)j << 49) + d) << 12 | 0x5a5);
  for (int64_t k : {1ll, 2ll, (1ll << 52) - 2})
    w2.push_back((uint64_t)k << 12);
  std::vector<uint32_t> pw;
  for (uint64_t a : w1)
    for (uint64_t b : w2) {
      pw.push_back((uint32_t)a); pw.push_back((uint32_t)(a >> 32));
      pw.push_back((uint32_t)b); pw.push_back((uint32_t)(b >> 32));
    }
  const int np_named = (int)pw.size() / 4;
  for (int i = 0; i < 1000000; ++i) {
    const uint64_t a = rng(), b = rng();
    pw.push_back((uint32_t)a); pw.push_back((uint32_t)(a >> 32));
    pw.push_back((uint32_t)b); pw.push_back((uint32_t)(b >> 32));
  }
  const int np = (int)pw.size() / 4;

  uint32_t *dlo = D.put(lo), *dhi = D.put(hi), *dpw = D.put(pw);
  double *dfast = D.out(nu), *dtwo = D.out(nu);
  double *dlu = D.put(lu), *dly = D.out(nl), *dsa = D.put(sa), *dsy = D.out(ns);
  double *dtt = D.put(tt), *dts = D.out(nt), *dtc = D.out(nt), *dz1 = D.out(np), *dz2 = D.out(np);
  if (!ok) return 2;
  hipLaunchKernelGGL(k_u01, blocks(nu), dim3(256), 0, 0, dlo, dhi, dfast, dtwo, nu);
  hipLaunchKernelGGL(k_nlog, blocks(nl), dim3(256), 0, 0, dlu, dly, nl);
  hipLaunchKernelGGL(k_sqrt, blocks(ns), dim3(256), 0, 0, dsa, dsy, ns);
  hipLaunchKernelGGL(k_scp, blocks(nt), dim3(256), 0, 0, dtt, dts, dtc, nt);
  hipLaunchKernelGGL(k_pair, blocks(np), dim3(256), 0, 0, dpw, dz1, dz2, np);
  if (!launched()) return 3;
  std::vector<double> fast(nu), two(nu), ly(nl), sy(ns), ts(nt), tc(nt), z1(np), z2(np);
  D.get(fast, dfast); D.get(two, dtwo); D.get(ly, dly); D.get(sy, dsy); D.get(ts, dts); D.get(tc, dtc);
  D.get(z1, dz1); D.get(z2, dz2);
  if (!ok) return 3;

  for (int i = 0; i < n_named; ++i)
    printf("u01 %08x %08x %016llx %016llx\n", lo[i], hi[i], (unsigned long long)bits(fast[i]),
           (unsigned long long)bits(two[i]));
  long long mism = 0;
  for (int i = n_named; i < nu; ++i) {
    const double want = hh::u01_from_bits(lo[i], hi[i]);
    mism += bits(fast[i]) != bits(want) || bits(two[i]) != bits(2.0 * want);
  }
  printf("u01_random %d %lld\n", nu - n_named, mism);

  double wl = 0.0, wl_arg = 0.0, wb[54] = {0};
  int nb[54] = {0};
  for (int i = 0; i < nl; ++i) {
    const double e = ulp_err(ly[i], -2.0L * logl((long double)lu[i]));
    if (!(e <= wl)) { wl = e; wl_arg = lu[i]; }
    const int b = lbin[i] + 53;
    wb[b] = std::max(wb[b], e);
    nb[b] += 1;
  }
  printf("nlog %d %.3f %016llx\n", nl, wl, (unsigned long long)bits(wl_arg));
  for (int b = 0; b < 53; ++b) printf("nlog_binade %d %d %.3f\n", b - 53, nb[b], wb[b]);

  double wsq = 0.0, wsq_arg = 0.0;
  for (int i = 0; i < ns; ++i) {
    const double e = ulp_err(sy[i], sqrtl((long double)sa[i]));
    if (!(e <= wsq)) { wsq = e; wsq_arg = sa[i]; }
  }
  printf("sqrt %d %.3f %016llx\n", ns, wsq, (unsigned long long)bits(wsq_arg));

  double ws = 0.0, ws_arg = 0.0, wc = 0.0, wc_arg = 0.0;
  long long sign_bad = 0;
  for (int i = 0; i < nt; ++i) {
    long double s, c;
    sincospi_ref(tt[i], s, c);
    const double es = ulp_err(ts[i], s), ec = ulp_err(tc[i], c);
    if (!(es <= ws)) { ws = es; ws_arg = tt[i]; }
    if (!(ec <= wc)) { wc = ec; wc_arg = tt[i]; }
    sign_bad += std::signbit(ts[i]) != (s < 0.0L) || std::signbit(tc[i]) != (c < 0.0L);
  }
  printf("sin %d %.3f %016llx\ncos %d %.3f %016llx\nsign_mismatch %lld\n", nt, ws, (unsigned long long)bits(ws_arg), nt,
         wc, (unsigned long long)bits(wc_arg), sign_bad);

  double wp = 0.0;
  int wp_i = 0;
  for (int i = 0; i < np; ++i) {
    const uint32_t* w = &pw[4 * i];
    const double u1 = hh::u01_from_bits(w[0], w[1]), t = 2.0 * hh::u01_from_bits(w[2], w[3]);
    const long double R = sqrtl(-2.0L * logl((long double)u1));
    long double s, c;
    sincospi_ref(t, s, c);
    const long double r1 = R * c, r2 = R * s;
    const double e = (double)(std::max(fabsl((long double)z1[i] - r1) / fabsl(r1), fabsl((long double)z2[i] - r2) / fabsl(r2)) /
                              0x1p-52L);
    if (!(e <= wp)) { wp = e; wp_i = i; }
    if (i < np_named)
      printf("pairbits %08x %08x %08x %08x %016llx %016llx\n", w[0], w[1], w[2], w[3], (unsigned long long)bits(z1[i]),
             (unsigned long long)bits(z2[i]));
  }
  printf("pair %d %.3f %08x %08x %08x %08x\n", np, wp, pw[4 * wp_i], pw[4 * wp_i + 1], pw[4 * wp_i + 2], pw[4 * wp_i + 3]);
  return 0;
}
