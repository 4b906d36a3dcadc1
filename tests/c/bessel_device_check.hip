// Device-side check of hedgehog.jl_amd/csrc/hh_bessel.h in the waves the Broadie–Kaya kernels run it in.  Reads
// "nu re im" lines grouped by order; per order the tables are made on the host by bessel_table(ν) and
// bessel_table(ν − n_int), as the Broadie–Kaya set-up does, and reach the kernel through a device pointer to a
// BesselTable[2], as bk_cf_kernel reads them: one order per launch.  The Horner loops run to the longest count
// among a wave's active lanes and per-lane guards skip the steps a lane does not need, so a lane's result must not
// depend on which lanes share its wave.  One launch per order evaluates every case in four lane layouts, each a
// run of whole waves (a lane holding no case returns at once):
//   0 isolated      one case per wave, lane 0 the only active lane
//   1 sweep         the cases in order, the last wave ragged
//   2 shuffle       a seeded permutation, the last wave ragged
//   3 adversarial   each case beside 63 lanes holding, for this order, the case with the longest series sum, the
//                   longest Hankel sum or one of the recurrence branch (one wave per kind, then one mixing all
//                   kinds), and a ragged last wave mixing them
// Output:
//   iso nu re im lg.re lg.im mul.re mul.im [re.lg re.mul]   isolated results, bits; the last two from
//                                                          besseli_logmul_re on the positive real axis
//   layout ν_index layout lanes mismatches                 active lanes whose bits differ from the isolated ones
//   table-bound-violated                                   bessel_table() found no series length for an order
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "hh_bessel.h"

struct Tabs {
  hh::BesselTable t[2];  // order ν, base order ν0
};

struct Res {
  double lg_re, lg_im, mul_re, mul_im, re_lg, re_mul;
};

__global__ void k_bessel(const Tabs* tabs, int n_int, const double* re, const double* im, const double* phi,
                         const int* lane_case, Res* out, int n_lanes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_lanes) return;
  const int c = lane_case[i];
  if (c < 0) return;
  const hh::BesselTable* bt = tabs->t;
  const hh::LogMul r = hh::besseli_logmul(bt[0], bt[1], n_int, {re[c], im[c]}, phi[c]);
  Res o{r.lg.re, r.lg.im, r.mul.re, r.mul.im, 0.0, 0.0};
  if (im[c] == 0.0 && re[c] > 0.0) {
    const hh::LogMulRe q = hh::besseli_logmul_re(bt[0], bt[1], n_int, re[c]);
    o.re_lg = q.lg;
    o.re_mul = q.mul;
  }
  out[i] = o;
}

static uint64_t bits(double x) {
  uint64_t b;
  memcpy(&b, &x, 8);
  return b;
}

// the regime besseli_logmul picks for z and the length of its loop there (host replica of the dispatch, with a
// correctly rounded |z|: only used to choose companions)
enum { kSeries = 0, kHankel = 1, kRecur = 2 };
static void regime(const hh::BesselTable& t, const hh::BesselTable& t0, int n_int, double re, double im, int& kind,
                   int& len) {
  if (re < 0.0) { re = -re; im = -im; }
  const double r = std::sqrt(std::fma(re, re, im * im));
  const bool hankel = n_int == 0 || r >= t.hankel_from;
  const hh::BesselTable& ta = hankel ? t : t0;
  if (r < hh::kSeriesR || (!hankel && r < t.series_rmax && (r - re <= 14.0 || im * im <= t.series_im2))) {
    kind = kSeries;
    len = (int)std::fma(t.series_n1, r, t.series_n0);  // hh::series_terms (device-only), uncapped
    return;
  }
  int M = (int)(r - 0.5);
  M = M < hh::kHankelPairs - 1 ? M : hh::kHankelPairs - 1;
  for (int m = hh::kHankelPairs - 2; m >= 3; --m) M = r >= ta.hankel_rmin[m] ? m : M;
  kind = hankel ? kHankel : kRecur;
  len = hankel ? M : n_int + (int)r;
}

static bool same(const Res& a, const Res& b) { return memcmp(&a, &b, sizeof(Res)) == 0; }

int main() {
  std::vector<double> nus, res, ims;
  {
    double nu, re, im;
    while (std::scanf("%lf %lf %lf", &nu, &re, &im) == 3) {
      nus.push_back(nu); res.push_back(re); ims.push_back(im);
    }
  }
  Tabs* dtabs = nullptr;
  if (hipMalloc(&dtabs, sizeof(Tabs)) != hipSuccess) return 2;
  std::mt19937_64 rng(31337);
  int rc = 0, nu_index = 0;
  for (size_t g0 = 0; g0 < nus.size() && rc == 0; ++nu_index) {
    size_t g1 = g0;
    while (g1 < nus.size() && nus[g1] == nus[g0]) ++g1;
    const double nu = nus[g0];
    const int n_int = nu >= 1.0 ? (int)std::floor(nu) : 0;
    Tabs tabs;
    if (!hh::bessel_table(nu, tabs.t[0]) || !hh::bessel_table(nu - n_int, tabs.t[1])) {
      std::printf("table-bound-violated\n");
      rc = 1;
      break;
    }
    const int nc = (int)(g1 - g0);
    std::vector<double> re(res.begin() + g0, res.begin() + g1), im(ims.begin() + g0, ims.begin() + g1), phi(nc);
    for (int c = 0; c < nc; ++c) phi[c] = std::atan2(im[c], re[c]);
    // companions: the longest series sum, the longest Hankel sum, a recurrence case (orders >= 1)
    int best[3] = {-1, -1, -1}, best_len[3] = {-1, -1, -1};
    for (int c = 0; c < nc; ++c) {
      int kind, len;
      regime(tabs.t[0], tabs.t[1], n_int, re[c], im[c], kind, len);
      if (len > best_len[kind]) { best_len[kind] = len; best[kind] = c; }
    }
    std::vector<int> comp;
    for (int k = 0; k < 3; ++k)
      if (best[k] >= 0) comp.push_back(best[k]);
    // the four layouts, each padded to whole waves with empty lanes
    std::vector<int> lane;
    int seg[5];
    auto pad = [&]() { while (lane.size() % 64) lane.push_back(-1); };
    seg[0] = 0;
    for (int c = 0; c < nc; ++c) { lane.push_back(c); for (int j = 1; j < 64; ++j) lane.push_back(-1); }
    seg[1] = (int)lane.size();
    for (int c = 0; c < nc; ++c) lane.push_back(c);
    pad();
    seg[2] = (int)lane.size();
    std::vector<int> perm(nc);
    for (int c = 0; c < nc; ++c) perm[c] = c;
    std::shuffle(perm.begin(), perm.end(), rng);
    for (int c : perm) lane.push_back(c);
    pad();
    seg[3] = (int)lane.size();
    for (int c = 0; c < nc; ++c) {
      for (int k : comp) { lane.push_back(c); for (int j = 1; j < 64; ++j) lane.push_back(k); }
      lane.push_back(c);
      for (int j = 1; j < 64; ++j) lane.push_back(comp[j % comp.size()]);
    }
    for (int j = 0; j < 37; ++j) lane.push_back(j % 2 ? comp[(j / 2) % comp.size()] : (int)(rng() % nc));  // ragged
    pad();
    seg[4] = (int)lane.size();
    const int nl = (int)lane.size();
    double *dre = nullptr, *dim = nullptr, *dphi = nullptr;
    int* dlane = nullptr;
    Res* dout = nullptr;
    std::vector<Res> out(nl);
    bool good = hipMalloc(&dre, nc * 8) == hipSuccess && hipMalloc(&dim, nc * 8) == hipSuccess &&
                hipMalloc(&dphi, nc * 8) == hipSuccess && hipMalloc(&dlane, nl * sizeof(int)) == hipSuccess &&
                hipMalloc(&dout, nl * sizeof(Res)) == hipSuccess;
    good = good && hipMemcpy(dtabs, &tabs, sizeof(Tabs), hipMemcpyHostToDevice) == hipSuccess &&
           hipMemcpy(dre, re.data(), nc * 8, hipMemcpyHostToDevice) == hipSuccess &&
           hipMemcpy(dim, im.data(), nc * 8, hipMemcpyHostToDevice) == hipSuccess &&
           hipMemcpy(dphi, phi.data(), nc * 8, hipMemcpyHostToDevice) == hipSuccess &&
           hipMemcpy(dlane, lane.data(), nl * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
    if (good) {
      hipLaunchKernelGGL(k_bessel, dim3((nl + 255) / 256), dim3(256), 0, 0, dtabs, n_int, dre, dim, dphi, dlane, dout, nl);
      good = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(out.data(), dout, nl * sizeof(Res), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(dre); (void)hipFree(dim); (void)hipFree(dphi); (void)hipFree(dlane); (void)hipFree(dout);
    if (!good) { rc = 3; break; }
    for (int c = 0; c < nc; ++c) {
      const Res& o = out[64 * c];
      std::printf("iso %.17g %.17g %.17g %016llx %016llx %016llx %016llx", nu, re[c], im[c], (unsigned long long)bits(o.lg_re),
                  (unsigned long long)bits(o.lg_im), (unsigned long long)bits(o.mul_re), (unsigned long long)bits(o.mul_im));
      if (im[c] == 0.0 && re[c] > 0.0)
        std::printf(" %016llx %016llx", (unsigned long long)bits(o.re_lg), (unsigned long long)bits(o.re_mul));
      std::printf("\n");
    }
    for (int L = 1; L < 4; ++L) {
      int active = 0, bad = 0;
      for (int i = seg[L]; i < seg[L + 1]; ++i) {
        if (lane[i] < 0) continue;
        ++active;
        if (!same(out[i], out[64 * lane[i]])) {
          if (bad == 0)
            std::printf("first-mismatch nu=%.17g layout=%d lane=%d z=(%.17g, %.17g)\n", nu, L, i, re[lane[i]], im[lane[i]]);
          ++bad;
        }
      }
      std::printf("layout %d %d %d %d %d\n", nu_index, L, active, bad, (int)comp.size());
    }
    g0 = g1;
  }
  (void)hipFree(dtabs);
  return rc;
}
