// Quasi-Monte Carlo on the device (include/hedgehog_mc.h, "Quasi-Monte Carlo"): Sobol' points in Gray-code order, their
// digital shift, and the fill of a tile-major REPLAY buffer from them — one lane per point, one workgroup per tile, a
// sibling of wiener_fill_kernel (hh_kernels.hip).
//
// The points of a tile.  Lane p of the tile that starts at point `base` holds point i = base + p.  Its Gray code
// g = i ^ (i >> 1) splits at bit 8: the low byte differs from lane to lane, the bits above are the Gray code of i >> 8 —
// ONE value for the whole tile, or two where the tile crosses a multiple of 256 (base is point_offset + 256·tile, and
// point_offset is any number).  So the XOR over the 24 high direction words, with the dimension's shift word folded in,
// is formed once per (tile, dimension) for both values (sobol_high_kernel: a lane per pair, 8 bytes each, 0.4 % of the
// bytes of the buffer they serve) and reaches the fill as a scalar load; per lane a point is one select between the
// two and eight v_bitop3 (x ^ (mask & v[b]), the masks formed once per lane, the eight low words a scalar load).
//
// The bridge.  n_steps + 1 values per factor and lane do not fit in registers or LDS.  The kernel walks the bisection
// tree from left to right instead (hh_sobol.h, sobol_bridge_ops): a node is built on the way down, an increment is
// written as soon as both its ends exist.  The steps then come out in ascending order, each written ONCE and never read
// back — the buffer's one write is all the kernel's HBM traffic — and what is alive at any moment is one value per level
// of the tree: ⌈log2 n⌉ + 2 slots per factor, a column of LDS per lane (252 Heston steps: 10 slots, 40 KB per
// workgroup).  A lane reads and writes its own column only, so the walk needs no barrier.  Every op of the walk is
// wave-uniform: the table entry, the direction words and the tile's high words are scalar loads.
#include "hh_kernels.h"
#include "hh_math.h"
#include "hh_rng.h"

namespace hh {

namespace {

// the shift word of dimension dim under randomisation r (include/hedgehog_mc.h)
__device__ __forceinline__ uint32_t sobol_shift_word(uint32_t dim, uint32_t r, uint64_t seed) {
  const Philox4 b = philox4x32_10(dim >> 2, r, 0u, kDomSobol, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t w = dim & 3u;
  return w == 0u ? b.c0 : w == 1u ? b.c1 : w == 2u ? b.c2 : b.c3;
}

// the XOR of v[8 + b] over the set bits b of the Gray code of h = point >> 8.  Only the 24 bits that have a direction word
// are read: h = 2^24 (the value past the crossing in a tile that ends at point 2^32, where no live lane lies) stays in bounds.
__device__ __forceinline__ uint32_t sobol_high(const uint32_t* __restrict__ v, uint32_t h) {
  const uint32_t g = h ^ (h >> 1);
  uint32_t x = 0u;
#pragma unroll
  for (uint32_t b = 0; b < kSobolBits - kSobolLowBits; ++b) x ^= (0u - ((g >> b) & 1u)) & v[kSobolLowBits + b];
  return x;
}

// high[tile][dim] = {the part of a point that the lanes before the crossing share, … the lanes past it}, shift included
__global__ __launch_bounds__(kTile) void sobol_high_kernel(const uint32_t* __restrict__ dirs, uint32_t n_dims, uint32_t offset,
                                                           uint64_t seed, uint32_t r, int shifted, uint2* __restrict__ high) {
  const uint32_t tile = blockIdx.x, d = blockIdx.y * kTile + threadIdx.x;
  if (d >= n_dims) return;
  const uint32_t* v = dirs + (size_t)d * kSobolBits;
  const uint32_t h = (offset + tile * (uint32_t)kTile) >> kSobolLowBits;
  const uint32_t s = shifted ? sobol_shift_word(d, r, seed) : 0u;
  high[(size_t)tile * n_dims + d] = make_uint2(sobol_high(v, h) ^ s, sobol_high(v, h + 1u) ^ s);
}

// what a lane keeps for all the dimensions of its point
struct SobolLane {
  uint32_t mask[kSobolLowBits];  // all ones where bit b of the point's Gray code is set
  bool crossed;                  // the point lies past the multiple of 256 its tile crosses
};

// base + lane wraps only in the padded lanes of a tile that ends past point 2^32 − 1: they are written as zeros
__device__ __forceinline__ SobolLane sobol_lane(uint32_t base, uint32_t lane) {
  const uint32_t i = base + lane, g = i ^ (i >> 1);
  SobolLane L;
#pragma unroll
  for (uint32_t b = 0; b < kSobolLowBits; ++b) L.mask[b] = 0u - ((g >> b) & 1u);
  L.crossed = (i >> kSobolLowBits) != (base >> kSobolLowBits);
  return L;
}

// the lane's word of the dimension whose direction words are v (wave-uniform) and whose high words for this tile are `high`
__device__ __forceinline__ uint32_t sobol_word(const uint32_t* __restrict__ v, uint2 high, const SobolLane& L) {
  uint32_t x = L.crossed ? high.y : high.x;
#pragma unroll
  for (uint32_t b = 0; b < kSobolLowBits; ++b)
    x = __builtin_amdgcn_bitop3_b32(x, L.mask[b], v[b], 0x78);  // x ^ (mask & v[b]): 0xF0 ^ (0xCC & 0xAA)
  return x;
}

constexpr uint32_t kPointDims = 64u;  // dimensions per workgroup of the points kernel

__global__ __launch_bounds__(kTile) void sobol_points_kernel(const uint32_t* __restrict__ dirs, const uint2* __restrict__ high,
                                                             uint32_t n_dims, uint64_t n_points, uint32_t offset,
                                                             uint32_t* __restrict__ dst) {
  const uint32_t tile = blockIdx.x, d0 = blockIdx.y * kPointDims;
  const uint64_t p = (uint64_t)tile * kTile + threadIdx.x;
  if (p >= n_points) return;
  const SobolLane L = sobol_lane(offset + tile * (uint32_t)kTile, threadIdx.x);
  for (uint32_t d = d0; d < d0 + kPointDims && d < n_dims; ++d)
    dst[(size_t)d * n_points + p] = sobol_word(dirs + (size_t)d * kSobolBits, high[(size_t)tile * n_dims + d], L);
}

struct SobolFillArgs {
  double rho, rho_c, sqrt_dt;
  uint64_t n_points;
  uint32_t n_steps, n_ops, offset;
};

// ops == nullptr: HH_SOBOL_INCREMENTAL.  Dynamic LDS (the bridge): slot[n_slots][NC][kTile] doubles.
template <int NC, bool BRIDGE>
__global__ __launch_bounds__(kTile) void sobol_fill_kernel(SobolFillArgs a, const uint32_t* __restrict__ dirs,
                                                           const uint2* __restrict__ high, const SobolOp* __restrict__ ops,
                                                           double* __restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) double slot[];
  const uint32_t tile = blockIdx.x, lane = threadIdx.x;
  const SobolLane L = sobol_lane(a.offset + tile * (uint32_t)kTile, lane);
  const bool live = (uint64_t)tile * kTile + lane < a.n_points;
  const uint2* __restrict__ tile_high = high + (size_t)tile * NC * a.n_steps;
  double* out = dst + (size_t)tile * a.n_steps * NC * kTile + lane;

  auto normal = [&](uint32_t d) {  // d is wave-uniform
    const uint32_t x = sobol_word(dirs + (size_t)d * kSobolBits, tile_high[d], L);
    return fm::normal_quantile(((double)x + 0.5) * 0x1p-32);
  };
  auto emit = [&](uint32_t k, double d1, double d2) {  // wiener_fill_kernel's form
    out[((size_t)k * NC + 0) * kTile] = live ? a.sqrt_dt * d1 : 0.0;
    if constexpr (NC == 2) out[((size_t)k * 2 + 1) * kTile] = live ? a.sqrt_dt * fma(a.rho, d1, a.rho_c * d2) : 0.0;
  };

  if constexpr (!BRIDGE) {
    for (uint32_t k = 0; k < a.n_steps; ++k) {
      const double z1 = normal(NC * k);
      const double z2 = NC == 2 ? normal(NC * k + 1u) : 0.0;
      emit(k, z1, z2);
    }
  } else {
    double* col = slot + lane;  // the lane's column: [slot][comp]
#pragma unroll
    for (int c = 0; c < NC; ++c) col[(size_t)c * kTile] = 0.0;  // slot 0: W_0
    for (uint32_t t = 0; t < a.n_ops; ++t) {
      const SobolOp op = ops[t];  // wave-uniform
      const double* wl = col + (size_t)op.slot_l * NC * kTile;
      const double* wr = col + (size_t)op.slot_r * NC * kTile;
      if (op.emit) {
        const double d1 = wr[0] - wl[0];
        const double d2 = NC == 2 ? wr[kTile] - wl[kTile] : 0.0;
        emit(op.index, d1, d2);
      } else {
        double* wm = col + (size_t)op.slot_m * NC * kTile;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const double z = normal(NC * op.index + c);
          wm[(size_t)c * kTile] = fma(op.wl, wl[(size_t)c * kTile], fma(op.wr, wr[(size_t)c * kTile], op.sd * z));
        }
      }
    }
  }
}

}  // namespace

int launch_sobol_high(const uint32_t* dirs_dev, uint32_t n_dims, uint64_t n_points, uint32_t offset, uint64_t seed,
                      uint32_t randomization, int shifted, uint32_t* high_dev, hipStream_t s) {
  const dim3 grid(tiles_for(n_points), (n_dims + kTile - 1) / kTile);
  hipLaunchKernelGGL(sobol_high_kernel, grid, dim3(kTile), 0, s, dirs_dev, n_dims, offset, seed, randomization, shifted,
                     (uint2*)high_dev);
  return (int)hipGetLastError();
}

int launch_sobol_points(const uint32_t* dirs_dev, const uint32_t* high_dev, uint32_t n_dims, uint64_t n_points,
                        uint32_t offset, uint32_t* dst_dev, hipStream_t s) {
  const dim3 grid(tiles_for(n_points), (n_dims + kPointDims - 1) / kPointDims);
  hipLaunchKernelGGL(sobol_points_kernel, grid, dim3(kTile), 0, s, dirs_dev, (const uint2*)high_dev, n_dims, n_points, offset,
                     dst_dev);
  return (int)hipGetLastError();
}

int launch_sobol_fill(int dynamics, double rho, double sqrt_dt, uint32_t n_steps, uint64_t n_points, uint32_t offset,
                      const uint32_t* dirs_dev, const uint32_t* high_dev, const SobolOp* ops_dev, uint32_t n_ops,
                      uint32_t n_slots, double* dst, hipStream_t s) {
  SobolFillArgs a{};
  a.rho = rho;
  a.rho_c = sqrt(1.0 - rho * rho);
  a.sqrt_dt = sqrt_dt;
  a.n_points = n_points;
  a.n_steps = n_steps;
  a.n_ops = n_ops;
  a.offset = offset;
  const dim3 grid(tiles_for(n_points)), block(kTile);
  const uint2* high = (const uint2*)high_dev;
  const int nc = dynamics == HH_HESTON ? 2 : 1;
  const size_t lds = ops_dev ? (size_t)n_slots * nc * kTile * sizeof(double) : 0;  // at most 13·2·2 KB (2048 Heston steps)
  if (ops_dev && nc == 2)
    hipLaunchKernelGGL((sobol_fill_kernel<2, true>), grid, block, lds, s, a, dirs_dev, high, ops_dev, dst);
  else if (ops_dev)
    hipLaunchKernelGGL((sobol_fill_kernel<1, true>), grid, block, lds, s, a, dirs_dev, high, ops_dev, dst);
  else if (nc == 2)
    hipLaunchKernelGGL((sobol_fill_kernel<2, false>), grid, block, 0, s, a, dirs_dev, high, ops_dev, dst);
  else
    hipLaunchKernelGGL((sobol_fill_kernel<1, false>), grid, block, 0, s, a, dirs_dev, high, ops_dev, dst);
  return (int)hipGetLastError();
}

}  // namespace hh
