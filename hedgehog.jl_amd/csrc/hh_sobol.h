// Sobol' points and the Brownian-bridge table of the quasi-Monte Carlo fill (include/hedgehog_mc.h, "Quasi-Monte Carlo"):
// the expansion of a dimension's polynomial and initial values (hh_sobol_table.h) to its 32 direction words, the point
// rule, and the bridge of n_steps unit-variance steps — as the list of its nodes in construction order and as the
// schedule the fill kernel walks.  A host compiler sees nothing of HIP in it, so that tests/c/sobol_host_check.cpp can
// hold it to the Python restatement and run it under the host sanitizers.  Internal; the public surface is
// include/hedgehog_mc.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/hedgehog_mc.h"
#include "hh_sobol_table.h"

namespace hh {

static_assert(kSobolTableDims == HH_SOBOL_MAX_DIMS, "hh_sobol_table.h holds HH_SOBOL_MAX_DIMS dimensions");

constexpr uint32_t kSobolBits = 32u;
// A tile is HH_TILE_PATHS = 2^8 consecutive points: the Gray code of a point splits into these low bits, which differ from
// lane to lane, and the bits above them, which are the Gray code of (point >> 8) — one value per tile, or two where the
// tile crosses a multiple of 256 (hh_sobol.hip)
constexpr uint32_t kSobolLowBits = 8u;
static_assert((1u << kSobolLowBits) == HH_TILE_PATHS, "the split of the Gray code follows the tile");

inline uint32_t sobol_degree(uint32_t dim) {  // dim >= 1
  uint32_t s = 0;
  for (uint32_t p = kSobolPoly[dim]; p > 1u; p >>= 1) ++s;
  return s;
}

// where dimension d's initial values start in kSobolM; formed once per process
inline const uint32_t* sobol_m_offsets() {
  static const std::vector<uint32_t> off = [] {
    std::vector<uint32_t> o(kSobolTableDims + 1u, 0u);
    for (uint32_t d = 1; d < kSobolTableDims; ++d) o[d + 1] = o[d] + sobol_degree(d);
    return o;
  }();
  return off.data();
}

// The 32 direction words of dimension dim < HH_SOBOL_MAX_DIMS: v[j] = m_{j+1} << (31 − j).  Dimension 0 is the van der
// Corput sequence (every m = 1); for the others m_1 … m_s come from the table and, with the polynomial
// x^s + a_1 x^(s−1) + … + a_(s−1) x + 1,   m_j = 2 a_1 m_(j−1) ^ 4 a_2 m_(j−2) ^ … ^ 2^s m_(j−s) ^ m_(j−s)   (Joe & Kuo 2008).
inline void sobol_expand(uint32_t dim, uint32_t v[kSobolBits]) {
  uint32_t m[kSobolBits];
  if (dim == 0u) {
    for (uint32_t j = 0; j < kSobolBits; ++j) m[j] = 1u;
  } else {
    const uint32_t p = kSobolPoly[dim], s = sobol_degree(dim);
    const uint16_t* init = kSobolM + sobol_m_offsets()[dim];
    for (uint32_t j = 0; j < s && j < kSobolBits; ++j) m[j] = init[j];
    for (uint32_t j = s; j < kSobolBits; ++j) {
      uint32_t t = m[j - s] ^ (m[j - s] << s);
      for (uint32_t k = 1; k < s; ++k)
        if ((p >> (s - k)) & 1u) t ^= m[j - k] << k;
      m[j] = t;
    }
  }
  for (uint32_t j = 0; j < kSobolBits; ++j) v[j] = m[j] << (kSobolBits - 1u - j);
}

// every dimension's words, [HH_SOBOL_MAX_DIMS][32]: what a context uploads; expanded once per process
inline const std::vector<uint32_t>& sobol_all_directions() {
  static const std::vector<uint32_t> all = [] {
    std::vector<uint32_t> a((size_t)kSobolTableDims * kSobolBits);
    for (uint32_t d = 0; d < kSobolTableDims; ++d) sobol_expand(d, a.data() + (size_t)d * kSobolBits);
    return a;
  }();
  return all;
}

// point i of the dimension with direction words v, in Gray-code order: the XOR of v[b] over the set bits b of i ^ (i >> 1)
inline uint32_t sobol_point(const uint32_t v[kSobolBits], uint32_t i) {
  const uint32_t g = i ^ (i >> 1);
  uint32_t x = 0u;
  for (uint32_t b = 0; b < kSobolBits; ++b)
    if ((g >> b) & 1u) x ^= v[b];
  return x;
}

// u = (x + 1/2)·2^-32: exact in fp64, in [2^-33, 1 − 2^-33]
inline double sobol_u(uint32_t x) { return ((double)x + 0.5) * 0x1p-32; }

// ---- the bridge over n unit-variance steps -----------------------------------------------------------------------------
// Node j of the construction: W_m = wl·W_l + wr·W_r + sd·z_j.  Node 0 is the terminal value (l = 0, m = r = n,
// wl = wr = 0, sd = sqrt(n)); the others bisect [0, n] breadth first.  depth: 0 for the first bisection.
struct SobolNode {
  uint32_t l, m, r, depth;
  double wl, wr, sd;
};

inline std::vector<SobolNode> sobol_bridge_nodes(uint32_t n) {
  struct Span { uint32_t l, r, depth; };
  std::vector<SobolNode> nodes;
  nodes.reserve(n);
  nodes.push_back(SobolNode{0u, n, n, 0u, 0.0, 0.0, sqrt((double)n)});
  std::vector<Span> queue;
  queue.reserve(2u * (size_t)n + 1u);
  queue.push_back(Span{0u, n, 0u});
  for (size_t head = 0; head < queue.size(); ++head) {
    const Span q = queue[head];
    if (q.r - q.l < 2u) continue;
    const uint32_t m = (q.l + q.r) / 2u;
    const double a = (double)(m - q.l), b = (double)(q.r - m), len = (double)(q.r - q.l);
    nodes.push_back(SobolNode{q.l, m, q.r, q.depth, b / len, a / len, sqrt(a * b / len)});
    queue.push_back(Span{q.l, m, q.depth + 1u});
    queue.push_back(Span{m, q.r, q.depth + 1u});
  }
  return nodes;
}

// The same bridge in the order the fill kernel walks it: the tree of the bisection from left to right, a node built on
// the way down, an increment written as soon as both its ends exist — so the steps come out in ascending order, each
// written once, and the values alive at any moment are one per level of the tree.  They live in slots: slot 0 holds
// W_0 = 0, slot 1 W_n, slot 2 + depth a node of that depth (its subtree is finished before the next node of that depth
// is built).
//   emit = 0: bridge index `index`: slot_m <- wl·[slot_l] + wr·[slot_r] + sd·z(index)
//   emit = 1: step `index`:         d = [slot_r] − [slot_l]
struct SobolOp {
  uint32_t emit, index, slot_l, slot_r, slot_m, reserved;
  double wl, wr, sd;
};

inline std::vector<SobolOp> sobol_bridge_ops(uint32_t n, uint32_t* n_slots) {
  const std::vector<SobolNode> nodes = sobol_bridge_nodes(n);
  std::vector<uint32_t> node_of(n + 1u, 0u), slot_of(n + 1u, 0u);
  uint32_t slots = 2u;
  slot_of[n] = 1u;
  for (uint32_t j = 1; j < nodes.size(); ++j) {
    node_of[nodes[j].m] = j;
    slot_of[nodes[j].m] = 2u + nodes[j].depth;
    if (3u + nodes[j].depth > slots) slots = 3u + nodes[j].depth;
  }
  std::vector<SobolOp> ops;
  ops.reserve(2u * (size_t)n);
  ops.push_back(SobolOp{0u, 0u, 0u, 0u, 1u, 0u, 0.0, 0.0, nodes[0].sd});
  struct Span { uint32_t l, r; };
  std::vector<Span> stack{Span{0u, n}};
  while (!stack.empty()) {
    const Span q = stack.back();
    stack.pop_back();
    if (q.r - q.l == 1u) {
      ops.push_back(SobolOp{1u, q.l, slot_of[q.l], slot_of[q.r], 0u, 0u, 0.0, 0.0, 0.0});
      continue;
    }
    const uint32_t m = (q.l + q.r) / 2u;
    const SobolNode& nd = nodes[node_of[m]];
    ops.push_back(SobolOp{0u, node_of[m], slot_of[q.l], slot_of[q.r], slot_of[m], 0u, nd.wl, nd.wr, nd.sd});
    stack.push_back(Span{m, q.r});
    stack.push_back(Span{q.l, m});
  }
  if (n_slots) *n_slots = slots;
  return ops;
}

}  // namespace hh
