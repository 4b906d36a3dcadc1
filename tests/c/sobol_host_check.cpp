// Host check of what the quasi-Monte Carlo fill shares with the host (csrc/hh_sobol.h): reads queries, one per line, from
// the file named on the command line and answers each on one or more lines:
//   dir d        ->  dir d v0 … v31                  the direction words of dimension d (hex)
//   pt d i       ->  pt d i x                        point i of dimension d (hex word)
//   u x          ->  u x (x + 1/2)·2^-32             (hex word, hex float)
//   bridge n     ->  node n j l m r depth wl wr sd   the bridge's nodes in construction order (hex floats), then
//                    op n t emit index slot_l slot_r slot_m wl wr sd   the kernel's walk, then   slots n count
// tests/test_sobol_host.py holds every answer to the Python restatement (tests/sobol_cases.py), bit for bit, and builds the
// program twice — plainly, and with -fsanitize=address,undefined.  The program itself checks the walk: run on the
// integers' own doubles z_j = j + 1 it must write every step once, in ascending order, read no slot before it was written,
// and give the steps the nodes give when they are evaluated in construction order (exit 3 otherwise).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../hedgehog.jl_amd/csrc/hh_sobol.h"

namespace {

bool walk_matches_nodes(uint32_t n, const std::vector<hh::SobolNode>& nodes, const std::vector<hh::SobolOp>& ops,
                        uint32_t n_slots) {
  std::vector<double> W(n + 1u, 0.0);
  for (size_t j = 0; j < nodes.size(); ++j) {
    const hh::SobolNode& nd = nodes[j];
    const double z = (double)(j + 1);
    W[nd.m] = j ? fma(nd.wl, W[nd.l], fma(nd.wr, W[nd.r], nd.sd * z)) : nd.sd * z;
  }
  std::vector<double> slot(n_slots, 0.0);
  std::vector<char> set(n_slots, 0);
  set[0] = 1;
  uint32_t next = 0;
  for (const hh::SobolOp& op : ops) {
    if (op.slot_l >= n_slots || op.slot_r >= n_slots || op.slot_m >= n_slots) return false;
    if (!set[op.slot_l] || !set[op.slot_r]) return false;
    if (op.emit) {
      if (op.index != next || next >= n) return false;
      if (slot[op.slot_r] - slot[op.slot_l] != W[next + 1u] - W[next]) return false;
      ++next;
    } else {
      if (op.index >= nodes.size() || op.slot_m == 0u) return false;
      slot[op.slot_m] = fma(op.wl, slot[op.slot_l], fma(op.wr, slot[op.slot_r], op.sd * (double)(op.index + 1u)));
      set[op.slot_m] = 1;
    }
  }
  return next == n;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s queries.txt\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  static_assert(sizeof(hh::SobolOp) == 48, "SobolOp is six words and three doubles");
  char kind[16];
  int bad = 0;
  while (std::fscanf(f, "%15s", kind) == 1) {
    if (!std::strcmp(kind, "dir")) {
      uint32_t d, v[32];
      if (std::fscanf(f, "%" SCNu32, &d) != 1 || d >= HH_SOBOL_MAX_DIMS) return 2;
      hh::sobol_expand(d, v);
      std::printf("dir %" PRIu32, d);
      for (int j = 0; j < 32; ++j) std::printf(" %" PRIx32, v[j]);
      std::printf("\n");
    } else if (!std::strcmp(kind, "pt")) {
      uint32_t d, i, v[32];
      if (std::fscanf(f, "%" SCNu32 " %" SCNu32, &d, &i) != 2 || d >= HH_SOBOL_MAX_DIMS) return 2;
      hh::sobol_expand(d, v);
      std::printf("pt %" PRIu32 " %" PRIu32 " %" PRIx32 "\n", d, i, hh::sobol_point(v, i));
    } else if (!std::strcmp(kind, "u")) {
      uint32_t x;
      if (std::fscanf(f, "%" SCNx32, &x) != 1) return 2;
      std::printf("u %" PRIx32 " %a\n", x, hh::sobol_u(x));
    } else if (!std::strcmp(kind, "bridge")) {
      uint32_t n, n_slots = 0;
      if (std::fscanf(f, "%" SCNu32, &n) != 1 || n == 0u || n > HH_SOBOL_MAX_DIMS) return 2;
      const std::vector<hh::SobolNode> nodes = hh::sobol_bridge_nodes(n);
      const std::vector<hh::SobolOp> ops = hh::sobol_bridge_ops(n, &n_slots);
      for (size_t j = 0; j < nodes.size(); ++j)
        std::printf("node %" PRIu32 " %zu %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %a %a %a\n", n, j, nodes[j].l,
                    nodes[j].m, nodes[j].r, nodes[j].depth, nodes[j].wl, nodes[j].wr, nodes[j].sd);
      for (size_t t = 0; t < ops.size(); ++t)
        std::printf("op %" PRIu32 " %zu %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %a %a %a\n", n, t,
                    ops[t].emit, ops[t].index, ops[t].slot_l, ops[t].slot_r, ops[t].slot_m, ops[t].wl, ops[t].wr, ops[t].sd);
      std::printf("slots %" PRIu32 " %" PRIu32 "\n", n, n_slots);
      if (nodes.size() != n || ops.size() != 2u * (size_t)n || !walk_matches_nodes(n, nodes, ops, n_slots)) {
        std::fprintf(stderr, "bridge %" PRIu32 ": the walk does not give the nodes' steps\n", n);
        ++bad;
      }
    } else {
      std::fprintf(stderr, "unknown query %s\n", kind);
      return 2;
    }
  }
  std::fclose(f);
  return bad ? 3 : 0;
}
