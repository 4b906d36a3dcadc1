// hedgehog.jl_amd/csrc/hh_layout.h compiled for the host: every offset and total of the device scratch layouts for
// the shapes named on standard input (tests/test_scratch_layout_host.py).  A request is
//   lsm <ntot> <n_steps> <degree> | bk <n_chain> <term_cache> <sizeof_args> <sizeof_tables> | sort <n_chain>
// and the answer repeats it, then " : " and the numbers in the order of tests/golden/scratch_layouts.json's fields.
#include <cstdio>
#include <cstring>

#include "hh_layout.h"

int main() {
  char kind[16];
  unsigned long long n;
  while (std::scanf("%15s %llu", kind, &n) == 2) {
    if (!std::strcmp(kind, "lsm")) {
      unsigned n_steps;
      int degree;
      if (std::scanf("%u %d", &n_steps, &degree) != 2) return 2;
      const hh::LsmScratch s(n, n_steps, degree);
      std::printf("lsm %llu %u %d : %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u %d\n", n, n_steps, degree, s.sync,
                  s.ring, s.rec_stats, s.rowstat, s.rec_pow, s.P, s.recB, s.disc_pow, s.counters, s.stamps, s.total,
                  s.rows, s.nch, s.q);
    } else if (!std::strcmp(kind, "bk")) {
      int term_cache;
      size_t sizeof_args, sizeof_tables;
      if (std::scanf("%d %zu %zu", &term_cache, &sizeof_args, &sizeof_tables) != 3) return 2;
      const hh::BkScratch s(n, term_cache, sizeof_args, sizeof_tables);
      std::printf("bk %llu %d %zu %zu : %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %zu\n", n, term_cache,
                  sizeof_args, sizeof_tables, s.long_mask, s.slot_lines, s.counters, s.args, s.tables, s.phi_cache,
                  s.draws, s.iv, s.diag, s.total, s.cache_columns, s.cache_cap, s.lanes);
    } else if (!std::strcmp(kind, "sort")) {
      const hh::BkSortScratch s(n);
      std::printf("sort %llu : %zu %zu %zu %zu %zu %u\n", n, s.perm, s.counts, s.totals, s.keys, s.total, s.n_runs);
    } else {
      return 3;
    }
  }
  return 0;
}
