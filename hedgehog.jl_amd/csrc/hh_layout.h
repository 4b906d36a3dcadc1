// How the device scratch buffers are carved: the LSM induction's, the path statistics', the Broadie–Kaya chain's and
// the grid sort's.
// Each layout is stated ONCE, as a struct of region offsets that one constructor fills by walking a cursor; the
// allocation's size, the kernels' pointers and the host's read-backs all come from it (hh_lsm.hip, hh_bk.hip,
// hh_api.hip).  A region is added here and nowhere else.  Plain size_t arithmetic, no HIP types: a host compiler
// builds it for tests/test_scratch_layout_host.py.
#pragma once
#include "../../include/hedgehog_mc.h"  // HH_TILE_PATHS; <stddef.h>, <stdint.h>

namespace hh {

constexpr int kTile = HH_TILE_PATHS;  // paths per tile == paths per workgroup
inline uint32_t tiles_for(uint64_t n_paths) { return (uint32_t)((n_paths + kTile - 1) / kTile); }

// the regions of a layout in order: take(n, a) is where the next one, of n units on a boundary of a, starts
struct LayoutCursor {
  size_t at = 0;
  size_t take(size_t n, size_t a = 1) {
    at = ((at + a - 1) & ~(a - 1)) + n;
    return at - n;
  }
};

// ---- LSM (hh_lsm.hip) ------------------------------------------------------------------------------------------

constexpr int kLsmWg = 512;     // threads per workgroup of every kernel that forms canonical sums
constexpr int kLsmQSmall = 1024 / kLsmWg, kLsmQLarge = 8192 / kLsmWg;  // trajectories per lane
constexpr uint64_t kLsmQ1Max = 1ull << 18;  // up to here chunks of 1024 trajectories, beyond it 8192
constexpr int kLsmMaxResident = 256;        // chunks the persistent form handles (one per workgroup)
constexpr int kLsmRing = 16;                // record slots of the persistent all-gather (2 suffice for
                                            // correctness; 16 dates between two uses of a slot make it all
                                            // but certain that no L2 still holds the slot's previous lines)
// slots behind the row counters that hh_lsm_debug_read returns (the phase stamps of a diagnostic build that has
// been removed; profiles/ has its measurements).  Nothing writes them now: their contents are unspecified.
constexpr int kLsmStampSlots = 8;

// Trajectories per lane: the smallest of 2, 4, 8, 16 (x 512 lanes = chunks of 1024 … 8192) with which
// the ensemble fits 256 chunks — one workgroup per CU in the persistent form, whose date is bounded by
// what ONE workgroup has to do (a 10^6-trajectory induction in chunks of 8192 would keep half the chip
// idle and every busy CU twice as long).  The chunk size is part of the summation tree: both forms of
// the induction (and every phase of the sharded one) use lsm_q() of the same ensemble.
inline int lsm_q(uint64_t ntot) {
  int q = kLsmQSmall;
  for (uint64_t cap = kLsmQ1Max; q < kLsmQLarge && ntot > cap; cap <<= 1) q <<= 1;
  return q;
}
inline uint32_t lsm_nch(uint64_t ntot) {
  const uint64_t per = (uint64_t)kLsmWg * lsm_q(ntot);
  return (uint32_t)((ntot + per - 1) / per);
}

// offsets in doubles
struct LsmScratch {
  size_t sync, ring, rec_stats, rowstat, rec_pow, P, recB, disc_pow, counters, stamps, total;
  uint32_t rows, nch;
  int q;
  LsmScratch(uint64_t ntot, uint32_t n_steps, int degree) : rows(n_steps + 1), nch(lsm_nch(ntot)), q(lsm_q(ntot)) {
    const size_t r = rows, ch = nch, nv = 2 * (size_t)degree + 1;
    LayoutCursor c;
    // persistent form: the uint32 status word, padded to 16 bytes, and the record ring of records of 32 granules of
    // 16 bytes; the two are zeroed per launch, [sync, rec_stats)
    sync = c.take(2);
    ring = c.take((size_t)kLsmRing * kLsmMaxResident * 32 * 2);
    rec_stats = c.take(r * ch * 3);            // [rows][nch][3]
    rowstat = c.take(r * 3);                   // [rows] RowStat = 3 doubles
    rec_pow = c.take(r * ch * nv);             // [rows][nch][2D+1]
    P = c.take(r * nv);                        // [rows][2D+1]
    recB = c.take(r * ch * (degree + 1));      // [rows][nch][D+1]
    disc_pow = c.take(r);                      // [rows]
    // rows regressed, rows skipped, and the stamp slots: zeroed together when an induction starts, [counters, total)
    counters = c.take(2);
    stamps = c.take(kLsmStampSlots);
    total = c.at;
  }
};

// ---- LSM on several state rows (hh_lsm_multi.hip) ---------------------------------------------------------------

constexpr int kLsmMultiPad = 48;         // a padded basis: three tiles of 16 (HH_LSM_MAX_BASIS = 45 functions)
constexpr int kLsmMultiStats = 1 + 2 * HH_MAX_ASSETS;  // n, Σv_i (μ_i), Σv_i² (isd_i) of a date
constexpr int kLsmMultiTileDoubles = 6 * 256;  // a chunk's Gram record: the 6 tile products of the upper block triangle
constexpr int kLsmMultiRowBlock = 8;     // dates whose Gram records are held at a time

// offsets in doubles; the chunk rule is the one-variable induction's (lsm_q, lsm_nch)
struct LsmMultiScratch {
  size_t rec_stats, rowstat, rec_gram, G, recB, coef, have_fit, disc_pow, counters, total;
  uint32_t rows, nch;
  int q;
  LsmMultiScratch(uint64_t ntot, uint32_t n_dates) : rows(n_dates + 1), nch(lsm_nch(ntot)), q(lsm_q(ntot)) {
    const size_t r = rows, ch = nch;
    LayoutCursor c;
    rec_stats = c.take(r * ch * kLsmMultiStats);                        // [date][chunk][17]
    rowstat = c.take(r * kLsmMultiStats);                               // [date][17]
    rec_gram = c.take((size_t)kLsmMultiRowBlock * ch * kLsmMultiTileDoubles);  // [date of the block][chunk][6][256]
    G = c.take(r * kLsmMultiPad * kLsmMultiPad);                        // [date][48][48]
    recB = c.take(r * ch * kLsmMultiPad);                               // [date][chunk][48]
    // zeroed together when an induction starts, [coef, total): the coefficients [date][48], the fit flags (an int32 per
    // date), the discount table [date] and the counters (rows regressed, rows skipped)
    coef = c.take(r * kLsmMultiPad);
    have_fit = c.take((r + 1) / 2);
    disc_pow = c.take(r);
    counters = c.take(2);
    total = c.at;
  }
};

// ---- path statistics (hh_path.hip) ----------------------------------------------------------------------------

// What path_stats_kernel leaves of every trajectory and path_payoff_kernel reads: one row per statistic (enum
// hh_path_stat), step-major like the path grids — stats[stat][column], column i = trajectory i, column n_paths + i
// its antithetic mirror.  `rows`: HH_PATH_STATS, or HH_PATH_STATS_BRIDGE when the two continuous extremes follow the
// five.  Offsets in doubles.  (constexpr: the two kernels index with it too)
struct PathStatsLayout {
  size_t n_total, total;
  constexpr PathStatsLayout(uint64_t n_paths, bool antithetic, int rows = HH_PATH_STATS)
      : n_total((size_t)n_paths * (antithetic ? 2 : 1)), total((size_t)rows * n_total) {}
  constexpr size_t row(int stat) const { return (size_t)stat * n_total; }
};

// What path_tangent_kernel leaves of every trajectory and path_payoff_tangent_kernel reads (include/hedgehog_mc.h,
// "Pathwise derivatives of path-dependent payoffs"): the five value rows of PathStatsLayout, the three date rows, then
// five tangent rows per carried basis slot — rows[row][column], the same columns.  Offsets in doubles.
struct PathTangentLayout {
  size_t n_total, total;
  int n_active;
  constexpr PathTangentLayout(uint64_t n_paths, bool antithetic, int n_active_)
      : n_total((size_t)n_paths * (antithetic ? 2 : 1)),
        total((size_t)(HH_PATH_STATS + HH_TANGENT_DATE_ROWS + HH_TANGENT_ROWS_PER_SLOT * n_active_) * n_total),
        n_active(n_active_) {}
  constexpr size_t row(int r) const { return (size_t)r * n_total; }
  // tangent row `which` (enum hh_path_tangent_row) of carried slot b
  constexpr size_t slot_row(int b, int which) const {
    return (size_t)(HH_PATH_STATS + HH_TANGENT_DATE_ROWS + HH_TANGENT_ROWS_PER_SLOT * b + which) * n_total;
  }
};

// ---- Broadie–Kaya (hh_bk.hip) ----------------------------------------------------------------------------------

// Columns of cached series terms.  A lane's column belongs to a workgroup SLOT that a workgroup of the
// CF kernel (or of the ladder kernel behind it) takes when it starts and gives back when it is done —
// not to the trajectory: the cache is kSlots x 256 columns however many trajectories the chain has
// (1536 slots: the CF kernel takes 95 registers since its real-axis evaluations, so FIVE of its workgroups are
// resident per CU, 1280 in all — with 1024 slots the fifth spun for a slot and the kernel ran 3 % slower than at a
// forced four; with a slot for it, 5 % faster (profiles/r05_h_bk_ab.txt).  A bitmap word is 64 slots, hence 192
// per XCD.  256 terms of 8 bytes: 0.81 GB for 10^4 and for 10^8 trajectories alike).  A trajectory's terms are only needed again if its secant fails (2 % of
// them): the ladder kernel re-derives those.
constexpr int kSlots = 1536;
constexpr int kHeavyGrid = 64;   // workgroups of the tail kernel (169 registers: it holds the whole-trajectory
                                  // code, idle with the reference's controls and the whole job when no series fits the
                                  // term cache; its first kRecStride workgroups then add the records)
static_assert(kHeavyGrid <= kSlots, "the tail kernel's workgroup b uses slot b");
constexpr int kXcds = 8, kSlotLineWords = 16, kSlotLineBytes = 8 * kSlotLineWords;  // a 128-byte line of slot bitmap words per XCD
// series terms cached per column: HH_OPT_BK_TERM_CACHE; 0 = this
constexpr int kBkTermCacheDefault = 256;
constexpr int kSortRun = 1024;  // consecutive pairs per wave of the grid sort

// Offsets in bytes.  The head (everything in front of phi_cache) depends on the chain's size and on nothing else: a
// grid's last, shorter batch of dates has its tables at a place of its own.
struct BkScratch {
  size_t long_mask, slot_lines, counters, args, tables, phi_cache, draws, iv, diag, total;
  size_t zeroed_bytes;  // from slot_lines: the bitmaps and the counters start from zero, and every chain leaves them so
  size_t cache_columns, lanes;
  int cache_cap;
  uint32_t n_tiles;
  BkScratch(uint64_t n_chain, int term_cache, size_t sizeof_args, size_t sizeof_tables)
      : cache_cap(term_cache > 0 ? term_cache : kBkTermCacheDefault), n_tiles(tiles_for(n_chain)) {
    // columns of cached terms: one per lane of a workgroup slot (fewer slots than tiles are never needed), so the
    // cache does not grow with the ensemble
    const size_t slots = n_tiles < (uint32_t)kHeavyGrid ? kHeavyGrid : n_tiles < (uint32_t)kSlots ? n_tiles : kSlots;
    cache_columns = slots * kTile;
    lanes = (size_t)n_tiles * kTile;
    LayoutCursor c;
    long_mask = c.take((size_t)n_tiles * (kTile / 64) * sizeof(uint64_t));  // ballots of the too-long trajectories
    slot_lines = c.take(kXcds * kSlotLineBytes, kSlotLineBytes);  // slot bitmaps: one 128-byte line per XCD
    counters = c.take(kSlotLineBytes);          // the line behind them: BkArgs::counters (word 1: records written)
    zeroed_bytes = c.at - slot_lines;
    args = c.take(sizeof_args, 256);            // device copy of the argument block
    tables = c.take(sizeof_tables, 256);        // Bessel tables and ϕ(0) constants
    phi_cache = c.take(cache_columns * (size_t)cache_cap * sizeof(double), 256);  // [cache_cap][cache_columns]
    draws = c.take(4 * lanes * sizeof(double));                                   // per lane from here on: [4][lanes]
    iv = c.take(lanes * sizeof(double));                                          // ∫V [lanes]
    diag = c.take(2 * lanes * sizeof(uint32_t));  // decision words [lanes], then series lengths [lanes]
    total = c.at;
  }
};

// the ordered form of a grid chain over n_chain pairs; offsets in bytes
struct BkSortScratch {
  size_t perm, counts, totals, keys, total;
  uint32_t n_runs;
  explicit BkSortScratch(uint64_t n_chain) : n_runs((uint32_t)((n_chain + kSortRun - 1) / kSortRun)) {
    const size_t lanes = (size_t)tiles_for(n_chain) * kTile;
    LayoutCursor c;
    perm = c.take(lanes * sizeof(uint32_t));                   // the order [lanes] x uint32
    counts = c.take((size_t)256 * n_runs * sizeof(uint32_t));  // [256][n_runs] x uint32
    totals = c.take(256 * sizeof(uint32_t));                   // [256] x uint32
    keys = c.take(lanes + 256);                                // [lanes] x uint8, and 256 bytes to spare
    total = c.at;
  }
};

}  // namespace hh
