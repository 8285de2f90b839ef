// Host-only sizing arithmetic of the histogram-free partition (no HIP: tests/cpp/test_part_sizing.cpp compiles it alone).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

// slot of a histogram-free partition with mean m records: m + 7 sigma (hashed keys: Poisson) + a little
// (vf: variance of a partition's fill over its mean -- 1 for distinct keys (Poisson in the records); a batch with duplicates fills its partitions
//  key by key, E[m^2] / E[m] records at a time: insert_core estimates that factor from the duplicate sample)
static inline uint64_t slack_slot(double mean, double vf = 1.0) { return (uint64_t)(mean + 7.0 * std::sqrt(mean * vf) + 16.0); }

// Sizing of the eight sub-slots of a level-1 slot (XCD-private write fronts, KhPartParams::sub_slot).  Workgroup w of the first pass
// appends to sub-slot w & 7, so a sub-slot takes the records of ceil(ntiles / 8) tiles of `tile` records at most: mean1 = that many
// tiles' records over the nb1 buckets.  The sub-slots are used when
//  - nb1 is a multiple of eight (the second pass hands buckets x, x + 8, ... to XCD x) and nb1 * 8 <= nb1 * nb2 (k_init_cursors2 has one
//    thread per final partition and sets the nb1 * 8 level-1 cursors with them),
//  - the slot divides by eight and an eighth of it holds mean1 + 7 sigma (slack_slot),
//  - mean1 is at least min_tiles tiles: the second pass cuts every sub-slot into tiles of its own, the last of them partly filled; below a
//    few tiles per sub-slot it would run more and shorter tiles than without sub-slots (shorter output runs, more reservations).
// Returns the sub-slot's size (0: one cursor per bucket) and, in *tps, the tiles the second pass cuts a sub-slot into (mean1 + 9 sigma,
// like the whole slots).
static inline uint64_t xcd_sub_slot(uint64_t n, uint32_t nb1, uint32_t nb2, uint64_t slot1, double vf, uint32_t tile, uint32_t min_tiles, uint32_t* tps) {
  *tps = 0;
  if (nb1 < 8 || nb2 < 8 || slot1 % 8 != 0 || n == 0) return 0;
  const uint64_t ntiles = (n + tile - 1) / tile;
  const double mean1 = (double)std::min<uint64_t>(n, ((ntiles + 7) / 8) * (uint64_t)tile) / (double)nb1;
  if (mean1 < (double)min_tiles * (double)tile) return 0;
  const uint64_t sub = slot1 / 8;
  if (sub < slack_slot(mean1, vf)) return 0;
  const uint64_t fill_cap = std::min<uint64_t>(sub, (uint64_t)(mean1 + 9.0 * std::sqrt(mean1 * vf) + 16.0));
  *tps = (uint32_t)((fill_cap + tile - 1) / tile);
  return sub;
}
