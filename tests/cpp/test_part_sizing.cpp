// Host-only check of the sub-slot sizing of the histogram-free partition (kmerhash_amd/csrc/kh_part_sizing.h): no GPU, no HIP.
#include "../../kmerhash_amd/csrc/kh_part_sizing.h"

#include <cstdio>
#include <cstdlib>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static const uint32_t TILE = 8192;

// what partition_batch computes for a batch that is no streamed piece
static uint64_t sub_of(uint64_t n, uint32_t PB, double vf, uint32_t min_tiles, uint32_t* tps, uint64_t* slot1_out = nullptr) {
  const uint32_t B1 = (PB + 1) / 2, B2 = PB - B1, nb1 = 1u << B1, nb2 = 1u << B2;
  const uint64_t slot = slack_slot((double)n / (double)(1ull << PB), vf), slot1 = slot * nb2;
  if (slot1_out) *slot1_out = slot1;
  return xcd_sub_slot(n, nb1, nb2, slot1, vf, TILE, min_tiles, tps);
}

int main() {
  uint32_t tps = 99;
  uint64_t slot1 = 0;
  // the benchmark shape: 107374184 records, 2^16 partitions: slot 1937, sub-slot 32 * 1937 = 61984, 7 tiles per sub-slot
  CHECK(slack_slot(107374184.0 / 65536.0) == 1937);
  CHECK(sub_of(107374184ull, 16, 1.0, 4, &tps, &slot1) == 61984 && tps == 7 && slot1 == 61984ull * 8);
  // the sub-slot holds its own mean + 7 sigma with the mean of ceil(ntiles / 8) tiles
  { const uint64_t ntiles = (107374184ull + TILE - 1) / TILE; const double m = (double)(((ntiles + 7) / 8) * TILE) / 256.0; CHECK(61984 >= slack_slot(m)); }
  // 6e6 records into 2^12 partitions: 1.4 tiles per sub-slot -- used from min_tiles = 1, not at the default of 4
  CHECK(sub_of(6000000, 12, 1.0, 4, &tps) == 0 && tps == 0);
  CHECK(sub_of(6000000, 12, 1.0, 1, &tps) == 13984 && tps == 2);
  CHECK(sub_of(6000001, 12, 1.0, 1, &tps) == 13984 && tps == 2);
  // fall-backs: fewer than eight buckets or digits, a slot that does not divide by eight, an empty batch
  CHECK(xcd_sub_slot(1000000, 4, 64, 8000, 1.0, TILE, 0, &tps) == 0 && tps == 0);
  CHECK(xcd_sub_slot(1000000, 64, 4, 8000, 1.0, TILE, 0, &tps) == 0);
  CHECK(xcd_sub_slot(1000000, 64, 64, 20001, 1.0, TILE, 0, &tps) == 0);
  CHECK(xcd_sub_slot(0, 64, 64, 8000, 1.0, TILE, 0, &tps) == 0);
  // fall-back: an eighth of the slot below the sub-slot's mean + 7 sigma (a large variance factor; a slot only just above the mean)
  CHECK(xcd_sub_slot(6000000, 64, 64, 8 * 12000, 1.0, TILE, 0, &tps) == 0);        // mean1 = 92 tiles * 8192 / 64 = 11776, + 7 sigma = 12551
  CHECK(xcd_sub_slot(6000000, 64, 64, 8 * 12552, 1.0, TILE, 0, &tps) == 12552);
  CHECK(xcd_sub_slot(6000000, 64, 64, 8 * 12552, 4.0, TILE, 0, &tps) == 0);
  // sweep: whenever sub-slots are used, the invariants the kernels rely on hold
  for (uint32_t PB = 12; PB <= 22; ++PB)
    for (uint64_t n = 256ull << PB; n < (4096ull << PB) && n < 0xFFFFFFF0ull; n += n / 3 + 12345)
      for (double vf : {1.0, 2.5, 7.0})
        for (uint32_t mt : {0u, 1u, 4u}) {
          const uint64_t sub = sub_of(n, PB, vf, mt, &tps, &slot1);
          if (!sub) { CHECK(tps == 0); continue; }
          const uint32_t nb1 = 1u << ((PB + 1) / 2);
          const uint64_t ntiles = (n + TILE - 1) / TILE;
          const double m = (double)std::min<uint64_t>(n, ((ntiles + 7) / 8) * (uint64_t)TILE) / (double)nb1;
          CHECK(sub * 8 == slot1);
          CHECK(sub >= slack_slot(m, vf));
          CHECK(m >= (double)mt * TILE);
          CHECK(tps >= 1 && (uint64_t)(tps - 1) * TILE < sub);                     // every tile of a sub-slot starts inside it
          CHECK((uint64_t)nb1 * 8 * tps < 0xFFFFFFFFull);                          // the second pass' grid
          CHECK((uint64_t)nb1 * 8 <= (1ull << PB));                                // k_init_cursors2: one thread per partition covers the cursors
        }
  if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
  std::printf("part sizing ok\n");
  return 0;
}
