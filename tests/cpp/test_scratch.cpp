// Host-only check of the scratch carver (kmerhash_amd/csrc/kh_scratch.h): no GPU, no HIP.  The carving pass runs over a fake base
// address and nothing is dereferenced, so the huge counts cost nothing.
#include "../../kmerhash_amd/csrc/kh_scratch.h"

#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

struct E16 { uint64_t a, b; };
struct Arr { uintptr_t at; uint64_t bytes; uint64_t count; };

static const uint64_t kCounts[] = {0, 1, 63, 64, 65, (uint64_t(1) << 32) + 1};
static const unsigned kNC = sizeof(kCounts) / sizeof(kCounts[0]);
static const uintptr_t kBase = uintptr_t(1) << 40;      // 256-byte aligned, as a pooled block is

// one array of `count` elements of `esize` bytes from the carver; what it got goes to `got` (carving pass only)
static void take_one(KhCarver& c, unsigned esize, uint64_t count, std::vector<Arr>* got) {
  void* p = nullptr;
  switch (esize) {
    case 1: p = c.take<uint8_t>(count); break;
    case 4: p = c.take<uint32_t>(count); break;
    case 8: p = c.take<uint64_t>(count); break;
    default: p = c.take<E16>(count); break;
  }
  if (got) got->push_back(Arr{reinterpret_cast<uintptr_t>(p), count * esize, count});
}

// a layout of three arrays, described once and run in both modes
static void check_layout(const unsigned es[3], const uint64_t cn[3]) {
  std::vector<Arr> got;
  auto layout = [&](KhCarver& c, std::vector<Arr>* g) { for (int i = 0; i < 3; ++i) take_one(c, es[i], cn[i], g); };
  // measuring: every take is null, and the size is what the carving pass ends at
  std::vector<Arr> meas;
  KhCarver m;
  CHECK(m.measuring());
  layout(m, &meas);
  for (const Arr& a : meas) CHECK(a.at == 0);
  CHECK(kh_layout_size([&](KhCarver& c) { layout(c, nullptr); }) == m.size());
  KhCarver c(reinterpret_cast<void*>(kBase));
  CHECK(!c.measuring());
  layout(c, &got);
  CHECK(c.size() == m.size());
  uintptr_t end = kBase;      // the end of the last non-empty array
  for (size_t i = 0; i < got.size(); ++i) {
    const Arr& a = got[i];
    if (a.count == 0) { CHECK(a.at == 0); continue; }      // zero elements: null, nothing consumed
    CHECK(a.at % 256 == 0);
    CHECK(a.at >= kBase && a.at + a.bytes <= kBase + c.size());
    CHECK(a.at >= end && a.at - end < 256);                 // in the order taken, at the first boundary after the one before
    end = a.at + a.bytes;
    for (size_t j = 0; j < i; ++j)
      if (got[j].count) CHECK(got[j].at + got[j].bytes <= a.at || a.at + a.bytes <= got[j].at);
  }
  CHECK(c.size() - (end - kBase) < 256);                    // at most the last array's padding after it
  uint64_t payload = 0, arrays = 0;
  for (const Arr& a : got) { payload += a.bytes; arrays += a.count != 0; }
  CHECK(c.size() >= payload && c.size() <= payload + 255 * arrays);      // a block grows by up to 255 bytes per array
}

int main() {
  const unsigned esz[] = {1, 4, 8, 16};
  for (unsigned e0 : esz) for (unsigned e1 : esz) for (unsigned e2 : esz)
    for (unsigned i = 0; i < kNC; ++i) for (unsigned j = 0; j < kNC; ++j) for (unsigned k = 0; k < kNC; ++k) {
      const unsigned es[3] = {e0, e1, e2};
      const uint64_t cn[3] = {kCounts[i], kCounts[j], kCounts[k]};
      check_layout(es, cn);
    }
  // nothing taken, or only empty arrays: no block at all
  { KhCarver c; CHECK(c.size() == 0); CHECK(c.take<uint32_t>(0) == nullptr && c.size() == 0); }
  { KhCarver c(reinterpret_cast<void*>(kBase)); CHECK(c.take<E16>(0) == nullptr && c.size() == 0);
    CHECK(reinterpret_cast<uintptr_t>(c.take<uint8_t>(1)) == kBase && c.size() == 256);
    CHECK(c.take<uint64_t>(0) == nullptr && c.size() == 256);      // an empty array between two others moves neither
    CHECK(reinterpret_cast<uintptr_t>(c.take<uint32_t>(64)) == kBase + 256 && c.size() == 512);
    CHECK(reinterpret_cast<uintptr_t>(c.take<uint32_t>(65)) == kBase + 512 && c.size() == 1024); }
  if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
  std::printf("scratch layout ok\n");
  return 0;
}
