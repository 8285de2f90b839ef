// Layout of a scratch block, described once (no HIP: tests/cpp/test_scratch.cpp compiles it alone).
//
// A call writes its layout as ONE function of a carver -- a sequence of take<T>(count) -- and runs it twice: over a null base, where it
// only measures (every take returns null), and over the block of size() bytes it then allocates, where it hands out the pointers.  Size
// and pointers come from the same lines, so they cannot disagree.
//
// Contract of take<T>(count):
//  - count > 0: the next array of count elements.  It starts at a multiple of 256 bytes from the base (the base itself is 256-byte
//    aligned: a pooled block, hipMalloc's alignment) and the arrays follow one another in the order taken, each at the first such
//    multiple at or after the end of the one before it -- arrays taken in a row can be cleared with one memset.
//  - count == 0: null, in both modes, and nothing is consumed.  An optional array that is not wanted costs nothing and cannot be
//    mistaken for a usable pointer; a null array never aliases a neighbour.
#pragma once
#include <cstddef>
#include <cstdint>

struct KhCarver {
  static constexpr size_t kAlign = 256;
  explicit KhCarver(void* base = nullptr) : base_(reinterpret_cast<uintptr_t>(base)), off_(0) {}
  bool measuring() const { return base_ == 0; }
  size_t size() const { return off_; }      // bytes a block must have to hold everything taken so far
  template <typename T>
  T* take(uint64_t count) {
    static_assert(kAlign % alignof(T) == 0, "256-byte alignment covers the element type");
    if (count == 0) return nullptr;
    T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    off_ += (static_cast<size_t>(count) * sizeof(T) + kAlign - 1) & ~(kAlign - 1);
    return p;
  }

 private:
  uintptr_t base_;
  size_t off_;
};

// the size of a layout: its function run in measuring mode
template <typename F>
inline size_t kh_layout_size(F&& layout) {
  KhCarver c;
  layout(c);
  return c.size();
}
