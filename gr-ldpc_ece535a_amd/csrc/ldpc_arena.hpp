// ldpc_arena.hpp -- cutting one buffer into 256-byte-aligned regions (host).
//
// A layout is written once, as a walk of take<T>(count) calls.  Over a null
// base the walk only measures: every take returns nullptr and bytes() is the
// size to allocate.  Over the allocated buffer the same walk hands out the
// regions, so a size and its carve cannot drift apart.  The one definition of
// the 256-byte rounding in csrc/.
#pragma once

#include <stddef.h>

namespace ldpc {

class Arena {
 public:
  explicit Arena(void *base = nullptr) : base_((char *)base) {}
  // the next region: count elements of T, the walk advanced to the next
  // multiple of 256 bytes
  template <typename T>
  T *take(size_t count) {
    const size_t at = used_;
    used_ += (count * sizeof(T) + 255) & ~(size_t)255;
    return base_ ? (T *)(base_ + at) : nullptr;
  }
  size_t bytes() const { return used_; }

 private:
  char *base_;
  size_t used_ = 0;
};

}  // namespace ldpc
