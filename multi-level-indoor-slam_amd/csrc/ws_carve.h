// Carving a caller-allocated workspace into typed buffers.
//
// Every pipeline has ONE carve function, `size_t x_carve(<shape>, void* base, XBufs* out)`:
// the only place its buffer sizes are written, as element counts of each buffer's real type.
// With base == nullptr it is the size query (every pointer null, nothing dereferenced); with
// the caller's workspace it yields the pointers the kernels get.  Both passes run the same
// takes, so the size a caller allocated and the layout the kernels write cannot disagree.
// Plain C++17, no HIP: tests/native/ws_carve_test.cpp checks it under the sanitizers.
#pragma once
#include <stddef.h>

// every region starts on a 256-byte boundary of the workspace
inline size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

class WsCarver {
  public:
    explicit WsCarver(void* base) : base_(static_cast<char*>(base)) {}
    // `count` elements of T at the current position (null in a size query); count 0 is
    // legal: the current position, no advance
    template <class T>
    T* take(size_t count) {
        T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
        off_ += a256(count * sizeof(T));
        return p;
    }
    size_t total() const { return off_; }

  private:
    char* base_;
    size_t off_ = 0;
};
