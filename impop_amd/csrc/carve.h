// carve.h — the layout of one allocation cut into sub-buffers (plain C++, no HIP: tests/fuzz/carve_layout.cc compiles it on the host).
#pragma once
#include <stddef.h>

#include <functional>
#include <vector>

namespace impop {

// sub-buffers of one allocation start on 256-byte boundaries
inline size_t round_up_256(size_t x) { return (x + 255) / 256 * 256; }

// Hands out the offsets of consecutive sub-buffers and remembers the total: build the layout, ask ctx_scratch / ctx_pinned for
// total() bytes, then take pointers with at<T>(base, off) — from the device base and, where a region is mirrored in page-locked
// memory, from the host base with the same offsets.  A sub-buffer of zero bytes gets the offset of whatever follows it.
struct Carve {
    size_t used = 0;
    size_t take_bytes(size_t bytes) {
        const size_t off = round_up_256(used);
        used = off + bytes;
        return off;
    }
    template <typename T>
    size_t take(size_t count) { return take_bytes(count * sizeof(T)); }
    size_t total() const { return round_up_256(used); }  // a whole number of 256-byte units: the next region of a larger layout can follow
    template <typename T>
    static T *at(void *base, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(base) + off); }
};

// A Carve that also remembers whose pointer each sub-buffer is: list the sub-buffers once with sub(), allocate total() bytes, then
// bind(base) points every listed pointer into the allocation.  The size and the pointers cannot disagree: both come from one list.
struct Layout : Carve {
    std::vector<std::function<void(char *)>> binders;
    template <typename T>
    void sub(T *&p, size_t count) {
        const size_t off = take<T>(count);
        binders.push_back([&p, off](char *base) { p = reinterpret_cast<T *>(base + off); });
    }
    void bind(void *base) const {
        for (const auto &b : binders) b(static_cast<char *>(base));
    }
};

}  // namespace impop
