// Who owns device memory (host only): one move-only owner per hipMalloc / hipHostMalloc allocation, the front-to-back layout of
// the pieces inside one, and the all-or-nothing first allocation of a feature's arrays.  Nothing outside this header calls hipFree.
#pragma once

#include <string>
#include <utility>

#include "common.h"

namespace tl {

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// one allocation laid out front to back: carve(bytes) is where the next 256-byte-aligned piece starts, carve.off the bytes taken so far
struct Carve {
    size_t off = 0;
    size_t operator()(size_t bytes) {
        const size_t at = off;
        off = align_up(off + bytes, 256);
        return at;
    }
};

// One allocation on the device (alloc) or in pinned host memory (alloc_pinned), freed with its owner.  alloc on a block that holds
// memory releases that first; a failed alloc leaves the block empty.  `what` is the whole message of the failure.
class DeviceBlock {
  public:
    DeviceBlock() = default;
    DeviceBlock(DeviceBlock &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)), pinned_(o.pinned_) {}
    DeviceBlock &operator=(DeviceBlock &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr), bytes_ = std::exchange(o.bytes_, 0), pinned_ = o.pinned_;
        }
        return *this;
    }
    DeviceBlock(const DeviceBlock &) = delete;
    DeviceBlock &operator=(const DeviceBlock &) = delete;
    ~DeviceBlock() { reset(); }

    int alloc(size_t bytes, const std::string &what) { return take(bytes, false, what); }
    int alloc_pinned(size_t bytes, const std::string &what) { return take(bytes, true, what); }
    void reset() {
        if (p_) (void)(pinned_ ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr, bytes_ = 0;
    }
    template <class T = char>
    T *at(size_t off = 0) const {
        return (T *)((char *)p_ + off);
    }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }

  private:
    int take(size_t bytes, bool pinned, const std::string &what) {
        reset();
        void *p = nullptr;
        if ((pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes)) != hipSuccess) return fail(TL_ERR_HIP, what);
        p_ = p, bytes_ = bytes, pinned_ = pinned;
        return TL_OK;
    }
    void *p_ = nullptr;
    size_t bytes_ = 0;
    bool pinned_ = false;
};

// A feature's first allocation, all or nothing: a fresh block of `bytes`, then `fill(base)` -- the memsets, launches and copies that
// give the pieces their first values; it returns TL_OK or its own failure -- and only then does `dst` own the block.  After any
// failure the block is released and `dst` is what it was (empty), so the caller's "allocated already?" test stays true to the memory.
template <class Fill>
static int alloc_filled(DeviceBlock &dst, size_t bytes, const std::string &what, Fill fill) {
    DeviceBlock b;
    const int rc = b.alloc(bytes, what);
    if (rc != TL_OK) return rc;
    const int filled = fill(b.at<char>());
    if (filled != TL_OK) return filled;
    dst = std::move(b);
    return TL_OK;
}

}  // namespace tl
