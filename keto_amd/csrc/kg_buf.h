// kg_buf.h -- the one owner of device and pinned-host memory in libketogpu, and the size-class pool of
// the tree outputs.  No HIP here: the memory comes from a policy `Mem` with
//   static int alloc(void** p, size_t bytes);   // 0 or the allocator's error code
//   static void free(void* p);
// (DeviceMem / PinnedMem in kg_snapshot.h; a counting malloc in tests/buf_check.cpp).
#pragma once
#include <stddef.h>

#include <mutex>
#include <vector>

namespace kg {

template <class T> struct buf_unit { static constexpr size_t bytes = sizeof(T); };
template <> struct buf_unit<void> { static constexpr size_t bytes = 1; };

// Move-only owner of a T* and its capacity in elements (bytes for T = void).  The caller decides how
// much to ask for (minimums, doubling, back-off): reserve neither rounds nor pads.
template <class T, class Mem>
class Buf {
  T* p_ = nullptr;
  size_t cap_ = 0;

 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~Buf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }
  size_t cap() const { return cap_; }
  bool empty() const { return !p_; }

  // Room for n elements, contents not kept: a buffer that is too small is freed before the new one is
  // allocated (peak = max(old, new), not the sum).  On failure the buffer is empty and the
  // allocator's code is returned.
  int reserve(size_t n) {
    if (p_ && n <= cap_) return 0;
    reset();
    void* q = nullptr;
    const int e = Mem::alloc(&q, n * buf_unit<T>::bytes);
    if (e) return e;
    p_ = static_cast<T*>(q);
    cap_ = n;
    return 0;
  }
  void reset() {
    if (p_) Mem::free(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // Hands the block on (to a pool, across the C ABI); the caller frees it.
  T* release() {
    T* p = p_;
    p_ = nullptr;
    cap_ = 0;
    return p;
  }
};

// Blocks in power-of-two size classes from 1 MiB, cached per key (the device of HBM blocks, 0 for
// pinned memory) when they come back, up to `keep` bytes per key; past that they are freed.
template <class Mem>
class BlockPool {
  struct Blk {
    int key;
    size_t cls;
    void* p;
  };
  const size_t keep_;
  std::mutex mu_;
  std::vector<Blk> free_;

 public:
  explicit BlockPool(size_t keep) : keep_(keep) {}
  BlockPool(const BlockPool&) = delete;
  static size_t size_class(size_t bytes) {
    size_t c = 1 << 20;
    while (c < bytes) c <<= 1;
    return c;
  }
  // A cached block of the class and key, or a fresh one (nullptr: the allocation failed).
  void* get(int key, size_t bytes) {
    const size_t c = size_class(bytes);
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (Blk& b : free_)
        if (b.key == key && b.cls == c) {
          void* p = b.p;
          b = free_.back();
          free_.pop_back();
          return p;
        }
    }
    void* p = nullptr;
    return Mem::alloc(&p, c) ? nullptr : p;
  }
  // Caches p if the key's cached bytes stay within `keep`; false: the caller still owns p.
  bool keep(int key, void* p, size_t bytes) {
    const size_t c = size_class(bytes);
    std::lock_guard<std::mutex> lk(mu_);
    size_t cached = 0;
    for (const Blk& b : free_)
      if (b.key == key) cached += b.cls;
    if (cached + c > keep_) return false;
    free_.push_back(Blk{key, c, p});
    return true;
  }
  void put(int key, void* p, size_t bytes) {
    if (p && !keep(key, p, bytes)) Mem::free(p);
  }
};

}  // namespace kg
