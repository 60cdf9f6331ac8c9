// buf_check.cpp -- keto_amd/csrc/kg_buf.h (Buf and BlockPool) over a counting malloc, built with the host
// sanitizers and run as a child process by tests/test_host.py::test_buf_under_sanitizers.  Exit status 0:
// every property below held and the sanitizers saw no leak, double free or overflow.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "kg_buf.h"

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

// malloc with a size header: counts calls and live bytes, and fails the next allocation on request.
struct CountMem {
  static inline size_t allocs = 0, frees = 0, live = 0, high = 0;
  static inline int fail_next = 0;  // the code the next alloc returns (then cleared)
  static int alloc(void** p, size_t bytes) {
    if (fail_next) {
      const int e = fail_next;
      fail_next = 0;
      return e;
    }
    size_t* h = static_cast<size_t*>(malloc(bytes + 16));
    if (!h) return 2;
    h[0] = bytes;
    allocs++;
    live += bytes;
    if (live > high) high = live;
    *p = reinterpret_cast<char*>(h) + 16;
    return 0;
  }
  static void free(void* p) {
    size_t* h = reinterpret_cast<size_t*>(static_cast<char*>(p) - 16);
    frees++;
    live -= h[0];
    ::free(h);
  }
  static void restart() { allocs = frees = live = high = 0; }
};

template <class T>
using B = kg::Buf<T, CountMem>;

static void reserve_within_capacity() {
  CountMem::restart();
  B<int> b;
  CHECK(b.empty() && b.cap() == 0 && b.get() == nullptr);
  CHECK(b.reserve(100) == 0);
  int* p = b.get();
  for (int i = 0; i < 100; i++) p[i] = i;  // the whole block is ours (ASan checks)
  CHECK(b.reserve(100) == 0 && b.reserve(1) == 0 && b.reserve(0) == 0);
  CHECK(b.get() == p && b.cap() == 100);
  CHECK(CountMem::allocs == 1 && CountMem::frees == 0);
}

static void growing_reserve_frees_first() {
  CountMem::restart();
  {
    B<int> b;
    CHECK(b.reserve(100) == 0);
    CHECK(b.reserve(250) == 0);
    CHECK(b.cap() == 250 && !b.empty());
    CHECK(CountMem::allocs == 2 && CountMem::frees == 1);
    CHECK(CountMem::high == 250 * sizeof(int));  // max(old, new): the old block went first
    CHECK(CountMem::live == 250 * sizeof(int));
    b.get()[249] = 1;
    B<void> v;  // bytes
    CHECK(v.reserve(33) == 0 && v.cap() == 33);
    CHECK(CountMem::live == 250 * sizeof(int) + 33);
  }
  CHECK(CountMem::live == 0 && CountMem::allocs == CountMem::frees);
}

static void failed_allocation() {
  CountMem::restart();
  B<int> b;
  CHECK(b.reserve(10) == 0);
  CountMem::fail_next = 77;
  CHECK(b.reserve(20) == 77);  // the policy's code, unchanged
  CHECK(b.empty() && b.cap() == 0 && b.get() == nullptr);
  CHECK(CountMem::live == 0 && CountMem::frees == 1);
  CHECK(b.reserve(20) == 0 && b.cap() == 20 && !b.empty());
  CountMem::fail_next = 5;  // a failure on an empty buffer
  B<int> c;
  CHECK(c.reserve(1) == 5 && c.empty() && c.cap() == 0);
}

static void moves() {
  CountMem::restart();
  {
    B<int> a;
    CHECK(a.reserve(8) == 0);
    int* p = a.get();
    B<int> b(std::move(a));
    CHECK(a.empty() && a.cap() == 0 && b.get() == p && b.cap() == 8);
    B<int> c;
    CHECK(c.reserve(4) == 0);
    c = std::move(b);  // c's own block is freed here
    CHECK(b.empty() && b.cap() == 0 && c.get() == p && c.cap() == 8);
    CHECK(CountMem::frees == 1);
    B<int>& self = c;
    c = std::move(self);
    CHECK(c.get() == p && c.cap() == 8);
  }
  CHECK(CountMem::allocs == 2 && CountMem::frees == 2 && CountMem::live == 0);
}

static void reset_and_release() {
  CountMem::restart();
  int* kept = nullptr;
  {
    B<int> a, b;
    CHECK(a.reserve(8) == 0 && b.reserve(8) == 0);
    a.reset();
    CHECK(a.empty() && a.cap() == 0 && CountMem::frees == 1);
    a.reset();  // again: nothing to free
    CHECK(CountMem::frees == 1);
    kept = b.release();
    CHECK(kept && b.empty() && b.cap() == 0);
  }
  CHECK(CountMem::frees == 1 && CountMem::live == 8 * sizeof(int));  // the released block is the caller's
  kept[7] = 1;
  CountMem::free(kept);
  CHECK(CountMem::live == 0);
}

static void pool() {
  CountMem::restart();
  constexpr size_t MiB = 1 << 20;
  {
    kg::BlockPool<CountMem> P(4 * MiB);
    CHECK(P.size_class(1) == MiB && P.size_class(MiB) == MiB && P.size_class(MiB + 1) == 2 * MiB);
    void* a = P.get(0, 1000);
    CHECK(a && CountMem::live == MiB);  // a whole class, whatever was asked for
    P.put(0, a, 1000);
    CHECK(CountMem::frees == 0);  // cached
    void* other_class = P.get(0, MiB + 1);
    void* other_key = P.get(1, 1000);
    CHECK(other_class != a && other_key != a && CountMem::allocs == 3);
    void* again = P.get(0, 5000);  // same class, same key: the cached block
    CHECK(again == a && CountMem::allocs == 3);
    P.put(0, nullptr, 1000);  // nothing
    // key 0 keeps at most 4 MiB: 1 + 2 fit, a second 2 MiB block does not and is freed
    void* c2 = P.get(0, 2 * MiB);
    CHECK(CountMem::allocs == 4);
    P.put(0, a, 1000);
    P.put(0, other_class, MiB + 1);
    CHECK(CountMem::frees == 0);
    P.put(0, c2, 2 * MiB);
    CHECK(CountMem::frees == 1 && CountMem::live == 4 * MiB);  // a, other_class cached; other_key held by us
    CHECK(!P.keep(0, other_key, 2 * MiB));                    // 3 + 2 > 4: not taken, still ours
    P.put(1, other_key, 1000);                                // key 1 has its own allowance
    CHECK(CountMem::frees == 1);
    CHECK(P.get(1, 1) == other_key && P.get(0, 2 * MiB) == other_class && P.get(0, 1) == a);
    CHECK(CountMem::allocs == 4);
    CountMem::fail_next = 9;
    CHECK(P.get(0, 1) == nullptr);  // nothing cached, and the allocation fails
    // the pool does not free what it still caches (a process-wide pool lives as long as the process);
    // hand everything back and take it out again so that this program ends with nothing live
    for (void* p : {a, other_class, other_key}) CountMem::free(p);
  }
  CHECK(CountMem::live == 0);
}

int main() {
  reserve_within_capacity();
  growing_reserve_frees_first();
  failed_allocation();
  moves();
  reset_and_release();
  pool();
  puts("buf_check ok");
  return 0;
}
