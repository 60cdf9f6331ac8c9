// kg_lookup.hip -- reverse lookup: the objects of a namespace a subject has a relation on
// (OpenFGA ListObjects / SpiceDB LookupResources; no reference counterpart in Keto).
//
// The answer of a request (ns, rel, subject, max_depth) is defined through the check: the ascending
// object ids o with a node (ns, o, *) for which CheckIsMember(ns:o#rel@subject, max_depth) is IsMember.
// A request is answered in one of three modes (k_lk_resolve):
//   reverse        (ns, rel) has no rewrite or is a materialised union, and the reverse indexes exist:
//                  every member is a node of (ns, rel); a PURE node is a member iff its reverse distance
//                  from a holder of the subject is <= D-1 (what k_back decides for one root), so one
//                  target-free reverse walk lists them.  IMPURE nodes of (ns, rel) are confirmed.
//   confirm-nodes  the same without reverse indexes: every node of (ns, rel) is confirmed.
//   confirm-all    any other relation (interpreter / formula split / undeclared): every object of the
//                  namespace is confirmed.
// "Confirmed" = run through check_batch_device as kg_query rows built on the device; no check kernel
// is touched.  The walk is level-synchronous and bit-parallel over groups of 64 requests: a dense u64
// visited mask per node (bit = request), a frontier list per level, work assigned per reverse edge
// through a prefix over the frontier rows' lengths.  The masks are cleared by replaying the list of
// touched nodes, so a lookup costs what it reaches, not n_nodes.
//
// Subject lookup (kg_lookup_subjects, the second half of this file) is the mirror image: the subject ids
// that hold a relation on one object.  A pure root of such a relation is answered by a FORWARD walk over
// adj with the same masks, lists and output tail; everything else by a check of every subject id.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "kg_bfs.h"
#include "kg_internal.h"
#include "kg_snapshot.h"

namespace kg {
namespace {

typedef unsigned long long u64;

enum : uint32_t { LK_REVERSE = 0, LK_NODES = 1, LK_ALL = 2 };

// A resolved request.
struct LReq {
  uint32_t subj;    // tagged subject or NONE
  int32_t depth;    // clamped rest depth (>= 1)
  uint32_t mode;    // LK_*
  uint32_t hfirst, hcount;  // the subject's holders hold[hfirst, hfirst + hcount) (reverse mode)
  uint32_t pad;
};

// Device counters of one call.  Counts are TRUE counts: a count above its list's capacity means the
// list overflowed (nothing was written past it) and the step is rerun with a larger list.
struct LkCtl {
  u64 ocount;     // output keys (request << 32 | object)
  u64 edges;      // reverse edges read
  u64 ccount;     // candidate checks
  u64 dcount;     // domain keys (namespace slot << 32 | object)
  u64 confirmed;  // candidates answered IsMember
  u64 nuniq;      // output keys after the duplicates are dropped
  uint32_t fcount[2];  // the two frontier lists
  uint32_t tcount;     // touched nodes
  uint32_t over;       // a node list overflowed (they hold n_nodes entries: cannot happen)
};

// One request bit of a walk group.
struct GReq {
  uint32_t ns, rel, req;
  uint32_t root;  // forward walk: the request's root node
};

struct Walk {
  u64* vis;           // [n_nodes] request bits that reached the node
  u64* next;          // [n_nodes] bits that reached it at the level being built
  uint32_t* fout;     // the frontier list being built
  uint32_t fsel;      // its counter (LkCtl::fcount[fsel])
  uint32_t* touched;  // nodes whose vis left 0 (cleared by replay)
  uint32_t lcap;      // entries of the node lists
  u64* okeys;         // output keys
  u64 ocap;
  const GReq* greq;   // the group's requests, by bit
  LkCtl* ctl;
};

// The candidate tables of a call: the distinct (ns, rel) of its reverse / confirm-nodes requests and
// the distinct namespaces of its confirm-all requests, each with the requests that share it.
struct CandTab {
  const u64* keys;        // [K] ascending (ns << 32 | rel)
  const uint32_t* kall;   // [K] 1: every node of the key is a candidate (confirm-nodes), 0: impure nodes only
  const uint32_t* koff;   // [K + 1] into kreq
  const uint32_t* kreq;
  uint32_t K;
  const uint32_t* nsv;    // [M] ascending namespaces
  const uint32_t* nsoff;  // [M + 1] into nsreq
  const uint32_t* nsreq;
  uint32_t M;
};

__device__ __forceinline__ u64 wave_bcast64(u64 v, int src) { return shfl64(v, src); }

// Appends val where pred; one atomic per wave; entries past cap are dropped and flagged.
__device__ __forceinline__ void lk_append32(bool pred, uint32_t val, uint32_t* list, uint32_t* count, uint32_t cap,
                                            uint32_t* over) {
  const uint64_t m = __ballot(pred);
  if (!m) return;
  const int leader = __ffsll((unsigned long long)m) - 1;
  uint32_t base = 0;
  if (lane_id() == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
  base = __shfl(base, leader, 64);
  if (pred) {
    const uint32_t pos = base + lanes_below(m);
    if (pos < cap) list[pos] = val;
    else *over = 1;
  }
}
__device__ __forceinline__ void lk_append64(bool pred, u64 val, u64* list, u64* count, u64 cap) {
  const uint64_t m = __ballot(pred);
  if (!m) return;
  const int leader = __ffsll((unsigned long long)m) - 1;
  u64 base = 0;
  if (lane_id() == leader) base = atomicAdd(count, (u64)__popcll(m));
  base = wave_bcast64(base, leader);
  if (pred) {
    const u64 pos = base + lanes_below(m);
    if (pos < cap) list[pos] = val;
  }
}

__device__ __forceinline__ uint32_t lk_find64(const u64* a, uint32_t n, u64 key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && a[lo] == key ? lo : NONE;
}
__device__ __forceinline__ uint32_t lk_find32(const uint32_t* a, uint32_t n, uint32_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && a[lo] == key ? lo : NONE;
}

// ------------------------------------------------------------------ request mapping
__global__ __launch_bounds__(256) void k_lk_resolve(DevSnap s, const kg_lookup* __restrict__ q, uint32_t n,
                                                    int32_t global, uint64_t hold_n, LReq* __restrict__ lr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const kg_lookup x = q[i];
  uint32_t subj;
  if (x.sns == KG_SUBJECT_ID) {
    subj = x.sobj < 0x7FFFFFFFu ? x.sobj : NONE;
  } else {
    const uint32_t sn = nmap_find(s, x.sns, x.srel, x.sobj);
    subj = sn == NONE ? NONE : (SET_BIT | sn);
  }
  int32_t d = x.max_depth;
  if (d <= 0 || global < d) d = global;  // engine.go:68-70
  const uint8_t rf = relflag(s, x.ns, x.rel);
  const bool virt = s.virt && x.ns < s.n_ns && x.rel < s.n_rel && s.virt[(size_t)x.ns * s.n_rel + x.rel];
  const uint32_t mode = (rf == 0 || virt) ? (s.radj ? LK_REVERSE : LK_NODES) : LK_ALL;
  uint2 h = make_uint2(0, 0);
  if (mode == LK_REVERSE) {
    h = holders_find(s, subj);
    if ((uint64_t)h.x + h.y > hold_n) h = make_uint2(0, 0);  // never read past hold[]
  }
  lr[i] = LReq{subj, d, mode, h.x, h.y, 0};
}

// ------------------------------------------------------------------ the reverse walk
// Request bits m arrive at node p.  Called by every lane of a wave (act: this lane has a node).  New
// bits are recorded in vis / next (and returned), p joins the next frontier when it had no new bit yet
// and the touched list when it had no bit at all.
__device__ __forceinline__ u64 lk_mark(const DevSnap& s, const Walk& W, bool act, uint32_t p, u64 m) {
  u64 nb = 0;
  bool first = false, fresh = false;
  if (act && p < s.n_nodes && m) {
    const u64 old = atomicOr(&W.vis[p], m);
    nb = m & ~old;
    first = old == 0;
    if (nb) fresh = atomicOr(&W.next[p], nb) == 0;
  }
  lk_append32(fresh, p, W.fout, &W.ctl->fcount[W.fsel], W.lcap, &W.ctl->over);
  lk_append32(first, p, W.touched, &W.ctl->tcount, W.lcap, &W.ctl->over);
  return nb;
}

// The reverse walk's arrival: every new bit whose request asks for p's (ns, rel) lists p's object if p is
// pure.  Impure nodes are candidates of the confirmation (every ancestor of one is impure too).
__device__ __forceinline__ void lk_visit(const DevSnap& s, const Walk& W, bool act, uint32_t p, u64 m) {
  const u64 nb = lk_mark(s, W, act, p, m);
  uint32_t c = 0, pns = 0, prel = 0;
  if (nb && !(s.nflags && (s.nflags[p] & NF_IMPURE))) {
    pns = s.nd_ns[p];
    prel = s.nd_rel[p];
    for (u64 b = nb; b; b &= b - 1) {
      const GReq g = W.greq[__ffsll(b) - 1];
      c += (g.ns == pns && g.rel == prel) ? 1u : 0u;
    }
  }
  uint32_t tot;
  const uint32_t ex = wave_excl_scan(c, &tot);
  if (tot) {
    u64 base = 0;
    if (lane_id() == 0) base = atomicAdd(&W.ctl->ocount, (u64)tot);
    base = wave_bcast64(base, 0);
    if (c) {
      const uint32_t pobj = s.nd_obj[p];
      u64 pos = base + ex;
      for (u64 b = nb; b; b &= b - 1) {
        const GReq g = W.greq[__ffsll(b) - 1];
        if (g.ns == pns && g.rel == prel) {
          if (pos < W.ocap) W.okeys[pos] = ((u64)g.req << 32) | pobj;
          pos++;
        }
      }
    }
  }
}

// Level 0: one workgroup per request of the group strides over the subject's holders.
__global__ __launch_bounds__(256) void k_lk_seed(DevSnap s, Walk W, const LReq* __restrict__ lr) {
  const uint32_t b = blockIdx.x;
  const LReq r = lr[W.greq[b].req];
  for (uint32_t base = 0; base < r.hcount; base += 256) {
    const uint32_t i = base + threadIdx.x;
    const bool act = i < r.hcount;
    const uint32_t v = act ? s.hold[r.hfirst + i] : NONE;
    lk_visit(s, W, act, v, 1ull << b);
  }
}

// Before level j: every frontier node hands its new bits over (cmask, restricted to the requests
// whose depth still reaches level j) and frees next[]; len = its parent row, 0 when nothing is left to
// carry or the node is impure.  Thread F writes the sentinel and resets the list the level will build.
__device__ __forceinline__ u64 lk_prep_one(const DevSnap& s, u64* next, const uint32_t* cur, u64* cmask, uint32_t i,
                                           u64 live) {
  const uint32_t v = cur[i];
  u64 m = next[v];
  next[v] = 0;
  if (s.nflags && (s.nflags[v] & NF_IMPURE)) m = 0;
  m &= live;
  cmask[i] = m;
  return m ? s.radj_off[v + 1] - s.radj_off[v] : 0ull;
}

__global__ __launch_bounds__(256) void k_lk_prep(DevSnap s, u64* next, const uint32_t* __restrict__ cur, uint32_t F,
                                                 u64 live, u64* __restrict__ cmask, u64* __restrict__ len,
                                                 uint32_t* fcount_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < F) len[i] = lk_prep_one(s, next, cur, cmask, i, live);
  else if (i == F) {
    len[F] = 0;
    *fcount_out = 0;
  }
}

// One workgroup of 256: pref[i] = the sum of f(0 .. i - 1) for i in [0, F]; thread t calls f(i) for
// i = t, t + 256, ...
template <class Fn>
__device__ __forceinline__ void lk_block_prefix(uint32_t F, u64* __restrict__ pref, Fn f) {
  __shared__ u64 wsum[4];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  u64 carry = 0;
  for (uint32_t base = 0; base < F; base += 256) {
    const uint32_t i = base + threadIdx.x;
    const u64 x = i < F ? f(i) : 0ull;
    // wave inclusive scan of a 64-bit value
    u64 v = x;
    for (int o = 1; o < 64; o <<= 1) {
      const u64 t = shfl_up64(v, o);
      if (lane >= o) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    u64 off = 0, tot = 0;
    for (int w = 0; w < 4; w++) {
      const u64 t = wsum[w];
      if (w < wave) off += t;
      tot += t;
    }
    if (i < F) pref[i] = carry + off + v - x;
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) pref[F] = carry;
}

// k_lk_prep with the prefix in the launch, for frontiers one workgroup scans in a few steps.
__global__ __launch_bounds__(256) void k_lk_prep_scan(DevSnap s, u64* next, const uint32_t* __restrict__ cur,
                                                      uint32_t F, u64 live, u64* __restrict__ cmask,
                                                      u64* __restrict__ pref, uint32_t* fcount_out) {
  lk_block_prefix(F, pref, [&](uint32_t i) { return lk_prep_one(s, next, cur, cmask, i, live); });
  if (threadIdx.x == 0) *fcount_out = 0;
}

// Level j: one lane per reverse edge of the frontier (owner search in the prefix of the row lengths).
__global__ __launch_bounds__(256) void k_lk_level(DevSnap s, Walk W, const uint32_t* __restrict__ cur,
                                                  const u64* __restrict__ cmask, const u64* __restrict__ pref,
                                                  uint32_t F, uint64_t n_edges) {
  const u64 total = pref[F];
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&W.ctl->edges, total);
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < total; base += stride) {
    const u64 e = base + lane_id();
    bool act = e < total;
    uint32_t p = NONE;
    u64 m = 0;
    if (act) {
      const uint32_t own = csr_owner((const uint64_t*)pref, F, e);
      const u64 idx = s.radj_off[cur[own]] + (e - pref[own]);
      act = idx < n_edges;
      if (act) {
        p = s.radj[idx];
        m = cmask[own];
      }
    }
    lk_visit(s, W, act, p, m);
  }
}

// After a group: the masks of every touched node back to 0, the node lists empty.
__global__ __launch_bounds__(256) void k_lk_clear(u64* vis, u64* next, const uint32_t* __restrict__ touched,
                                                  uint32_t lcap, LkCtl* ctl) {
  const uint32_t n = min(ctl->tcount, lcap);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t v = touched[i];
    vis[v] = 0;
    next[v] = 0;
  }
}
__global__ void k_lk_lists_reset(LkCtl* ctl) {
  ctl->fcount[0] = ctl->fcount[1] = 0;
  ctl->tcount = 0;
}

// ------------------------------------------------------------------ the forward walk (subject lookup)
// A resolved subject-lookup request.
enum : uint32_t { LS_WALK = 0, LS_EMPTY = 1, LS_CONFIRM = 2 };
struct SReq {
  uint32_t root;  // root node (walk mode)
  int32_t depth;  // clamped rest depth (>= 1)
  uint32_t mode;  // LS_*
  uint32_t pad;
};

// The subject-free part of k_resolve.  A relation without a rewrite or a materialised union: a missing
// root answers every check NotMember (k_resolve routes it DONE), a pure root is walked, an impure one
// confirmed.  Every other relation (interpreter, formula split, undeclared) is confirmed.
__global__ __launch_bounds__(256) void k_ls_resolve(DevSnap s, const kg_lookup_subj* __restrict__ q, uint32_t n,
                                                    int32_t global, SReq* __restrict__ sr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const kg_lookup_subj x = q[i];
  int32_t d = x.max_depth;
  if (d <= 0 || global < d) d = global;  // engine.go:68-70
  const uint8_t rf = relflag(s, x.ns, x.rel);
  const bool virt = s.virt && x.ns < s.n_ns && x.rel < s.n_rel && s.virt[(size_t)x.ns * s.n_rel + x.rel];
  uint32_t mode = LS_CONFIRM, root = NONE;
  if (rf == 0 || virt) {
    root = nmap_find(s, x.ns, x.rel, x.obj);
    if (root >= s.n_nodes) mode = LS_EMPTY;
    else mode = (s.nflags && (s.nflags[root] & NF_IMPURE)) ? LS_CONFIRM : LS_WALK;
  }
  sr[i] = SReq{root, d, mode, 0};
}

// Level 0: bit b on the root of request b of the group.
__global__ __launch_bounds__(64) void k_ls_seed(DevSnap s, Walk W, uint32_t gn) {
  const uint32_t b = threadIdx.x;
  const bool act = b < gn;
  lk_mark(s, W, act, act ? W.greq[b].root : NONE, 1ull << b);
}

// Before level j: every frontier node hands its new bits over (cmask, restricted to the requests whose
// depth still probes level j: D-1 >= j) and frees next[].  Two row lengths per node: its check row, whose
// subject ids the level lists, and -- for the bits that go one level further (xlive: D-1 >= j+1) -- its
// adj row.  Everything a pure root reaches is pure, so no node flag is read.
__device__ __forceinline__ u64 ls_prep_one(const uint64_t* coff, u64* next, const uint32_t* cur, u64* cmask,
                                           uint32_t i, u64 live) {
  const uint32_t v = cur[i];
  const u64 m = next[v] & live;
  next[v] = 0;
  cmask[i] = m;
  return m ? coff[v + 1] - coff[v] : 0ull;
}
__device__ __forceinline__ u64 ls_adj_one(const DevSnap& s, const uint32_t* cur, const u64* cmask, uint32_t i,
                                          u64 xlive) {
  const uint32_t v = cur[i];
  return (cmask[i] & xlive) ? s.adj_off[v + 1] - s.adj_off[v] : 0ull;
}

// Frontiers one workgroup scans in a few steps: both prefixes in one launch (check rows -> epref, adj
// rows -> apref).
__global__ __launch_bounds__(256) void k_ls_prep_scan(DevSnap s, const uint64_t* __restrict__ coff, u64* next,
                                                      const uint32_t* __restrict__ cur, uint32_t F, u64 live,
                                                      u64 xlive, u64* cmask, u64* __restrict__ epref,
                                                      u64* __restrict__ apref, uint32_t* fcount_out) {
  lk_block_prefix(F, epref, [&](uint32_t i) { return ls_prep_one(coff, next, cur, cmask, i, live); });
  lk_block_prefix(F, apref, [&](uint32_t i) { return ls_adj_one(s, cur, cmask, i, xlive); });  // i: this thread's own cmask
  if (threadIdx.x == 0) *fcount_out = 0;
}
// Larger frontiers: one launch per kind of row writes the lengths, hipcub scans them.
__global__ __launch_bounds__(256) void k_ls_prep(const uint64_t* __restrict__ coff, u64* next,
                                                 const uint32_t* __restrict__ cur, uint32_t F, u64 live,
                                                 u64* __restrict__ cmask, u64* __restrict__ len, uint32_t* fcount_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < F) len[i] = ls_prep_one(coff, next, cur, cmask, i, live);
  else if (i == F) {
    len[F] = 0;
    *fcount_out = 0;
  }
}
__global__ __launch_bounds__(256) void k_ls_prep_adj(DevSnap s, const uint32_t* __restrict__ cur, uint32_t F, u64 xlive,
                                                     const u64* __restrict__ cmask, u64* __restrict__ len) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < F) len[i] = ls_adj_one(s, cur, cmask, i, xlive);
  else if (i == F) len[F] = 0;
}

// Level j, emit: one lane per check-row entry of the frontier.  An untagged entry is a subject id every
// request bit of its node lists (request << 32 | id); subject sets -- `...` ones included -- are skipped.
// An id the check maps to no subject (>= 2^31 - 1, k_resolve) is never a member.
__global__ __launch_bounds__(256) void k_ls_emit(Walk W, const uint64_t* __restrict__ coff,
                                                 const uint32_t* __restrict__ csub, const uint32_t* __restrict__ cur,
                                                 const u64* __restrict__ cmask, const u64* __restrict__ pref, uint32_t F,
                                                 uint64_t n_rows) {
  const u64 total = pref[F];
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&W.ctl->edges, total);
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < total; base += stride) {
    const u64 e = base + lane_id();
    uint32_t sub = NONE;
    u64 m = 0;
    if (e < total) {
      const uint32_t own = csr_owner((const uint64_t*)pref, F, e);
      const u64 idx = coff[cur[own]] + (e - pref[own]);
      if (idx < n_rows) {
        sub = csub[idx];
        m = cmask[own];
      }
    }
    const uint32_t c = sub < 0x7FFFFFFFu ? (uint32_t)__popcll(m) : 0u;
    uint32_t tot;
    const uint32_t ex = wave_excl_scan(c, &tot);
    if (!tot) continue;
    u64 at = 0;
    if (lane_id() == 0) at = atomicAdd(&W.ctl->ocount, (u64)tot);
    at = wave_bcast64(at, 0) + ex;
    for (u64 b = c ? m : 0ull; b; b &= b - 1, at++)
      if (at < W.ocap) W.okeys[at] = ((u64)W.greq[__ffsll(b) - 1].req << 32) | sub;
  }
}

// Level j, expand: one lane per adj edge of the frontier; the bits that go one level further arrive at
// the child.
__global__ __launch_bounds__(256) void k_ls_expand(DevSnap s, Walk W, const uint32_t* __restrict__ cur,
                                                   const u64* __restrict__ cmask, const u64* __restrict__ pref,
                                                   uint32_t F, u64 xlive, uint64_t n_edges) {
  const u64 total = pref[F];
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&W.ctl->edges, total);
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < total; base += stride) {
    const u64 e = base + lane_id();
    bool act = e < total;
    uint32_t c = NONE;
    u64 m = 0;
    if (act) {
      const uint32_t own = csr_owner((const uint64_t*)pref, F, e);
      const u64 idx = s.adj_off[cur[own]] + (e - pref[own]);
      act = idx < n_edges;
      if (act) {
        c = s.adj[idx];
        m = cmask[own] & xlive;
      }
    }
    lk_mark(s, W, act, c, m);
  }
}

// The domain of the confirmation: the subject ids that occur in a tuple.  The holder bitmap has exactly
// these ids; without it the untagged entries of the check rows are listed (sorted and deduplicated next).
__global__ __launch_bounds__(256) void k_ls_dom_bits(const uint32_t* __restrict__ hbits, uint32_t nbits, uint32_t* dom,
                                                     u64 dcap, LkCtl* ctl) {
  const uint32_t words = (nbits + 31) / 32;
  const uint32_t stride = gridDim.x * 256;
  for (uint32_t base = blockIdx.x * 256 + (threadIdx.x & ~63u); base < words; base += stride) {
    const uint32_t wi = base + lane_id();
    uint32_t bits = wi < words ? hbits[wi] : 0u;
    if (wi == words - 1 && (nbits & 31)) bits &= (1u << (nbits & 31)) - 1;
    uint32_t tot;
    const uint32_t ex = wave_excl_scan((uint32_t)__popc(bits), &tot);
    if (!tot) continue;
    u64 at = 0;
    if (lane_id() == 0) at = atomicAdd(&ctl->dcount, (u64)tot);
    at = wave_bcast64(at, 0) + ex;
    for (; bits; bits &= bits - 1, at++)
      if (at < dcap) dom[at] = wi * 32 + (__ffs(bits) - 1);
  }
}
__global__ __launch_bounds__(256) void k_ls_dom_rows(const uint32_t* __restrict__ csub, u64 n_rows, uint32_t* dom, u64 dcap,
                                                     LkCtl* ctl) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n_rows; base += stride) {
    const u64 i = base + lane_id();
    const uint32_t sub = i < n_rows ? csub[i] : NONE;
    const bool pred = !(sub & SET_BIT);
    const uint64_t m = __ballot(pred);
    if (!m) continue;
    u64 at = 0;
    if (lane_id() == 0) at = atomicAdd(&ctl->dcount, (u64)__popcll(m));
    at = wave_bcast64(at, 0) + lanes_below(m);
    if (pred && at < dcap) dom[at] = sub;
  }
}

// Candidate checks [at, at + m) of the confirmation: pair p = (subject id p / C of the domain, confirm
// request p % C) becomes the kg_query ns:obj#rel@id of that request.
__global__ __launch_bounds__(256) void k_ls_cands(const uint32_t* __restrict__ dom, u64 n_dom,
                                                  const uint32_t* __restrict__ conf, uint32_t C,
                                                  const kg_lookup_subj* __restrict__ q, u64 at, u64 m, kg_query* cq,
                                                  uint32_t* creq) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < m; i += stride) {
    const u64 p = at + i, d = p / C;
    if (d >= n_dom) continue;
    const uint32_t r = conf[p % C];
    const kg_lookup_subj x = q[r];
    kg_query y;
    y.t = kg_tuple{x.ns, x.obj, x.rel, KG_SUBJECT_ID, dom[d], 0};
    y.max_depth = x.max_depth;
    cq[i] = y;
    creq[i] = r;
  }
}

// ------------------------------------------------------------------ candidates
// c candidate checks of object obj, one per request of reqs[0, c).  Called by every lane of a wave.
__device__ __forceinline__ void lk_emit_cands(uint32_t c, const uint32_t* reqs, uint32_t obj,
                                              const kg_lookup* __restrict__ q, kg_query* cq, uint32_t* creq, u64 ccap,
                                              LkCtl* ctl) {
  uint32_t tot;
  const uint32_t ex = wave_excl_scan(c, &tot);
  if (!tot) return;
  u64 base = 0;
  if (lane_id() == 0) base = atomicAdd(&ctl->ccount, (u64)tot);
  base = wave_bcast64(base, 0) + ex;
  for (uint32_t t = 0; t < c; t++) {
    const u64 pos = base + t;
    if (pos >= ccap) break;
    const uint32_t r = reqs[t];
    const kg_lookup x = q[r];
    kg_query y;
    y.t = kg_tuple{x.ns, obj, x.rel, x.sns, x.sobj, x.srel};
    y.max_depth = x.max_depth;
    cq[pos] = y;
    creq[pos] = r;
  }
}

// One pass over the nodes: the candidate nodes of the reverse / confirm-nodes requests become checks,
// the objects of the confirm-all requests' namespaces become domain keys (sorted and deduplicated next).
__global__ __launch_bounds__(256) void k_lk_scan(DevSnap s, CandTab T, const kg_lookup* __restrict__ q, kg_query* cq,
                                                 uint32_t* creq, u64 ccap, u64* dkeys, u64 dcap, LkCtl* ctl) {
  const uint32_t stride = gridDim.x * 256;
  for (uint32_t base = blockIdx.x * 256 + (threadIdx.x & ~63u); base < s.n_nodes; base += stride) {
    const uint32_t v = base + lane_id();
    uint32_t c = 0, k = 0, slot = NONE, obj = 0;
    if (v < s.n_nodes) {
      const uint32_t ns = s.nd_ns[v], rel = s.nd_rel[v];
      obj = s.nd_obj[v];
      if (T.K) {
        k = lk_find64(T.keys, T.K, ((u64)ns << 32) | rel);
        if (k != NONE && (T.kall[k] || (s.nflags && (s.nflags[v] & NF_IMPURE)))) c = T.koff[k + 1] - T.koff[k];
      }
      if (T.M) slot = lk_find32(T.nsv, T.M, ns);
    }
    lk_emit_cands(c, c ? T.kreq + T.koff[k] : nullptr, obj, q, cq, creq, ccap, ctl);
    lk_append64(slot != NONE, ((u64)slot << 32) | obj, dkeys, &ctl->dcount, dcap);
  }
}

// The sorted domain keys: the first key of every run is one object of the namespace; it becomes a check
// for every confirm-all request of that namespace.
__global__ __launch_bounds__(256) void k_lk_domain(CandTab T, const u64* __restrict__ dk, u64 nd,
                                                   const kg_lookup* __restrict__ q, kg_query* cq, uint32_t* creq,
                                                   u64 ccap, LkCtl* ctl) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < nd; base += stride) {
    const u64 i = base + lane_id();
    uint32_t c = 0, slot = 0, obj = 0;
    if (i < nd) {
      const u64 key = dk[i];
      if (i == 0 || dk[i - 1] != key) {
        slot = (uint32_t)(key >> 32);
        obj = (uint32_t)key;
        if (slot < T.M) c = T.nsoff[slot + 1] - T.nsoff[slot];
      }
    }
    lk_emit_cands(c, c ? T.nsreq + T.nsoff[slot] : nullptr, obj, q, cq, creq, ccap, ctl);
  }
}

// The candidates' answers: members join the output keys; errors are counted per request, with the code
// of the lowest object id (errmin: object << 32 | code, atomicMin).  SUBJ: the candidates of a subject
// lookup -- the listed id is the query's subject id.
template <bool SUBJ>
__global__ __launch_bounds__(256) void k_lk_collect(const kg_query* __restrict__ cq, const uint32_t* __restrict__ creq,
                                                    const uint8_t* __restrict__ out, const uint32_t* __restrict__ err,
                                                    u64 n, u64* okeys, u64 ocap, int count_errs, u64* n_errors,
                                                    u64* errmin, LkCtl* ctl) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n; base += stride) {
    const u64 i = base + lane_id();
    bool mem = false;
    u64 key = 0;
    if (i < n) {
      const uint8_t o = out[i];
      const uint32_t r = creq[i], obj = SUBJ ? cq[i].t.sobj : cq[i].t.obj;
      mem = o == KG_IS_MEMBER;
      key = ((u64)r << 32) | obj;
      if (o == KG_ERROR && count_errs) {
        atomicAdd(&n_errors[r], 1ull);
        atomicMin(&errmin[r], ((u64)obj << 32) | err[i]);
      }
    }
    if (count_errs) {
      const uint64_t mm = __ballot(mem);
      if (mm && lane_id() == 0) atomicAdd(&ctl->confirmed, (u64)__popcll(mm));
    }
    lk_append64(mem, key, okeys, &ctl->ocount, ocap);
  }
}

// ------------------------------------------------------------------ output
__global__ __launch_bounds__(256) void k_lk_finish(const u64* __restrict__ uk, u64 m, uint32_t n_reqs,
                                                   uint64_t* __restrict__ req_off, uint32_t* __restrict__ objs,
                                                   const u64* __restrict__ errmin, uint32_t* __restrict__ err_code) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < m || i <= n_reqs; i += stride) {
    if (i < m) objs[i] = (uint32_t)uk[i];
    if (i <= n_reqs) {  // first key of request i or later
      const u64 key = i << 32;
      u64 lo = 0, hi = m;
      while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (uk[mid] < key) lo = mid + 1;
        else hi = mid;
      }
      req_off[i] = lo;
      if (i < n_reqs) err_code[i] = errmin[i] == ~0ull ? 0u : (uint32_t)errmin[i];
    }
  }
}

// The device buffers of lookups on one lane, kept between calls.
struct LookupBufs {
  PinBuf<kg_lookup> h_req;
  DevBuf<kg_lookup> d_req;
  DevBuf<LReq> d_lr;
  PinBuf<LReq> h_lr;
  // the same of a subject lookup
  PinBuf<kg_lookup_subj> h_sreq;
  DevBuf<kg_lookup_subj> d_sreq;
  DevBuf<SReq> d_sr;
  PinBuf<SReq> h_sr;
  DevBuf<uint32_t> dom, dom2;  // subject ids of the confirmation's domain
  DevBuf<LkCtl> ctl;
  // walk
  DevBuf<u64> vis, next, cmask, len, pref;
  DevBuf<uint32_t> fl[2], touched;
  uint32_t walk_nodes = 0;  // nodes the walk buffers hold (0: not allocated)
  bool dirty = false;       // a walk ended without its clear: the masks are zeroed wholesale
  DevBuf<GReq> greq;
  DevBuf<void> tmp;  // hipcub temporaries
  // candidates
  DevBuf<uint32_t> tab;
  DevBuf<kg_query> cq;
  DevBuf<uint32_t> creq, cerr;
  DevBuf<uint8_t> cout;
  DevBuf<u64> dkeys, dkeys2;
  DevBuf<u64> n_errors, errmin;
  // output
  DevBuf<u64> okeys, okeys2;
  DevBuf<uint64_t> d_off;
  DevBuf<uint32_t> d_objs, d_ecode;
  hipEvent_t ev[2] = {};
  ~LookupBufs() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

template <class T>
int grow_keep(DevBuf<T>& b, size_t n, size_t keep, hipStream_t st) {
  if (n <= b.cap()) return 0;
  DevBuf<T> nb;
  HIPC(nb.reserve(n));
  if (keep) HIPC(hipMemcpyAsync(nb.get(), b.get(), keep * sizeof(T), hipMemcpyDeviceToDevice, st));
  HIPC(hipStreamSynchronize(st));
  b = std::move(nb);
  return 0;
}

int read_ctl(Workspace* w, LookupBufs& B, hipStream_t st, LkCtl* h) {
  void* hb = w->host_buf(65536);
  if (!hb) return set_error(-1, "pinned host buffer");
  HIPC(hipMemcpyAsync(hb, B.ctl.get(), sizeof(LkCtl), hipMemcpyDeviceToHost, st));
  if (int rc = w->wait(st, true)) return rc;
  memcpy(h, hb, sizeof(LkCtl));
  return 0;
}

// The start of a call: the timing events, the counters and the per-request error words, all cleared.
int lk_begin(LookupBufs& B, size_t n, hipStream_t st) {
  if (!B.ev[0])
    for (auto& e : B.ev) HIPC(hipEventCreate(&e));
  HIPC(B.ctl.reserve(1));
  HIPC(B.n_errors.reserve(n));
  HIPC(B.errmin.reserve(n));
  HIPC(hipEventRecord(B.ev[0], st));
  HIPC(hipMemsetAsync(B.ctl.get(), 0, sizeof(LkCtl), st));
  HIPC(hipMemsetAsync(B.n_errors.get(), 0, n * 8, st));
  HIPC(hipMemsetAsync(B.errmin.get(), 0xFF, n * 8, st));
  return 0;
}

// The walk buffers of a lane (both walks use them): allocated for nn nodes on first use, the masks all
// clear on return, the group's request bits on the device.  *scan_bytes: hipcub's scan temporaries.
int walk_reserve(LookupBufs& B, uint32_t nn, const std::vector<GReq>& greq, hipStream_t st, size_t* scan_bytes) {
  if (B.walk_nodes < nn) {
    B.walk_nodes = 0;
    HIPC(B.vis.reserve(nn));
    HIPC(B.next.reserve(nn));
    HIPC(B.cmask.reserve(nn));
    HIPC(B.len.reserve((size_t)nn + 1));
    HIPC(B.pref.reserve((size_t)nn + 1));
    HIPC(B.fl[0].reserve(nn));
    HIPC(B.fl[1].reserve(nn));
    HIPC(B.touched.reserve(nn));
    B.walk_nodes = nn;
    B.dirty = true;
  }
  if (B.dirty) {
    HIPC(hipMemsetAsync(B.vis.get(), 0, (size_t)B.walk_nodes * 8, st));
    HIPC(hipMemsetAsync(B.next.get(), 0, (size_t)B.walk_nodes * 8, st));
    B.dirty = false;
  }
  HIPC(B.greq.reserve(greq.size()));
  HIPC(hipMemcpyAsync(B.greq.get(), greq.data(), greq.size() * sizeof(GReq), hipMemcpyHostToDevice, st));
  HIPC(hipStreamSynchronize(st));  // greq is pageable
  *scan_bytes = 0;
  HIPC(hipcub::DeviceScan::ExclusiveSum(nullptr, *scan_bytes, B.len.get(), B.pref.get(), (size_t)nn + 1, st));
  HIPC(B.tmp.reserve(*scan_bytes + 16));
  return 0;
}

// After a group: the masks cleared by replaying the touched list, the node lists empty.  h: the
// counters as the group's last launch left them.
int walk_finish(Snapshot* s, LookupBufs& B, hipStream_t st, const LkCtl& h) {
  hipLaunchKernelGGL(k_lk_clear, dim3((uint32_t)s->n_cu * 4), dim3(256), 0, st, B.vis.get(), B.next.get(),
                     (const uint32_t*)B.touched.get(), B.walk_nodes, B.ctl.get());
  hipLaunchKernelGGL(k_lk_lists_reset, dim3(1), dim3(1), 0, st, B.ctl.get());
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(st));
  B.dirty = h.over != 0;  // an overflowed touched list did not name every node to clear
  if (h.over) return set_error(KG_ERR_RESOURCE_CODE, "lookup: a node list overflowed");
  return 0;
}

// The output keys of a call (request << 32 | id).  The list grows when a step's true count passes it;
// the step is then rerun.
struct OutKeys {
  LookupBufs& B;
  Workspace* w;
  hipStream_t st;
  u64 cap = 0;
  u64 have = 0;  // keys of the finished steps
  int init(const Snapshot* s) {
    cap = s->lookup_cap ? s->lookup_cap : std::max<u64>(65536, B.okeys.cap());
    HIPC(B.okeys.reserve((size_t)cap));
    return 0;
  }
  // a list of at least `need` keys that keeps the finished steps', and the device counter back at them
  int regrow(u64 need) {
    cap = std::max<u64>(need, 2 * cap);
    if (int rc = grow_keep(B.okeys, (size_t)cap, (size_t)have, st)) return rc;
    void* hb = w->host_buf(65536);
    if (!hb) return set_error(-1, "pinned host buffer");
    memcpy(hb, &have, 8);
    HIPC(hipMemcpyAsync(&B.ctl.get()->ocount, hb, 8, hipMemcpyHostToDevice, st));
    HIPC(hipStreamSynchronize(st));  // the pinned word is reused by the next readback
    return 0;
  }
};

// The candidates' answers join the output keys (k_lk_collect); errors are counted on the first pass only.
template <bool SUBJ>
int collect(Snapshot* s, Workspace* w, LookupBufs& B, hipStream_t st, u64 n_cand, OutKeys& O, u64* n_conf) {
  for (int pass = 0;; pass++) {
    hipLaunchKernelGGL(k_lk_collect<SUBJ>, dim3((uint32_t)std::min<u64>((u64)s->n_cu * 4, n_cand / 256 + 1)), dim3(256),
                       0, st, (const kg_query*)B.cq.get(), (const uint32_t*)B.creq.get(), (const uint8_t*)B.cout.get(),
                       (const uint32_t*)B.cerr.get(), n_cand, B.okeys.get(), O.cap, pass == 0 ? 1 : 0, B.n_errors.get(),
                       B.errmin.get(), B.ctl.get());
    HIPC(hipGetLastError());
    LkCtl h;
    if (int rc = read_ctl(w, B, st, &h)) return rc;
    if (h.ocount > O.cap) {
      if (pass) return set_error(KG_ERR_RESOURCE_CODE, "lookup: output list overflowed twice");
      if (int rc = O.regrow(h.ocount)) return rc;
      continue;
    }
    O.have = h.ocount;
    *n_conf = h.confirmed;
    return 0;
  }
}

// The end of a call: the keys sorted, duplicates dropped, split by request, and the four output arrays
// in one pinned block.
int lk_output(Snapshot* s, Workspace* w, LookupBufs& B, hipStream_t st, size_t n, u64 o_have, kg_lookup_buf* out);

}  // namespace

void lookup_bufs_free(void* p) { delete static_cast<LookupBufs*>(p); }

// Runs on lane L (its stream and workspace; the caller holds the workspace's mutex).
int lookup_objects(Snapshot* s, Lane* L, const kg_lookup* reqs, size_t n, int32_t gmax, kg_lookup_buf* out) {
  if (gmax < 1) gmax = 5;  // as check_batch_begin
  if (n > 0x7FFFFFFFull) return set_error(-2, "batch too large");
  HIPC(hipSetDevice(s->device));
  hipStream_t st = L->stream;
  Workspace* w = L->w;
  if (!L->lk) L->lk = new LookupBufs();
  LookupBufs& B = *static_cast<LookupBufs*>(L->lk);
  const DevSnap& ds = s->ds;
  const uint32_t nn = ds.n_nodes;
  const uint32_t grid_wide = (uint32_t)s->n_cu * 4;
  HIPC(B.h_req.reserve(n));
  HIPC(B.d_req.reserve(n));
  HIPC(B.d_lr.reserve(n));
  HIPC(B.h_lr.reserve(n));
  memcpy(B.h_req.get(), reqs, n * sizeof(kg_lookup));
  if (int rc = lk_begin(B, n, st)) return rc;
  HIPC(hipMemcpyAsync(B.d_req.get(), B.h_req.get(), n * sizeof(kg_lookup), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_lk_resolve, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, ds, B.d_req.get(), (uint32_t)n,
                     gmax, (uint64_t)s->n_check_rows, B.d_lr.get());
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(B.h_lr.get(), B.d_lr.get(), n * sizeof(LReq), hipMemcpyDeviceToHost, st));
  if (int rc = w->wait(st, true)) return rc;
  const LReq* lr = B.h_lr.get();

  // ---- plan: walk groups and candidate tables
  std::vector<GReq> greq;
  std::map<u64, std::vector<uint32_t>> by_key;
  std::map<uint32_t, std::vector<uint32_t>> by_ns;
  for (size_t i = 0; i < n; i++) {
    if (lr[i].mode == LK_ALL) {
      by_ns[reqs[i].ns].push_back((uint32_t)i);
      continue;
    }
    if (lr[i].mode == LK_REVERSE && lr[i].hcount) greq.push_back(GReq{reqs[i].ns, reqs[i].rel, (uint32_t)i, 0});
    // candidates of a reverse request: impure nodes -- none without node flags
    if (lr[i].mode == LK_NODES || ds.nflags) by_key[((u64)reqs[i].ns << 32) | reqs[i].rel].push_back((uint32_t)i);
  }

  OutKeys O{B, w, st};
  if (int rc = O.init(s)) return rc;
  uint64_t st_edges = 0, st_levels = 0;

  // ---- the reverse walk, 64 requests per group
  if (!greq.empty()) {
    size_t scan_bytes = 0;
    if (int rc = walk_reserve(B, nn, greq, st, &scan_bytes)) return rc;
    for (size_t g0 = 0; g0 < greq.size();) {
      const uint32_t gn = (uint32_t)std::min<size_t>(64, greq.size() - g0);
      int32_t max_d = 1;
      for (uint32_t b = 0; b < gn; b++) max_d = std::max(max_d, lr[greq[g0 + b].req].depth);
      Walk W{B.vis.get(), B.next.get(), B.fl[0].get(), 0, B.touched.get(), B.walk_nodes, B.okeys.get(), O.cap,
             B.greq.get() + g0, B.ctl.get()};
      B.dirty = true;
      hipLaunchKernelGGL(k_lk_seed, dim3(gn), dim3(256), 0, st, ds, W, (const LReq*)B.d_lr.get());
      HIPC(hipGetLastError());
      LkCtl h;
      if (int rc = read_ctl(w, B, st, &h)) return rc;
      uint32_t cur = 0, F = std::min(h.fcount[0], B.walk_nodes);
      for (int32_t j = 1; j <= max_d - 1 && F; j++) {
        u64 live = 0;  // requests whose depth reaches level j
        for (uint32_t b = 0; b < gn; b++)
          if (lr[greq[g0 + b].req].depth - 1 >= j) live |= 1ull << b;
        W.fout = B.fl[cur ^ 1].get();
        W.fsel = cur ^ 1;
        uint32_t* fc_out = &B.ctl.get()->fcount[cur ^ 1];
        if (F <= 4096) {
          hipLaunchKernelGGL(k_lk_prep_scan, dim3(1), dim3(256), 0, st, ds, B.next.get(), (const uint32_t*)B.fl[cur].get(),
                             F, live, B.cmask.get(), B.pref.get(), fc_out);
        } else {
          hipLaunchKernelGGL(k_lk_prep, dim3(F / 256 + 1), dim3(256), 0, st, ds, B.next.get(),
                             (const uint32_t*)B.fl[cur].get(), F, live, B.cmask.get(), B.len.get(), fc_out);
          HIPC(hipcub::DeviceScan::ExclusiveSum(B.tmp.get(), scan_bytes, B.len.get(), B.pref.get(), (size_t)F + 1, st));
        }
        hipLaunchKernelGGL(k_lk_level, dim3(grid_wide), dim3(256), 0, st, ds, W, (const uint32_t*)B.fl[cur].get(),
                           (const u64*)B.cmask.get(), (const u64*)B.pref.get(), F, (uint64_t)s->n_set_edges);
        HIPC(hipGetLastError());
        if (int rc = read_ctl(w, B, st, &h)) return rc;
        cur ^= 1;
        F = std::min(h.fcount[cur], B.walk_nodes);
        st_levels++;
      }
      if (int rc = walk_finish(s, B, st, h)) return rc;
      if (h.ocount > O.cap) {  // the group's keys did not fit: a larger list, the group again
        if (int rc = O.regrow(h.ocount)) return rc;
        continue;
      }
      O.have = h.ocount;
      st_edges = h.edges;  // summed on the device over every run, reruns included
      g0 += gn;
    }
  }
  const u64 n_exact = O.have;

  // ---- candidates: one pass over the nodes, then the sorted domains of the confirm-all namespaces
  u64 n_cand = 0, n_conf = 0;
  if (!by_key.empty() || !by_ns.empty()) {
    std::vector<uint32_t> blob;
    const uint32_t K = (uint32_t)by_key.size(), M = (uint32_t)by_ns.size();
    // layout (u32 words): keys[2K] | kall[K] | koff[K+1] | kreq[..] | nsv[M] | nsoff[M+1] | nsreq[..]
    std::vector<u64> keys;
    std::vector<uint32_t> kall, koff{0}, kreq, nsv, nsoff{0}, nsreq;
    for (auto& kv : by_key) {
      keys.push_back(kv.first);
      kall.push_back(lr[kv.second[0]].mode == LK_NODES ? 1u : 0u);
      kreq.insert(kreq.end(), kv.second.begin(), kv.second.end());
      koff.push_back((uint32_t)kreq.size());
    }
    for (auto& kv : by_ns) {
      nsv.push_back(kv.first);
      nsreq.insert(nsreq.end(), kv.second.begin(), kv.second.end());
      nsoff.push_back((uint32_t)nsreq.size());
    }
    blob.resize(2 * (size_t)K);
    if (K) memcpy(blob.data(), keys.data(), (size_t)K * 8);
    size_t o_kall = blob.size();
    blob.insert(blob.end(), kall.begin(), kall.end());
    size_t o_koff = blob.size();
    blob.insert(blob.end(), koff.begin(), koff.end());
    size_t o_kreq = blob.size();
    blob.insert(blob.end(), kreq.begin(), kreq.end());
    size_t o_nsv = blob.size();
    blob.insert(blob.end(), nsv.begin(), nsv.end());
    size_t o_nsoff = blob.size();
    blob.insert(blob.end(), nsoff.begin(), nsoff.end());
    size_t o_nsreq = blob.size();
    blob.insert(blob.end(), nsreq.begin(), nsreq.end());
    blob.push_back(0);
    HIPC(B.tab.reserve(blob.size() + 2));
    HIPC(hipMemcpyAsync(B.tab.get(), blob.data(), blob.size() * 4, hipMemcpyHostToDevice, st));
    HIPC(hipStreamSynchronize(st));  // blob is pageable
    const uint32_t* tb = B.tab.get();
    const CandTab T{(const u64*)tb, tb + o_kall, tb + o_koff, tb + o_kreq, K, tb + o_nsv, tb + o_nsoff, tb + o_nsreq, M};
    u64 ccap = std::max<u64>(65536, B.cq.cap()), dcap = M ? std::max<u64>(65536, B.dkeys.cap()) : 0;
    for (;;) {
      HIPC(B.cq.reserve((size_t)ccap));
      HIPC(B.creq.reserve((size_t)ccap));
      if (dcap) HIPC(B.dkeys.reserve((size_t)dcap));
      HIPC(hipMemsetAsync(&B.ctl.get()->ccount, 0, 16, st));  // ccount, dcount
      hipLaunchKernelGGL(k_lk_scan, dim3(std::max(1u, std::min(grid_wide, nn / 256 + 1))), dim3(256), 0, st, ds, T,
                         (const kg_lookup*)B.d_req.get(), B.cq.get(), B.creq.get(), ccap, B.dkeys.get(), dcap,
                         B.ctl.get());
      HIPC(hipGetLastError());
      LkCtl h;
      if (int rc = read_ctl(w, B, st, &h)) return rc;
      if (h.dcount > dcap) {
        dcap = h.dcount;
        ccap = std::max(ccap, h.ccount);
        continue;
      }
      if (h.ccount <= ccap && h.dcount) {
        const size_t nd = (size_t)h.dcount;
        HIPC(B.dkeys2.reserve(nd));
        hipcub::DoubleBuffer<u64> kb(B.dkeys.get(), B.dkeys2.get());
        size_t sort_bytes = 0;
        HIPC(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, kb, nd, 0, 64, st));
        HIPC(B.tmp.reserve(sort_bytes + 16));
        HIPC(hipcub::DeviceRadixSort::SortKeys(B.tmp.get(), sort_bytes, kb, nd, 0, 64, st));
        hipLaunchKernelGGL(k_lk_domain, dim3((uint32_t)std::min<u64>(grid_wide, nd / 256 + 1)), dim3(256), 0, st, T,
                           (const u64*)kb.Current(), (u64)nd, (const kg_lookup*)B.d_req.get(), B.cq.get(),
                           B.creq.get(), ccap, B.ctl.get());
        HIPC(hipGetLastError());
        if (int rc = read_ctl(w, B, st, &h)) return rc;
      }
      if (h.ccount > ccap) {
        ccap = h.ccount;
        continue;
      }
      n_cand = h.ccount;
      break;
    }
  }
  if (n_cand) {
    HIPC(B.cout.reserve((size_t)n_cand));
    HIPC(B.cerr.reserve((size_t)n_cand));
    constexpr u64 CHUNK = 1ull << 28;
    for (u64 at = 0; at < n_cand; at += CHUNK) {
      const size_t m = (size_t)std::min(CHUNK, n_cand - at);
      if (int rc = check_batch_device(s, w, B.cq.get() + at, m, gmax, B.cout.get() + at, B.cerr.get() + at, nullptr))
        return rc;
    }
    if (int rc = collect<false>(s, w, B, st, n_cand, O, &n_conf)) return rc;
  }
  if (int rc = lk_output(s, w, B, st, n, O.have, out)) return rc;
  out->exact = n_exact;
  out->candidates = n_cand;
  out->confirmed = n_conf;
  out->reverse_edges = st_edges;
  out->levels = st_levels;
  return 0;
}

namespace {

int lk_output(Snapshot* s, Workspace* w, LookupBufs& B, hipStream_t st, size_t n, u64 o_have, kg_lookup_buf* out) {
  const uint32_t grid_wide = (uint32_t)s->n_cu * 4;
  u64 m = 0;
  const u64* uk = B.okeys.get();
  if (o_have) {
    HIPC(B.okeys2.reserve((size_t)std::max<u64>(o_have, 1)));
    hipcub::DoubleBuffer<u64> kb(B.okeys.get(), B.okeys2.get());
    int end_bit = 33;
    while (end_bit < 64 && ((u64)n >> (end_bit - 32))) end_bit++;
    size_t sort_bytes = 0, uniq_bytes = 0;
    HIPC(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, kb, (size_t)o_have, 0, end_bit, st));
    HIPC(hipcub::DeviceSelect::Unique(nullptr, uniq_bytes, (u64*)nullptr, (u64*)nullptr, (u64*)nullptr, (size_t)o_have, st));
    HIPC(B.tmp.reserve(std::max(sort_bytes, uniq_bytes) + 16));
    HIPC(hipcub::DeviceRadixSort::SortKeys(B.tmp.get(), sort_bytes, kb, (size_t)o_have, 0, end_bit, st));
    HIPC(hipcub::DeviceSelect::Unique(B.tmp.get(), uniq_bytes, kb.Current(), kb.Alternate(), &B.ctl.get()->nuniq,
                                      (size_t)o_have, st));
    LkCtl h;
    if (int rc = read_ctl(w, B, st, &h)) return rc;
    m = std::min(h.nuniq, o_have);
    uk = kb.Alternate();
  }
  HIPC(B.d_off.reserve(n + 1));
  HIPC(B.d_objs.reserve((size_t)std::max<u64>(m, 1)));
  HIPC(B.d_ecode.reserve(n));
  hipLaunchKernelGGL(k_lk_finish, dim3((uint32_t)std::min<u64>(grid_wide, std::max<u64>(m, n + 1) / 256 + 1)), dim3(256),
                     0, st, uk, m, (uint32_t)n, B.d_off.get(), B.d_objs.get(), (const u64*)B.errmin.get(),
                     B.d_ecode.get());
  HIPC(hipGetLastError());
  // one pinned block: req_off[n + 1] | n_errors[n] | objs[m] | err_code[n]
  const size_t bytes = ((size_t)n + 1) * 8 + (size_t)n * 8 + (size_t)m * 4 + (size_t)n * 4;
  char* blk = (char*)tree_pool_get(bytes);
  if (!blk) return set_error(KG_ERR_RESOURCE_CODE, "lookup: pinned output allocation failed");
  uint64_t* o_off = (uint64_t*)blk;
  uint64_t* o_nerr = o_off + n + 1;
  uint32_t* o_objs = (uint32_t*)(o_nerr + n);
  uint32_t* o_ecode = o_objs + m;
  int rc = 0;
  if (hipMemcpyAsync(o_off, B.d_off.get(), (n + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(o_nerr, B.n_errors.get(), n * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      (m && hipMemcpyAsync(o_objs, B.d_objs.get(), (size_t)m * 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipMemcpyAsync(o_ecode, B.d_ecode.get(), n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipEventRecord(B.ev[1], st) != hipSuccess)
    rc = set_error(-1, "lookup: D2H copy failed");
  if (!rc) rc = w->wait(st, true);
  float ms = 0;
  if (!rc && hipEventElapsedTime(&ms, B.ev[0], B.ev[1]) != hipSuccess) {
    (void)hipGetLastError();
    ms = 0;
  }
  if (rc) {
    (void)hipStreamSynchronize(st);
    tree_pool_put(blk, bytes);
    return rc;
  }
  out->req_off = o_off;
  out->objs = o_objs;
  out->err_code = o_ecode;
  out->n_errors = o_nerr;
  out->n_reqs = n;
  out->n_objs = m;
  out->kernel_ms = ms;
  out->pinned = bytes;
  return 0;
}

}  // namespace

// kg_lookup_subjects on lane L (as lookup_objects).  Walk-mode requests are listed by the forward walk,
// 64 per group; the others by a check of every subject id of the domain, in chunks of CHUNK pairs.
int lookup_subjects(Snapshot* s, Lane* L, const kg_lookup_subj* reqs, size_t n, int32_t gmax, kg_lookup_buf* out) {
  if (gmax < 1) gmax = 5;  // as check_batch_begin
  if (n > 0x7FFFFFFFull) return set_error(-2, "batch too large");
  HIPC(hipSetDevice(s->device));
  hipStream_t st = L->stream;
  Workspace* w = L->w;
  if (!L->lk) L->lk = new LookupBufs();
  LookupBufs& B = *static_cast<LookupBufs*>(L->lk);
  const DevSnap& ds = s->ds;
  const uint32_t nn = ds.n_nodes;
  const uint32_t grid_wide = (uint32_t)s->n_cu * 4;
  const uint64_t* coff = ds.crow_off ? ds.crow_off : ds.row_off;
  const uint32_t* csub = ds.crow_off ? ds.crow_subj : ds.row_subj;
  const uint64_t n_rows = s->n_check_rows;
  HIPC(B.h_sreq.reserve(n));
  HIPC(B.d_sreq.reserve(n));
  HIPC(B.d_sr.reserve(n));
  HIPC(B.h_sr.reserve(n));
  memcpy(B.h_sreq.get(), reqs, n * sizeof(kg_lookup_subj));
  if (int rc = lk_begin(B, n, st)) return rc;
  HIPC(hipMemcpyAsync(B.d_sreq.get(), B.h_sreq.get(), n * sizeof(kg_lookup_subj), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_ls_resolve, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, ds,
                     (const kg_lookup_subj*)B.d_sreq.get(), (uint32_t)n, gmax, B.d_sr.get());
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(B.h_sr.get(), B.d_sr.get(), n * sizeof(SReq), hipMemcpyDeviceToHost, st));
  if (int rc = w->wait(st, true)) return rc;
  const SReq* sr = B.h_sr.get();

  std::vector<GReq> greq;      // walk mode, by group and bit
  std::vector<uint32_t> conf;  // confirm mode
  for (size_t i = 0; i < n; i++) {
    if (sr[i].mode == LS_WALK && sr[i].root < nn) greq.push_back(GReq{reqs[i].ns, reqs[i].rel, (uint32_t)i, sr[i].root});
    else if (sr[i].mode == LS_CONFIRM) conf.push_back((uint32_t)i);
  }

  OutKeys O{B, w, st};
  if (int rc = O.init(s)) return rc;
  uint64_t st_edges = 0, st_levels = 0;

  // ---- the forward walk
  if (!greq.empty()) {
    size_t scan_bytes = 0;
    if (int rc = walk_reserve(B, nn, greq, st, &scan_bytes)) return rc;
    for (size_t g0 = 0; g0 < greq.size();) {
      const uint32_t gn = (uint32_t)std::min<size_t>(64, greq.size() - g0);
      int32_t max_d = 1;
      std::vector<uint32_t> roots;
      for (uint32_t b = 0; b < gn; b++) {
        max_d = std::max(max_d, sr[greq[g0 + b].req].depth);
        roots.push_back(greq[g0 + b].root);
      }
      std::sort(roots.begin(), roots.end());
      Walk W{B.vis.get(), B.next.get(), B.fl[0].get(), 0, B.touched.get(), B.walk_nodes, B.okeys.get(), O.cap,
             B.greq.get() + g0, B.ctl.get()};
      B.dirty = true;
      hipLaunchKernelGGL(k_ls_seed, dim3(1), dim3(64), 0, st, ds, W, gn);
      HIPC(hipGetLastError());
      // the first frontier is the group's distinct roots: no readback before level 0
      uint32_t cur = 0, F = (uint32_t)(std::unique(roots.begin(), roots.end()) - roots.begin());
      LkCtl h;
      bool h_now = false;  // h holds the counters as they are on the device
      for (int32_t j = 0; j <= max_d - 1 && F; j++) {
        h_now = false;
        u64 live = 0, xlive = 0;  // requests that probe level j / expand it into level j + 1
        for (uint32_t b = 0; b < gn; b++) {
          const int32_t d = sr[greq[g0 + b].req].depth;
          if (d - 1 >= j) live |= 1ull << b;
          if (d - 1 >= j + 1) xlive |= 1ull << b;
        }
        W.fout = B.fl[cur ^ 1].get();
        W.fsel = cur ^ 1;
        uint32_t* fc_out = &B.ctl.get()->fcount[cur ^ 1];
        const uint32_t* fl = B.fl[cur].get();
        const u64* apref = B.pref.get();  // the prefix of the adj rows
        if (F <= 4096) {
          hipLaunchKernelGGL(k_ls_prep_scan, dim3(1), dim3(256), 0, st, ds, coff, B.next.get(), fl, F, live, xlive,
                             B.cmask.get(), B.pref.get(), B.len.get(), fc_out);
          apref = B.len.get();
        } else {
          hipLaunchKernelGGL(k_ls_prep, dim3(F / 256 + 1), dim3(256), 0, st, coff, B.next.get(), fl, F, live,
                             B.cmask.get(), B.len.get(), fc_out);
          HIPC(hipcub::DeviceScan::ExclusiveSum(B.tmp.get(), scan_bytes, B.len.get(), B.pref.get(), (size_t)F + 1, st));
        }
        hipLaunchKernelGGL(k_ls_emit, dim3(grid_wide), dim3(256), 0, st, W, coff, csub, fl, (const u64*)B.cmask.get(),
                           (const u64*)B.pref.get(), F, n_rows);
        HIPC(hipGetLastError());
        st_levels++;
        if (!xlive) break;
        if (F > 4096) {  // the emit has read pref: the same two buffers take the adj rows
          hipLaunchKernelGGL(k_ls_prep_adj, dim3(F / 256 + 1), dim3(256), 0, st, ds, fl, F, xlive,
                             (const u64*)B.cmask.get(), B.len.get());
          HIPC(hipcub::DeviceScan::ExclusiveSum(B.tmp.get(), scan_bytes, B.len.get(), B.pref.get(), (size_t)F + 1, st));
        }
        hipLaunchKernelGGL(k_ls_expand, dim3(grid_wide), dim3(256), 0, st, ds, W, fl, (const u64*)B.cmask.get(), apref, F,
                           xlive, (uint64_t)s->n_set_edges);
        HIPC(hipGetLastError());
        if (int rc = read_ctl(w, B, st, &h)) return rc;
        h_now = true;
        cur ^= 1;
        F = std::min(h.fcount[cur], B.walk_nodes);
      }
      if (!h_now)
        if (int rc = read_ctl(w, B, st, &h)) return rc;
      if (int rc = walk_finish(s, B, st, h)) return rc;
      if (h.ocount > O.cap) {  // the group's keys did not fit: a larger list, the group again
        if (int rc = O.regrow(h.ocount)) return rc;
        continue;
      }
      O.have = h.ocount;
      st_edges = h.edges;  // summed on the device over every run, reruns included
      g0 += gn;
    }
  }
  const u64 n_exact = O.have;

  // ---- confirmation: the domain once, then every (subject id, request) pair through the check
  u64 n_cand = 0, n_conf = 0, n_dom = 0;
  const uint32_t* dom = nullptr;
  if (!conf.empty() && n_rows && csub) {
    const bool bits = ds.hbits && !s->lookup_domain_rows;
    u64 dcap = std::max<u64>(65536, B.dom.cap());
    for (;;) {
      HIPC(B.dom.reserve((size_t)dcap));
      HIPC(hipMemsetAsync(&B.ctl.get()->dcount, 0, 8, st));
      if (bits)
        hipLaunchKernelGGL(k_ls_dom_bits, dim3(std::min(grid_wide, ds.hbits_n / 8192 + 1)), dim3(256), 0, st, ds.hbits,
                           ds.hbits_n, B.dom.get(), dcap, B.ctl.get());
      else
        hipLaunchKernelGGL(k_ls_dom_rows, dim3((uint32_t)std::min<u64>(grid_wide, n_rows / 256 + 1)), dim3(256), 0, st,
                           csub, (u64)n_rows, B.dom.get(), dcap, B.ctl.get());
      HIPC(hipGetLastError());
      LkCtl h;
      if (int rc = read_ctl(w, B, st, &h)) return rc;
      if (h.dcount > dcap) {
        dcap = h.dcount;
        continue;
      }
      n_dom = h.dcount;
      break;
    }
    dom = B.dom.get();
    if (!bits && n_dom) {  // an id per row entry that holds it: sort, one of each
      HIPC(B.dom2.reserve((size_t)n_dom));
      hipcub::DoubleBuffer<uint32_t> kb(B.dom.get(), B.dom2.get());
      size_t sort_bytes = 0, uniq_bytes = 0;
      HIPC(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, kb, (size_t)n_dom, 0, 31, st));
      HIPC(hipcub::DeviceSelect::Unique(nullptr, uniq_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (u64*)nullptr,
                                        (size_t)n_dom, st));
      HIPC(B.tmp.reserve(std::max(sort_bytes, uniq_bytes) + 16));
      HIPC(hipcub::DeviceRadixSort::SortKeys(B.tmp.get(), sort_bytes, kb, (size_t)n_dom, 0, 31, st));
      HIPC(hipcub::DeviceSelect::Unique(B.tmp.get(), uniq_bytes, kb.Current(), kb.Alternate(), &B.ctl.get()->nuniq,
                                        (size_t)n_dom, st));
      LkCtl h;
      if (int rc = read_ctl(w, B, st, &h)) return rc;
      n_dom = std::min(h.nuniq, n_dom);
      dom = kb.Alternate();
    }
  }
  if (n_dom) {
    const uint32_t C = (uint32_t)conf.size();
    HIPC(B.tab.reserve(C));
    HIPC(hipMemcpyAsync(B.tab.get(), conf.data(), (size_t)C * 4, hipMemcpyHostToDevice, st));
    HIPC(hipStreamSynchronize(st));  // conf is pageable
    n_cand = n_dom * C;
    constexpr u64 CHUNK = 1ull << 22;
    const size_t ccap = (size_t)std::min(CHUNK, n_cand);
    HIPC(B.cq.reserve(ccap));
    HIPC(B.creq.reserve(ccap));
    HIPC(B.cout.reserve(ccap));
    HIPC(B.cerr.reserve(ccap));
    for (u64 at = 0; at < n_cand; at += CHUNK) {
      const u64 m = std::min(CHUNK, n_cand - at);
      hipLaunchKernelGGL(k_ls_cands, dim3((uint32_t)std::min<u64>(grid_wide, m / 256 + 1)), dim3(256), 0, st, dom, n_dom,
                         (const uint32_t*)B.tab.get(), C, (const kg_lookup_subj*)B.d_sreq.get(), at, m, B.cq.get(),
                         B.creq.get());
      HIPC(hipGetLastError());
      if (int rc = check_batch_device(s, w, B.cq.get(), (size_t)m, gmax, B.cout.get(), B.cerr.get(), nullptr)) return rc;
      if (int rc = collect<true>(s, w, B, st, m, O, &n_conf)) return rc;
    }
  }
  if (int rc = lk_output(s, w, B, st, n, O.have, out)) return rc;
  out->exact = n_exact;
  out->candidates = n_cand;
  out->confirmed = n_conf;
  out->reverse_edges = st_edges;
  out->levels = st_levels;
  return 0;
}

void lookup_free(kg_lookup_buf* out) {
  if (out->pinned) tree_pool_put(out->req_off, (size_t)out->pinned);
  else free(out->req_off);
  memset(out, 0, sizeof *out);
}

}  // namespace kg
