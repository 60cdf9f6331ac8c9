// kg_lookup.hip -- the lookups, none with a reference counterpart in Keto: the objects of a
// namespace a subject has a relation on (kg_lookup_objects: OpenFGA ListObjects / SpiceDB LookupResources)
// and the subjects that hold a relation on one object (ListUsers / LookupSubjects) -- the subject ids
// (kg_lookup_subjects) or the subject sets of one namespace and relation, "which group:*#member may view
// this?" (kg_lookup_subject_sets: ListUsers' user filter {type, relation}; a request of it may ask for ids too).
//
// The answer is defined through the check: for a request (ns, rel, subject, max_depth) the ascending
// object ids o with a node (ns, o, *) for which CheckIsMember(ns:o#rel@subject, max_depth) is IsMember; for
// (ns, obj, rel, max_depth) the subject ids of tuples with that check on ns:obj#rel; for (ns, obj, rel, sns,
// srel, max_depth) the object ids o of the subject sets sns:o#srel of tuples -- `...` sets are sets like any
// other -- with that check of ns:obj#rel@(sns:o#srel).  An object request is
// answered in one of four modes (k_lk_resolve):
//   reverse        (ns, rel) has no rewrite or is a materialised union, and the reverse indexes exist:
//                  every member is a node of (ns, rel); a PURE node is a member iff its reverse distance
//                  from a holder of the subject is <= D-1 (what k_back decides for one root), so one
//                  target-free reverse walk lists them.  IMPURE nodes of (ns, rel) are confirmed.
//   confirm-nodes  the same without reverse indexes: every node of (ns, rel) is confirmed.
//   formula        (ns, rel) has a boolean-rewrite plan (kg_formula.hip) whose formula is NotMember when
//                  every leaf is (FPlan::lookup_ok), and the reverse indexes exist: the request's bit of
//                  the reverse walk listens to the plan's walk leaves J (FPlan::walk_leaves) instead of
//                  (ns, rel), and a pure node of one that it reaches is a CANDIDATE, not an answer.  So
//                  is the object of every impure node of (ns, rel) and of every leaf (J or not).  The
//                  candidate keys are made unique and confirmed.  An object outside them has no node of
//                  rel, its leaf nodes are absent or pure -- every leaf check is a definite answer
//                  without an error -- and its J leaves are unreached, NotMember: f is NotMember.
//   confirm-all    any other relation (interpreter / a plan with f(0) = true / undeclared; a formula
//                  without reverse indexes or with kg_snapshot_tune "lookup_formula" 0): every object
//                  of the namespace is confirmed.
// A subject request (k_ls_resolve) with a pure root of a reverse-mode relation is answered by a FORWARD
// walk over adj.  One on a lookup_ok plan whose object has no node of the relation and only pure leaf
// nodes walks from its J-leaf roots: the ids they list are its candidates (an id none of them lists is
// NotMember of every J leaf, so of f), made unique and confirmed.  Everything else confirms every
// subject id.  What a subject request lists does not change its mode.  The walk's one pass over the check
// rows of the nodes it reaches lists both kinds of entry (Emit): an untagged one is a subject id and goes
// to the bits that ask for ids, a tagged one SET_BIT | v is the subject set of node v and goes to the bits
// whose filter is (nd_ns[v], nd_rel[v]), which list nd_obj[v]; a group without such a bit (Walk::smask == 0)
// reads no tagged entry's node.  A set in the row of a node k hops below the root is listed iff k <= D-1, as
// an id is.  A formula request's walk lists its candidate sets the same way: a set none of the J leaves'
// walks lists is NotMember of every J leaf.  A request that confirms and lists sets takes the domain of its
// filter instead of the subject ids: one scan of the check rows per call (k_ls_dom_sets) emits filter slot
// << 32 | object id for the tagged entries of the call's distinct filters, sorted; every distinct set
// becomes a candidate key of each such request of that filter (k_lk_domain), checked once next to the
// formula requests' keys -- domain x requests checks.  "Confirmed" = run through check_batch_device as
// kg_query rows built on the device; no check kernel is touched.  Every confirmation -- the object lookup's
// candidates, the subject lookup's (subject id, request) pairs, either's candidate keys, a paged round -- is
// one call of confirm(): a launch that builds the rows (all of them through lk_row), the checks in chunks,
// one collect (k_lk_collect; where the errors go is its sink: counted per request, or listed for a paged
// call).
//
// There is one walk (walk_groups) with two direction policies (ReverseWalk, ForwardWalk).  It is level-
// synchronous and bit-parallel over groups of 64 requests: a dense u64 visited mask per node (bit =
// request), a frontier list per level, work assigned per edge through a prefix over the frontier rows'
// lengths.  The masks are cleared by replaying the list of touched nodes, so a lookup costs what it
// reaches, not n_nodes.
//
// The paged calls (kg_lookup_objects_page / kg_lookup_subjects_page: the first `limit` ids >= `from` of the
// unpaged answer) run the same steps with three differences.  A walk bit lists no id below its request's
// cursor (GReq::from).  Every candidate of a confirmation becomes a key request << 32 | id at or above the
// cursor -- the subject lookup's confirm requests for ids index the ascending domain instead -- and no check is
// built up front: the sorted unique keys are checked in ascending rounds (paged_tail, page_rounds: each round
// one confirm()), at most 64 of a request first, then at most as many again as it has checked, until
// limit + 1 of its members (walk keys and confirmed candidates) lie at or below the largest id it has
// checked, or its candidates run out.  A walk key above that id stays unplaced: an unchecked candidate may
// lie below it.  Last, one kernel cuts every request's page out of the sorted unique keys and only the pages
// go into the pinned block.
//
// The mask calls (kg_lookup_objects_mask_device / kg_lookup_subject_sets_mask_device) are the unpaged calls up
// to their key list and end in Call::finish_mask instead of Call::finish: every key sets its bit in its
// request's row of the caller's bitmap with an atomicOr, which asks for neither order nor distinct keys, so
// nothing is sorted, made unique or copied out as ids (k_lk_mask_bits, k_lk_mask_count).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <type_traits>
#include <vector>

#include "kg_bfs.h"
#include "kg_internal.h"
#include "kg_snapshot.h"

namespace kg {
namespace {

typedef unsigned long long u64;

enum : uint32_t { LK_REVERSE = 0, LK_NODES = 1, LK_ALL = 2, LK_FORMULA = 3 };

// A resolved request.
struct LReq {
  uint32_t subj;    // tagged subject or NONE
  int32_t depth;    // clamped rest depth (>= 1)
  uint32_t mode;    // LK_*
  uint32_t hfirst, hcount;  // the subject's holders hold[hfirst, hfirst + hcount) (reverse, formula mode)
  uint32_t plan;            // formula mode: the relation's plan
};

// Device counters of one call.  Counts are TRUE counts: a count above its list's capacity means the
// list overflowed (nothing was written past it) and the step is rerun with a larger list.
struct LkCtl {
  u64 ocount;     // output keys (request << 32 | object)
  u64 edges;      // reverse edges read
  u64 ccount;     // candidate checks
  u64 dcount;     // domain keys (namespace slot << 32 | object)
  u64 confirmed;  // candidates answered IsMember
  u64 nuniq;      // keys of a sorted list after the duplicates are dropped
  u64 kcount;     // candidate keys of the formula requests (request << 32 | id)
  uint32_t fcount[2];  // the two frontier lists
  uint32_t tcount;     // touched nodes
  uint32_t over;       // a node list overflowed (they hold n_nodes entries: cannot happen)
  u64 ptotal;          // paged calls: the candidates of the round being built / the ids of the pages
  u64 ecount;          // paged calls: erring (request, id) keys collected
};

// One request bit of a walk group.
struct GReq {
  uint32_t ns, rel, req;
  uint32_t root;  // forward walk: the bit's root node
  // reverse walk: the relations of ns the bit listens to -- rel itself, or a formula request's walk leaves
  uint32_t n_listen, listen[FP_LEAVES];
  uint32_t from;  // paged calls: the request's cursor -- the bit lists no id below it
  // forward walk: what the bit lists -- the subject sets sns:*#srel, or (sns == KG_SUBJECT_ID) subject ids
  uint32_t sns, srel;
};
// A request of a paged call: its page, and its run of candidates -- [lo, hi) of the call's sorted unique
// candidate keys or, `implicit` (a subject lookup's confirm request for ids), of the ascending subject domain.
// The rounds check [lo, cur); the round being built takes [base, cur).
struct PgReq {
  u64 lo, hi, cur, base;
  u64 nmem;  // members among the checked candidates
  uint32_t from, limit;
  uint32_t implicit, pad;
};

// A list of 64-bit keys a call fills step by step: `have` keys of the finished steps in a list of `cap`.
// The list grows when a step's true count passes it; the step is then rerun.
struct KeyList {
  u64 cap = 0, have = 0;
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
  u64 fmask;          // the group's formula bits: what they list goes to the candidate keys
  u64* kkeys;         // candidate keys
  u64 kcap;
  const GReq* greq;   // the group's requests, by bit
  LkCtl* ctl;
  bool paged;         // a paged call: a bit lists only the ids at or above its request's cursor
  u64 smask;          // the group's bits that list subject sets (GReq::sns / srel), not subject ids
};

// A group table: distinct ascending keys, each with a flag and the requests that share it.
template <class K>
struct GroupTab {
  const K* keys;         // [n] ascending
  const uint32_t* flag;  // [n]
  const uint32_t* off;   // [n + 1] into req
  const uint32_t* req;
  uint32_t n;
  __device__ uint32_t count(uint32_t k) const { return off[k + 1] - off[k]; }
  __device__ const uint32_t* reqs(uint32_t k) const { return req + off[k]; }
};
// The candidate tables of a call.
struct CandTab {
  // the (ns << 32 | rel) of the reverse / confirm-nodes requests; flag 1: every node of the key is a candidate
  // (confirm-nodes), 0: impure nodes only
  GroupTab<u64> rel;
  GroupTab<uint32_t> ns;  // the namespaces of the confirm-all requests (no flag)
  // the (ns << 32 | rel) of the formula requests' relations and leaves: a node of one gives every request of
  // the key a candidate KEY; flag 1: a request's own relation (every live node), 0: a leaf (impure nodes)
  GroupTab<u64> frel;
};

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
// The same behind a 64-bit TRUE count (nothing flagged: the count says so).
template <class V>
__device__ __forceinline__ void lk_append64(bool pred, V val, V* list, u64* count, u64 cap) {
  const u64 pos = wave_reserve64(count, pred ? 1u : 0u);
  if (pred && pos < cap) list[pos] = val;
}

// The first index of the ascending a[0, n) whose entry is >= key (n: none).
template <class T, class I>
__device__ __forceinline__ I lk_lower_bound(const T* a, I n, T key) {
  I lo = 0, hi = n;
  while (lo < hi) {
    const I mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// The index of key in the ascending a[0, n), or NONE.
template <class T>
__device__ __forceinline__ uint32_t lk_find(const T* a, uint32_t n, T key) {
  const uint32_t lo = lk_lower_bound(a, n, key);
  return lo < n && a[lo] == key ? lo : NONE;
}

// ------------------------------------------------------------------ request mapping
// fidx / plans: the formula plans (kg_formula.hip), nullptr: no request takes the formula mode.
__global__ __launch_bounds__(256) void k_lk_resolve(DevSnap s, const int32_t* __restrict__ fidx,
                                                    const FPlan* __restrict__ plans, const kg_lookup* __restrict__ q,
                                                    uint32_t n, int32_t global, uint64_t hold_n, LReq* __restrict__ lr) {
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
  uint32_t mode =
      (relflag(s, x.ns, x.rel) == 0 || rel_is_union(s, x.ns, x.rel)) ? (s.radj ? LK_REVERSE : LK_NODES) : LK_ALL;
  uint32_t plan = 0;
  if (mode == LK_ALL && fidx && s.radj && x.ns < s.n_ns && x.rel < s.n_rel) {
    const int32_t p = fidx[(size_t)x.ns * s.n_rel + x.rel];
    if (p >= 0 && plans[p].lookup_ok) {
      mode = LK_FORMULA;
      plan = (uint32_t)p;
    }
  }
  uint2 h = make_uint2(0, 0);
  if (mode == LK_REVERSE || mode == LK_FORMULA) {
    h = holders_find(s, subj);
    if ((uint64_t)h.x + h.y > hold_n) h = make_uint2(0, 0);  // never read past hold[]
  }
  lr[i] = LReq{subj, clamp_depth(x.max_depth, global), mode, h.x, h.y, plan};
}

// A resolved subject-lookup request.
enum : uint32_t { LS_WALK = 0, LS_EMPTY = 1, LS_CONFIRM = 2, LS_FORMULA = 3 };
struct SReq {
  uint32_t root;  // root node (walk mode)
  int32_t depth;  // clamped rest depth (>= 1)
  uint32_t mode;  // LS_*
  uint32_t n_froot;           // formula mode: the object's nodes of the plan's walk leaves
  uint32_t froot[FP_LEAVES];
};

// The subject-free part of k_resolve.  A relation without a rewrite or a materialised union: a missing
// root answers every check NotMember (k_resolve routes it DONE), a pure root is walked, an impure one
// confirmed.  A relation with a lookup_ok plan (fidx / plans; nullptr: none) whose object has no node of
// the relation and no impure leaf node -- the condition under which k_fsplit splits its checks -- walks
// from the object's nodes of the walk leaves, or is empty without one.  Every other relation
// (interpreter, undeclared) is confirmed.  What the request lists (subject ids, or the subject sets of a
// filter) plays no part.
__global__ __launch_bounds__(256) void k_ls_resolve(DevSnap s, const int32_t* __restrict__ fidx,
                                                    const FPlan* __restrict__ plans,
                                                    const kg_lookup_subj_set* __restrict__ q, uint32_t n,
                                                    int32_t global, SReq* __restrict__ sr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const kg_lookup_subj_set x = q[i];
  uint32_t mode = LS_CONFIRM, root = NONE;
  if (relflag(s, x.ns, x.rel) == 0 || rel_is_union(s, x.ns, x.rel)) {
    root = nmap_find(s, x.ns, x.rel, x.obj);
    if (root >= s.n_nodes) mode = LS_EMPTY;
    else mode = (s.nflags && (s.nflags[root] & NF_IMPURE)) ? LS_CONFIRM : LS_WALK;
  }
  SReq r{root, clamp_depth(x.max_depth, global), mode, 0, {NONE, NONE, NONE, NONE}};
  if (mode == LS_CONFIRM && fidx && x.ns < s.n_ns && x.rel < s.n_rel) {
    const int32_t p = fidx[(size_t)x.ns * s.n_rel + x.rel];
    if (p >= 0 && plans[p].lookup_ok && nmap_find(s, x.ns, x.rel, x.obj) >= s.n_nodes) {
      const FPlan& P = plans[p];
      bool pure = true;
      for (uint32_t j = 0; j < P.n_leaves && j < (uint32_t)FP_LEAVES; j++) {
        const uint32_t v = nmap_find(s, x.ns, P.leaf[j], x.obj);
        if (v >= s.n_nodes) continue;
        if (s.nflags && (s.nflags[v] & NF_IMPURE)) pure = false;
        else if ((P.walk_leaves >> j) & 1u) r.froot[r.n_froot++] = v;
      }
      if (pure) r.mode = r.n_froot ? LS_FORMULA : LS_EMPTY;
    }
  }
  sr[i] = r;
}

// ------------------------------------------------------------------ the walk: arrivals and seeds
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

// Every request whose bit is in `bits` lists id (request << 32 | id): a formula bit into the candidate
// keys, any other into the output keys.  Called by every lane of a wave.
__device__ __forceinline__ void lk_list(const Walk& W, u64 bits, uint32_t id) {
  if (W.paged) {  // the same for every lane
    u64 keep = 0;
    for (u64 b = bits; b; b &= b - 1)
      if (id >= W.greq[__ffsll(b) - 1].from) keep |= b & -b;
    bits = keep;
  }
  u64 ob = bits & ~W.fmask;
  u64 at = wave_reserve64(&W.ctl->ocount, (uint32_t)__popcll(ob));
  for (; ob; ob &= ob - 1, at++)
    if (at < W.ocap) W.okeys[at] = ((u64)W.greq[__ffsll(ob) - 1].req << 32) | id;
  if (!W.fmask) return;  // the same for every lane
  u64 kb = bits & W.fmask;
  at = wave_reserve64(&W.ctl->kcount, (uint32_t)__popcll(kb));
  for (; kb; kb &= kb - 1, at++)
    if (at < W.kcap) W.kkeys[at] = ((u64)W.greq[__ffsll(kb) - 1].req << 32) | id;
}

// The reverse walk's arrival: every new bit that listens to p's (ns, rel) lists p's object if p is pure.
// Impure nodes are candidates of the confirmation (every ancestor of one is impure too).
__device__ __forceinline__ void lk_visit(const DevSnap& s, const Walk& W, bool act, uint32_t p, u64 m) {
  const u64 nb = lk_mark(s, W, act, p, m);
  u64 want = 0;
  if (nb && !(s.nflags && (s.nflags[p] & NF_IMPURE))) {
    const uint32_t pns = s.nd_ns[p], prel = s.nd_rel[p];
    for (u64 b = nb; b; b &= b - 1) {
      const GReq& g = W.greq[__ffsll(b) - 1];
      bool hit = false;
      for (uint32_t t = 0; t < g.n_listen && t < (uint32_t)FP_LEAVES; t++) hit |= g.listen[t] == prel;
      if (g.ns == pns && hit) want |= b & -b;  // the lowest bit of b
    }
  }
  lk_list(W, want, want ? s.nd_obj[p] : 0u);
}

// Reverse, level 0: one workgroup per request of the group strides over the subject's holders.
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

// Forward, level 0: bit b on the root of request b of the group.
__global__ __launch_bounds__(64) void k_ls_seed(DevSnap s, Walk W, uint32_t gn) {
  const uint32_t b = threadIdx.x;
  const bool act = b < gn;
  lk_mark(s, W, act, act ? W.greq[b].root : NONE, 1ull << b);
}

// ------------------------------------------------------------------ the walk: one level
// The frontier of level j: entry i is node cur[i] and carries the request bits cmask[i].
struct Frontier {
  const uint32_t* cur;
  u64* cmask;
  uint32_t F;
};
// One kind of row of the nodes: node v owns val[off[v], off[v + 1]) of val[0, n).
struct Rows {
  const uint64_t* off;
  const uint32_t* val;
  uint64_t n;
};

// Before level j, entry i's row length.  TAKE: the node first hands its new bits over (cmask[i],
// restricted to live: the requests whose depth still reaches level j, D-1 >= j; none from an impure node)
// and frees next[].  Forward, nflags == nullptr: everything a pure root reaches is pure, so no node flag
// is read.  !TAKE: the bits cmask[i] holds, restricted to live.
template <bool TAKE>
struct RowLen {
  Frontier f;
  const uint64_t* off;
  u64 live;
  u64* next;
  const uint8_t* nflags;
  __device__ u64 operator()(uint32_t i) const {
    const uint32_t v = f.cur[i];
    u64 m;
    if (TAKE) {
      m = next[v] & live;
      next[v] = 0;
      if (nflags && (nflags[v] & NF_IMPURE)) m = 0;
      f.cmask[i] = m;
    } else m = f.cmask[i] & live;
    return m ? off[v + 1] - off[v] : 0ull;
  }
};
struct NoLen {
  uint32_t none;  // a kernel argument: not an empty struct
};

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

// Frontiers one workgroup scans in a few steps (F <= PREFIX_IN_KERNEL): the lengths and their prefix in
// one launch, of both kinds of row for the forward walk (LenB = NoLen: of one).  The second prefix reads
// the cmask[i] that the same thread wrote during the first.  Resets the list the level will build.
constexpr uint32_t PREFIX_IN_KERNEL = 4096;
template <class LenA, class LenB>
__global__ __launch_bounds__(256) void k_lk_prep_scan(uint32_t F, LenA len_a, u64* __restrict__ pref_a, LenB len_b,
                                                      u64* __restrict__ pref_b, uint32_t* fcount_out) {
  lk_block_prefix(F, pref_a, len_a);
  if constexpr (!std::is_same<LenB, NoLen>::value) lk_block_prefix(F, pref_b, len_b);
  if (threadIdx.x == 0) *fcount_out = 0;
}
// Larger frontiers: one launch per kind of row writes the lengths, hipcub scans them.  Thread F writes
// the sentinel and (fcount_out: the level's first prepare) resets the list the level will build.
template <class Len>
__global__ __launch_bounds__(256) void k_lk_prep(uint32_t F, Len len_of, u64* __restrict__ len, uint32_t* fcount_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < F) len[i] = len_of(i);
  else if (i == F) {
    len[F] = 0;
    if (fcount_out) *fcount_out = 0;
  }
}

// The level: one lane per entry of the frontier's rows (owner search in the prefix of the row lengths).
// Every lane of a wave calls body(v, m) -- v: the entry, m: its owner's bits; NONE, 0: the lane has none.
template <class Body>
__global__ __launch_bounds__(256) void k_lk_frontier_edges(Frontier f, Rows r, const u64* __restrict__ pref, LkCtl* ctl,
                                                           Body body) {
  const u64 total = pref[f.F];
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&ctl->edges, total);
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < total; base += stride) {
    const u64 e = base + lane_id();
    uint32_t v = NONE;
    u64 m = 0;
    if (e < total) {
      const uint32_t own = csr_owner((const uint64_t*)pref, f.F, e);
      const u64 idx = r.off[f.cur[own]] + (e - pref[own]);
      if (idx < r.n) {
        v = r.val[idx];
        m = f.cmask[own];
      }
    }
    body(v, m);
  }
}

// One hop over radj (reverse: every bit, and the arrival lists the node's object) or adj (forward: the
// bits that go one level further, xlive: D-1 >= j+1, and the arrival only marks).
template <bool LIST>
struct Hop {
  DevSnap s;
  Walk W;
  u64 on;
  __device__ void operator()(uint32_t p, u64 m) const {
    if (LIST) lk_visit(s, W, true, p, m & on);
    else lk_mark(s, W, true, p, m & on);
  }
};
// The forward walk's emit over the check rows.  An untagged entry is a subject id: the id bits of its node
// list it (request << 32 | id).  An id the check maps to no subject (>= 2^31 - 1, k_resolve) is never a
// member.  A tagged entry SET_BIT | v is the subject set of node v -- `...` sets are sets like any other --
// and the set bits whose filter is v's (namespace, relation) list v's object.  A group without a set bit
// (W.smask == 0, the same for every lane) never looks at a tagged entry.
struct Emit {
  DevSnap s;
  Walk W;
  __device__ void operator()(uint32_t sub, u64 m) const {
    if (!W.smask) {
      lk_list(W, sub < 0x7FFFFFFFu ? m : 0ull, sub);
      return;
    }
    u64 bits = 0;
    uint32_t id = sub;
    if (!(sub & SET_BIT)) bits = sub < 0x7FFFFFFFu ? m & ~W.smask : 0ull;
    else if ((m & W.smask) && (sub & ~SET_BIT) < s.n_nodes) {  // a lane without an entry has NONE and no bit
      const uint32_t v = sub & ~SET_BIT, vns = s.nd_ns[v], vrel = s.nd_rel[v];
      for (u64 b = m & W.smask; b; b &= b - 1) {
        const GReq& g = W.greq[__ffsll(b) - 1];
        if (g.sns == vns && g.srel == vrel) bits |= b & -b;
      }
      if (bits) id = s.nd_obj[v];
    }
    lk_list(W, bits, id);
  }
};

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

// ------------------------------------------------------------------ check rows
// SUBJ: a subject lookup (its requests list subject ids or subject sets), else an object lookup (object ids).
template <bool SUBJ>
using ReqOf = typename std::conditional<SUBJ, kg_lookup_subj_set, kg_lookup>::type;

// The check of request x on a candidate id: ns:id#rel@subject of an object lookup's request; of a subject
// lookup's ns:obj#rel@id, or ns:obj#rel@(sns:id#srel) where it lists the subject sets of a filter.
template <bool SUBJ>
__device__ __forceinline__ kg_query lk_row(const ReqOf<SUBJ>& x, uint32_t id) {
  kg_query y;
  if constexpr (SUBJ) y.t = kg_tuple{x.ns, x.obj, x.rel, x.sns, id, x.sns == KG_SUBJECT_ID ? 0u : x.srel};
  else y.t = kg_tuple{x.ns, id, x.rel, x.sns, x.sobj, x.srel};
  y.max_depth = x.max_depth;
  return y;
}

// ------------------------------------------------------------------ candidates of a subject lookup
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
    u64 at = wave_reserve64(&ctl->dcount, (uint32_t)__popc(bits));
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
    lk_append64(!(sub & SET_BIT), sub, dom, &ctl->dcount, dcap);
  }
}

// The domain of the confirm requests that list subject sets depends on their filter: every tagged entry
// SET_BIT | v of the check rows whose (nd_ns[v] << 32 | nd_rel[v]) is one of the call's distinct filters F
// becomes a domain key filter slot << 32 | nd_obj[v] (sorted next; k_lk_domain pairs the first key of every
// run with the slot's requests).
__global__ __launch_bounds__(256) void k_ls_dom_sets(DevSnap s, const uint32_t* __restrict__ csub, u64 n_rows,
                                                     GroupTab<u64> F, u64* dkeys, u64 dcap, LkCtl* ctl) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n_rows; base += stride) {
    const u64 i = base + lane_id();
    const uint32_t sub = i < n_rows ? csub[i] : NONE, v = sub & ~SET_BIT;
    uint32_t slot = NONE, obj = 0;
    if ((sub & SET_BIT) && v < s.n_nodes) {
      slot = lk_find(F.keys, F.n, ((u64)s.nd_ns[v] << 32) | s.nd_rel[v]);
      if (slot != NONE) obj = s.nd_obj[v];
    }
    lk_append64(slot != NONE, ((u64)slot << 32) | obj, dkeys, &ctl->dcount, dcap);
  }
}

// Candidate checks [at, at + m) of the confirmation: pair p = (subject id p / C of the domain, confirm
// request p % C) becomes the kg_query ns:obj#rel@id of that request.
__global__ __launch_bounds__(256) void k_ls_cands(const uint32_t* __restrict__ dom, u64 n_dom,
                                                  const uint32_t* __restrict__ conf, uint32_t C,
                                                  const kg_lookup_subj_set* __restrict__ q, u64 at, u64 m,
                                                  kg_query* cq, uint32_t* creq) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < m; i += stride) {
    const u64 p = at + i, d = p / C;
    if (d >= n_dom) continue;
    const uint32_t r = conf[p % C];
    cq[i] = lk_row<true>(q[r], dom[d]);
    creq[i] = r;
  }
}

// ------------------------------------------------------------------ candidates of an object lookup
// c candidate checks of object obj, one per request of reqs[0, c).  Called by every lane of a wave.
__device__ __forceinline__ void lk_emit_cands(uint32_t c, const uint32_t* reqs, uint32_t obj,
                                              const kg_lookup* __restrict__ q, kg_query* cq, uint32_t* creq, u64 ccap,
                                              LkCtl* ctl) {
  const u64 base = wave_reserve64(&ctl->ccount, c);
  for (uint32_t t = 0; t < c; t++) {
    const u64 pos = base + t;
    if (pos >= ccap) break;
    const uint32_t r = reqs[t];
    cq[pos] = lk_row<false>(q[r], obj);
    creq[pos] = r;
  }
}

// Object obj as a candidate key (request << 32 | obj) of every request of reqs[0, c) -- pg (a paged call's
// pages): of those whose cursor obj has reached.  Called by every lane of a wave.
__device__ __forceinline__ void lk_emit_keys(uint32_t c, const uint32_t* reqs, uint32_t obj,
                                             const PgReq* __restrict__ pg, u64* kkeys, u64 kcap, LkCtl* ctl) {
  uint32_t k = c;
  if (pg) {  // the same for every lane
    k = 0;
    for (uint32_t t = 0; t < c; t++) k += obj >= pg[reqs[t]].from ? 1u : 0u;
  }
  u64 at = wave_reserve64(&ctl->kcount, k);
  for (uint32_t t = 0; t < c; t++) {
    const uint32_t r = reqs[t];
    if (pg && obj < pg[r].from) continue;
    if (at < kcap) kkeys[at] = ((u64)r << 32) | obj;
    at++;
  }
}

// One pass over the nodes: the candidate nodes of the reverse / confirm-nodes requests become checks,
// the objects of the confirm-all requests' namespaces become domain keys (sorted and deduplicated next)
// and the nodes of the formula requests' relations and the impure nodes of their leaves candidate keys
// (the same); on a refreshed snapshot only live nodes give a domain key (DevSnap::nlive).  PAGED (pg: the
// requests' pages): no check is built -- every candidate at or above its request's cursor is a key.
template <bool PAGED>
__global__ __launch_bounds__(256) void k_lk_scan(DevSnap s, CandTab T, const kg_lookup* __restrict__ q, kg_query* cq,
                                                 uint32_t* creq, u64 ccap, u64* dkeys, u64 dcap, u64* kkeys, u64 kcap,
                                                 const PgReq* __restrict__ pg, LkCtl* ctl) {
  const uint32_t stride = gridDim.x * 256;
  for (uint32_t base = blockIdx.x * 256 + (threadIdx.x & ~63u); base < s.n_nodes; base += stride) {
    const uint32_t v = base + lane_id();
    uint32_t c = 0, k = 0, slot = NONE, obj = 0;
    if (v < s.n_nodes) {
      const uint32_t ns = s.nd_ns[v], rel = s.nd_rel[v];
      obj = s.nd_obj[v];
      if (T.rel.n) {
        k = lk_find(T.rel.keys, T.rel.n, ((u64)ns << 32) | rel);
        if (k != NONE && (T.rel.flag[k] || (s.nflags && (s.nflags[v] & NF_IMPURE)))) c = T.rel.count(k);
      }
      // the domain: objects that occur in a tuple -- not the node a refresh left behind without one
      if (T.ns.n && (!s.nlive || s.nlive[v])) slot = lk_find(T.ns.keys, T.ns.n, ns);
    }
    if constexpr (PAGED) lk_emit_keys(c, c ? T.rel.reqs(k) : nullptr, obj, pg, kkeys, kcap, ctl);
    else lk_emit_cands(c, c ? T.rel.reqs(k) : nullptr, obj, q, cq, creq, ccap, ctl);
    lk_append64(slot != NONE, ((u64)slot << 32) | obj, dkeys, &ctl->dcount, dcap);
    if (!T.frel.n) continue;  // the same for every lane
    // formula requests: the node's object as a candidate key of every request of its (ns, rel)
    uint32_t fc = 0, fk = 0;
    if (v < s.n_nodes) {
      // a node of the requests' own relation counts while it is live; a leaf's node when it is impure --
      // then it has check rows, so its object occurs (nlive is about raw rows: a union node has none)
      fk = lk_find(T.frel.keys, T.frel.n, ((u64)s.nd_ns[v] << 32) | s.nd_rel[v]);
      if (fk != NONE && (T.frel.flag[fk] ? (!s.nlive || s.nlive[v]) : (s.nflags && (s.nflags[v] & NF_IMPURE))))
        fc = T.frel.count(fk);
    }
    lk_emit_keys(fc, fc ? T.frel.reqs(fk) : nullptr, obj, PAGED ? pg : nullptr, kkeys, kcap, ctl);
  }
}

// Keys become the checks cq[0, m).  ID_HIGH false: candidate keys request << 32 | id (the formula requests'
// unique keys); true: id << 32 | request (a paged subject round sorted by subject id, k_pg_rows).
template <bool SUBJ, bool ID_HIGH>
__global__ __launch_bounds__(256) void k_lk_key_rows(const u64* __restrict__ keys, u64 m,
                                                     const ReqOf<SUBJ>* __restrict__ q, uint32_t n_reqs, kg_query* cq,
                                                     uint32_t* creq) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < m; i += stride) {
    const uint32_t hi = (uint32_t)(keys[i] >> 32), lo = (uint32_t)keys[i];
    const uint32_t r = min(ID_HIGH ? lo : hi, n_reqs - 1);
    cq[i] = lk_row<SUBJ>(q[r], ID_HIGH ? hi : lo);
    creq[i] = r;
  }
}

// The sorted domain keys: the first key of every run is one object of the namespace; it becomes a check
// for every confirm-all request of that namespace -- PAGED: a candidate key, as k_lk_scan.  The subject
// lookup's per-filter domains (k_ls_dom_sets) take the PAGED form with T.ns holding the filter slots'
// requests (pg == nullptr in an unpaged call: no cursor).
template <bool PAGED>
__global__ __launch_bounds__(256) void k_lk_domain(CandTab T, const u64* __restrict__ dk, u64 nd,
                                                   const kg_lookup* __restrict__ q, kg_query* cq, uint32_t* creq,
                                                   u64 ccap, u64* kkeys, u64 kcap, const PgReq* __restrict__ pg,
                                                   LkCtl* ctl) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < nd; base += stride) {
    const u64 i = base + lane_id();
    uint32_t c = 0, slot = 0, obj = 0;
    if (i < nd) {
      const u64 key = dk[i];
      if (i == 0 || dk[i - 1] != key) {
        slot = (uint32_t)(key >> 32);
        obj = (uint32_t)key;
        if (slot < T.ns.n) c = T.ns.count(slot);
      }
    }
    if constexpr (PAGED) lk_emit_keys(c, c ? T.ns.reqs(slot) : nullptr, obj, pg, kkeys, kcap, ctl);
    else lk_emit_cands(c, c ? T.ns.reqs(slot) : nullptr, obj, q, cq, creq, ccap, ctl);
  }
}

// Where a collect sends the first pass's members and errors.  Called by every lane of a wave (mem: the
// lane's candidate id of request r is a member; bad: it erred with `code`).
// An unpaged call: errors are counted per request, with the code of the lowest id (errmin: id << 32 | code).
struct ErrCount {
  u64* n_errors;
  u64* errmin;
  __device__ void operator()(bool, bool bad, uint32_t r, uint32_t id, uint32_t code, LkCtl*) const {
    if (!bad) return;
    atomicAdd(&n_errors[r], 1ull);
    atomicMin(&errmin[r], ((u64)id << 32) | code);
  }
};
// A paged call: a member joins its request's count; an erring id goes with its code to the error list
// (ekeys: request << 32 | id) -- which of them a page covers is known at the end (k_pg_errs).
struct ErrList {
  PgReq* pg;
  u64* ekeys;
  uint32_t* ecodes;
  u64 ecap;
  __device__ void operator()(bool mem, bool bad, uint32_t r, uint32_t id, uint32_t code, LkCtl* ctl) const {
    if (mem) atomicAdd(&pg[r].nmem, 1ull);
    const u64 ep = wave_reserve64(&ctl->ecount, bad ? 1u : 0u);
    if (bad && ep < ecap) {
      ekeys[ep] = ((u64)r << 32) | id;
      ecodes[ep] = code;
    }
  }
};

// The candidates' answers: members join the output keys (request << 32 | id) and the `confirmed` count,
// errors go to the sink.  SUBJ: the listed id is the query's subject id.  first == 0: a rerun after the
// output list grew -- only the output keys are written again.
template <bool SUBJ, class Sink>
__global__ __launch_bounds__(256) void k_lk_collect(const kg_query* __restrict__ cq, const uint32_t* __restrict__ creq,
                                                    const uint8_t* __restrict__ out, const uint32_t* __restrict__ err,
                                                    u64 n, u64* okeys, u64 ocap, int first, Sink sink, LkCtl* ctl) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n; base += stride) {
    const u64 i = base + lane_id();
    bool mem = false, bad = false;
    uint32_t r = 0, id = 0;
    if (i < n) {
      const uint8_t o = out[i];
      r = creq[i];
      id = SUBJ ? cq[i].t.sobj : cq[i].t.obj;
      mem = o == KG_IS_MEMBER;
      bad = o == KG_ERROR;
    }
    if (first) {
      const uint64_t mm = __ballot(mem);
      if (mm && lane_id() == 0) atomicAdd(&ctl->confirmed, (u64)__popcll(mm));
      sink(mem, bad, r, id, bad ? err[i] : 0u, ctl);
    }
    lk_append64(mem, ((u64)r << 32) | id, okeys, &ctl->ocount, ocap);
  }
}

// ------------------------------------------------------------------ output
__global__ __launch_bounds__(256) void k_lk_finish(const u64* __restrict__ uk, u64 m, uint32_t n_reqs,
                                                   uint64_t* __restrict__ req_off, uint32_t* __restrict__ objs,
                                                   const u64* __restrict__ errmin, uint32_t* __restrict__ err_code) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < m || i <= n_reqs; i += stride) {
    if (i < m) objs[i] = (uint32_t)uk[i];
    if (i <= n_reqs) {
      req_off[i] = lk_lower_bound(uk, m, i << 32);  // first key of request i or later
      if (i < n_reqs) err_code[i] = errmin[i] == ~0ull ? 0u : (uint32_t)errmin[i];
    }
  }
}

// ------------------------------------------------------------------ output as access masks
// The mask tail (Call::finish_mask): row r of the caller's bitmap, `row_words` words, takes bit id - base of
// every output key request << 32 | id with base <= id < base + n_bits.  The keys come as the steps left them,
// unsorted and with duplicates (a walk reaches an id through several nodes): an atomicOr sets a bit once
// however often and in whatever order it is asked to.  rows: the caller's buffer, cleared before this launch.
__global__ __launch_bounds__(256) void k_lk_mask_bits(const u64* __restrict__ okeys, u64 m, uint32_t n_reqs,
                                                      uint32_t base, uint32_t n_bits, uint32_t* rows, size_t row_words) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < m; i += stride) {
    const u64 key = okeys[i];
    const uint32_t r = (uint32_t)(key >> 32), id = (uint32_t)key, d = id - base;
    if (r >= n_reqs || id < base || d >= n_bits) continue;  // d >> 5 < ceil(n_bits / 32) <= row_words
    atomicOr(&rows[(size_t)r * row_words + (d >> 5)], 1u << (d & 31));
  }
}

// One wave per row, four rows per workgroup: the bits set in the row, and the request's error code out of
// errmin as k_lk_finish takes it.
__global__ __launch_bounds__(256) void k_lk_mask_count(const uint32_t* __restrict__ rows, size_t row_words,
                                                       uint32_t n_reqs, uint64_t* __restrict__ n_set,
                                                       const u64* __restrict__ errmin, uint32_t* __restrict__ err_code) {
  const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_reqs) return;  // the whole wave
  const uint32_t* row = rows + (size_t)r * row_words;
  u64 c = 0;
  for (size_t w = lane_id(); w < row_words; w += 64) c += (u64)__popc(row[w]);
  for (int o = 32; o; o >>= 1) c += shfl64(c, lane_id() ^ o);
  if (lane_id() == 0) {
    n_set[r] = c;
    err_code[r] = errmin[r] == ~0ull ? 0u : (uint32_t)errmin[r];
  }
}

// ------------------------------------------------------------------ paged calls: rounds and the page
constexpr u64 PG_FIRST = 64;           // a request's first round checks at most this many candidates
constexpr u64 PG_ROUND_MAX = 1ull << 22;  // and no round more than this many of one request
// The rows one check_batch_device call of a confirmation takes (confirm()).
// unpaged object candidates: the scan has built every row before the first check; the size was never measured
constexpr u64 CHUNK_OBJECTS = 1ull << 28;
// unpaged subject candidates: rows are built a chunk at a time, so this bounds the check buffers (4 Mi rows)
constexpr u64 CHUNK_SUBJECTS = 1ull << 22;
// a paged round: its rows are all built first, like the object candidates'; smaller than theirs, never measured
constexpr u64 CHUNK_ROUND = 1ull << 26;

// the id of entry i of request x's run of candidates
__device__ __forceinline__ uint32_t pg_cand(const PgReq& x, u64 i, const u64* __restrict__ uk,
                                            const uint32_t* __restrict__ dom) {
  return x.implicit ? dom[i] : (uint32_t)uk[i];
}

// The requests' runs: of the sorted unique candidate keys uk[0, m), or of the domain dom[0, n_dom) from
// the cursor on.
__global__ __launch_bounds__(256) void k_pg_init(PgReq* pg, uint32_t n, const u64* __restrict__ uk, u64 m,
                                                 const uint32_t* __restrict__ dom, u64 n_dom) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  PgReq x = pg[i];
  if (x.implicit) {
    x.lo = lk_lower_bound(dom, n_dom, x.from);
    x.hi = n_dom;
  } else {
    x.lo = lk_lower_bound(uk, m, ((u64)i << 32) | x.from);
    x.hi = lk_lower_bound(uk, m, ((u64)i + 1) << 32);
  }
  x.cur = x.base = x.lo;
  x.nmem = 0;
  pg[i] = x;
}

// What request i takes in the next round.  X: the largest candidate id it has checked; it is finished
// when limit + 1 members -- the walk's keys xk[0, mx) (sorted, unique) and the confirmed candidates -- lie
// at or below X: a key above X cannot be placed while an unchecked candidate may lie below it.
struct PgTake {
  PgReq* pg;
  const u64* uk;
  const uint32_t* dom;
  const u64* xk;
  u64 mx;
  __device__ u64 operator()(uint32_t i) const {
    PgReq& x = pg[i];
    const u64 cur = x.cur, left = x.hi - cur, done = cur - x.lo;
    u64 take = 0;
    if (left) {
      bool full = false;
      if (done) {
        const u64 top = (((u64)i << 32) | pg_cand(x, cur - 1, uk, dom)) + 1;
        const u64 below = lk_lower_bound(xk, mx, top) - lk_lower_bound(xk, mx, ((u64)i << 32) | x.from);
        full = x.nmem + below >= (u64)x.limit + 1;
      }
      if (!full) take = min(left, done ? min(done, PG_ROUND_MAX) : PG_FIRST);
    }
    x.base = cur;
    x.cur = cur + take;
    return take;
  }
};
// One workgroup: the round's slices pg[i].[base, cur), their prefix pref[0, n] and the total.
__global__ __launch_bounds__(256) void k_pg_plan(uint32_t n, PgTake take, u64* __restrict__ pref, LkCtl* ctl) {
  lk_block_prefix(n, pref, take);
  if (threadIdx.x == 0) ctl->ptotal = pref[n];
}

// The round's slices as kg_query rows, request-major -- or, keys != nullptr, as keys id << 32 | request: a
// subject lookup's round is sorted by them before its rows are built (k_lk_key_rows), so that neighbouring
// checks share their subject id, as the unpaged confirmation's pairs do -- the check tiers answer such a
// batch several times faster than one whose neighbours share the object.
constexpr u64 PG_SORT_MIN = 4096;  // smaller rounds are bound by their launches, not by the checks
template <bool SUBJ>
__global__ __launch_bounds__(256) void k_pg_rows(const PgReq* __restrict__ pg, uint32_t n, const u64* __restrict__ pref,
                                                 const u64* __restrict__ uk, const uint32_t* __restrict__ dom,
                                                 const ReqOf<SUBJ>* __restrict__ q, kg_query* cq, uint32_t* creq,
                                                 u64* __restrict__ keys) {
  const u64 total = pref[n], stride = (u64)gridDim.x * 256;
  for (u64 e = (u64)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const uint32_t r = csr_owner((const uint64_t*)pref, n, e);
    const PgReq& x = pg[r];
    const uint32_t id = pg_cand(x, min(x.base + (e - pref[r]), x.hi - 1), uk, dom);  // the slice lies in the run
    if (keys) {
      keys[e] = ((u64)id << 32) | r;
      continue;
    }
    cq[e] = lk_row<SUBJ>(q[r], id);
    creq[e] = r;
  }
}

// The page of request i in the call's sorted unique output keys fk[0, m): its keys from klo[i] on that
// lie at or below the largest candidate id it checked (all of them once its candidates ran out), the
// first `limit` kept; next: the last kept id + 1 while a further one follows, else KG_LOOKUP_END.
__global__ __launch_bounds__(256) void k_pg_finish(const PgReq* __restrict__ pg, uint32_t n, const u64* __restrict__ fk,
                                                   u64 m, const u64* __restrict__ uk, const uint32_t* __restrict__ dom,
                                                   u64* __restrict__ kept, u64* __restrict__ klo,
                                                   uint32_t* __restrict__ next) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const PgReq x = pg[i];
  const u64 lo = lk_lower_bound(fk, m, ((u64)i << 32) | x.from);
  u64 hi = lk_lower_bound(fk, m, ((u64)i + 1) << 32);
  if (x.cur < x.hi)
    hi = x.cur > x.lo ? min(hi, lk_lower_bound(fk, m, (((u64)i << 32) | pg_cand(x, x.cur - 1, uk, dom)) + 1)) : lo;
  hi = max(hi, lo);
  const u64 count = hi - lo, k = min(count, (u64)x.limit);
  kept[i] = k;
  klo[i] = lo;
  next[i] = count > k ? (uint32_t)fk[lo + k - 1] + 1u : KG_LOOKUP_END;
}

// The erring ids of the covered ranges [from, next): counted per request, with the code of the lowest.
__global__ __launch_bounds__(256) void k_pg_errs(const u64* __restrict__ ekeys, const uint32_t* __restrict__ ecodes,
                                                 u64 ne, const PgReq* __restrict__ pg, uint32_t n,
                                                 const uint32_t* __restrict__ next, u64* n_errors, u64* errmin) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 e = (u64)blockIdx.x * 256 + threadIdx.x; e < ne; e += stride) {
    const u64 key = ekeys[e];
    const uint32_t r = min((uint32_t)(key >> 32), n - 1), id = (uint32_t)key, nx = next[r];
    if (id < pg[r].from || (nx != KG_LOOKUP_END && id >= nx)) continue;
    atomicAdd(&n_errors[r], 1ull);
    atomicMin(&errmin[r], ((u64)id << 32) | ecodes[e]);
  }
}

struct PgKept {
  const u64* kept;
  __device__ u64 operator()(uint32_t i) const { return kept[i]; }
};
// One workgroup: req_off[0, n] from the kept counts, and the total.
__global__ __launch_bounds__(256) void k_pg_offsets(uint32_t n, PgKept kept, uint64_t* __restrict__ req_off, LkCtl* ctl) {
  lk_block_prefix(n, (u64*)req_off, kept);
  if (threadIdx.x == 0) ctl->ptotal = req_off[n];
}

// The kept ids of every page, and the error codes.
__global__ __launch_bounds__(256) void k_pg_gather(const u64* __restrict__ fk, const u64* __restrict__ klo,
                                                   const uint64_t* __restrict__ req_off, uint32_t n, u64 total,
                                                   uint32_t* __restrict__ objs, const u64* __restrict__ errmin,
                                                   uint32_t* __restrict__ err_code) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total || i < n; i += stride) {
    if (i < total) {
      const uint32_t r = csr_owner(req_off, n, i);
      objs[i] = (uint32_t)fk[klo[r] + (i - req_off[r])];
    }
    if (i < n) err_code[i] = errmin[i] == ~0ull ? 0u : (uint32_t)errmin[i];
  }
}

// ------------------------------------------------------------------ host: a lane's buffers, one call
// The device buffers of lookups on one lane, kept between calls.
struct LookupBufs {
  // the call's requests and what its resolve kernel made of them (bytes): a lane runs one call at a time
  PinBuf<void> h_req, h_res;
  DevBuf<void> d_req, d_res;
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
  DevBuf<u64> kkeys, kkeys2;  // candidate keys of the formula requests
  DevBuf<u64> n_errors, errmin;
  // output
  DevBuf<u64> okeys, okeys2;
  DevBuf<uint64_t> d_off;
  DevBuf<uint32_t> d_objs, d_ecode;
  // paged calls: the requests' pages and runs, a round's prefix, the error list, the pages' extents
  DevBuf<PgReq> pst;
  DevBuf<u64> ppref, ekeys, pkept, pklo, rkeys, rkeys2;
  DevBuf<uint32_t> ecodes, d_next;
  hipEvent_t ev[2] = {};
  hipEvent_t mask_ev = nullptr;  // a mask call: where the caller's stream stood when the call came in
  ~LookupBufs() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (mask_ev) (void)hipEventDestroy(mask_ev);
  }
};

// One lookup call on a lane: what its steps need, and the start and the end both lookups share.
struct Call {
  Snapshot* s;
  Workspace* w;
  hipStream_t st;
  LookupBufs& B;
  // The output keys (B.okeys) and the formula requests' candidate keys (B.kkeys; cap 0: the call has no
  // formula request): request << 32 | id.
  KeyList O, K;
  uint32_t grid_wide;
  int32_t gmax;
  size_t n = 0;
  u64 n_exact = 0, n_cand = 0, n_conf = 0;
  uint64_t st_edges = 0, st_levels = 0;
  // a paged call: the requests' pages (nullptr: unpaged), the rounds run, the erring keys collected
  const kg_lookup_page* pg = nullptr;
  u64 n_rounds = 0, n_ekeys = 0;
  // a mask call (unpaged): the answer goes into the caller's bitmap rows instead of id lists (nullptr: lists)
  const LookupMask* mask = nullptr;

  Call(Snapshot* s_, Lane* L, int32_t gmax_)
      : s(s_), w(L->w), st(L->stream), B(*static_cast<LookupBufs*>(L->lk ? L->lk : (L->lk = new LookupBufs()))),
        grid_wide((uint32_t)s_->n_cu * 4), gmax(gmax_ < 1 ? 5 : gmax_) {}  // as check_batch_begin

  // The start: the requests staged through pinned memory, the timing events, the counters and the
  // per-request error words cleared, the requests resolved (resolve() launches the kernel) and read back.
  template <class Req, class Res, class Resolve>
  int begin(const Req* reqs, size_t n_reqs, const Res** res, Resolve resolve) {
    n = n_reqs;
    if (n > 0x7FFFFFFFull) return set_error(-2, "batch too large");
    HIPC(hipSetDevice(s->device));
    HIPC(B.h_req.reserve(n * sizeof(Req)));
    HIPC(B.d_req.reserve(n * sizeof(Req)));
    HIPC(B.d_res.reserve(n * sizeof(Res)));
    HIPC(B.h_res.reserve(n * sizeof(Res)));
    memcpy(B.h_req.get(), reqs, n * sizeof(Req));
    if (!B.ev[0])
      for (auto& e : B.ev) HIPC(hipEventCreate(&e));
    HIPC(B.ctl.reserve(1));
    HIPC(B.n_errors.reserve(n));
    HIPC(B.errmin.reserve(n));
    HIPC(hipEventRecord(B.ev[0], st));
    HIPC(hipMemsetAsync(B.ctl.get(), 0, sizeof(LkCtl), st));
    HIPC(hipMemsetAsync(B.n_errors.get(), 0, n * 8, st));
    HIPC(hipMemsetAsync(B.errmin.get(), 0xFF, n * 8, st));
    HIPC(hipMemcpyAsync(B.d_req.get(), B.h_req.get(), n * sizeof(Req), hipMemcpyHostToDevice, st));
    resolve((uint32_t)((n + 255) / 256), (const Req*)B.d_req.get(), (Res*)B.d_res.get());
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(B.h_res.get(), B.d_res.get(), n * sizeof(Res), hipMemcpyDeviceToHost, st));
    if (int rc = w->wait(st, true)) return rc;
    *res = (const Res*)B.h_res.get();
    O.cap = s->knobs.lookup_cap ? s->knobs.lookup_cap : std::max<u64>(65536, B.okeys.cap());
    HIPC(B.okeys.reserve((size_t)O.cap));
    return 0;
  }

  // the candidate key list of a call with formula requests; starts at lookup_cap like the output keys
  int want_cand_keys() {
    K.cap = s->knobs.lookup_cap ? s->knobs.lookup_cap : std::max<u64>(65536, B.kkeys.cap());
    HIPC(B.kkeys.reserve((size_t)K.cap));
    return 0;
  }

  // a list of at least `need` keys that keeps the finished steps'
  int regrow(KeyList& l, DevBuf<u64>& buf, u64 need) {
    l.cap = std::max<u64>(need, 2 * l.cap);
    if (l.cap > buf.cap()) {
      DevBuf<u64> nb;
      HIPC(nb.reserve((size_t)l.cap));
      if (l.have) HIPC(hipMemcpyAsync(nb.get(), buf.get(), (size_t)l.have * 8, hipMemcpyDeviceToDevice, st));
      HIPC(hipStreamSynchronize(st));
      buf = std::move(nb);
    }
    return 0;
  }
  // both device counters back at the finished steps' keys: the step that overflowed a list is rerun
  int rewind() {
    u64* hb = (u64*)w->host_buf(65536);
    if (!hb) return set_error(-1, "pinned host buffer");
    hb[0] = O.have;
    hb[1] = K.have;
    HIPC(hipMemcpyAsync(&B.ctl.get()->ocount, &hb[0], 8, hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(&B.ctl.get()->kcount, &hb[1], 8, hipMemcpyHostToDevice, st));
    HIPC(hipStreamSynchronize(st));  // the pinned words are reused by the next readback
    return 0;
  }
  // after a step: true if a list was too small for the step's true counts h -- it has grown, the counters
  // are rewound and the step runs again; false: the step's keys are kept
  int settle(const LkCtl& h, bool* again) {
    *again = h.ocount > O.cap || h.kcount > K.cap;
    if (h.ocount > O.cap)
      if (int rc = regrow(O, B.okeys, h.ocount)) return rc;
    if (h.kcount > K.cap)
      if (int rc = regrow(K, B.kkeys, h.kcount)) return rc;
    if (*again) return rewind();
    O.have = h.ocount;
    K.have = h.kcount;
    return 0;
  }

  // a grid for n items, one per thread
  dim3 grid(u64 n) const { return dim3((uint32_t)std::min<u64>(grid_wide, n / 256 + 1)); }

  int read_ctl(LkCtl* h) {
    void* hb = w->host_buf(65536);
    if (!hb) return set_error(-1, "pinned host buffer");
    HIPC(hipMemcpyAsync(hb, B.ctl.get(), sizeof(LkCtl), hipMemcpyDeviceToHost, st));
    if (int rc = w->wait(st, true)) return rc;
    memcpy(h, hb, sizeof(LkCtl));
    return 0;
  }

  // The end: the keys sorted, duplicates dropped, split by request, the output arrays in one pinned block.
  int finish(kg_lookup_buf* out);
  // The end of a mask call: the keys as they are -- no sort, no unique step, no count read back -- set their
  // bits in the caller's rows; only the per-request words cross the bus.
  int finish_mask();
  // the end of an unpaged call
  int end(kg_lookup_buf* out) { return mask ? finish_mask() : finish(out); }
  // the m ids of B.d_objs with B.d_off / n_errors / d_ecode (and d_next: a paged call's next[n]) copied
  // into one pinned block; the call's counters
  int deliver(kg_lookup_buf* out, u64 m, uint32_t** next);
  // a paged call: the requests' cursors on the walk's bits, their pages on the device (implicit[i]: request
  // i's candidates are the domain)
  int page_upload(std::vector<GReq>& greq, const std::vector<uint8_t>& implicit);
  // the end of a paged call: every request's page cut out of the sorted unique keys
  int finish_page(kg_lookup_pages* out, const u64* uk, const uint32_t* dom);
};

// keys a[0, n) sorted over their bits [0, end_bit): *out (in a or b); with n_uniq, one of each.
template <class K>
int sort_keys(Call& c, DevBuf<K>& a, DevBuf<K>& b, size_t n, int end_bit, const K** out, u64* n_uniq) {
  LookupBufs& B = c.B;
  HIPC(b.reserve(n));
  hipcub::DoubleBuffer<K> kb(a.get(), b.get());
  size_t sort_bytes = 0, uniq_bytes = 0;
  HIPC(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, kb, n, 0, end_bit, c.st));
  if (n_uniq) HIPC(hipcub::DeviceSelect::Unique(nullptr, uniq_bytes, (K*)nullptr, (K*)nullptr, (u64*)nullptr, n, c.st));
  HIPC(B.tmp.reserve(std::max(sort_bytes, uniq_bytes) + 16));
  HIPC(hipcub::DeviceRadixSort::SortKeys(B.tmp.get(), sort_bytes, kb, n, 0, end_bit, c.st));
  *out = kb.Current();
  if (!n_uniq) return 0;
  HIPC(hipcub::DeviceSelect::Unique(B.tmp.get(), uniq_bytes, kb.Current(), kb.Alternate(), &B.ctl.get()->nuniq, n, c.st));
  LkCtl h;
  if (int rc = c.read_ctl(&h)) return rc;
  *n_uniq = std::min<u64>(h.nuniq, n);
  *out = kb.Alternate();
  return 0;
}

// the bits of a key request << 32 | id of a call with n requests
int key_bits(size_t n) {
  int end_bit = 33;
  while (end_bit < 64 && ((u64)n >> (end_bit - 32))) end_bit++;
  return end_bit;
}

int Call::finish(kg_lookup_buf* out) {
  u64 m = 0;
  const u64* uk = B.okeys.get();
  if (O.have)
    if (int rc = sort_keys(*this, B.okeys, B.okeys2, (size_t)O.have, key_bits(n), &uk, &m)) return rc;
  HIPC(B.d_off.reserve(n + 1));
  HIPC(B.d_objs.reserve((size_t)std::max<u64>(m, 1)));
  HIPC(B.d_ecode.reserve(n));
  hipLaunchKernelGGL(k_lk_finish, grid(std::max<u64>(m, n + 1)), dim3(256), 0, st, uk, m, (uint32_t)n, B.d_off.get(),
                     B.d_objs.get(), (const u64*)B.errmin.get(), B.d_ecode.get());
  HIPC(hipGetLastError());
  return deliver(out, m, nullptr);
}

int Call::deliver(kg_lookup_buf* out, u64 m, uint32_t** next) {
  // one pinned block: req_off[n + 1] | n_errors[n] | objs[m] | err_code[n] | next[n] (a paged call)
  const size_t bytes = ((size_t)n + 1) * 8 + (size_t)n * 8 + (size_t)m * 4 + (size_t)n * 4 + (next ? (size_t)n * 4 : 0);
  char* blk = (char*)tree_pool_get(bytes);
  if (!blk) return set_error(KG_ERR_RESOURCE_CODE, "lookup: pinned output allocation failed");
  uint64_t* o_off = (uint64_t*)blk;
  uint64_t* o_nerr = o_off + n + 1;
  uint32_t* o_objs = (uint32_t*)(o_nerr + n);
  uint32_t* o_ecode = o_objs + m;
  uint32_t* o_next = o_ecode + n;
  int rc = 0;
  if (hipMemcpyAsync(o_off, B.d_off.get(), (n + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(o_nerr, B.n_errors.get(), n * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      (m && hipMemcpyAsync(o_objs, B.d_objs.get(), (size_t)m * 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipMemcpyAsync(o_ecode, B.d_ecode.get(), n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      (next && hipMemcpyAsync(o_next, B.d_next.get(), n * 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
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
  out->exact = n_exact;
  out->candidates = n_cand;
  out->confirmed = n_conf;
  out->reverse_edges = st_edges;
  out->levels = st_levels;
  if (next) *next = o_next;
  return 0;
}

int Call::finish_mask() {
  const LookupMask& M = *mask;
  kg_lookup_mask_buf* out = M.out;
  // the lane's first write to the caller's buffer comes after what the caller's stream had enqueued on it
  // (nullptr: the null stream -- a framework's default stream is that one; nothing to wait for when it is idle)
  if (!B.mask_ev) HIPC(hipEventCreateWithFlags(&B.mask_ev, hipEventDisableTiming));
  HIPC(hipEventRecord(B.mask_ev, M.user));
  HIPC(hipStreamWaitEvent(st, B.mask_ev, 0));
  HIPC(hipMemsetAsync(M.d_mask, 0, n * M.row_words * 4, st));
  if (O.have)
    hipLaunchKernelGGL(k_lk_mask_bits, grid(O.have), dim3(256), 0, st, (const u64*)B.okeys.get(), O.have, (uint32_t)n,
                       M.base, M.n_bits, M.d_mask, M.row_words);
  HIPC(B.d_off.reserve(n));  // the rows' counts
  HIPC(B.d_ecode.reserve(n));
  hipLaunchKernelGGL(k_lk_mask_count, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, st, (const uint32_t*)M.d_mask,
                     M.row_words, (uint32_t)n, B.d_off.get(), (const u64*)B.errmin.get(), B.d_ecode.get());
  HIPC(hipGetLastError());
  // one pinned block: n_set[n] | n_errors[n] | err_code[n]
  const size_t bytes = (size_t)n * 8 + (size_t)n * 8 + (size_t)n * 4;
  char* blk = (char*)tree_pool_get(bytes);
  if (!blk) return set_error(KG_ERR_RESOURCE_CODE, "lookup: pinned output allocation failed");
  uint64_t* o_nset = (uint64_t*)blk;
  uint64_t* o_nerr = o_nset + n;
  uint32_t* o_ecode = (uint32_t*)(o_nerr + n);
  int rc = 0;
  if (hipMemcpyAsync(o_nset, B.d_off.get(), n * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(o_nerr, B.n_errors.get(), n * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(o_ecode, B.d_ecode.get(), n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipEventRecord(B.ev[1], st) != hipSuccess)
    rc = set_error(-1, "lookup: D2H copy failed");
  if (!rc) rc = w->wait(st, true);  // the mask is complete when the call returns
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
  out->n_set = o_nset;
  out->n_errors = o_nerr;
  out->err_code = o_ecode;
  out->n_reqs = n;
  out->exact = n_exact;
  out->candidates = n_cand;
  out->confirmed = n_conf;
  out->reverse_edges = st_edges;
  out->levels = st_levels;
  out->kernel_ms = ms;
  out->pinned = bytes;
  return 0;
}

// f(std::true_type) or f(std::false_type): a kernel's template flag from a runtime one.
template <class F>
void with_flag(bool flag, F f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

// The answers of the candidates B.cq[0, n_cand) join the output keys (k_lk_collect).  The output list grows
// once at most: the second pass writes the keys alone, members and errors are counted on the first.
template <bool SUBJ, class Sink>
int collect(Call& c, u64 n_cand, const Sink& sink) {
  LookupBufs& B = c.B;
  for (int pass = 0;; pass++) {
    hipLaunchKernelGGL((k_lk_collect<SUBJ, Sink>), c.grid(n_cand), dim3(256), 0, c.st, (const kg_query*)B.cq.get(),
                       (const uint32_t*)B.creq.get(), (const uint8_t*)B.cout.get(), (const uint32_t*)B.cerr.get(), n_cand,
                       B.okeys.get(), c.O.cap, pass == 0 ? 1 : 0, sink, B.ctl.get());
    HIPC(hipGetLastError());
    LkCtl h;
    if (int rc = c.read_ctl(&h)) return rc;
    bool again = false;
    if (int rc = c.settle(h, &again)) return rc;
    if (again) {
      if (pass) return set_error(KG_ERR_RESOURCE_CODE, "lookup: output list overflowed twice");
      continue;
    }
    c.n_conf = h.confirmed;
    c.n_ekeys = h.ecount;  // a paged call's error list (ErrList); 0 in an unpaged call
    return 0;
  }
}

// One confirmation: `total` candidates as kg_query rows through check_batch_device, `chunk` rows a call, and
// their answers collected.  whole: rows(0, total) builds every row (B.cq / B.creq [0, total)) before the
// first check and one collect follows the last; else rows(at, m) builds the rows of chunk [at, at + m) at
// the head of the buffers and each chunk is checked and collected before the next is built.
template <bool SUBJ, class Rows, class Sink>
int confirm(Call& c, u64 total, u64 chunk, bool whole, const Rows& rows, const Sink& sink) {
  if (!total) return 0;
  LookupBufs& B = c.B;
  const u64 span = whole ? total : std::min(chunk, total);  // rows built, and collected, at a time
  HIPC(B.cq.reserve((size_t)span));  // keeps what it holds when that is large enough (the scan's rows)
  HIPC(B.creq.reserve((size_t)span));
  HIPC(B.cout.reserve((size_t)span));
  HIPC(B.cerr.reserve((size_t)span));
  for (u64 at = 0; at < total; at += span) {
    const u64 m = std::min(span, total - at);
    if (int rc = rows(at, m)) return rc;
    HIPC(hipGetLastError());
    for (u64 k = 0; k < m; k += chunk) {
      const size_t kn = (size_t)std::min(chunk, m - k);
      if (int rc = check_batch_device(c.s, c.w, B.cq.get() + k, kn, c.gmax, B.cout.get() + k, B.cerr.get() + k, nullptr))
        return rc;
    }
    if (int rc = collect<SUBJ>(c, m, sink)) return rc;
  }
  c.n_cand += total;
  return 0;
}

// The keys[0, m) as the rows cq[0, m) (k_lk_key_rows).
template <bool SUBJ, bool ID_HIGH>
void launch_key_rows(Call& c, const u64* keys, u64 m, kg_query* cq, uint32_t* creq) {
  hipLaunchKernelGGL((k_lk_key_rows<SUBJ, ID_HIGH>), c.grid(m), dim3(256), 0, c.st, keys, m,
                     (const ReqOf<SUBJ>*)c.B.d_req.get(), (uint32_t)c.n, cq, creq);
}

// The call's candidate keys sorted, one of each: uk[0, *m) (a call without one: nullptr, 0).
int unique_cand_keys(Call& c, const u64** uk, u64* m) {
  *uk = nullptr;
  *m = 0;
  return !c.K.have ? 0 : sort_keys(c, c.B.kkeys, c.B.kkeys2, (size_t)c.K.have, key_bits(c.n), uk, m);
}

// buf holds at least `need` entries and still its first `keep`.
template <class T>
int keep_grow(Call& c, DevBuf<T>& buf, size_t keep, size_t need) {
  if (need <= buf.cap()) return 0;
  DevBuf<T> nb;
  HIPC(nb.reserve(std::max(need, 2 * buf.cap())));
  if (keep) HIPC(hipMemcpyAsync(nb.get(), buf.get(), keep * sizeof(T), hipMemcpyDeviceToDevice, c.st));
  HIPC(hipStreamSynchronize(c.st));
  buf = std::move(nb);
  return 0;
}

// ------------------------------------------------------------------ host: a paged call
int Call::page_upload(std::vector<GReq>& greq, const std::vector<uint8_t>& implicit) {
  for (GReq& g : greq) g.from = pg[g.req].from;
  std::vector<PgReq> h(n);
  for (size_t i = 0; i < n; i++) h[i] = PgReq{0, 0, 0, 0, 0, pg[i].from, pg[i].limit, implicit.empty() ? 0u : implicit[i], 0};
  HIPC(B.pst.reserve(n));
  HIPC(hipMemcpyAsync(B.pst.get(), h.data(), n * sizeof(PgReq), hipMemcpyHostToDevice, st));
  HIPC(hipStreamSynchronize(st));  // h is pageable
  return 0;
}

// The confirmation of a paged call in ascending rounds.  uk[0, m): the call's sorted unique candidate
// keys; dom[0, n_dom): the domain of the implicit requests (any_implicit: there is one).  A call without
// candidates takes no round.
template <bool SUBJ>
int page_rounds(Call& c, const u64* uk, u64 m, const uint32_t* dom, u64 n_dom, bool any_implicit) {
  LookupBufs& B = c.B;
  const uint32_t n = (uint32_t)c.n, blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_pg_init, dim3(blocks), dim3(256), 0, c.st, B.pst.get(), n, uk, m, dom, n_dom);
  HIPC(hipGetLastError());
  if (!m && !(any_implicit && n_dom)) return 0;
  // the walk's keys sorted, one of each, at the head of B.okeys: a round counts a request's keys below an id
  if (c.O.have) {
    HIPC(B.okeys2.reserve((size_t)c.O.cap));
    const u64* xk = nullptr;
    u64 mx = 0;
    if (int rc = sort_keys(c, B.okeys, B.okeys2, (size_t)c.O.have, key_bits(c.n), &xk, &mx)) return rc;
    if (xk != B.okeys.get()) std::swap(B.okeys, B.okeys2);
    c.O.have = mx;
    if (int rc = c.rewind()) return rc;
  }
  const u64 mx = c.O.have;
  HIPC(B.ppref.reserve((size_t)n + 1));
  for (;;) {
    // B.okeys may have grown: its head is read through the current pointer
    hipLaunchKernelGGL(k_pg_plan, dim3(1), dim3(256), 0, c.st, n, PgTake{B.pst.get(), uk, dom, B.okeys.get(), mx},
                       B.ppref.get(), B.ctl.get());
    HIPC(hipGetLastError());
    LkCtl h;
    if (int rc = c.read_ctl(&h)) return rc;
    const u64 total = h.ptotal;
    if (!total) return 0;
    c.n_rounds++;
    if (int rc = keep_grow(c, B.ekeys, (size_t)c.n_ekeys, (size_t)(c.n_ekeys + total))) return rc;
    if (int rc = keep_grow(c, B.ecodes, (size_t)c.n_ekeys, (size_t)(c.n_ekeys + total))) return rc;
    // the round's rows, request-major -- a subject round of PG_SORT_MIN checks or more ordered by subject id
    auto rows = [&](u64, u64) -> int {
      const bool by_subject = SUBJ && total >= PG_SORT_MIN;
      if (by_subject) HIPC(B.rkeys.reserve((size_t)total));
      hipLaunchKernelGGL(k_pg_rows<SUBJ>, c.grid(total), dim3(256), 0, c.st, (const PgReq*)B.pst.get(), n,
                         (const u64*)B.ppref.get(), uk, dom, (const ReqOf<SUBJ>*)B.d_req.get(), B.cq.get(), B.creq.get(),
                         by_subject ? B.rkeys.get() : nullptr);
      if (by_subject) {  // the round's keys sorted, then its rows
        HIPC(hipGetLastError());
        const u64* sk = nullptr;
        if (int rc = sort_keys(c, B.rkeys, B.rkeys2, (size_t)total, 64, &sk, (u64*)nullptr)) return rc;
        launch_key_rows<true, true>(c, sk, total, B.cq.get(), B.creq.get());
      }
      return 0;
    };
    const ErrList sink{B.pst.get(), B.ekeys.get(), B.ecodes.get(), (u64)std::min(B.ekeys.cap(), B.ecodes.cap())};
    if (int rc = confirm<SUBJ>(c, total, CHUNK_ROUND, true, rows, sink)) return rc;
  }
}

int Call::finish_page(kg_lookup_pages* out, const u64* uk, const uint32_t* dom) {
  u64 m = 0;
  const u64* fk = B.okeys.get();
  if (O.have)
    if (int rc = sort_keys(*this, B.okeys, B.okeys2, (size_t)O.have, key_bits(n), &fk, &m)) return rc;
  const uint32_t nr = (uint32_t)n, blocks = (nr + 255) / 256;
  HIPC(B.pkept.reserve(n));
  HIPC(B.pklo.reserve(n));
  HIPC(B.d_next.reserve(n));
  HIPC(B.d_off.reserve(n + 1));
  HIPC(B.d_ecode.reserve(n));
  hipLaunchKernelGGL(k_pg_finish, dim3(blocks), dim3(256), 0, st, (const PgReq*)B.pst.get(), nr, fk, m, uk, dom,
                     B.pkept.get(), B.pklo.get(), B.d_next.get());
  if (n_ekeys)
    hipLaunchKernelGGL(k_pg_errs, grid(n_ekeys), dim3(256), 0, st, (const u64*)B.ekeys.get(),
                       (const uint32_t*)B.ecodes.get(), n_ekeys, (const PgReq*)B.pst.get(), nr,
                       (const uint32_t*)B.d_next.get(), B.n_errors.get(), B.errmin.get());
  hipLaunchKernelGGL(k_pg_offsets, dim3(1), dim3(256), 0, st, nr, PgKept{B.pkept.get()}, B.d_off.get(), B.ctl.get());
  HIPC(hipGetLastError());
  LkCtl h;
  if (int rc = read_ctl(&h)) return rc;
  const u64 total = std::min(h.ptotal, m);
  HIPC(B.d_objs.reserve((size_t)std::max<u64>(total, 1)));
  hipLaunchKernelGGL(k_pg_gather, grid(std::max<u64>(total, n)), dim3(256), 0, st, fk, (const u64*)B.pklo.get(),
                     (const uint64_t*)B.d_off.get(), nr, total, B.d_objs.get(), (const u64*)B.errmin.get(),
                     B.d_ecode.get());
  HIPC(hipGetLastError());
  if (int rc = deliver(&out->list, total, &out->next)) return rc;
  out->rounds = n_rounds;
  out->pinned = out->list.pinned;
  return 0;
}

// ------------------------------------------------------------------ host: the walk
// The walk buffers of a lane: allocated for the snapshot's nodes on first use, the masks all clear on
// return, the call's request bits on the device.  *scan_bytes: hipcub's scan temporaries.
int walk_reserve(Call& c, const std::vector<GReq>& greq, size_t* scan_bytes) {
  LookupBufs& B = c.B;
  const uint32_t nn = c.s->ds.n_nodes;
  if (B.walk_nodes < nn) {
    B.walk_nodes = 0;
    for (auto* b : {&B.vis, &B.next, &B.cmask}) HIPC(b->reserve(nn));
    for (auto* b : {&B.len, &B.pref}) HIPC(b->reserve((size_t)nn + 1));
    for (auto* b : {&B.fl[0], &B.fl[1], &B.touched}) HIPC(b->reserve(nn));
    B.walk_nodes = nn;
    B.dirty = true;
  }
  if (B.dirty) {
    HIPC(hipMemsetAsync(B.vis.get(), 0, (size_t)B.walk_nodes * 8, c.st));
    HIPC(hipMemsetAsync(B.next.get(), 0, (size_t)B.walk_nodes * 8, c.st));
    B.dirty = false;
  }
  HIPC(B.greq.reserve(greq.size()));
  HIPC(hipMemcpyAsync(B.greq.get(), greq.data(), greq.size() * sizeof(GReq), hipMemcpyHostToDevice, c.st));
  HIPC(hipStreamSynchronize(c.st));  // greq is pageable
  *scan_bytes = 0;
  HIPC(hipcub::DeviceScan::ExclusiveSum(nullptr, *scan_bytes, B.len.get(), B.pref.get(), (size_t)nn + 1, c.st));
  HIPC(B.tmp.reserve(*scan_bytes + 16));
  return 0;
}

// After a group: the masks cleared by replaying the touched list, the node lists empty.  h: the
// counters as the group's last launch left them.
int walk_finish(Call& c, const LkCtl& h) {
  LookupBufs& B = c.B;
  hipLaunchKernelGGL(k_lk_clear, dim3(c.grid_wide), dim3(256), 0, c.st, B.vis.get(), B.next.get(),
                     (const uint32_t*)B.touched.get(), B.walk_nodes, B.ctl.get());
  hipLaunchKernelGGL(k_lk_lists_reset, dim3(1), dim3(1), 0, c.st, B.ctl.get());
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(c.st));
  B.dirty = h.over != 0;  // an overflowed touched list did not name every node to clear
  if (h.over) return set_error(KG_ERR_RESOURCE_CODE, "lookup: a node list overflowed");
  return 0;
}

// A frontier above PREFIX_IN_KERNEL entries: its row lengths (B.len) and their prefix (B.pref).
template <class Len>
int prep_large(Call& c, uint32_t F, Len len_of, uint32_t* fcount_out, size_t scan_bytes) {
  hipLaunchKernelGGL(k_lk_prep<Len>, dim3(F / 256 + 1), dim3(256), 0, c.st, F, len_of, c.B.len.get(), fcount_out);
  HIPC(hipcub::DeviceScan::ExclusiveSum(c.B.tmp.get(), scan_bytes, c.B.len.get(), c.B.pref.get(), (size_t)F + 1, c.st));
  return 0;
}

// The level's first prepare: lengths len_a -> B.pref, resetting the list the level builds; a frontier of
// up to PREFIX_IN_KERNEL entries in one launch, together with len_b -> B.len (the forward walk's adj rows).
template <class LenA, class LenB>
int prep_first(Call& c, const Walk& W, uint32_t F, LenA len_a, LenB len_b, size_t scan_bytes) {
  uint32_t* fc_out = &c.B.ctl.get()->fcount[W.fsel];
  if (F > PREFIX_IN_KERNEL) return prep_large(c, F, len_a, fc_out, scan_bytes);
  hipLaunchKernelGGL((k_lk_prep_scan<LenA, LenB>), dim3(1), dim3(256), 0, c.st, F, len_a, c.B.pref.get(), len_b,
                     c.B.len.get(), fc_out);
  return 0;
}

template <class Body>
void launch_edges(Call& c, const Frontier& f, const Rows& r, const u64* pref, const Body& body) {
  hipLaunchKernelGGL(k_lk_frontier_edges<Body>, dim3(c.grid_wide), dim3(256), 0, c.st, f, r, pref, c.B.ctl.get(), body);
}

// The direction policies of walk_groups.  res: the resolved requests (.depth); formula(): the request's
// bits list candidate keys; sets(): the bit lists subject sets (Walk::smask); seed(): the launch of
// level 0 -- true: *F is its frontier's size, false: read it back; level(): the launches of level j >=
// FIRST_LEVEL on the frontier f -- *expanded == false: they built no next frontier, the group's walk ends.
//
// Reverse: the seed lists the subject's holders; level j = 1 .. D-1 follows the frontier's reverse edges.
struct ReverseWalk {
  const LReq* res;
  bool formula(uint32_t req) const { return res[req].mode == LK_FORMULA; }
  bool sets(const GReq&) const { return false; }
  static constexpr int32_t FIRST_LEVEL = 1;
  bool seed(Call& c, const Walk& W, const GReq*, uint32_t gn, uint32_t*) const {
    hipLaunchKernelGGL(k_lk_seed, dim3(gn), dim3(256), 0, c.st, c.s->ds, W, (const LReq*)c.B.d_res.get());
    return false;
  }
  int level(Call& c, const Walk& W, const Frontier& f, u64 live, u64, size_t scan_bytes, bool* expanded) const {
    const DevSnap& ds = c.s->ds;
    const RowLen<true> take{f, ds.radj_off, live, c.B.next.get(), ds.nflags};
    if (int rc = prep_first(c, W, f.F, take, NoLen{}, scan_bytes)) return rc;
    launch_edges(c, f, Rows{ds.radj_off, ds.radj, c.s->n_set_edges}, c.B.pref.get(), Hop<true>{ds, W, ~0ull});
    *expanded = true;
    return 0;
  }
};

// Forward: level j = 0 .. D-1 lists the subject ids and subject sets of the frontier's check rows (emit) and,
// for the requests that go one level further (xlive), follows its adj rows (expand).
struct ForwardWalk {
  const SReq* res;
  bool formula(uint32_t req) const { return res[req].mode == LS_FORMULA; }
  bool sets(const GReq& g) const { return g.sns != KG_SUBJECT_ID; }
  Rows check;  // the check rows
  static constexpr int32_t FIRST_LEVEL = 0;
  // the first frontier is the group's distinct roots: no readback before level 0
  bool seed(Call& c, const Walk& W, const GReq* g, uint32_t gn, uint32_t* F) const {
    hipLaunchKernelGGL(k_ls_seed, dim3(1), dim3(64), 0, c.st, c.s->ds, W, gn);
    std::set<uint32_t> roots;
    for (uint32_t b = 0; b < gn; b++) roots.insert(g[b].root);
    *F = (uint32_t)roots.size();
    return true;
  }
  int level(Call& c, const Walk& W, const Frontier& f, u64 live, u64 xlive, size_t scan_bytes, bool* expanded) const {
    const DevSnap& ds = c.s->ds;
    const RowLen<true> take{f, check.off, live, c.B.next.get(), nullptr};
    const RowLen<false> kept{f, ds.adj_off, xlive, nullptr, nullptr};
    if (int rc = prep_first(c, W, f.F, take, kept, scan_bytes)) return rc;
    launch_edges(c, f, check, c.B.pref.get(), Emit{ds, W});
    *expanded = xlive != 0;
    if (!xlive) return 0;
    const u64* apref = c.B.len.get();  // the prefix of the adj rows
    if (f.F > PREFIX_IN_KERNEL) {  // the emit has read pref: the same two buffers take the adj rows
      if (int rc = prep_large(c, f.F, kept, (uint32_t*)nullptr, scan_bytes)) return rc;
      apref = c.B.pref.get();
    }
    launch_edges(c, f, Rows{ds.adj_off, ds.adj, c.s->n_set_edges}, apref, Hop<false>{ds, W, xlive});
    return 0;
  }
};

// The walk of a call, 64 requests per group.  The counters are read back after every level that built a
// frontier, and once more at the end if the last one did not.
template <class Dir>
int walk_groups(Call& c, const std::vector<GReq>& greq, const Dir& dir) {
  if (greq.empty()) return 0;
  LookupBufs& B = c.B;
  size_t scan_bytes = 0;
  if (int rc = walk_reserve(c, greq, &scan_bytes)) return rc;
  for (size_t g0 = 0; g0 < greq.size();) {
    const uint32_t gn = (uint32_t)std::min<size_t>(64, greq.size() - g0);
    int32_t max_d = 1;
    for (uint32_t b = 0; b < gn; b++) max_d = std::max(max_d, dir.res[greq[g0 + b].req].depth);
    u64 fmask = 0, smask = 0;
    for (uint32_t b = 0; b < gn; b++) {
      if (dir.formula(greq[g0 + b].req)) fmask |= 1ull << b;
      if (dir.sets(greq[g0 + b])) smask |= 1ull << b;
    }
    Walk W{B.vis.get(), B.next.get(), B.fl[0].get(), 0, B.touched.get(), B.walk_nodes, B.okeys.get(), c.O.cap,
           fmask, B.kkeys.get(), c.K.cap, B.greq.get() + g0, B.ctl.get(), c.pg != nullptr, smask};
    B.dirty = true;
    LkCtl h;
    uint32_t cur = 0, F = 0;
    bool h_now = !dir.seed(c, W, &greq[g0], gn, &F);  // h holds the counters as they are on the device
    HIPC(hipGetLastError());
    if (h_now) {
      if (int rc = c.read_ctl(&h)) return rc;
      F = std::min(h.fcount[0], B.walk_nodes);
    }
    for (int32_t j = Dir::FIRST_LEVEL; j <= max_d - 1 && F; j++) {
      u64 live = 0, xlive = 0;  // requests whose depth reaches level j / goes on into level j + 1
      for (uint32_t b = 0; b < gn; b++) {
        const int32_t d = dir.res[greq[g0 + b].req].depth;
        if (d - 1 >= j) live |= 1ull << b;
        if (d - 1 >= j + 1) xlive |= 1ull << b;
      }
      W.fout = B.fl[cur ^ 1].get();
      W.fsel = cur ^ 1;
      bool expanded = false;
      h_now = false;
      const Frontier f{B.fl[cur].get(), B.cmask.get(), F};
      if (int rc = dir.level(c, W, f, live, xlive, scan_bytes, &expanded)) return rc;
      HIPC(hipGetLastError());
      c.st_levels++;
      if (!expanded) break;
      if (int rc = c.read_ctl(&h)) return rc;
      h_now = true;
      cur ^= 1;
      F = std::min(h.fcount[cur], B.walk_nodes);
    }
    if (!h_now)
      if (int rc = c.read_ctl(&h)) return rc;
    if (int rc = walk_finish(c, h)) return rc;
    bool again = false;  // the group's keys did not fit: a larger list, the group again
    if (int rc = c.settle(h, &again)) return rc;
    if (again) continue;
    c.st_edges = h.edges;  // summed on the device over every run, reruns included
    g0 += gn;
  }
  c.n_exact = c.O.have;
  return 0;
}

// ------------------------------------------------------------------ host: the ends both lookups share
// The end of a paged call: every candidate is a key -- one of each, checked in ascending rounds (a subject
// lookup's confirm requests index the domain dom[0, n_dom) instead) -- and the pages cut out.
template <bool SUBJ>
int paged_tail(Call& c, const uint32_t* dom, u64 n_dom, bool any_implicit, kg_lookup_pages* out) {
  const u64* uk;
  u64 m;
  if (int rc = unique_cand_keys(c, &uk, &m)) return rc;
  if (int rc = page_rounds<SUBJ>(c, uk, m, dom, n_dom, any_implicit)) return rc;
  return c.finish_page(out, uk, dom);
}

// ------------------------------------------------------------------ host: the steps of an object lookup
// The plan: the walk's request bits, and the requests grouped by what makes a node their candidate.
struct ObjPlan {
  std::vector<GReq> greq;
  std::map<u64, std::vector<uint32_t>> by_rel, by_frel;  // ns << 32 | rel -> requests (CandTab::rel, ::frel)
  std::map<uint32_t, std::vector<uint32_t>> by_ns;       // CandTab::ns
  bool tables() const { return !by_rel.empty() || !by_ns.empty() || !by_frel.empty(); }
};
int plan_objects(Call& c, const kg_lookup* reqs, const LReq* lr, ObjPlan* P) {
  const Snapshot* s = c.s;
  for (size_t i = 0; i < c.n; i++) {
    if (lr[i].mode == LK_ALL) {
      P->by_ns[reqs[i].ns].push_back((uint32_t)i);
      continue;
    }
    if (lr[i].mode == LK_FORMULA) {
      if (lr[i].plan >= s->h_fplans.size()) return set_error(-1, "lookup: formula plan out of range");
      const FPlan& F = s->h_fplans[lr[i].plan];
      // the walk listens to the walk leaves; the scan takes the relation and every leaf
      GReq g{reqs[i].ns, reqs[i].rel, (uint32_t)i, 0, 0, {}};
      P->by_frel[((u64)reqs[i].ns << 32) | reqs[i].rel].push_back((uint32_t)i);
      for (uint32_t j = 0; j < F.n_leaves && j < (uint32_t)FP_LEAVES; j++) {
        P->by_frel[((u64)reqs[i].ns << 32) | F.leaf[j]].push_back((uint32_t)i);
        if ((F.walk_leaves >> j) & 1u) g.listen[g.n_listen++] = F.leaf[j];
      }
      if (lr[i].hcount && g.n_listen) P->greq.push_back(g);
      continue;
    }
    if (lr[i].mode == LK_REVERSE && lr[i].hcount)
      P->greq.push_back(GReq{reqs[i].ns, reqs[i].rel, (uint32_t)i, 0, 1, {reqs[i].rel}});
    // candidates of a reverse request: impure nodes -- none without node flags
    if (lr[i].mode == LK_NODES || s->ds.nflags) P->by_rel[((u64)reqs[i].ns << 32) | reqs[i].rel].push_back((uint32_t)i);
  }
  return 0;
}

// The table of `by` appended to blob (u32 words, 64-bit keys on 8 bytes, low word first): keys[n] | flag[n] |
// off[n + 1] | req[..]; returns where it starts.  flag(key, its requests): the key's flag.
template <class K, class Flag>
size_t tab_append(std::vector<uint32_t>& blob, const std::map<K, std::vector<uint32_t>>& by, Flag flag) {
  if (blob.size() & 1) blob.push_back(0);
  const size_t at = blob.size();
  for (auto& kv : by) {
    blob.push_back((uint32_t)kv.first);
    if (sizeof(K) == 8) blob.push_back((uint32_t)((u64)kv.first >> 32));
  }
  for (auto& kv : by) blob.push_back(flag(kv.first, kv.second) ? 1u : 0u);
  uint32_t n_req = 0;
  for (auto& kv : by) {
    blob.push_back(n_req);
    n_req += (uint32_t)kv.second.size();
  }
  blob.push_back(n_req);
  for (auto& kv : by) blob.insert(blob.end(), kv.second.begin(), kv.second.end());
  return at;
}
// The table of n keys that tab_append put at word `at` of the blob, now at base on the device.
template <class K>
GroupTab<K> tab_on(const uint32_t* base, size_t at, size_t n) {
  const uint32_t* flag = base + at + n * (sizeof(K) / 4);
  return GroupTab<K>{(const K*)(base + at), flag, flag + n, flag + 2 * n + 1, (uint32_t)n};
}

// The plan's three tables, uploaded as one blob (B.tab).
int upload_tables(Call& c, const ObjPlan& P, const kg_lookup* reqs, const LReq* lr, CandTab* T) {
  typedef const std::vector<uint32_t>& Reqs;
  std::vector<uint32_t> blob;
  const size_t rel = tab_append(blob, P.by_rel, [&](u64, Reqs rs) { return lr[rs[0]].mode == LK_NODES; });
  const size_t ns = tab_append(blob, P.by_ns, [](uint32_t, Reqs) { return false; });
  // every node of a request's own relation (its rows join the answer), the impure nodes of a leaf
  const size_t frel = tab_append(blob, P.by_frel, [&](u64 key, Reqs rs) {
    bool own = false;
    for (uint32_t r : rs) own |= reqs[r].rel == (uint32_t)key;
    return own;
  });
  blob.push_back(0);
  HIPC(c.B.tab.reserve(blob.size() + 2));
  HIPC(hipMemcpyAsync(c.B.tab.get(), blob.data(), blob.size() * 4, hipMemcpyHostToDevice, c.st));
  HIPC(hipStreamSynchronize(c.st));  // blob is pageable
  const uint32_t* tb = c.B.tab.get();
  *T = CandTab{tab_on<u64>(tb, rel, P.by_rel.size()), tab_on<uint32_t>(tb, ns, P.by_ns.size()),
               tab_on<u64>(tb, frel, P.by_frel.size())};
  return 0;
}

// One pass over the nodes (k_lk_scan) into lists of ccap checks and dcap domain keys; *h: the counters after.
int scan_nodes(Call& c, const CandTab& T, u64 ccap, u64 dcap, LkCtl* h) {
  LookupBufs& B = c.B;
  const bool paged = c.pg != nullptr;
  HIPC(B.cq.reserve((size_t)ccap));
  HIPC(B.creq.reserve((size_t)ccap));
  if (dcap) HIPC(B.dkeys.reserve((size_t)dcap));
  HIPC(hipMemsetAsync(&B.ctl.get()->ccount, 0, 16, c.st));  // ccount, dcount
  if (T.frel.n || paged)  // the candidate keys back at the walk's
    if (int rc = c.rewind()) return rc;
  const dim3 grid(std::max(1u, std::min(c.grid_wide, c.s->ds.n_nodes / 256 + 1)));
  with_flag(paged, [&](auto P) {
    hipLaunchKernelGGL(k_lk_scan<decltype(P)::value>, grid, dim3(256), 0, c.st, c.s->ds, T, (const kg_lookup*)B.d_req.get(),
                       B.cq.get(), B.creq.get(), ccap, B.dkeys.get(), dcap, B.kkeys.get(), c.K.cap,
                       (const PgReq*)B.pst.get(), B.ctl.get());
  });
  HIPC(hipGetLastError());
  return c.read_ctl(h);
}
// The nd domain keys sorted, every distinct object a candidate of its namespace's requests (k_lk_domain).
int scan_domain(Call& c, const CandTab& T, u64 ccap, size_t nd, LkCtl* h) {
  LookupBufs& B = c.B;
  const u64* dk = nullptr;
  if (int rc = sort_keys(c, B.dkeys, B.dkeys2, nd, 64, &dk, (u64*)nullptr)) return rc;
  with_flag(c.pg != nullptr, [&](auto P) {
    hipLaunchKernelGGL(k_lk_domain<decltype(P)::value>, c.grid(nd), dim3(256), 0, c.st, T, dk, (u64)nd,
                       (const kg_lookup*)B.d_req.get(), B.cq.get(), B.creq.get(), ccap, B.kkeys.get(), c.K.cap,
                       (const PgReq*)B.pst.get(), B.ctl.get());
  });
  HIPC(hipGetLastError());
  return c.read_ctl(h);
}
// The candidates: one pass over the nodes, then the sorted domains of the confirm-all namespaces; both again
// when a list was too small.  *n_rows: the checks built (B.cq / B.creq; none in a paged call).
int object_candidates(Call& c, const CandTab& T, u64* n_rows) {
  LookupBufs& B = c.B;
  u64 ccap = std::max<u64>(65536, B.cq.cap()), dcap = T.ns.n ? std::max<u64>(65536, B.dkeys.cap()) : 0;
  for (;;) {
    LkCtl h;
    if (int rc = scan_nodes(c, T, ccap, dcap, &h)) return rc;
    if (h.dcount > dcap || h.kcount > c.K.cap) {
      dcap = std::max(dcap, h.dcount);
      ccap = std::max(ccap, h.ccount);
      if (h.kcount > c.K.cap)
        if (int rc = c.regrow(c.K, B.kkeys, h.kcount)) return rc;
      continue;
    }
    if (h.ccount <= ccap && h.dcount)
      if (int rc = scan_domain(c, T, ccap, (size_t)h.dcount, &h)) return rc;
    if (h.ccount > ccap) {
      ccap = h.ccount;
      continue;
    }
    if (h.kcount > c.K.cap) {  // a paged call: the domain's keys did not fit
      if (int rc = c.regrow(c.K, B.kkeys, h.kcount)) return rc;
      continue;
    }
    *n_rows = h.ccount;
    c.K.have = h.kcount;
    return 0;
  }
}

// The end of an unpaged call: the formula requests' candidate keys, one of each, as rows behind the scan's
// n_rows; every row through the check, the answers collected, the output.
int unpaged_objects_tail(Call& c, u64 n_rows, kg_lookup_buf* out) {
  LookupBufs& B = c.B;
  const u64* uk;
  u64 m;
  if (int rc = unique_cand_keys(c, &uk, &m)) return rc;
  if (int rc = keep_grow(c, B.cq, (size_t)n_rows, (size_t)(n_rows + m))) return rc;
  if (int rc = keep_grow(c, B.creq, (size_t)n_rows, (size_t)(n_rows + m))) return rc;
  auto key_rows = [&](u64, u64) -> int {  // the scan has built the others
    if (m) launch_key_rows<false, false>(c, uk, m, B.cq.get() + n_rows, B.creq.get() + n_rows);
    return 0;
  };
  if (int rc = confirm<false>(c, n_rows + m, CHUNK_OBJECTS, true, key_rows, ErrCount{B.n_errors.get(), B.errmin.get()}))
    return rc;
  return c.end(out);
}

// ------------------------------------------------------------------ host: the steps of a subject lookup
// The plan: the walk's bits (walk mode: the root; formula mode: one per root of a walk leaf, any_formula),
// each with what its request lists, and the confirm-mode requests: those that list subject ids (conf) and
// those that list subject sets, by filter sns << 32 | srel (by_filter).
struct SubjPlan {
  std::vector<GReq> greq;
  std::vector<uint32_t> conf;
  std::map<u64, std::vector<uint32_t>> by_filter;
  bool any_formula = false;
};
void plan_subjects(Call& c, const kg_lookup_subj_set* reqs, const SReq* sr, SubjPlan* P) {
  const uint32_t nn = c.s->ds.n_nodes;
  for (size_t i = 0; i < c.n; i++) {
    const kg_lookup_subj_set& x = reqs[i];
    const bool ids = x.sns == KG_SUBJECT_ID;
    if (sr[i].mode == LS_WALK && sr[i].root < nn)
      P->greq.push_back(GReq{x.ns, x.rel, (uint32_t)i, sr[i].root, 0, {}, 0, x.sns, x.srel});
    else if (sr[i].mode == LS_FORMULA) {
      for (uint32_t t = 0; t < sr[i].n_froot && t < (uint32_t)FP_LEAVES; t++)
        if (sr[i].froot[t] < nn) {
          P->greq.push_back(GReq{x.ns, x.rel, (uint32_t)i, sr[i].froot[t], 0, {}, 0, x.sns, x.srel});
          P->any_formula = true;
        }
    } else if (sr[i].mode == LS_CONFIRM) {
      if (ids) P->conf.push_back((uint32_t)i);
      else P->by_filter[((u64)x.sns << 32) | x.srel].push_back((uint32_t)i);
    }
  }
}

// The domain of the confirmation, dom[0, *n_dom): the subject ids that occur in a tuple, one of each --
// ascending when listed from the check rows csub[0, n_rows) or for a paged call, which indexes it by id (the
// bitmap's distinct ids come in the order its waves reserved their entries).
int subject_domain(Call& c, const uint32_t* csub, u64 n_rows, const uint32_t** dom, u64* n_dom) {
  LookupBufs& B = c.B;
  const DevSnap& ds = c.s->ds;
  const bool bits = ds.hbits && !c.s->knobs.lookup_domain_rows;
  u64 dcap = std::max<u64>(65536, B.dom.cap());
  for (;;) {
    HIPC(B.dom.reserve((size_t)dcap));
    HIPC(hipMemsetAsync(&B.ctl.get()->dcount, 0, 8, c.st));
    if (bits)
      hipLaunchKernelGGL(k_ls_dom_bits, dim3(std::min(c.grid_wide, ds.hbits_n / 8192 + 1)), dim3(256), 0, c.st, ds.hbits,
                         ds.hbits_n, B.dom.get(), dcap, B.ctl.get());
    else
      hipLaunchKernelGGL(k_ls_dom_rows, c.grid(n_rows), dim3(256), 0, c.st, csub, n_rows, B.dom.get(), dcap,
                         B.ctl.get());
    HIPC(hipGetLastError());
    LkCtl h;
    if (int rc = c.read_ctl(&h)) return rc;
    if (h.dcount > dcap) {
      dcap = h.dcount;
      continue;
    }
    *n_dom = h.dcount;
    break;
  }
  *dom = B.dom.get();
  if (!bits && *n_dom)  // an id per row entry that holds it: sort, one of each
    return sort_keys(c, B.dom, B.dom2, (size_t)*n_dom, 31, dom, n_dom);
  if (bits && *n_dom && c.pg) return sort_keys(c, B.dom, B.dom2, (size_t)*n_dom, 32, dom, (u64*)nullptr);
  return 0;
}

// The candidates of the confirm requests that list subject sets: the per-filter domains out of the check rows
// csub[0, n_rows) (k_ls_dom_sets), sorted; every distinct set of a filter becomes a candidate key request
// << 32 | object id of that filter's requests (k_lk_domain) -- a paged call's at or above the request's cursor --
// next to the formula requests' keys.  A step whose list was too small runs again.
int set_candidates(Call& c, const std::map<u64, std::vector<uint32_t>>& by_filter, const uint32_t* csub, u64 n_rows) {
  LookupBufs& B = c.B;
  std::vector<uint32_t> blob;
  const size_t at = tab_append(blob, by_filter, [](u64, const std::vector<uint32_t>&) { return false; });
  blob.push_back(0);
  HIPC(B.tab.reserve(blob.size() + 2));
  HIPC(hipMemcpyAsync(B.tab.get(), blob.data(), blob.size() * 4, hipMemcpyHostToDevice, c.st));
  HIPC(hipStreamSynchronize(c.st));  // blob is pageable
  const GroupTab<u64> F = tab_on<u64>(B.tab.get(), at, by_filter.size());
  CandTab T{};
  T.ns = GroupTab<uint32_t>{nullptr, F.flag, F.off, F.req, F.n};  // k_lk_domain reads the slots' requests only
  u64 dcap = std::max<u64>(65536, B.dkeys.cap()), nd = 0;
  for (;;) {
    HIPC(B.dkeys.reserve((size_t)dcap));
    HIPC(hipMemsetAsync(&B.ctl.get()->dcount, 0, 8, c.st));
    hipLaunchKernelGGL(k_ls_dom_sets, c.grid(n_rows), dim3(256), 0, c.st, c.s->ds, csub, n_rows, F, B.dkeys.get(), dcap,
                       B.ctl.get());
    HIPC(hipGetLastError());
    LkCtl h;
    if (int rc = c.read_ctl(&h)) return rc;
    if (h.dcount > dcap) {
      dcap = h.dcount;
      continue;
    }
    nd = h.dcount;
    break;
  }
  if (!nd) return 0;
  const u64* dk = nullptr;
  if (int rc = sort_keys(c, B.dkeys, B.dkeys2, (size_t)nd, 64, &dk, (u64*)nullptr)) return rc;
  for (;;) {
    hipLaunchKernelGGL(k_lk_domain<true>, c.grid(nd), dim3(256), 0, c.st, T, dk, nd, (const kg_lookup*)nullptr,
                       (kg_query*)nullptr, (uint32_t*)nullptr, (u64)0, B.kkeys.get(), c.K.cap,
                       c.pg ? (const PgReq*)B.pst.get() : nullptr, B.ctl.get());
    HIPC(hipGetLastError());
    LkCtl h;
    if (int rc = c.read_ctl(&h)) return rc;
    if (h.kcount > c.K.cap) {
      if (int rc = c.regrow(c.K, B.kkeys, h.kcount)) return rc;
      if (int rc = c.rewind()) return rc;
      continue;
    }
    c.K.have = h.kcount;
    return 0;
  }
}

// The end of an unpaged call: every (subject id of the domain, confirm request) pair, subject-id-major, then
// the candidate keys (the formula requests', the subject sets of the confirm requests' filters), one of each,
// through the check in chunks; the output.
int unpaged_subjects_tail(Call& c, const std::vector<uint32_t>& conf, const uint32_t* dom, u64 n_dom, kg_lookup_buf* out) {
  LookupBufs& B = c.B;
  const ErrCount sink{B.n_errors.get(), B.errmin.get()};
  if (n_dom) {
    const uint32_t C = (uint32_t)conf.size();
    HIPC(B.tab.reserve(C));
    HIPC(hipMemcpyAsync(B.tab.get(), conf.data(), (size_t)C * 4, hipMemcpyHostToDevice, c.st));
    HIPC(hipStreamSynchronize(c.st));  // conf is pageable
    auto pair_rows = [&](u64 at, u64 m) -> int {
      hipLaunchKernelGGL(k_ls_cands, c.grid(m), dim3(256), 0, c.st, dom, n_dom, (const uint32_t*)B.tab.get(), C,
                         (const kg_lookup_subj_set*)B.d_req.get(), at, m, B.cq.get(), B.creq.get());
      return 0;
    };
    if (int rc = confirm<true>(c, n_dom * C, CHUNK_SUBJECTS, false, pair_rows, sink)) return rc;
  }
  const u64* uk;
  u64 nk;
  if (int rc = unique_cand_keys(c, &uk, &nk)) return rc;
  auto key_rows = [&](u64 at, u64 m) -> int {
    launch_key_rows<true, false>(c, uk + at, m, B.cq.get(), B.creq.get());
    return 0;
  };
  if (int rc = confirm<true>(c, nk, CHUNK_SUBJECTS, false, key_rows, sink)) return rc;
  return c.end(out);
}

}  // namespace

void lookup_bufs_free(void* p) { delete static_cast<LookupBufs*>(p); }

// kg_lookup_objects on lane L (its stream and workspace; the caller holds the workspace's mutex).  pages:
// kg_lookup_objects_page -- the same steps, with the candidates as keys checked in rounds, into pout.
static int lookup_objects_on(Snapshot* s, Lane* L, const kg_lookup* reqs, const kg_lookup_page* pages, size_t n,
                             int32_t gmax, kg_lookup_buf* out, kg_lookup_pages* pout, const LookupMask* mask = nullptr) {
  Call c(s, L, gmax);
  c.pg = pages;
  c.mask = mask;
  const LReq* lr = nullptr;
  const bool formula = s->knobs.lookup_formula && s->n_fplans && s->d_fidx;
  if (int rc = c.begin(reqs, n, &lr, [&](uint32_t blocks, const kg_lookup* d_req, LReq* d_lr) {
        hipLaunchKernelGGL(k_lk_resolve, dim3(blocks), dim3(256), 0, c.st, s->ds, formula ? s->d_fidx : nullptr,
                           (const FPlan*)s->d_fplans, d_req, (uint32_t)n, c.gmax, (uint64_t)s->n_check_rows, d_lr);
      }))
    return rc;
  ObjPlan P;
  if (int rc = plan_objects(c, reqs, lr, &P)) return rc;
  if (pages)
    if (int rc = c.page_upload(P.greq, {})) return rc;
  // the formula requests' candidates are keys; a paged call's all are
  if (!P.by_frel.empty() || (pages && (!P.by_rel.empty() || !P.by_ns.empty())))
    if (int rc = c.want_cand_keys()) return rc;
  if (int rc = walk_groups(c, P.greq, ReverseWalk{lr})) return rc;
  u64 n_rows = 0;
  if (P.tables()) {
    CandTab T;
    if (int rc = upload_tables(c, P, reqs, lr, &T)) return rc;
    if (int rc = object_candidates(c, T, &n_rows)) return rc;
  }
  if (pages) return paged_tail<false>(c, nullptr, 0, false, pout);
  return unpaged_objects_tail(c, n_rows, out);
}

// kg_lookup_subject_sets on lane L (as lookup_objects; kg_lookup_subjects: every request lists ids).  Walk-mode
// requests are listed by the forward walk, 64 bits per group; formula-mode requests take a bit per walk-leaf
// root there, and what those list is checked; the others by a check of every subject id of the domain, or of
// every subject set of their filter's domain.
static int lookup_subjects_on(Snapshot* s, Lane* L, const kg_lookup_subj_set* reqs, const kg_lookup_page* pages, size_t n,
                              int32_t gmax, kg_lookup_buf* out, kg_lookup_pages* pout, const LookupMask* mask = nullptr) {
  Call c(s, L, gmax);
  c.pg = pages;
  c.mask = mask;
  const DevSnap& ds = s->ds;
  const uint32_t* csub = ds.crow_off ? ds.crow_subj : ds.row_subj;
  const uint64_t n_rows = s->n_check_rows;
  const SReq* sr = nullptr;
  const bool formula = s->knobs.lookup_formula && s->n_fplans && s->d_fidx;
  if (int rc = c.begin(reqs, n, &sr, [&](uint32_t blocks, const kg_lookup_subj_set* d_req, SReq* d_sr) {
        hipLaunchKernelGGL(k_ls_resolve, dim3(blocks), dim3(256), 0, c.st, ds, formula ? s->d_fidx : nullptr,
                           (const FPlan*)s->d_fplans, d_req, (uint32_t)n, c.gmax, d_sr);
      }))
    return rc;
  SubjPlan P;
  plan_subjects(c, reqs, sr, &P);
  if (pages) {  // the confirm requests for ids index the domain, the others their unique keys
    std::vector<uint8_t> implicit(n, 0);
    for (uint32_t r : P.conf) implicit[r] = 1;
    if (int rc = c.page_upload(P.greq, implicit)) return rc;
  }
  if (P.any_formula || !P.by_filter.empty())
    if (int rc = c.want_cand_keys()) return rc;
  if (int rc = walk_groups(c, P.greq, ForwardWalk{sr, Rows{ds.crow_off ? ds.crow_off : ds.row_off, csub, n_rows}}))
    return rc;
  u64 n_dom = 0;
  const uint32_t* dom = nullptr;
  if (!P.conf.empty() && n_rows && csub)
    if (int rc = subject_domain(c, csub, n_rows, &dom, &n_dom)) return rc;
  if (!P.by_filter.empty() && n_rows && csub)
    if (int rc = set_candidates(c, P.by_filter, csub, n_rows)) return rc;
  if (pages) return paged_tail<true>(c, dom, n_dom, !P.conf.empty(), pout);
  return unpaged_subjects_tail(c, P.conf, dom, n_dom, out);
}

int lookup_objects(Snapshot* s, Lane* L, const kg_lookup* reqs, size_t n, int32_t gmax, kg_lookup_buf* out) {
  return lookup_objects_on(s, L, reqs, nullptr, n, gmax, out, nullptr);
}
// kg_lookup_subjects' requests as requests that list ids
static std::vector<kg_lookup_subj_set> id_requests(const kg_lookup_subj* reqs, size_t n) {
  std::vector<kg_lookup_subj_set> v(n);
  for (size_t i = 0; i < n; i++)
    v[i] = kg_lookup_subj_set{reqs[i].ns, reqs[i].obj, reqs[i].rel, KG_SUBJECT_ID, 0, reqs[i].max_depth};
  return v;
}
int lookup_subjects(Snapshot* s, Lane* L, const kg_lookup_subj* reqs, size_t n, int32_t gmax, kg_lookup_buf* out) {
  return lookup_subjects_on(s, L, id_requests(reqs, n).data(), nullptr, n, gmax, out, nullptr);
}
int lookup_subject_sets(Snapshot* s, Lane* L, const kg_lookup_subj_set* reqs, size_t n, int32_t gmax,
                        kg_lookup_buf* out) {
  return lookup_subjects_on(s, L, reqs, nullptr, n, gmax, out, nullptr);
}
int lookup_subject_sets_page(Snapshot* s, Lane* L, const kg_lookup_subj_set* reqs, const kg_lookup_page* pages, size_t n,
                             int32_t gmax, kg_lookup_pages* out) {
  return lookup_subjects_on(s, L, reqs, pages, n, gmax, &out->list, out);
}
int lookup_objects_page(Snapshot* s, Lane* L, const kg_lookup* reqs, const kg_lookup_page* pages, size_t n, int32_t gmax,
                        kg_lookup_pages* out) {
  return lookup_objects_on(s, L, reqs, pages, n, gmax, &out->list, out);
}
int lookup_subjects_page(Snapshot* s, Lane* L, const kg_lookup_subj* reqs, const kg_lookup_page* pages, size_t n,
                         int32_t gmax, kg_lookup_pages* out) {
  return lookup_subjects_on(s, L, id_requests(reqs, n).data(), pages, n, gmax, &out->list, out);
}

// The mask calls: the unpaged steps, ending in Call::finish_mask.
int lookup_objects_mask(Snapshot* s, Lane* L, const kg_lookup* reqs, size_t n, int32_t gmax, const LookupMask& mask) {
  return lookup_objects_on(s, L, reqs, nullptr, n, gmax, nullptr, nullptr, &mask);
}
int lookup_subject_sets_mask(Snapshot* s, Lane* L, const kg_lookup_subj_set* reqs, size_t n, int32_t gmax,
                             const LookupMask& mask) {
  return lookup_subjects_on(s, L, reqs, nullptr, n, gmax, nullptr, nullptr, &mask);
}
void lookup_mask_free(kg_lookup_mask_buf* out) {
  if (out->pinned) tree_pool_put(out->n_set, (size_t)out->pinned);
  memset(out, 0, sizeof *out);
}

void lookup_free(kg_lookup_buf* out) {
  if (out->pinned) tree_pool_put(out->req_off, (size_t)out->pinned);
  else free(out->req_off);
  memset(out, 0, sizeof *out);
}

}  // namespace kg
