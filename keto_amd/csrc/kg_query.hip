// kg_query.hip -- kg_snapshot_query: the reference's list call (relationtuple.Manager.GetRelationTuples,
// internal/persistence/sql/relationtuples.go:203-244) on the device snapshot: a RelationQuery whose every
// field is optional, rows in order-key order, keyset paging.  Raw rows only (row_off / row_subj), as
// kg_rows.hip: a materialised union node's merged check rows are not tuples of its relation.
//
// A request is a filter plus a "smallest `limit` keys above `after`" selection:
//   node stage   (ns, obj, rel) all set: one node-map probe; the scan is that node's row, entered at the
//                first key above `after` (the keys ascend inside a node).  Some set: one pass over the
//                nodes compacts the matching ones, a prefix over their row lengths spreads their entries
//                over the grid (owner search, as k_lk_frontier_edges).  None set: every row entry.
//   row scan     one lane per entry (per four consecutive entries of a plain range: one 16-byte load of
//                their subjects) tests the subject, then key > after; the matches are counted, their
//                smallest and largest key kept, and their (key, position) pairs appended to a list of
//                `cap` entries -- cap = max("query_cap", min(limit, entries)) -- while they fit.
//   selection    matches that fit the list are sorted and cut.  Otherwise the composite (key, position)
//                is narrowed 11 bits a pass, from the highest bit in which the smallest and the largest
//                matching key differ: a pass histograms the next digit of the matches inside the current
//                prefix, the host takes the bucket in which the running count reaches `limit`, and the
//                matches at or below that bucket are all that can be on the page.  When they fit the list
//                (at least `limit` of them do exist) one more scan compacts them.  The composite is
//                unique, so the narrowing ends for any key distribution -- at the latest with one entry in
//                the bucket -- and equal keys come out in position order.
//   decode       the page's positions become kg_tuple records (owner by search in row_off).
// Memory: the list (two arrays of cap u64, twice for the sort), 20 B per node for the node stage, the
// 2048-bucket histogram.  Nothing grows with the rows or with the matches.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kg_bfs.h"
#include "kg_internal.h"
#include "kg_snapshot.h"

namespace kg {
namespace {

typedef unsigned long long u64;

constexpr uint32_t Q_DIGIT = 11, Q_BUCKETS = 1u << Q_DIGIT;
enum : uint32_t { QS_ANY = 0, QS_EQ = 1, QS_NONE = 2 };

// A resolved request.
struct QRes {
  uint32_t smode;  // QS_*: any subject / row_subj == subj / no row can match
  uint32_t subj;   // tagged subject (QS_EQ)
  uint32_t node;   // (ns, obj, rel) all set: the node, or NONE
  uint32_t pad;
  u64 lo, hi;      // ... and the part of its row whose keys are above `after`
};

// What a scan tests: the row entries [lo, lo + total), or -- m > 0 -- the rows of nodes[0, m), entry e
// owned by the node j with pref[j] <= e < pref[j + 1].
struct QDom {
  u64 lo, total;
  const uint32_t* nodes;
  const u64* pref;
  uint32_t m;
};
struct QSel {
  uint32_t smode, subj;
  u64 after;
};
// The prefix the narrowing has fixed: the top kbits of the key are `key` and -- kbits == 64 -- the top pbits
// of the position are `pos`.
struct QBound {
  u64 key, pos;
  uint32_t kbits, pbits;
};
struct QCtl {
  u64 count;   // matches (scan), matches at or below the bound (compaction): TRUE counts
  u64 minkey, maxkey;
  u64 nsel;    // nodes the node stage kept
  u64 hist[Q_BUCKETS];
};

__device__ __forceinline__ bool q_in_bucket(const QBound& b, u64 k, u64 p) {
  if (b.kbits && (k >> (64 - b.kbits)) != b.key) return false;
  return !b.pbits || (p >> (64 - b.pbits)) == b.pos;
}
__device__ __forceinline__ bool q_at_or_below(const QBound& b, u64 k, u64 p) {
  if (!b.kbits) return true;
  const u64 kp = k >> (64 - b.kbits);
  if (kp != b.key) return kp < b.key;
  return !b.pbits || (p >> (64 - b.pbits)) <= b.pos;
}
// the next d bits below the prefix (d <= what is left of the field the prefix ends in)
__device__ __forceinline__ uint32_t q_digit(const QBound& b, u64 k, u64 p, uint32_t d) {
  if (b.kbits < 64) return (uint32_t)(k >> (64 - b.kbits - d)) & ((1u << d) - 1);
  return (uint32_t)(p >> (64 - b.pbits - d)) & ((1u << d) - 1);
}

__device__ __forceinline__ u64 q_pos(const DevSnap& s, const QDom& d, u64 e) {
  if (!d.m) return d.lo + e;
  const uint32_t own = csr_owner((const uint64_t*)d.pref, d.m, e);
  return s.row_off[d.nodes[own]] + (e - d.pref[own]);
}

// ------------------------------------------------------------------ request mapping
__global__ __launch_bounds__(256) void k_q_resolve(DevSnap s, const kg_row_query* __restrict__ q, uint32_t n,
                                                   const uint64_t* __restrict__ rkey, QRes* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const kg_row_query x = q[i];
  QRes r{QS_ANY, 0, NONE, 0, 0, 0};
  if (x.mask & KG_Q_SUBJECT) {
    if (x.t.sns == KG_SUBJECT_ID) {
      r.smode = x.t.sobj & SET_BIT ? QS_NONE : QS_EQ;  // an untagged entry is an id below 2^31
      r.subj = x.t.sobj;
    } else {
      const uint32_t sn = s.n_nodes ? nmap_find(s, x.t.sns, x.t.srel, x.t.sobj) : NONE;
      r.smode = sn < s.n_nodes ? QS_EQ : QS_NONE;
      r.subj = SET_BIT | sn;
    }
  }
  if ((x.mask & 7u) == 7u && s.n_nodes) {
    const uint32_t v = nmap_find(s, x.t.ns, x.t.rel, x.t.obj);
    if (v < s.n_nodes) {
      r.node = v;
      u64 lo = s.row_off[v];
      const u64 hi = s.row_off[v + 1];
      if (rkey) {  // the first entry whose key is above `after`
        u64 a = lo, b = hi;
        while (a < b) {
          const u64 mid = (a + b) >> 1;
          if (rkey[mid] <= x.after) a = mid + 1;
          else b = mid;
        }
        lo = a;
      } else {  // key = position + 1
        lo = max(lo, min((u64)x.after, hi));
      }
      r.lo = lo;
      r.hi = hi;
    }
  }
  out[i] = r;
}

// ------------------------------------------------------------------ node stage
// The nodes with a row whose triple matches the fields of mask.
__global__ __launch_bounds__(256) void k_q_nodes(DevSnap s, uint32_t mask, uint32_t ns, uint32_t obj, uint32_t rel,
                                                 uint32_t* __restrict__ nodes, QCtl* ctl) {
  const uint32_t stride = gridDim.x * 256;
  for (uint32_t base = blockIdx.x * 256 + (threadIdx.x & ~63u); base < s.n_nodes; base += stride) {
    const uint32_t v = base + lane_id();
    bool hit = false;
    if (v < s.n_nodes) {
      hit = (!(mask & KG_Q_NS) || s.nd_ns[v] == ns) && (!(mask & KG_Q_OBJ) || s.nd_obj[v] == obj) &&
            (!(mask & KG_Q_REL) || s.nd_rel[v] == rel) && s.row_off[v + 1] > s.row_off[v];
    }
    const u64 at = wave_reserve64(&ctl->nsel, hit ? 1u : 0u);
    if (hit && at < s.n_nodes) nodes[at] = v;
  }
}
// len[j] = the row length of nodes[j]; len[m] = 0 (the scan's sentinel)
__global__ __launch_bounds__(256) void k_q_node_len(DevSnap s, const uint32_t* __restrict__ nodes, uint32_t m,
                                                    u64* __restrict__ len) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) len[j] = s.row_off[nodes[j] + 1] - s.row_off[nodes[j]];
  else if (j == m) len[m] = 0;
}

// ------------------------------------------------------------------ row scan
enum : int { SCAN_COUNT = 0, SCAN_HIST = 1, SCAN_TAKE = 2 };
// One lane per entry of the domain -- VEC (a range of row entries): per four consecutive entries, their
// subjects in one 16-byte load where the four lie inside the range.  SCAN_COUNT: counts the matches, keeps
// their smallest and largest key and appends them while they fit; SCAN_HIST: histograms the next `digit`
// bits of the matches inside the bound's prefix; SCAN_TAKE: appends the matches at or below the bound.
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void k_q_scan(DevSnap s, QDom d, QSel f, const uint64_t* __restrict__ rkey, QBound b,
                                                uint32_t digit, u64* __restrict__ ckey, u64* __restrict__ cpos, u64 cap,
                                                QCtl* ctl) {
  constexpr int V = VEC ? 4 : 1;
  __shared__ uint32_t hist[MODE == SCAN_HIST ? Q_BUCKETS : 1];
  if (MODE == SCAN_HIST) {
    for (uint32_t i = threadIdx.x; i < Q_BUCKETS; i += 256) hist[i] = 0;
    __syncthreads();
  }
  u64 mn = ~0ull, mx = 0, tail = 0;
  bool full = false;  // wave-uniform: an append of this wave reached the end of the list
  const u64 head = VEC ? (d.lo & 3) : 0, end = d.lo + d.total;  // VEC: item i is the entries lo - head + 4i ..+3
  const u64 items = VEC ? (d.total + head + 3) / 4 : d.total;
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < items; base += stride) {
    const u64 it = base + lane_id();
    bool hit[V];
    u64 key[V], pos[V];
#pragma unroll
    for (int j = 0; j < V; j++) hit[j] = false, key[j] = 0, pos[j] = 0;
    if (it < items) {
      if (VEC) {
        const u64 p0 = d.lo - head + 4 * it;
        uint32_t sv[4] = {~f.subj, ~f.subj, ~f.subj, ~f.subj};  // never the subject asked for
        if (f.smode == QS_EQ) {
          if (p0 >= d.lo && p0 + 3 < end) {  // 16-byte aligned: row_subj is, p0 is a multiple of 4
            const uint4 x = *reinterpret_cast<const uint4*>(s.row_subj + p0);
            sv[0] = x.x, sv[1] = x.y, sv[2] = x.z, sv[3] = x.w;
          } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
              if (p0 + j >= d.lo && p0 + j < end) sv[j] = s.row_subj[p0 + j];
          }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const u64 p = p0 + j;
          if (p >= d.lo && p < end && (f.smode == QS_ANY || sv[j] == f.subj)) {
            pos[j] = p;
            key[j] = rkey ? rkey[p] : p + 1;
            hit[j] = key[j] > f.after;
          }
        }
      } else {
        pos[0] = q_pos(s, d, it);
        if (f.smode == QS_ANY || s.row_subj[pos[0]] == f.subj) {
          key[0] = rkey ? rkey[pos[0]] : pos[0] + 1;
          hit[0] = key[0] > f.after;
        }
      }
    }
    if (MODE == SCAN_HIST) {
      // neighbouring entries mostly share a digit where the keys follow the positions: one LDS atomic for
      // the wave then, not 64 on one counter
#pragma unroll
      for (int j = 0; j < V; j++) {
        const bool act = hit[j] && q_in_bucket(b, key[j], pos[j]);
        const uint32_t dj = act ? q_digit(b, key[j], pos[j], digit) : 0u;
        const uint64_t m = __ballot(act);
        if (m) {
          const int first = __ffsll((unsigned long long)m) - 1;
          const uint32_t d0 = __shfl(dj, first, 64);
          if (__ballot(act && dj == d0) == m) {
            if (lane_id() == first) atomicAdd(&hist[d0], (uint32_t)__popcll(m));
          } else if (act) {
            atomicAdd(&hist[dj], 1u);
          }
        }
      }
    } else {
      uint32_t cnt = 0;
#pragma unroll
      for (int j = 0; j < V; j++) {
        if (MODE == SCAN_TAKE) hit[j] = hit[j] && q_at_or_below(b, key[j], pos[j]);
        if (MODE == SCAN_COUNT && hit[j]) {
          mn = min(mn, key[j]);
          mx = max(mx, key[j]);
        }
        cnt += hit[j] ? 1u : 0u;
      }
      if (full) {  // nothing more fits the list: the count alone, added once at the end
        tail += cnt;
      } else {
        u64 at = wave_reserve64(&ctl->count, cnt);
#pragma unroll
        for (int j = 0; j < V; j++)
          if (hit[j]) {
            if (at < cap) {
              ckey[at] = key[j];
              cpos[at] = pos[j];
            }
            at++;
          }
        full = __ballot(at >= cap) != 0;  // the counter only grows: every later entry would be dropped too
      }
    }
  }
  if (MODE != SCAN_HIST) {
    for (int o = 32; o; o >>= 1) tail += shfl64(tail, lane_id() ^ o);
    if (lane_id() == 0 && tail) atomicAdd(&ctl->count, tail);
  }
  if (MODE == SCAN_HIST) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < Q_BUCKETS; i += 256)
      if (hist[i]) atomicAdd(&ctl->hist[i], (u64)hist[i]);
  }
  if (MODE == SCAN_COUNT) {  // one atomic pair per wave that saw a match
    for (int o = 32; o; o >>= 1) {
      mn = min(mn, shfl64(mn, lane_id() ^ o));
      mx = max(mx, shfl64(mx, lane_id() ^ o));
    }
    if (lane_id() == 0 && mn <= mx) {
      atomicMin(&ctl->minkey, mn);
      atomicMax(&ctl->maxkey, mx);
    }
  }
}

// ------------------------------------------------------------------ decode
// The page: the first `take` sorted (key, position) pairs as kg_tuple records (k_rows_fill's decoding).
__global__ __launch_bounds__(256) void k_q_decode(DevSnap s, const u64* __restrict__ skey, const u64* __restrict__ spos,
                                                  uint32_t take, kg_tuple* __restrict__ rows, uint64_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= take) return;
  const u64 pos = spos[i];
  const uint32_t v = csr_owner(s.row_off, s.n_nodes, pos);
  const uint32_t x = s.row_subj[pos];
  kg_tuple t{s.nd_ns[v], s.nd_obj[v], s.nd_rel[v], KG_SUBJECT_ID, x, 0};
  if (x & SET_BIT) {
    const uint32_t c = x & ~SET_BIT;
    t.sns = s.nd_ns[c];
    t.sobj = s.nd_obj[c];
    t.srel = s.nd_rel[c];
  }
  rows[i] = t;
  keys[i] = skey[i];
}

// ------------------------------------------------------------------ host: a lane's buffers, one call
struct QueryBufs {
  PinBuf<void> h_req, h_res, h_rb, h_out;  // requests, resolved requests, control-block readback, one page
  DevBuf<void> d_req, d_res;
  DevBuf<QCtl> ctl;
  DevBuf<uint32_t> nodes;
  DevBuf<u64> len, pref;
  DevBuf<u64> ckey, cpos, ckey2, cpos2;
  DevBuf<kg_tuple> d_rows;
  DevBuf<uint64_t> d_keys;
  DevBuf<void> tmp;  // hipcub temporaries
  hipEvent_t ev[2] = {};
  ~QueryBufs() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

struct QCall {
  Snapshot* s;
  Workspace* w;
  hipStream_t st;
  QueryBufs& B;
  uint32_t grid_wide;
  uint64_t scanned = 0, passes = 0;

  QCall(Snapshot* s_, Lane* L)
      : s(s_), w(L->w), st(L->stream), B(*static_cast<QueryBufs*>(L->qr ? L->qr : (L->qr = new QueryBufs()))),
        grid_wide((uint32_t)s_->n_cu * 8) {}

  int reset_ctl() {
    HIPC(hipMemsetAsync(B.ctl.get(), 0, sizeof(QCtl), st));
    HIPC(hipMemsetAsync(&B.ctl.get()->minkey, 0xFF, 8, st));
    return 0;
  }
  // the control block without (head) or with the histogram
  int read_ctl(const QCtl** h, bool with_hist) {
    HIPC(hipMemcpyAsync(B.h_rb.get(), B.ctl.get(), with_hist ? sizeof(QCtl) : offsetof(QCtl, hist), hipMemcpyDeviceToHost,
                        st));
    if (int rc = w->wait(st, true)) return rc;
    *h = (const QCtl*)B.h_rb.get();
    return 0;
  }
  uint32_t grid_for(u64 total) const { return (uint32_t)std::max<u64>(1, std::min<u64>(grid_wide, (total + 255) / 256)); }

  template <int MODE>
  void scan(const QDom& d, const QSel& f, const QBound& b, uint32_t digit, u64 cap) {
    if (d.m)
      hipLaunchKernelGGL((k_q_scan<MODE, false>), dim3(grid_for(d.total)), dim3(256), 0, st, s->ds, d, f,
                         (const uint64_t*)s->d_row_key, b, digit, B.ckey.get(), B.cpos.get(), cap, B.ctl.get());
    else
      hipLaunchKernelGGL((k_q_scan<MODE, true>), dim3(grid_for(d.total / 4 + 1)), dim3(256), 0, st, s->ds, d, f,
                         (const uint64_t*)s->d_row_key, b, digit, B.ckey.get(), B.cpos.get(), cap, B.ctl.get());
    scanned += d.total;
    passes++;
  }

  // One request: its page in B.d_rows / B.d_keys (*take entries) and the count of its matches.
  int one(const kg_row_query& x, const QRes& r, uint32_t* take, uint64_t* matched);
  int node_stage(const kg_row_query& x, QDom* d);
  int narrow(const QDom& d, const QSel& f, u64 limit, u64 matched, u64 cap, u64 mn, u64 mx, QBound* out);
  int sort_pairs(size_t n, uint32_t key_bits, const u64** skey, const u64** spos);
};

// Some of (ns, obj, rel) set: the matching nodes and the prefix of their row lengths.
int QCall::node_stage(const kg_row_query& x, QDom* d) {
  const DevSnap& ds = s->ds;
  const uint32_t nn = ds.n_nodes;
  HIPC(B.nodes.reserve(nn));
  HIPC(B.len.reserve((size_t)nn + 1));
  HIPC(B.pref.reserve((size_t)nn + 1));
  if (int rc = reset_ctl()) return rc;
  hipLaunchKernelGGL(k_q_nodes, dim3(grid_for(nn)), dim3(256), 0, st, ds, x.mask, x.t.ns, x.t.obj, x.t.rel, B.nodes.get(),
                     B.ctl.get());
  HIPC(hipGetLastError());
  const QCtl* h;
  if (int rc = read_ctl(&h, false)) return rc;
  const uint32_t m = (uint32_t)std::min<u64>(h->nsel, nn);
  d->m = m;
  d->total = 0;
  if (!m) return 0;
  hipLaunchKernelGGL(k_q_node_len, dim3(m / 256 + 1), dim3(256), 0, st, ds, (const uint32_t*)B.nodes.get(), m, B.len.get());
  size_t bytes = 0;
  HIPC(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, B.len.get(), B.pref.get(), (size_t)m + 1, st));
  HIPC(B.tmp.reserve(bytes + 16));
  HIPC(hipcub::DeviceScan::ExclusiveSum(B.tmp.get(), bytes, B.len.get(), B.pref.get(), (size_t)m + 1, st));
  HIPC(hipMemcpyAsync(B.h_rb.get(), B.pref.get() + m, 8, hipMemcpyDeviceToHost, st));
  if (int rc = w->wait(st, true)) return rc;
  d->total = *(const u64*)B.h_rb.get();
  d->nodes = B.nodes.get();
  d->pref = B.pref.get();
  return 0;
}

// More matches than the list holds: the prefix of (key, position) at or below which the page lies and whose
// matches fit the list.
int QCall::narrow(const QDom& d, const QSel& f, u64 limit, u64 matched, u64 cap, u64 mn, u64 mx, QBound* out) {
  QBound b{0, 0, 0, 0};
  if (mn == mx) {
    b.kbits = 64;
    b.key = mn;
  } else {
    b.kbits = (uint32_t)__builtin_clzll(mn ^ mx);  // the bits every matching key shares
    b.key = b.kbits ? mn >> (64 - b.kbits) : 0;
  }
  uint32_t pos_bits = 1;  // bits a position takes
  while (pos_bits < 64 && (s->h_row_off_last >> pos_bits)) pos_bits++;
  u64 below = 0, inside = matched;  // matches below the prefix / inside it
  while (below + inside > cap) {
    if (b.kbits == 64 && !b.pbits) b.pbits = 64 - pos_bits;  // the bits no position has set
    if (b.kbits == 64 && b.pbits == 64) return set_error(-1, "query: the selection did not converge");
    const uint32_t digit = std::min(Q_DIGIT, b.kbits < 64 ? 64 - b.kbits : 64 - b.pbits);
    HIPC(hipMemsetAsync(B.ctl.get()->hist, 0, sizeof(u64) * Q_BUCKETS, st));
    scan<SCAN_HIST>(d, f, b, digit, 0);
    HIPC(hipGetLastError());
    const QCtl* h;
    if (int rc = read_ctl(&h, true)) return rc;
    uint32_t pick = 0;
    u64 run = below;
    for (;; pick++) {  // the bucket in which the running count reaches limit
      if (pick == (1u << digit)) return set_error(-1, "query: a narrowing pass lost matches");
      if (run + h->hist[pick] >= limit) break;
      run += h->hist[pick];
    }
    below = run;
    inside = h->hist[pick];
    if (b.kbits < 64) {
      b.key = (b.key << digit) | pick;
      b.kbits += digit;
    } else {
      b.pos = (b.pos << digit) | pick;
      b.pbits += digit;
    }
  }
  *out = b;
  return 0;
}

// The list's first n pairs by (key, position): a stable sort by key after one by position (which keys
// position + 1 make redundant).
int QCall::sort_pairs(size_t n, uint32_t key_bits, const u64** skey, const u64** spos) {
  HIPC(B.ckey2.reserve(B.ckey.cap()));
  HIPC(B.cpos2.reserve(B.cpos.cap()));
  hipcub::DoubleBuffer<u64> kb(B.ckey.get(), B.ckey2.get()), pb(B.cpos.get(), B.cpos2.get());
  if (n > 1) {
    int pos_bits = 1;
    while (pos_bits < 64 && (s->h_row_off_last >> pos_bits)) pos_bits++;
    size_t bytes = 0;
    HIPC(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, pb, kb, n, 0, 64, st));
    HIPC(B.tmp.reserve(bytes + 16));
    if (s->d_row_key) HIPC(hipcub::DeviceRadixSort::SortPairs(B.tmp.get(), bytes, pb, kb, n, 0, pos_bits, st));
    if (key_bits) HIPC(hipcub::DeviceRadixSort::SortPairs(B.tmp.get(), bytes, kb, pb, n, 0, (int)key_bits, st));
  }
  *skey = kb.Current();
  *spos = pb.Current();
  return 0;
}

int QCall::one(const kg_row_query& x, const QRes& r, uint32_t* take, uint64_t* matched) {
  *take = 0;
  *matched = 0;
  const u64 total = s->h_row_off_last;
  if (r.smode == QS_NONE || !total) return 0;
  QDom d{0, 0, nullptr, nullptr, 0};
  if ((x.mask & 7u) == 7u) {
    if (r.node == NONE) return 0;
    d.lo = r.lo;
    d.total = r.hi - r.lo;
  } else if (!(x.mask & 7u)) {
    d.lo = s->d_row_key ? 0 : std::min<u64>(x.after, total);  // key = position + 1
    d.total = total - d.lo;
  } else if (int rc = node_stage(x, &d)) {
    return rc;
  }
  if (!d.total) return 0;
  if (d.lo + d.total > total && !d.m) return set_error(-1, "query: a row range past the rows");
  const QSel f{r.smode, r.subj, x.after};
  const u64 cap = std::max<u64>(s->knobs.query_cap ? s->knobs.query_cap : (1ull << 20), std::min<u64>(x.limit, d.total));
  HIPC(B.ckey.reserve((size_t)cap));
  HIPC(B.cpos.reserve((size_t)cap));
  if (int rc = reset_ctl()) return rc;
  scan<SCAN_COUNT>(d, f, QBound{0, 0, 0, 0}, 0, cap);
  HIPC(hipGetLastError());
  const QCtl* h;
  if (int rc = read_ctl(&h, false)) return rc;
  const u64 m = h->count, mn = h->minkey, mx = h->maxkey;
  *matched = m;
  if (!m) return 0;
  u64 n = m;
  if (m > cap) {
    QBound b;
    if (int rc = narrow(d, f, x.limit, m, cap, mn, mx, &b)) return rc;
    HIPC(hipMemsetAsync(&B.ctl.get()->count, 0, 8, st));
    scan<SCAN_TAKE>(d, f, b, 0, cap);
    HIPC(hipGetLastError());
    if (int rc = read_ctl(&h, false)) return rc;
    n = h->count;
    if (n > cap || n < std::min<u64>(x.limit, m)) return set_error(-1, "query: the selection kept %llu of %llu", n, m);
  }
  const u64 *skey, *spos;
  if (int rc = sort_pairs((size_t)n, mn == mx ? 0u : 64u - (uint32_t)__builtin_clzll(mn ^ mx), &skey, &spos)) return rc;
  const uint32_t k = (uint32_t)std::min<u64>(x.limit, n);
  HIPC(B.d_rows.reserve(k));
  HIPC(B.d_keys.reserve(k));
  hipLaunchKernelGGL(k_q_decode, dim3((k + 255) / 256), dim3(256), 0, st, s->ds, skey, spos, k, B.d_rows.get(),
                     B.d_keys.get());
  HIPC(hipGetLastError());
  *take = k;
  return 0;
}

}  // namespace

void query_bufs_free(void* p) { delete static_cast<QueryBufs*>(p); }

// kg_snapshot_query on lane L (its stream and workspace; the caller holds the workspace's mutex).  The
// requests run one after another on the lane's stream.
int query_rows(Snapshot* s, Lane* L, const kg_row_query* reqs, size_t n, kg_query_buf* out) {
  if (n > 0x7FFFFFFFull) return set_error(-2, "batch too large");
  for (size_t i = 0; i < n; i++)
    if (!reqs[i].limit) return set_error(-2, "kg_snapshot_query: request %zu has limit 0", i);
  QCall c(s, L);
  QueryBufs& B = c.B;
  hipStream_t st = c.st;
  HIPC(hipSetDevice(s->device));
  HIPC(B.h_req.reserve(n * sizeof(kg_row_query)));
  HIPC(B.d_req.reserve(n * sizeof(kg_row_query)));
  HIPC(B.h_res.reserve(n * sizeof(QRes)));
  HIPC(B.d_res.reserve(n * sizeof(QRes)));
  HIPC(B.h_rb.reserve(sizeof(QCtl)));
  HIPC(B.ctl.reserve(1));
  if (!B.ev[0])
    for (auto& e : B.ev) HIPC(hipEventCreate(&e));
  memcpy(B.h_req.get(), reqs, n * sizeof(kg_row_query));
  HIPC(hipEventRecord(B.ev[0], st));
  HIPC(hipMemcpyAsync(B.d_req.get(), B.h_req.get(), n * sizeof(kg_row_query), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_q_resolve, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, s->ds,
                     (const kg_row_query*)B.d_req.get(), (uint32_t)n, (const uint64_t*)s->d_row_key, (QRes*)B.d_res.get());
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(B.h_res.get(), B.d_res.get(), n * sizeof(QRes), hipMemcpyDeviceToHost, st));
  if (int rc = c.w->wait(st, true)) return rc;
  const QRes* res = (const QRes*)B.h_res.get();

  std::vector<kg_tuple> rows;
  std::vector<uint64_t> keys, off(n + 1, 0), next(n, 0), matched(n, 0);
  for (size_t i = 0; i < n; i++) {
    uint32_t take = 0;
    if (int rc = c.one(reqs[i], res[i], &take, &matched[i])) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
    if (take) {  // the page through pinned staging
      const size_t rb = (size_t)take * sizeof(kg_tuple);
      HIPC(B.h_out.reserve(rb + (size_t)take * 8));
      char* ho = (char*)B.h_out.get();
      HIPC(hipMemcpyAsync(ho, B.d_rows.get(), rb, hipMemcpyDeviceToHost, st));
      HIPC(hipMemcpyAsync(ho + rb, B.d_keys.get(), (size_t)take * 8, hipMemcpyDeviceToHost, st));
      if (int rc = c.w->wait(st, true)) return rc;
      rows.insert(rows.end(), (const kg_tuple*)ho, (const kg_tuple*)ho + take);
      keys.insert(keys.end(), (const uint64_t*)(ho + rb), (const uint64_t*)(ho + rb) + take);
      if (matched[i] > take) next[i] = keys.back();
    }
    off[i + 1] = rows.size();
  }
  HIPC(hipEventRecord(B.ev[1], st));
  if (int rc = c.w->wait(st, true)) return rc;
  float ms = 0;
  if (hipEventElapsedTime(&ms, B.ev[0], B.ev[1]) != hipSuccess) {
    (void)hipGetLastError();
    ms = 0;
  }
  // one pinned block: req_off[n + 1] | next[n] | matched[n] | keys[m] | rows[m]
  const size_t m = rows.size();
  const size_t bytes = (n + 1) * 8 + n * 8 + n * 8 + m * 8 + m * sizeof(kg_tuple);
  char* blk = (char*)tree_pool_get(bytes);
  if (!blk) return set_error(KG_ERR_RESOURCE_CODE, "query: pinned output allocation failed");
  out->req_off = (uint64_t*)blk;
  out->next = out->req_off + n + 1;
  out->matched = out->next + n;
  out->keys = out->matched + n;
  out->rows = (kg_tuple*)(out->keys + m);
  memcpy(out->req_off, off.data(), (n + 1) * 8);
  memcpy(out->next, next.data(), n * 8);
  memcpy(out->matched, matched.data(), n * 8);
  if (m) {
    memcpy(out->keys, keys.data(), m * 8);
    memcpy(out->rows, rows.data(), m * sizeof(kg_tuple));
  }
  out->n_reqs = n;
  out->n_rows = m;
  out->rows_scanned = c.scanned;
  out->passes = c.passes;
  out->kernel_ms = ms;
  out->pinned = bytes;
  return 0;
}

void query_free(kg_query_buf* out) {
  if (out->pinned) tree_pool_put(out->req_off, (size_t)out->pinned);
  else free(out->req_off);
  memset(out, 0, sizeof *out);
}

}  // namespace kg
