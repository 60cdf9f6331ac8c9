// kg_delete.hip -- kg_snapshot_delete_matching: the reference's delete-by-query
// (relationtuple.Manager.DeleteAllRelationTuples, internal/persistence/sql/relationtuples.go:187-201: one
// DELETE ... WHERE over the RelationQuery's conditions, :146-162 and whereSubject :124-145) on the device
// snapshot.  The SQL persister never learns which rows went, so there is no tuple delta to hand to
// kg_snapshot_apply; here the query itself goes to where the rows live:
//   resolve     one wave maps the <= 64 queries: the (ns, obj, rel) fields each names, a subject mode
//               (any / equal / none, k_q_resolve's rules: a subject set goes through the node map, an
//               unknown one matches nothing) and a tagged subject
//   node stage  one lane per node: nm[v] = the word of the queries whose named fields equal the node's
//               triple.  Skipped when no query names a node field (every bit would be set)
//   row stage   one lane per four consecutive row entries (one 16-byte load of their subjects): an entry's
//               hit word = nm[owner] & the word of the queries whose subject test it passes;
//               keep = (hit == 0).  The owner is searched once per lane and walked forward, and not at all
//               without a node stage.  Per-query counts: ballot popcounts kept per wave in LDS, one atomic
//               per wave and matched query at the end
//   compaction  kr = exclusive scan of keep; new_off[v] = kr[row_off[v]]; one scatter of the kept subjects
//               (and keys) to kr[i].  The deleted entries' keys, when asked for, go to i - kr[i] and -- on a
//               keyed base, where they follow the nodes, not the keys -- through a radix sort
//   the rest    Snapshot::derive_from_rows (kg_delta.hip): what every refresh rebuilds
// Raw rows only (row_off / row_subj), as kg_query.hip.  Node ids, the order of the kept rows and their
// keys do not change.  Temporaries: 4 B + 8 B per row entry (keep, kr), 8 B per node with a node stage.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "kg_bfs.h"
#include "kg_internal.h"
#include "kg_snapshot.h"

namespace kg {
namespace {

typedef unsigned long long u64;

constexpr uint32_t DQ = KG_DELETE_MAX_QUERIES;
static_assert(DQ == 64, "one bit per query in a 64-bit hit word, one lane per query in k_del_resolve");
enum : uint32_t { DS_ANY = 0, DS_EQ = 1, DS_NONE = 2 };

// The resolved queries, as the kernels stage them in LDS.
struct DelQ {
  u64 any_w;       // the queries whose subject test every entry passes
  uint32_t n, n_eq;
  uint32_t mask[DQ], ns[DQ], obj[DQ], rel[DQ];  // KG_Q_NS | KG_Q_OBJ | KG_Q_REL bits and those fields
  uint32_t eq_subj[DQ], eq_bit[DQ];             // the n_eq queries that ask for one tagged subject: it, their index
};

// ------------------------------------------------------------------ resolve (one wave)
__global__ __launch_bounds__(64) void k_del_resolve(DevSnap s, const kg_row_query* __restrict__ q, uint32_t n,
                                                    DelQ* __restrict__ out) {
  const uint32_t i = threadIdx.x;
  uint32_t smode = DS_NONE, subj = 0;
  if (i < n) {
    const kg_row_query x = q[i];
    smode = DS_ANY;
    if (x.mask & KG_Q_SUBJECT) {
      if (x.t.sns == KG_SUBJECT_ID) {
        smode = x.t.sobj & SET_BIT ? DS_NONE : DS_EQ;  // an untagged entry is an id below 2^31
        subj = x.t.sobj;
      } else {
        const uint32_t sn = s.n_nodes ? nmap_find(s, x.t.sns, x.t.srel, x.t.sobj) : NONE;
        smode = sn < s.n_nodes ? DS_EQ : DS_NONE;
        subj = SET_BIT | sn;
      }
    }
    out->mask[i] = x.mask & 7u;
    out->ns[i] = x.t.ns;
    out->obj[i] = x.t.obj;
    out->rel[i] = x.t.rel;
  }
  const u64 anyb = __ballot(smode == DS_ANY), eqb = __ballot(smode == DS_EQ);
  if (smode == DS_EQ) {
    const uint32_t k = (uint32_t)__popcll(eqb & ((1ull << i) - 1));
    out->eq_subj[k] = subj;
    out->eq_bit[k] = i;
  }
  if (i == 0) {
    out->any_w = anyb;
    out->n = n;
    out->n_eq = (uint32_t)__popcll(eqb);
  }
}

// ------------------------------------------------------------------ node stage
__global__ __launch_bounds__(256) void k_del_nodes(DevSnap s, const DelQ* __restrict__ dq, u64* __restrict__ nm) {
  __shared__ uint32_t qm[DQ], qn[DQ], qo[DQ], qr[DQ];
  const uint32_t n = dq->n;
  if (threadIdx.x < n) {
    qm[threadIdx.x] = dq->mask[threadIdx.x];
    qn[threadIdx.x] = dq->ns[threadIdx.x];
    qo[threadIdx.x] = dq->obj[threadIdx.x];
    qr[threadIdx.x] = dq->rel[threadIdx.x];
  }
  __syncthreads();
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 v = (u64)blockIdx.x * 256 + threadIdx.x; v < s.n_nodes; v += stride) {
    const uint32_t a = s.nd_ns[v], b = s.nd_obj[v], c = s.nd_rel[v];
    u64 w = 0;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t m = qm[i];
      const bool ok = (!(m & KG_Q_NS) || a == qn[i]) && (!(m & KG_Q_OBJ) || b == qo[i]) && (!(m & KG_Q_REL) || c == qr[i]);
      w |= (u64)ok << i;
    }
    nm[v] = w;
  }
}

// ------------------------------------------------------------------ row stage
// Item i is the entries 4i .. 4i+3 (row_subj is 16-byte aligned; the last item may be short).  OWNER: a node
// stage ran and nm[] holds its words; else every query passes every node.
template <bool OWNER>
__global__ __launch_bounds__(256) void k_del_rows(DevSnap s, u64 total, const DelQ* __restrict__ dq,
                                                  const u64* __restrict__ nm, uint32_t* __restrict__ keep,
                                                  u64* __restrict__ matched) {
  __shared__ uint32_t es[DQ], eb[DQ];
  __shared__ u64 cnt[4][DQ];  // per wave and query: entries hit (written by the wave's lane 0 only)
  const uint32_t n_eq = dq->n_eq;
  const u64 any_w = dq->any_w;
  if (threadIdx.x < n_eq) {
    es[threadIdx.x] = dq->eq_subj[threadIdx.x];
    eb[threadIdx.x] = dq->eq_bit[threadIdx.x];
  }
  cnt[threadIdx.x >> 6][threadIdx.x & 63] = 0;
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6;
  const u64 items = (total + 3) / 4, stride = (u64)gridDim.x * 256;
  for (u64 base = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); base < items; base += stride) {  // wave-uniform
    const u64 it = base + lane_id();
    u64 h[4] = {0, 0, 0, 0};
    if (it < items) {
      const u64 p0 = 4 * it;
      const bool whole = p0 + 3 < total;
      uint32_t sv[4] = {0, 0, 0, 0};
      if (n_eq) {
        if (whole) {
          const uint4 x = *reinterpret_cast<const uint4*>(s.row_subj + p0);
          sv[0] = x.x, sv[1] = x.y, sv[2] = x.z, sv[3] = x.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (p0 + j < total) sv[j] = s.row_subj[p0 + j];
        }
      }
      uint32_t v = OWNER ? csr_owner(s.row_off, s.n_nodes, p0) : 0u;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (p0 + j >= total) break;
        u64 w = any_w;
        for (uint32_t k = 0; k < n_eq; k++) w |= (u64)(sv[j] == es[k]) << eb[k];
        if (OWNER) {
          if (j) v = csr_advance(s.row_off, s.n_nodes, v, p0 + j);
          w &= nm[v];
        }
        h[j] = w;
      }
      if (whole) {
        *reinterpret_cast<uint4*>(keep + p0) = make_uint4(h[0] ? 0u : 1u, h[1] ? 0u : 1u, h[2] ? 0u : 1u, h[3] ? 0u : 1u);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (p0 + j < total) keep[p0 + j] = h[j] ? 0u : 1u;
      }
    }
    u64 wor = h[0] | h[1] | h[2] | h[3];
    if (__ballot(wor != 0)) {  // the queries some lane of the wave hit: a ballot popcount each
      for (int o = 32; o; o >>= 1) wor |= shfl64(wor, lane_id() ^ o);
      while (wor) {
        const int b = __ffsll(wor) - 1;
        wor &= wor - 1;
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) c += (uint32_t)__popcll(__ballot((h[j] >> b) & 1));
        if (lane_id() == 0) cnt[wave][b] += c;
      }
    }
  }
  __syncthreads();
  const u64 c = cnt[wave][lane_id()];  // one atomic per wave and matched query
  if (c) atomicAdd(&matched[lane_id()], c);
}

// ------------------------------------------------------------------ compaction
__global__ __launch_bounds__(256) void k_del_newoff(const uint64_t* __restrict__ row_off, uint32_t n,
                                                    const uint64_t* __restrict__ kr, uint64_t* __restrict__ new_off) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 v = (u64)blockIdx.x * 256 + threadIdx.x; v <= n; v += stride) new_off[v] = kr[row_off[v]];
}
__global__ __launch_bounds__(256) void k_del_scatter(const uint32_t* __restrict__ row_subj,
                                                     const uint64_t* __restrict__ row_key, u64 total,
                                                     const uint32_t* __restrict__ keep, const uint64_t* __restrict__ kr,
                                                     uint32_t* __restrict__ new_subj, uint64_t* __restrict__ new_key) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    if (!keep[i]) continue;
    const u64 at = kr[i];
    new_subj[at] = row_subj[i];
    if (new_key) new_key[at] = row_key[i];
  }
}
// The deleted entries' order keys (position + 1 without keys), in position order.
__global__ __launch_bounds__(256) void k_del_keys(const uint64_t* __restrict__ row_key, u64 total,
                                                  const uint32_t* __restrict__ keep, const uint64_t* __restrict__ kr,
                                                  uint64_t* __restrict__ out) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride)
    if (!keep[i]) out[i - kr[i]] = row_key ? row_key[i] : i + 1;
}

struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  int init() {
    HIPC(hipEventCreate(&a));
    HIPC(hipEventCreate(&b));
    return 0;
  }
  double ms() const {
    float t = 0;
    if (hipEventElapsedTime(&t, a, b) != hipSuccess) {
      (void)hipGetLastError();
      t = 0;
    }
    return t;
  }
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

// streaming passes: a grid-stride loop over two workgroups per CU (one for the per-node passes)
uint32_t del_grid(const Snapshot* s, u64 items, uint32_t per_cu) {
  return (uint32_t)std::max<u64>(1, std::min<u64>((u64)s->n_cu * per_cu, (items + 255) / 256));
}

}  // namespace

int delete_match(Snapshot* base, hipStream_t st, const kg_row_query* q, size_t n, bool want_keys, DeleteMatch* m) {
  const DevSnap& ds = base->ds;
  const u64 total = base->h_row_off_last;
  m->total = m->kept = total;
  m->matched.assign(n, 0);
  if (!n || !total || !ds.n_nodes) return 0;
  uint32_t fields = 0;  // the node fields some query names
  for (size_t i = 0; i < n; i++) fields |= q[i].mask & 7u;
  EventPair ev;
  if (int rc = ev.init()) return rc;
  DevTemps& tmp = m->tmp;
  kg_row_query* d_q;
  DelQ* d_dq;
  u64 *d_matched, *d_nm = nullptr;
  if (tmp.alloc((void**)&d_q, n * sizeof(kg_row_query)) || tmp.alloc((void**)&d_dq, sizeof(DelQ)) ||
      tmp.alloc((void**)&d_matched, DQ * 8) || tmp.alloc((void**)&m->keep, (total + 1) * 4 + 16) ||
      tmp.alloc((void**)&m->kr, (total + 1) * 8))
    return -1;
  if (fields && tmp.alloc((void**)&d_nm, (size_t)ds.n_nodes * 8)) return -1;
  size_t tb = 0;
  void* scratch;
  HIPC(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, m->keep, m->kr, (size_t)total + 1, st));
  if (tmp.alloc(&scratch, tb + 16)) return -1;
  HIPC(hipMemcpyAsync(d_q, q, n * sizeof(kg_row_query), hipMemcpyHostToDevice, st));
  HIPC(hipEventRecord(ev.a, st));
  HIPC(hipMemsetAsync(d_matched, 0, DQ * 8, st));
  HIPC(hipMemsetAsync(m->keep + total, 0, 4, st));
  hipLaunchKernelGGL(k_del_resolve, dim3(1), dim3(64), 0, st, ds, (const kg_row_query*)d_q, (uint32_t)n, d_dq);
  if (fields)
    hipLaunchKernelGGL(k_del_nodes, dim3(del_grid(base, ds.n_nodes, 1)), dim3(256), 0, st, ds, (const DelQ*)d_dq, d_nm);
  const uint32_t g_rows = del_grid(base, (total + 3) / 4, 2);
  if (fields)
    hipLaunchKernelGGL((k_del_rows<true>), dim3(g_rows), dim3(256), 0, st, ds, total, (const DelQ*)d_dq, (const u64*)d_nm,
                       m->keep, d_matched);
  else
    hipLaunchKernelGGL((k_del_rows<false>), dim3(g_rows), dim3(256), 0, st, ds, total, (const DelQ*)d_dq,
                       (const u64*)nullptr, m->keep, d_matched);
  HIPC(hipGetLastError());
  HIPC(hipcub::DeviceScan::ExclusiveSum(scratch, tb, m->keep, m->kr, (size_t)total + 1, st));
  HIPC(hipEventRecord(ev.b, st));
  u64 h_matched[DQ];
  HIPC(hipMemcpyAsync(h_matched, d_matched, DQ * 8, hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(&m->kept, m->kr + total, 8, hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  m->ms = ev.ms();
  if (m->kept > total) return set_error(-1, "delete: the scan kept %llu of %llu entries", (u64)m->kept, total);
  for (size_t i = 0; i < n; i++) m->matched[i] = h_matched[i];
  const u64 gone = total - m->kept;
  if (!want_keys || !gone) return 0;
  // the deleted entries' keys: position order is key order only without keys
  uint64_t *dk, *dk2 = nullptr;
  if (tmp.alloc((void**)&dk, gone * 8)) return -1;
  hipcub::DoubleBuffer<uint64_t> kb(dk, dk);
  size_t sb = 0;
  void* sscratch = nullptr;
  if (base->d_row_key && gone > 1) {
    if (tmp.alloc((void**)&dk2, gone * 8)) return -1;
    kb = hipcub::DoubleBuffer<uint64_t>(dk, dk2);
    HIPC(hipcub::DeviceRadixSort::SortKeys(nullptr, sb, kb, (size_t)gone, 0, 64, st));
    if (tmp.alloc(&sscratch, sb + 16)) return -1;
  }
  HIPC(hipEventRecord(ev.a, st));
  hipLaunchKernelGGL(k_del_keys, dim3(del_grid(base, total, 2)), dim3(256), 0, st, (const uint64_t*)base->d_row_key, total,
                     (const uint32_t*)m->keep, (const uint64_t*)m->kr, dk);
  HIPC(hipGetLastError());
  if (dk2) HIPC(hipcub::DeviceRadixSort::SortKeys(sscratch, sb, kb, (size_t)gone, 0, 64, st));
  HIPC(hipEventRecord(ev.b, st));
  HIPC(hipStreamSynchronize(st));
  m->ms += ev.ms();
  m->d_keys = kb.Current();
  return 0;
}

int Snapshot::create_from_delete(Snapshot* base, const kg_row_query* q, size_t n, DeleteMatch* pre, const kg_dict* dict,
                                 const kg_rewrite_prog* prog) {
  if (base->shard_n > 1) return set_error(-2, "kg_snapshot_apply: sharded snapshots rebuild instead");
  if (base->device != device) return set_error(-2, "kg_snapshot_delete_matching: replica on another device");
  const uint32_t n0 = base->ds.n_nodes;
  wildcard_rel = dict ? dict->wildcard_rel : base->wildcard_rel;
  ds.wildcard_rel = wildcard_rel;
  ds.n_nodes = n0;
  // the node map: handed on as kg_snapshot_apply does (no node is added or dropped); a base without one
  // leaves the next apply to rebuild it from the device triples
  {
    std::lock_guard<std::mutex> base_lk(base->mu);
    if (!base->hmap.k.empty() && base->h_nd_ns.size() == n0) {
      hmap = std::move(base->hmap);
      h_nd_ns = std::move(base->h_nd_ns);
      h_nd_obj = std::move(base->h_nd_obj);
      h_nd_rel = std::move(base->h_nd_rel);
      base->hmap = HostMap{};
    }
  }
  DeleteMatch own;
  DeleteMatch* m = pre;
  if (!m) {
    m = &own;
    if (int rc = delete_match(base, stream, q, n, false, m)) return rc;
  }
  const uint64_t total = m->total, kept = m->kept;
  EventPair ev;
  if (int rc = ev.init()) return rc;
  uint32_t *d_ns, *d_obj, *d_rel, *d_rs;
  uint64_t* d_ro;
  if (alloc((void**)&d_ns, (size_t)n0 * 4) || alloc((void**)&d_obj, (size_t)n0 * 4) || alloc((void**)&d_rel, (size_t)n0 * 4) ||
      alloc((void**)&d_ro, ((size_t)n0 + 1) * 8) || alloc((void**)&d_rs, kept * 4 + 4))
    return -1;
  const bool keyed = base->d_row_key != nullptr;
  if (keyed && alloc((void**)&d_row_key, kept * 8 + 8)) return -1;
  if (n0) {
    HIPC(hipMemcpyAsync(d_ns, base->ds.nd_ns, (size_t)n0 * 4, hipMemcpyDeviceToDevice, stream));
    HIPC(hipMemcpyAsync(d_obj, base->ds.nd_obj, (size_t)n0 * 4, hipMemcpyDeviceToDevice, stream));
    HIPC(hipMemcpyAsync(d_rel, base->ds.nd_rel, (size_t)n0 * 4, hipMemcpyDeviceToDevice, stream));
  }
  HIPC(hipEventRecord(ev.a, stream));
  if (m->kr) {
    hipLaunchKernelGGL(k_del_newoff, dim3(del_grid(this, (u64)n0 + 1, 1)), dim3(256), 0, stream, base->ds.row_off, n0,
                       (const uint64_t*)m->kr, d_ro);
    hipLaunchKernelGGL(k_del_scatter, dim3(del_grid(this, total, 2)), dim3(256), 0, stream, base->ds.row_subj,
                       (const uint64_t*)base->d_row_key, total, (const uint32_t*)m->keep, (const uint64_t*)m->kr, d_rs,
                       d_row_key);
    HIPC(hipGetLastError());
  } else {  // a base without rows: nothing was matched, every offset is 0
    HIPC(hipMemsetAsync(d_ro, 0, ((size_t)n0 + 1) * 8, stream));
  }
  HIPC(hipEventRecord(ev.b, stream));
  HIPC(hipStreamSynchronize(stream));
  m->ms += ev.ms();
  m->tmp.bufs.clear();  // keep, kr and the keys' sort buffers: the rest needs the memory
  m->keep = nullptr;
  m->kr = nullptr;
  return derive_from_rows(d_ro, d_rs, d_ns, d_obj, d_rel, kept, dict, prog);
}

}  // namespace kg
