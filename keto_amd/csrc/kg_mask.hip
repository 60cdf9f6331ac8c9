// kg_mask.hip -- ranked select through an access mask (kg_mask_select_device): every row of ranked candidate
// ids is filtered by its row of a bitmap over object ids -- what kg_lookup_objects_mask_device or
// kg_lookup_subject_sets_mask_device wrote, or any bitmap of that layout -- and the first `limit` allowed ids
// are kept in rank order.  The consumer is a search or a feed whose candidates are already in HBM: the top-K
// of a vector search goes in, the ids the subject may see come out, nothing crosses the bus.
#include <hip/hip_runtime.h>

#include "kg_bfs.h"
#include "kg_internal.h"
#include "kg_snapshot.h"

namespace kg {
namespace {

// One wave per row, four rows per workgroup.  The wave takes the row 64 candidates at a time: a ballot of
// "allowed", and a lane's place in the output is the allowed count of the chunks before plus that of the
// lanes below it, so the order is the candidates' and no atomic or LDS is needed.  An id is allowed when it
// lies in [base, base + n_bits) and its bit is set; base + n_bits <= 0xFFFFFFFF (checked by the caller) keeps
// KG_LOOKUP_END out.  Lanes past k_in carry no candidate.
__global__ __launch_bounds__(256) void k_mask_select(const uint32_t* __restrict__ mask, size_t row_words, uint32_t base,
                                                     uint32_t n_bits, const uint32_t* __restrict__ cand, size_t n,
                                                     uint32_t k_in, uint32_t limit, uint32_t* __restrict__ out,
                                                     uint32_t* __restrict__ count) {
  const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;  // the whole wave
  const uint32_t* row = mask + r * row_words;
  const uint32_t* c = cand + r * k_in;
  uint32_t* o = out + r * limit;
  uint32_t have = 0;  // allowed so far: the same in every lane
  for (uint64_t at = 0; at < k_in; at += 64) {
    const uint64_t i = at + lane_id();
    uint32_t id = 0;
    bool ok = false;
    if (i < k_in) {
      id = c[i];
      const uint32_t d = id - base;
      ok = id >= base && d < n_bits && ((row[d >> 5] >> (d & 31)) & 1u);  // d >> 5 < ceil(n_bits / 32) <= row_words
    }
    const uint64_t m = __ballot(ok);
    const uint32_t pos = have + lanes_below(m);
    if (ok && pos < limit) o[pos] = id;
    have += (uint32_t)__popcll(m);
  }
  for (uint64_t i = (uint64_t)min(have, limit) + lane_id(); i < limit; i += 64) o[i] = KG_LOOKUP_END;
  if (lane_id() == 0) count[r] = have;
}

}  // namespace

int mask_select(Snapshot* s, const uint32_t* d_mask, size_t row_words, uint32_t base, uint32_t n_bits,
                const uint32_t* d_cand, size_t n, uint32_t k_in, uint32_t limit, uint32_t* d_out, uint32_t* d_count,
                hipStream_t st) {
  HIPC(hipSetDevice(s->device));
  hipLaunchKernelGGL(k_mask_select, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, st ? st : s->stream, d_mask, row_words,
                     base, n_bits, d_cand, n, k_in, limit, d_out, d_count);
  HIPC(hipGetLastError());
  return 0;
}

}  // namespace kg
