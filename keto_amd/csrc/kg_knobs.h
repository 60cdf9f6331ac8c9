// kg_knobs.h -- the engine knobs of kg_snapshot_tune: one table of key, field, type, default and range.
// struct Knobs and knob_set's rows are generated from it, kg_abi.cpp's tune_one calls knob_set, and
// include/ketogpu.h describes the keys to callers.  No HIP here: a host compiler builds this header alone
// (tests/test_knobs_host.py).
#pragma once
#include <cstdint>
#include <cstring>

namespace kg {

enum KnobKind {
  KNOB_RANGE,  // lo <= value <= hi
  KNOB_POW2,   // a power of two in [lo, hi]
};

// X(key, field, type, default, lo, hi, kind): kg_snapshot_tune(key) stores (type)value in Knobs::field.
// "grid_reserve" is not here: it is an action of tune_one and stores nothing.
#define KG_KNOBS(X)                                                                                                    \
  /* ---- check tiers */                                                                                               \
  /* stream-tier edge budget per query (0 = none) */                                                                   \
  X(stream_ecap, stream_ecap, uint32_t, 512, 0, 0xFFFFFFFFll, KNOB_RANGE)                                              \
  /* XCD ranges a k_stream4 wave dequeues from */                                                                      \
  X(stream_steal, stream_steal, uint32_t, 4, 1, 8, KNOB_RANGE)                                                         \
  /* Occupancy defaults (library-wide, measured with several batches in flight, the way a server keeps them: C2 and  \
     C3 A/Bs in profiles/r2gw_tier_wgs_sweep.jsonl, r2v_occupancy_sweep.jsonl, r2bw_back_wgs_ab.jsonl; a              \
     one-batch-at-a-time caller loses < 5 % with them).  C2 (round 4, profiles/r4w_grid_stream_wgs_ab.jsonl):         \
     k_grid_level 2 and k_stream4 2 workgroups per CU (the LDS a third stream workgroup held now serves the other     \
     batches' tail tiers): 7.00 -> 7.20 x 10^9; C3 keeps 4 / 3 through bench.py */                                     \
  /* k_grid_level workgroups per CU */                                                                                 \
  X(grid_wgs, grid_wgs, int, 2, 1, 64, KNOB_RANGE)                                                                     \
  /* k_stream4 workgroups per CU (0 = 2; LDS left to other batches) */                                                 \
  X(stream_wgs, stream_wgs, int, 2, 0, 8, KNOB_RANGE)                                                                  \
  /* k_back workgroups per CU (LDS allows 3; C3 prefers 1).  3: one wave per query for up to 3 Ki hand-ons (C2 hands  \
     on ~2.2 k per 1 M batch: at 2, ~170 of them waited for a second pass on a freed wave; 6.3 -> 6.8 x 10^9          \
     checks/s, profiles/r4s_back_wgs_ab.jsonl) */                                                                      \
  X(back_wgs, back_wgs, int, 3, 1, 3, KNOB_RANGE)                                                                      \
  /* k_back<64>'s reverse-edge budget per query (0 = 2^12) */                                                          \
  X(back_edges, back_edges, uint32_t, 0, 0, 1 << 20, KNOB_RANGE)                                                       \
  /* k_resolve prunes by the holder signatures (0: the bitmap only; tests, A/B) */                                     \
  X(holder_sig, holder_sig, int, 1, 0, 1, KNOB_RANGE)                                                                  \
  /* pass-2 BFS list cap of the rewrite path (0 = 256 Ki) */                                                           \
  X(interp_cap2, interp_cap2, uint32_t, 0, 0, 1 << 22, KNOB_RANGE)                                                     \
  /* workspace grid-log entries (0 = 16 Mi; tests) */                                                                  \
  X(grid_cap, grid_small_cap, uint64_t, 0, 0, 1ll << 34, KNOB_RANGE)                                                   \
  /* grid-tier queries as MS-BFS when the dense masks fit (0: off) */                                                  \
  X(grid_ms, grid_ms, int, 1, 0, 1, KNOB_RANGE)                                                                        \
  /* MS-BFS mask budget per workspace */                                                                               \
  X(grid_ms_bytes, grid_ms_bytes, size_t, 1ull << 30, 1 << 20, 1ll << 40, KNOB_RANGE)                                  \
  /* 64-bit words per MS-BFS mask (64 queries each) */                                                                 \
  X(grid_ms_words, grid_ms_words, int, 8, 1, 16, KNOB_POW2)                                                            \
  /* holders above which MS-BFS probes dset instead */                                                                 \
  X(grid_ms_tg_cap, grid_ms_tg_cap, uint32_t, 256, 0, 0x7FFFFFFF, KNOB_RANGE)                                          \
  /* MS-BFS entries per level buffer (0 = 16 Mi; tests) */                                                             \
  X(grid_ms_cap, grid_ms_cap, uint64_t, 0, 0, 1ll << 28, KNOB_RANGE)                                                   \
  /* batches with stats time every tail-tier level launch with a HIP event pair (kg_stats tail_ms); off by default -- \
     the records leave gaps between the launches */                                                                    \
  X(level_events, level_events, int, 0, 0, 1, KNOB_RANGE)                                                              \
  /* concurrent host-buffer calls: lane sets in the snapshot's pool (sets already created stay in it).  Read and      \
     written under Snapshot::lane_mu */                                                                                \
  X(max_lanes, lane_cap, size_t, 32, 1, 1024, KNOB_RANGE)                                                              \
  /* ---- expand */                                                                                                    \
  /* pass-1 overflows of kg_expand_batch run gather-then-walk (1) or the hash pass directly (0) */                     \
  X(expand_gw, expand_gw, int, 1, 0, 1, KNOB_RANGE)                                                                    \
  /* (tests) 1 = every root skips the LDS passes, 2 = the 16-lane walkers (pass 0) are skipped and the 64-lane pass    \
     takes every root */                                                                                               \
  X(expand_skip_lds, expand_skip_lds, int, 0, 0, 2, KNOB_RANGE)                                                        \
  /* (tests) visited sets per hash-pass slot; small values reach the bitmap pass */                                    \
  X(expand_hash_cap, expand_hash_cap, uint32_t, 1u << 18, 4, 1 << 18, KNOB_RANGE)                                      \
  /* k_expand_gw: longest wait (us) of a large slot for a small slot's hand-on before it gives its ticket up */        \
  X(expand_gw_wait_us, expand_gw_wait_us, uint32_t, 100000, 0, 10000000, KNOB_RANGE)                                   \
  /* ---- lookups and listing */                                                                                       \
  /* initial output entries of a lookup (0 = 64 Ki; tests) */                                                          \
  X(lookup_cap, lookup_cap, uint64_t, 0, 0, 1ll << 32, KNOB_RANGE)                                                     \
  /* (tests) 1 = kg_lookup_subjects lists its domain from the check rows even where the holder bitmap exists (what a  \
     snapshot without reverse indexes does) */                                                                         \
  X(lookup_domain_rows, lookup_domain_rows, int, 0, 0, 1, KNOB_RANGE)                                                  \
  /* 1 = a lookup on a boolean rewrite takes its candidates from a walk over the plan's leaves; 0 = from the whole    \
     domain (tests, A/B: the answers are the same) */                                                                  \
  X(lookup_formula, lookup_formula, int, 1, 0, 1, KNOB_RANGE)                                                          \
  /* (key, position) pairs a listing sorts directly (0 = 1 Mi; tests) */                                               \
  X(query_cap, query_cap, uint64_t, 0, 0, 1ll << 32, KNOB_RANGE)                                                       \
  /* ---- hash-sharded mode */                                                                                         \
  /* log2 of the per-batch (query, node) visited table; a batch that overflows it grows it */                          \
  X(shard_vis, shard_vis_log2, int, 23, 10, 34, KNOB_RANGE)                                                            \
  /* first bucket size of new in-library bindings (0: by batch) */                                                     \
  X(shard_bucket, shard_bucket0, uint32_t, 0, 0, 1ll << 26, KNOB_RANGE)                                                \
  /* set rows longer than this go to k_shard_heavy (r3p A/B) */                                                        \
  X(shard_heavy, shard_heavy, uint32_t, 64, 0, 0xFFFFFFFFll, KNOB_RANGE)                                               \
  /* forward set edges per query and rank (0 = off) */                                                                 \
  X(shard_budget, shard_budget, uint32_t, 0, 0, 0xFFFFFFFFll, KNOB_RANGE)                                              \
  /* reverse edges per query and rank */                                                                               \
  X(shard_back_budget, shard_back_budget, uint32_t, 1u << 14, 0, 0xFFFFFFFFll, KNOB_RANGE)                             \
  /* one rank runs the replica tier chain */                                                                           \
  X(shard_local, shard_local, int, 1, 0, 1, KNOB_RANGE)                                                                \
  /* one rank runs the N > 1 protocol */                                                                               \
  X(shard_force_exchange, shard_force_exchange, int, 0, 0, 1, KNOB_RANGE)                                              \
  /* bind-time remote child metadata (DevSnap) */                                                                      \
  X(shard_remote_meta, shard_remote_meta, int, 1, 0, 1, KNOB_RANGE)                                                    \
  /* overflow reruns per batch (0: max(4, exchanges)) */                                                               \
  X(shard_max_reruns, shard_max_reruns, uint32_t, 0, 0, 64, KNOB_RANGE)                                                \
  /* bucket buffers cap (0: 1/4 of free HBM); no upper bound */                                                        \
  X(shard_max_bytes, shard_max_bytes, uint64_t, 0, 0, INT64_MAX, KNOB_RANGE)                                           \
  /* tests -- every run overflows */                                                                                   \
  X(shard_force_overflow, shard_force_overflow, int, 0, 0, 1, KNOB_RANGE)

struct Knobs {
#define X(key, field, type, def, lo, hi, kind) type field = def;
  KG_KNOBS(X)
#undef X
};

struct Knob {
  const char* key;
  int64_t lo, hi;
  KnobKind kind;
  void (*store)(Knobs&, int64_t);
};

inline const Knob KNOBS[] = {
#define X(key, field, type, def, lo, hi, kind) {#key, lo, hi, kind, [](Knobs& k, int64_t v) { k.field = (type)v; }},
    KG_KNOBS(X)
#undef X
};
constexpr size_t N_KNOBS = sizeof KNOBS / sizeof *KNOBS;

constexpr int KNOB_UNKNOWN = 1, KNOB_OUT_OF_RANGE = 2;

// Stores `value` under `key`: 0, KNOB_UNKNOWN (*which = nullptr) or KNOB_OUT_OF_RANGE (k unchanged).  *which: the
// key's row, for the caller's message.  Touches nothing but k.
inline int knob_set(Knobs& k, const char* key, int64_t value, const Knob** which) {
  *which = nullptr;
  for (const Knob& r : KNOBS) {
    if (strcmp(key, r.key) != 0) continue;
    *which = &r;
    if (value < r.lo || value > r.hi || (r.kind == KNOB_POW2 && (value & (value - 1)))) return KNOB_OUT_OF_RANGE;
    r.store(k, value);
    return 0;
  }
  return KNOB_UNKNOWN;
}

}  // namespace kg
