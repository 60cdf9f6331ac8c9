"""Access masks against what a caller did before them, and the ranked select against torch indexing.

  python tools/mask_bench.py [--tuples 2000000] [--depth 10] [--reps 20] [--warmup 5] [--rows 64] [--cands 1024]

The graph and the requests are tools/lookup_bench.py's: Snapshot.synthetic(--tuples), doc#viewer, the 64 users
around the median of the number of rows that hold them, one request and all 64.

mask:    kg_lookup_objects_mask_device -- the bitmap rows written in HBM -- against kg_lookup_objects, a bitmap
         built from its id lists on the host with numpy, and an upload through torch, which is how a caller got
         the same tensor before.  Both end with the mask usable on the device.
select:  kg_mask_select_device on --rows rows of --cands ranked ids (random objects of the namespace, two thirds
         of them from the row's own answer) against the equivalent torch expression: gather the bit of every
         candidate, a cumulative sum for the places, a scatter of the first `limit` into an END-filled row.

The answers of both sides are compared before anything is timed.  Prints one JSON line: median wall-clock
milliseconds of --reps calls after --warmup, each side, and their ratio.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NS_DOC, SUBJECT_ID = 0, 0xFFFFFFFF  # the synthetic generator's ids (include/ketogpu.h)


def median_ms(fn, reps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def host_bitmap(off, objs, n, n_bits, row_words):
    """The mask rows out of an unpaged answer, vectorised: what a caller's host code did."""
    m = np.zeros((n, row_words), np.uint32)
    keep = objs < n_bits
    rows = np.repeat(np.arange(n), np.diff(off).astype(np.int64))[keep]
    ids = objs[keep]
    np.bitwise_or.at(m, (rows, ids >> 5), np.uint32(1) << (ids & 31).astype(np.uint32))
    return m


def torch_select(torch, mask, cand, limit, n_bits):
    """kg_mask_select_device (base 0) as torch indexing on the device."""
    n, k = cand.shape
    c = cand.long()
    inr = (c >= 0) & (c < n_bits)  # END reads as -1
    safe = torch.where(inr, c, torch.zeros_like(c))
    bit = (torch.gather(mask, 1, safe >> 5) >> (safe & 31).int()) & 1
    ok = inr & (bit != 0)
    pos = torch.cumsum(ok, 1) - 1
    take = ok & (pos < limit)
    out = torch.full((n, limit + 1), -1, dtype=torch.int32, device=cand.device)
    out.scatter_(1, torch.where(take, pos, torch.full_like(pos, limit)), torch.where(take, cand, torch.full_like(cand, -1)))
    return out[:, :limit].contiguous(), ok.sum(1).int()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuples", type=int, default=2_000_000)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--cands", type=int, default=1024)
    ap.add_argument("--limit", type=int, default=100)
    a = ap.parse_args(argv)
    import torch
    from keto_amd.engine import Config, Engine, Snapshot
    dev = torch.device("cuda", 0)
    snap = Snapshot.synthetic(a.tuples)
    eng = Engine(snap, Config(a.depth))
    rel = snap.interner.rel_id("viewer")
    rows = snap.export()
    doc = rows[rows[:, 0] == NS_DOC]
    domain = np.unique(np.concatenate([doc[:, 1], rows[rows[:, 3] == NS_DOC][:, 4]]))
    users, deg = np.unique(rows[rows[:, 3] == SUBJECT_ID, 4], return_counts=True)
    order = np.argsort(deg, kind="stable")
    mid = order[len(order) // 2 - 32:len(order) // 2 + 32]
    reqs64 = np.zeros((64, 6), np.uint32)
    reqs64[:, 0], reqs64[:, 1], reqs64[:, 2], reqs64[:, 3] = NS_DOC, rel, SUBJECT_ID, users[mid]
    n_bits = int(domain.max()) + 1
    row_words = (n_bits + 31) // 32
    sync = torch.cuda.synchronize
    out = {"gpu": torch.cuda.get_device_name(0), "tuples": int(len(rows)), "domain_objects": int(len(domain)),
           "n_bits": n_bits, "row_words": row_words, "depth": a.depth, "holder_rows_of_user": int(deg[mid[32]])}
    for name, reqs in (("one", reqs64[32:33]), ("batch64", reqs64)):
        n = len(reqs)
        buf = torch.empty((n, row_words), dtype=torch.int32, device=dev)

        def before():
            off, objs, _, _ = eng.lookup_objects_ids(reqs)
            return torch.from_numpy(host_bitmap(off, objs, n, n_bits, row_words).view(np.int32)).to(dev)

        def masked():
            return eng.lookup_objects_mask_ids(reqs, 0, n_bits, out=buf)

        mask, n_set, _, _ = masked()
        if not torch.equal(mask, before()):
            raise SystemExit(f"{name}: the mask differs from the host-built bitmap")
        t_before = median_ms(before, a.reps, a.warmup, sync)
        t_mask = median_ms(masked, a.reps, a.warmup, sync)
        out[name] = {"lookup_host_bitmap_upload_ms": round(t_before, 3), "mask_call_ms": round(t_mask, 3),
                     "ratio": round(t_before / t_mask, 2), "members": int(n_set.sum()),
                     "mask_bytes": n * row_words * 4}
    # the select: --rows rows (the 64 requests' masks, repeated) of --cands ranked ids
    mask64, _, _, _ = eng.lookup_objects_mask_ids(reqs64, 0, n_bits)
    off, objs, _, _ = eng.lookup_objects_ids(reqs64)
    rng = np.random.default_rng(7)
    pick = np.arange(a.rows) % 64
    cand = rng.choice(domain, (a.rows, a.cands)).astype(np.uint32)
    for i, r in enumerate(pick):
        own = objs[int(off[r]):int(off[r + 1])]
        if len(own):
            k = (2 * a.cands) // 3
            cand[i, rng.permutation(a.cands)[:k]] = rng.choice(own, k)
    d_mask = mask64[torch.from_numpy(pick).to(dev)].contiguous()
    d_cand = torch.from_numpy(cand.view(np.int32)).to(dev)
    got, cnt = eng.mask_select(d_mask, d_cand, a.limit, 0, n_bits)
    want, wcnt = torch_select(torch, d_mask, d_cand, a.limit, n_bits)
    if not (torch.equal(got, want) and torch.equal(cnt, wcnt)):
        raise SystemExit("select: the kernel and the torch expression differ")
    t_k = median_ms(lambda: eng.mask_select(d_mask, d_cand, a.limit, 0, n_bits), a.reps, a.warmup, sync)
    t_t = median_ms(lambda: torch_select(torch, d_mask, d_cand, a.limit, n_bits), a.reps, a.warmup, sync)
    out["select"] = {"rows": a.rows, "cands": a.cands, "limit": a.limit, "allowed_mean": round(float(cnt.float().mean()), 1),
                     "mask_select_ms": round(t_k, 4), "torch_ms": round(t_t, 4), "ratio": round(t_t / t_k, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
