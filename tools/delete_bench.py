"""Delete by query on the device against the route a caller had before it: page the matching rows out with
kg_snapshot_query, then hand them to kg_snapshot_apply as deletes.

  python tools/delete_bench.py [--tuples 2000000] [--reps 7] [--warmup 2] [--page 65536]

Three deletes on the synthetic graph: the row of the node with the most entries (namespace, object and
relation), a subject id held in many rows (the user most rows hold), and a whole namespace (the groups).
Every delete starts from the same base; both routes run in one process, alternating, and the medians after
the warm-up are reported.  The two results' exports are compared before anything is timed.  Prints one JSON
line: per delete the rows matched, the median wall-clock milliseconds of kg_snapshot_delete_matching
(delete_ms, with keys), its kernel_ms (match + compaction) and the share of the call outside them (the
rebuild of the derived structures, the allocations and the call itself), and the old route's paging and apply
times.  The synthetic base has no host node map, so each kg_snapshot_apply of the old route also rebuilds
that map from the device triples (a tuple-built base hands its map on instead); page_ms alone is free of it.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NS_GROUP, SUBJECT_ID = 1, 0xFFFFFFFF  # the synthetic generator's ids (include/ketogpu.h)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuples", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--page", type=int, default=65536, help="rows a kg_snapshot_query page of the old route holds")
    a = ap.parse_args(argv)
    import torch
    from keto_amd.engine import Snapshot, row_queries
    base = Snapshot.synthetic(a.tuples)
    rows = base.export()
    packed = (rows[:, 0].astype(np.uint64) << 48) | (rows[:, 2].astype(np.uint64) << 32) | rows[:, 1]
    _, first, cnt = np.unique(packed, return_index=True, return_counts=True)
    hub = rows[first[np.argmax(cnt)], :3]
    users, deg = np.unique(rows[rows[:, 3] == SUBJECT_ID, 4], return_counts=True)
    user = users[np.argmax(deg)]
    shapes = [("hub_row", 7, [*hub, 0, 0, 0]), ("subject_id", 8, [0, 0, 0, SUBJECT_ID, user, 0]),
              ("namespace", 1, [NS_GROUP, 0, 0, 0, 0, 0])]
    out = {"gpu": torch.cuda.get_device_name(0), "tuples": int(len(rows)), "nodes": base.info()["nodes"], "page": a.page}
    none = np.zeros((0, 6), np.uint32)

    def page_out(mask, t):
        """Every matching row, page by page, as the host gets them today."""
        got, after = [], 0
        while True:
            r, keys, _, nxt, _ = base.query(row_queries([mask], t[None, :], after, a.page))
            got.append(r)
            after = int(nxt[0])
            if not after:
                return np.concatenate(got) if got else none

    for name, mask, t in shapes:
        t = np.asarray(t, np.uint32)
        req = row_queries([mask], t[None, :])
        new, matched, keys, st = base.delete_matching(req, want_keys=True, with_stats=True)
        old = base.apply(none, page_out(mask, t))
        assert new is not None and np.array_equal(new.export(), old.export()), name  # the same rows both ways
        assert int(matched[0]) == len(keys) == len(rows) - new.info()["rows"], name
        new.close()
        old.close()
        d_ms, k_ms, p_ms, a_ms = [], [], [], []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            new, _, _, st = base.delete_matching(req, want_keys=True, with_stats=True)
            t1 = time.perf_counter()
            new.close()
            t2 = time.perf_counter()
            dels = page_out(mask, t)
            t3 = time.perf_counter()
            old = base.apply(none, dels)
            t4 = time.perf_counter()
            old.close()
            if k >= a.warmup:
                d_ms.append((t1 - t0) * 1e3)
                k_ms.append(st["kernel_ms"])
                p_ms.append((t3 - t2) * 1e3)
                a_ms.append((t4 - t3) * 1e3)
        med = statistics.median
        out[name] = {"matched": int(matched[0]), "delete_ms": round(med(d_ms), 3), "kernel_ms": round(med(k_ms), 4),
                     "share_outside_kernels": round(1 - med(k_ms) / med(d_ms), 4),
                     "page_ms": round(med(p_ms), 3), "apply_ms": round(med(a_ms), 3),
                     "old_over_new": round((med(p_ms) + med(a_ms)) / med(d_ms), 2)}
    base.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
