"""Tuple listing on the device against the only route there was before it: kg_snapshot_export of every row
plus a numpy filter on the host.

  python tools/list_bench.py [--tuples 2000000] [--limit 100] [--reps 20] [--warmup 5] [--host-reps N] [--scan-only]

Five queries on the synthetic graph: a full (namespace, object, relation) key, a namespace alone, a subject
id alone (a user at the median holder count), an unfiltered first page and an unfiltered page from the
middle.  Prints one JSON line: per query the median wall-clock milliseconds of kg_snapshot_query and of
export + filter, their ratio, and the call's matched / rows_scanned / passes / kernel_ms, the entries tested
per second of device time and, for the query that names a subject, the share of the 8 TB/s roofline (4 B per
entry; the synthetic snapshot has no key array, so a scan without a subject reads no memory per entry).  The two answers are compared before anything is timed.  --scan-only: snapshots too large to
export -- the subject-id and the two unfiltered queries alone, no host route and no comparison.
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
ROOFLINE = 8e12  # B/s


def host_page(rows, mask, t, after, limit):
    """Filter, keep keys (position + 1) above `after`, cut: what a caller did with the exported rows."""
    m = np.ones(len(rows), bool)
    m[:after] = False
    for bit, col in ((1, 0), (2, 1), (4, 2)):
        if mask & bit:
            m &= rows[:, col] == t[col]
    if mask & 8:
        m &= (rows[:, 3] == t[3]) & (rows[:, 4] == t[4])
    idx = np.nonzero(m)[0]
    return rows[idx[:limit]], len(idx)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuples", type=int, default=2_000_000)
    ap.add_argument("--limit", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=0, help="calls of the export + filter route (0: as --reps and --warmup)")
    ap.add_argument("--scan-only", action="store_true", help="no export: the scanning queries alone")
    a = ap.parse_args(argv)
    import torch
    from keto_amd.engine import Snapshot, row_queries
    snap = Snapshot.synthetic(a.tuples)
    n = snap.info()["rows"]
    out = {"gpu": torch.cuda.get_device_name(0), "tuples": int(n), "nodes": snap.info()["nodes"], "limit": a.limit}
    if a.scan_only:
        ids = snap.synth_ids()
        rows = None
        queries = [("subject_id", 8, [0, 0, 0, SUBJECT_ID, ids["user_obj0"] + ids["n_users"] // 2, 0], 0)]
    else:
        rows = snap.export()
        # the node with the longest row, and a user at the median of the number of rows that hold them
        packed = (rows[:, 0].astype(np.uint64) << 48) | (rows[:, 2].astype(np.uint64) << 32) | rows[:, 1]
        _, first, cnt = np.unique(packed, return_index=True, return_counts=True)
        hub = rows[first[np.argmax(cnt)], :3]
        users, deg = np.unique(rows[rows[:, 3] == SUBJECT_ID, 4], return_counts=True)
        user = users[np.argsort(deg, kind="stable")[len(users) // 2]]
        queries = [("full_key", 7, [*hub, 0, 0, 0], 0), ("namespace", 1, [NS_DOC, 0, 0, 0, 0, 0], 0),
                   ("subject_id", 8, [0, 0, 0, SUBJECT_ID, user, 0], 0)]
        out.update({"hub_row": int(cnt.max()), "holder_rows_of_user": int(np.median(deg))})
    queries += [("unfiltered_first", 0, [0] * 6, 0), ("unfiltered_middle", 0, [0] * 6, n // 2)]

    def timed(fn, warmup=a.warmup, reps=a.reps):
        xs = []
        for k in range(warmup + reps):
            t0 = time.perf_counter()
            fn()
            if k >= warmup:
                xs.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(xs)

    for name, mask, t, after in queries:
        t = np.asarray(t, np.uint32)
        req = row_queries([mask], t[None, :], after, a.limit)
        got, keys, off, nxt, matched = snap.query(req)
        n_match = int(matched[0])
        assert (int(nxt[0]) != 0) == (n_match > a.limit)
        h_ms = None
        if rows is not None:
            want, n_want = host_page(rows, mask, t, after, a.limit)  # the same answer both ways, before anything is timed
            assert np.array_equal(got, want) and n_match == n_want, name
            h_ms = timed(lambda: host_page(snap.export(), mask, t, after, a.limit),
                         *((1, a.host_reps) if a.host_reps else ()))
        q_ms = timed(lambda: snap.query(req))
        st = snap.query(req, with_stats=True)[-1]  # a warm call's counters
        out[name] = {"matched": n_match, "rows_scanned": st["rows_scanned"], "passes": st["passes"],
                     "kernel_ms": round(st["kernel_ms"], 4), "query_ms": round(q_ms, 4),
                     "export_filter_ms": round(h_ms, 2) if h_ms is not None else None,
                     "export_over_query": round(h_ms / q_ms, 1) if h_ms is not None else None,
                     "entries_per_s": round(st["rows_scanned"] / (st["kernel_ms"] * 1e-3)) if st["kernel_ms"] else None,
                     # the call's device time (launches, readbacks, sort and decode included) against the bytes its
                     # scans read: the subject of every entry where the query names one; no key array here
                     "roofline_share": round(st["rows_scanned"] * 4 / ROOFLINE / (st["kernel_ms"] * 1e-3), 4)
                     if mask & 8 and st["kernel_ms"] else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
