"""Reverse lookup against the brute force a caller needed before it: kg_lookup_objects for one request
and for a batch of 64, and for the same requests every object of the namespace through
kg_check_batch_device (queries resident in HBM, so the brute force pays no host transfer).

  python tools/lookup_bench.py [--mode objects|subjects|subject-sets] [--tuples 2000000] [--depth 10] [--reps 20] [--warmup 5]
                               [--preset 0|1] [--relation NAME] [--page N]

--mode subjects measures the mirror image the same way: kg_lookup_subjects for one doc and for 64 docs
against every subject id of the snapshot's tuples through kg_check_batch_device.

--mode subject-sets measures kg_lookup_subject_sets for the same docs with the filter group#member ("which
groups may do this on the doc?") against what a caller did before it: every subject set of the filter's domain
(the group#member sets that occur as a tuple's subject) through kg_check_batch_device.  It prints both times,
the domain size and `parity`, the number of requests whose two answers differ (it must be 0).  With --page N
the paged call is timed beside the same brute force and the page compared with the brute force's first N.

--preset 1 builds the C3 graph with its program (keto_amd/synth.py) and asks for --relation, by default
the permission doc#share = view & !blocked: a boolean rewrite, which the lookups answer in formula mode
(candidates from a walk over the plan's leaves).  The lookup is then timed twice, with kg_snapshot_tune
"lookup_formula" 1 and 0 (0: candidates from the whole domain; a library without the key is timed once, as
it is), and each run's candidates / confirmed / n_objs are printed under "lookup_formula".  --relation
view gives the number of doc#view members of the same subjects: what a share request's candidates must equal.

Prints one JSON line: median wall-clock milliseconds of both paths, their ratio, and the lookup call's
reverse_edges / levels / n_objs.  The two answers are compared before anything is timed.

--page N times the paged call (kg_lookup_objects_page / kg_lookup_subjects_page: the first N ids of every
request) against what a caller did before it, the unpaged call plus a slice on the host, for one request and
for 64, in every mode the other options select (--preset 0: the walk; --preset 1: "lookup_formula" 1 and
0).  The page is compared with the slice of the unpaged answer before anything is timed; no brute force is
run.  Each entry carries the paged call's candidates, rounds and n_objs beside the unpaged call's.  A library
without the paged calls (an older build through KG_LIB_PATH) is timed for the unpaged call and the slice alone.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NS_DOC, REL_VIEWER, SUBJECT_ID = 0, 1, 0xFFFFFFFF  # the synthetic generator's ids (include/ketogpu.h)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("objects", "subjects", "subject-sets"), default="objects")
    ap.add_argument("--tuples", type=int, default=2_000_000)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preset", type=int, choices=(0, 1), default=0)
    ap.add_argument("--relation", default=None, help="default: viewer (preset 0), share (preset 1)")
    ap.add_argument("--page", type=int, default=0, help="time the paged call for the first N ids against unpaged + slice")
    a = ap.parse_args(argv)
    import torch
    from keto_amd import _lib
    from keto_amd.engine import Config, Engine, Snapshot
    dev = torch.device("cuda", 0)
    snap = Snapshot.synthetic(a.tuples, preset=a.preset)
    eng = Engine(snap, Config(a.depth))
    L = _lib.load()
    relation = a.relation or ("share" if a.preset else "viewer")
    rel = snap.interner.rel_id(relation)
    keys = [None]  # the values of "lookup_formula" the lookup is timed with
    if a.preset:
        try:
            snap.tune("lookup_formula", 1)
            keys = [1, 0]
        except _lib.KetoGPUError:  # a library from before the key: its one mode
            pass
    rows = snap.export()
    doc = rows[rows[:, 0] == NS_DOC]
    sets = rows[(rows[:, 3] == NS_DOC)]
    domain = np.unique(np.concatenate([doc[:, 1], sets[:, 4]]))  # the objects of namespace doc
    # mid-degree users: the 64 users around the median of the number of rows that hold them
    users, deg = np.unique(rows[rows[:, 3] == SUBJECT_ID, 4], return_counts=True)
    order = np.argsort(deg, kind="stable")
    mid = order[len(order) // 2 - 32:len(order) // 2 + 32]
    subj = users[mid]
    reqs64 = np.zeros((64, 6), np.uint32)
    reqs64[:, 0], reqs64[:, 1], reqs64[:, 2], reqs64[:, 3] = NS_DOC, rel, SUBJECT_ID, subj
    out = {"gpu": torch.cuda.get_device_name(0), "preset": a.preset, "relation": relation, "tuples": int(len(rows)),
           "nodes": snap.info()["nodes"],
           "domain_objects": int(len(domain)), "depth": a.depth, "holder_rows_of_user": int(deg[mid[32]])}
    if a.mode == "subjects":
        # mid-reach docs: the 64 doc#viewer nodes around the median check-row length; the domain is every subject id
        viewer = doc[doc[:, 2] == REL_VIEWER]
        docs, rlen = np.unique(viewer[:, 1], return_counts=True)
        order = np.argsort(rlen, kind="stable")
        mid = order[len(order) // 2 - 32:len(order) // 2 + 32]
        domain = users
        reqs64 = np.zeros((64, 4), np.uint32)
        reqs64[:, 0], reqs64[:, 1], reqs64[:, 2] = NS_DOC, docs[mid], rel
        out = {"gpu": out["gpu"], "preset": a.preset, "relation": relation, "tuples": out["tuples"], "nodes": out["nodes"],
               "domain_subject_ids": int(len(domain)),
               "depth": a.depth, "check_row_of_doc": int(rlen[mid[32]])}
    if a.mode == "subject-sets":
        print(json.dumps(subject_sets(a, eng, snap, L, keys, rows, relation, dev)))
        return
    if a.page:
        out["page"] = a.page
        for name, reqs in (("one", reqs64[32:33]), ("batch64", reqs64)):
            out[name] = page_entry(a, eng, snap, keys, reqs, hasattr(L, "kg_lookup_objects_page"))
        print(json.dumps(out))
        return
    stream = torch.cuda.current_stream(dev)
    for name, reqs in (("one", reqs64[32:33]), ("batch64", reqs64)):
        n = len(reqs)
        q = torch.zeros((n, len(domain), 7), dtype=torch.int32, device=dev)  # kg_query rows, built in HBM
        q[:, :, 0], q[:, :, 2], q[:, :, 3] = NS_DOC, rel, -1  # -1: KG_SUBJECT_ID
        d_dom = torch.from_numpy(domain.view(np.int32)).to(dev)[None, :]
        d_req = torch.from_numpy(reqs[:, 3 if a.mode == "objects" else 1].copy().view(np.int32)).to(dev)[:, None]
        q[:, :, 1], q[:, :, 4] = (d_dom, d_req) if a.mode == "objects" else (d_req, d_dom)
        dq = q.reshape(-1, 7).contiguous()
        d_out = torch.zeros(dq.shape[0], dtype=torch.uint8, device=dev)
        d_err = torch.zeros(dq.shape[0], dtype=torch.int32, device=dev)

        def brute():
            _lib.check(L.kg_check_batch_device(snap.handle, dq.data_ptr(), dq.shape[0], a.depth, d_out.data_ptr(),
                                               d_err.data_ptr(), None, C.c_void_p(stream.cuda_stream)), "check")
            torch.cuda.synchronize()

        def lookup():
            if a.mode == "subjects":
                return eng.lookup_subjects_ids(reqs, with_stats=True)
            return eng.lookup_objects_ids(reqs, with_stats=True)

        def median_ms(fn):
            xs = []
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                fn()
                if k >= a.warmup:
                    xs.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(xs)

        brute()
        member = (d_out.cpu().numpy() == 1).reshape(n, len(domain))
        t, by_key = {}, {}
        for key in reversed(keys):  # the default (None, or 1) last: its figures are the entry's own
            if key is not None:
                snap.tune("lookup_formula", key)
            off, objs, err, nerr = lookup()
            for i in range(n):  # the same answer both ways, before anything is timed
                assert np.array_equal(objs[int(off[i]):int(off[i + 1])], domain[member[i]]), (key, i)
            assert not nerr.any()
            t["lookup_ms"] = median_ms(lookup)
            lookup()
            st = eng.last_stats
            by_key[str(key)] = {"lookup_ms": round(t["lookup_ms"], 4), "lookup_kernel_ms": round(st["kernel_ms"], 4),
                                "candidates": int(st["candidates"]), "confirmed": int(st["confirmed"]),
                                "n_objs": int(st["n_objs"])}
        t["brute_ms"] = median_ms(brute)
        out[name] = {"requests": n, "checks_brute": int(dq.shape[0]), "lookup_ms": round(t["lookup_ms"], 4),
                     "brute_ms": round(t["brute_ms"], 4), "brute_over_lookup": round(t["brute_ms"] / t["lookup_ms"], 2),
                     "lookup_kernel_ms": round(st["kernel_ms"], 4), "reverse_edges": int(st["reverse_edges"]),
                     "levels": int(st["levels"]), "n_objs": int(st["n_objs"]), "exact": int(st["exact"]), "candidates": int(st["candidates"]),
                     "confirmed": int(st["confirmed"])}
        if a.preset:
            out[name]["lookup_formula"] = by_key
        del q, dq, d_out, d_err
    print(json.dumps(out))


def subject_sets(a, eng, snap, L, keys, rows, relation, dev):
    """--mode subject-sets: the groups (group#member) that hold `relation` on one doc and on 64 docs, by the
    lookup and by a check of every set of the filter's domain; --page: the first N of them by the paged call."""
    import torch
    from keto_amd import _lib
    it = snap.interner
    rel, sns, srel = it.rel_id(relation), it.ns_id("group"), it.rel_id("member")
    domain = np.unique(rows[(rows[:, 3] == sns) & (rows[:, 5] == srel), 4])
    # mid-reach docs: the 64 doc#viewer nodes around the median row length
    viewer = rows[(rows[:, 0] == NS_DOC) & (rows[:, 2] == REL_VIEWER)]
    docs, rlen = np.unique(viewer[:, 1], return_counts=True)
    order = np.argsort(rlen, kind="stable")
    mid = order[len(order) // 2 - 32:len(order) // 2 + 32]
    reqs64 = np.zeros((64, 6), np.uint32)
    reqs64[:, 0], reqs64[:, 1], reqs64[:, 2], reqs64[:, 3], reqs64[:, 4] = NS_DOC, docs[mid], rel, sns, srel
    out = {"gpu": torch.cuda.get_device_name(0), "mode": "subject-sets", "preset": a.preset, "relation": relation,
           "filter": "group#member", "tuples": int(len(rows)), "nodes": snap.info()["nodes"],
           "domain_sets": int(len(domain)), "depth": a.depth, "row_of_doc": int(rlen[mid[32]])}
    if a.page:
        out["page"] = a.page
    stream = torch.cuda.current_stream(dev)

    def median_ms(fn):
        xs = []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            fn()
            if k >= a.warmup:
                xs.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(xs)

    for name, reqs in (("one", reqs64[32:33]), ("batch64", reqs64)):
        n = len(reqs)
        q = torch.zeros((n, len(domain), 7), dtype=torch.int32, device=dev)  # kg_query rows, built in HBM
        q[:, :, 0], q[:, :, 2], q[:, :, 3], q[:, :, 5] = NS_DOC, rel, sns, srel
        q[:, :, 1] = torch.from_numpy(reqs[:, 1].copy().view(np.int32)).to(dev)[:, None]
        q[:, :, 4] = torch.from_numpy(domain.view(np.int32)).to(dev)[None, :]
        dq = q.reshape(-1, 7).contiguous()
        d_out = torch.zeros(dq.shape[0], dtype=torch.uint8, device=dev)
        d_err = torch.zeros(dq.shape[0], dtype=torch.int32, device=dev)
        pages = np.stack([np.zeros(n, np.uint32), np.full(n, max(a.page, 1), np.uint32)], 1)

        def brute():
            _lib.check(L.kg_check_batch_device(snap.handle, dq.data_ptr(), dq.shape[0], a.depth, d_out.data_ptr(),
                                               d_err.data_ptr(), None, C.c_void_p(stream.cuda_stream)), "check")
            torch.cuda.synchronize()

        def lookup():
            if a.page:
                return eng.lookup_subject_sets_page_ids(reqs, pages, with_stats=True)[:4]
            return eng.lookup_subject_sets_ids(reqs, with_stats=True)

        brute()
        member = (d_out.cpu().numpy() == 1).reshape(n, len(domain))
        entry = {"requests": n, "checks_brute": int(dq.shape[0])}
        for key in reversed(keys):  # the default (None, or 1) last
            if key is not None:
                snap.tune("lookup_formula", key)
            off, ids, err, nerr = lookup()
            want = [domain[member[i]][:a.page] if a.page else domain[member[i]] for i in range(n)]
            parity = sum(not np.array_equal(ids[int(off[i]):int(off[i + 1])], want[i]) for i in range(n)) + int(nerr.any())
            ms = median_ms(lookup)
            lookup()
            st = eng.last_stats
            e = {"lookup_ms": round(ms, 4), "lookup_kernel_ms": round(st["kernel_ms"], 4), "parity": int(parity),
                 "n_objs": int(st["n_objs"]), "exact": int(st["exact"]), "candidates": int(st["candidates"]),
                 "confirmed": int(st["confirmed"]), "levels": int(st["levels"])}
            if a.page:
                e["rounds"] = int(st["rounds"])
            entry["lookup_formula=" + str(key)] = e
        entry["brute_ms"] = round(median_ms(brute), 4)
        entry["brute_over_lookup"] = round(entry["brute_ms"] / ms, 2)  # against the default mode
        entry["parity"] = sum(v["parity"] for v in entry.values() if isinstance(v, dict))
        out[name] = entry
        del q, dq, d_out, d_err
    out["parity"] = out["one"]["parity"] + out["batch64"]["parity"]
    return out


def page_entry(a, eng, snap, keys, reqs, have_paged):
    """--page: per value of "lookup_formula" the medians of the paged call and of the unpaged call plus the
    host slice, with both calls' counters."""
    n = len(reqs)
    pages = np.stack([np.zeros(n, np.uint32), np.full(n, a.page, np.uint32)], 1)
    unpaged = eng.lookup_subjects_ids if a.mode == "subjects" else eng.lookup_objects_ids
    paged = eng.lookup_subjects_page_ids if a.mode == "subjects" else eng.lookup_objects_page_ids

    def median_ms(fn):
        xs = []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            fn()
            if k >= a.warmup:
                xs.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(xs)

    def sliced():
        off, objs, err, nerr = unpaged(reqs, with_stats=True)
        return [objs[int(off[i]):int(off[i + 1])][:a.page] for i in range(n)], off

    entry = {"requests": n}
    for key in keys:
        if key is not None:
            snap.tune("lookup_formula", key)
        want, off = sliced()
        st = eng.last_stats
        e = {"unpaged_slice_ms": None, "unpaged_n_objs": int(st["n_objs"]), "unpaged_candidates": int(st["candidates"]),
             "unpaged_exact": int(st["exact"])}
        if have_paged:
            poff, ids, err, nerr, nxt = paged(reqs, pages, with_stats=True)
            for i in range(n):  # the page is the slice, before anything is timed
                assert np.array_equal(ids[int(poff[i]):int(poff[i + 1])], want[i]), (key, i)
                assert (int(nxt[i]) == 0xFFFFFFFF) == (int(off[i + 1] - off[i]) <= a.page), (key, i)
            e["page_ms"] = round(median_ms(lambda: paged(reqs, pages, with_stats=True)), 4)
            st = eng.last_stats
            e.update({"page_kernel_ms": round(st["kernel_ms"], 4), "n_objs": int(st["n_objs"]), "exact": int(st["exact"]),
                      "candidates": int(st["candidates"]), "confirmed": int(st["confirmed"]), "rounds": int(st["rounds"])})
        e["unpaged_slice_ms"] = round(median_ms(sliced), 4)
        if have_paged:
            e["unpaged_over_page"] = round(e["unpaged_slice_ms"] / e["page_ms"], 2)
        entry[str(key)] = e
    return entry


if __name__ == "__main__":
    main()
