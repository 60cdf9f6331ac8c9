"""GPU tests of the tuple listing (kg_snapshot_query): filtered, key-ordered, paged row queries.  The
expected answer is always computed here with numpy -- filter the known rows, sort stably by key, cut the
page -- and compared exactly: rows, keys, next and matched."""
import threading

import numpy as np
import pytest

from golden_cases import Case, load
from keto_amd import _lib
from keto_amd.engine import Registry, Snapshot, row_queries
from keto_amd.mapper import Interner, SUBJECT_ID

pytestmark = pytest.mark.gpu

NS, OBJ, REL, SUBJ = _lib.KG_Q_NS, _lib.KG_Q_OBJ, _lib.KG_Q_REL, _lib.KG_Q_SUBJECT
N_NS, N_REL, N_OBJ, N_USERS = 3, 4, 150, 80
HUB = (0, 0, 1)  # (ns, obj, rel) of the node with 700 entries: more than two 256-thread workgroups
LIMITS = (1, 7, 100, 5000)


def interner():
    it = Interner()
    for i in range(N_NS):
        it.ns_id(f"n{i}")
    for i in range(N_REL):
        it.rel_id(f"r{i}")  # ids 1..4; 0 is `...`
    return it


def graph():
    """About 3,000 tuples in id space: 3 namespaces, relations 1..4, objects 0..149, users 150..229 and (the
    hub's) 1000..1599; subject ids and subject sets, `...` sets among them; duplicates; distinct random
    64-bit keys, rows in key order."""
    rng = np.random.default_rng(20260101)
    n = 2300
    t = np.zeros((n, 6), np.uint32)
    t[:, 0] = rng.integers(N_NS, size=n)
    t[:, 1] = rng.integers(N_OBJ, size=n)
    t[:, 2] = rng.integers(1, N_REL + 1, size=n)
    is_set = rng.random(n) < 0.45
    t[:, 3] = np.where(is_set, rng.integers(N_NS, size=n), SUBJECT_ID)
    t[:, 4] = np.where(is_set, rng.integers(N_OBJ, size=n), N_OBJ + rng.integers(N_USERS, size=n))
    t[:, 5] = np.where(is_set, np.where(rng.random(n) < 0.2, 0, rng.integers(1, N_REL + 1, size=n)), 0)
    hub = np.zeros((700, 6), np.uint32)
    hub[:, :3] = HUB
    hub[:600, 3], hub[:600, 4] = SUBJECT_ID, 1000 + np.arange(600)
    hub[600:, 3], hub[600:, 4], hub[600:, 5] = 1, rng.integers(N_OBJ, size=100), rng.integers(0, N_REL + 1, size=100)
    dup = t[rng.integers(n, size=50)]
    rows = np.concatenate([t, hub, dup, hub[:5]])
    rows = rows[rng.permutation(len(rows))]
    keys = np.unique(rng.integers(1, 2**64 - 1, size=len(rows) + 64, dtype=np.uint64))
    keys = np.sort(rng.permutation(keys)[:len(rows)])
    return np.ascontiguousarray(rows), keys


def expect(rows, keys, mask, t, after, limit):
    """(page rows, page keys, next, matched) of one request over the known rows."""
    m = keys > np.uint64(after)
    for bit, col in ((NS, 0), (OBJ, 1), (REL, 2)):
        if mask & bit:
            m &= rows[:, col] == t[col]
    if mask & SUBJ:
        m &= (rows[:, 3] == t[3]) & (rows[:, 4] == t[4])
        if t[3] != SUBJECT_ID:
            m &= rows[:, 5] == t[5]
    idx = np.nonzero(m)[0]
    idx = idx[np.argsort(keys[idx], kind="stable")]
    page = idx[:limit]
    return rows[page], keys[page], (int(keys[page[-1]]) if len(idx) > limit else 0), len(idx)


def cases(rows):
    """(mask, tuple) pairs: every mask with a subject-id row, a subject-set row, a `...`-set row, the hub,
    two rows' fields mixed (mostly absent), and ids larger than any in the snapshot."""
    rng = np.random.default_rng(5)
    sid = rows[rows[:, 3] == SUBJECT_ID]
    sset = rows[(rows[:, 3] != SUBJECT_ID) & (rows[:, 5] != 0)]
    wild = rows[(rows[:, 3] != SUBJECT_ID) & (rows[:, 5] == 0)]
    hub = rows[(rows[:, :3] == HUB).all(axis=1)]
    out = []
    for mask in range(16):
        a, b = sid[rng.integers(len(sid))], sset[rng.integers(len(sset))]
        mixed = a.copy()
        mixed[1], mixed[4] = b[1], sid[rng.integers(len(sid))][4]
        mixed_set = b.copy()
        mixed_set[2], mixed_set[5] = a[2], (b[5] % N_REL) + 1
        big = a.copy()
        big[1], big[4] = 5_000_000, 0x90000000
        big_set = b.copy()
        big_set[0], big_set[4] = 7, 0x7FFFFFFF
        out += [(mask, x) for x in (a, b, wild[rng.integers(len(wild))], hub[0], hub[-1], mixed, mixed_set, big, big_set)]
    return out


def run(snap, reqs, with_stats=False):
    return snap.query(reqs, with_stats=with_stats)


def check_call(snap, rows, keys, qs, afters, limits):
    """One call with a request per (mask, tuple, after, limit); every answer compared exactly."""
    reqs = row_queries([m for m, _ in qs], np.asarray([t for _, t in qs]), afters, limits)
    got_rows, got_keys, off, nxt, matched = run(snap, reqs)
    assert off[0] == 0 and off[-1] == len(got_rows) == len(got_keys)
    for i, (mask, t) in enumerate(qs):
        wr, wk, wn, wm = expect(rows, keys, mask, t, int(reqs["after"][i]), int(reqs["limit"][i]))
        lo, hi = int(off[i]), int(off[i + 1])
        what = (i, mask, t.tolist(), int(reqs["after"][i]), int(reqs["limit"][i]))
        assert int(matched[i]) == wm and int(nxt[i]) == wn, what
        assert np.array_equal(got_keys[lo:hi], wk), what
        assert np.array_equal(got_rows[lo:hi], wr), what
    return nxt, matched


def page_walk(snap, rows, keys, qs, limit=7):
    """Every query page by page, `next` fed back as `after`, all queries of a round in one call: the
    concatenation equals the one-shot answer and matched shrinks by `limit` a page."""
    live = list(range(len(qs)))
    after = np.zeros(len(qs), np.uint64)
    seen = [[] for _ in qs]
    left = [None] * len(qs)
    while live:
        sub = [qs[i] for i in live]
        reqs = row_queries([m for m, _ in sub], np.asarray([t for _, t in sub]), after[live], limit)
        got_rows, got_keys, off, nxt, matched = run(snap, reqs)
        nxt_live = []
        for j, i in enumerate(live):
            if left[i] is not None:
                assert int(matched[j]) == left[i] - limit, (i, qs[i][0])
            left[i] = int(matched[j])
            seen[i].append((got_rows[int(off[j]):int(off[j + 1])], got_keys[int(off[j]):int(off[j + 1])]))
            assert (int(nxt[j]) != 0) == (left[i] > limit)
            if nxt[j]:
                assert int(nxt[j]) == int(got_keys[int(off[j + 1]) - 1])
                after[i] = nxt[j]
                nxt_live.append(i)
        live = nxt_live
    for i, (mask, t) in enumerate(qs):
        wr, wk, wn, wm = expect(rows, keys, mask, t, 0, 1 << 30)
        assert np.array_equal(np.concatenate([k for _, k in seen[i]]), wk), (i, mask)
        assert np.array_equal(np.concatenate([r for r, _ in seen[i]]), wr), (i, mask)


@pytest.fixture(scope="module")
def keyed():
    rows, keys = graph()
    snap = Snapshot(rows, interner(), keys=keys)
    yield snap, rows, keys
    snap.close()


@pytest.fixture(scope="module")
def keyless():
    rows, _ = graph()
    snap = Snapshot(rows, interner())
    ex = snap.export()  # the order the keys i + 1 number
    assert sorted(map(tuple, ex.tolist())) == sorted(map(tuple, rows.tolist()))
    yield snap, ex, np.arange(1, len(ex) + 1, dtype=np.uint64)
    snap.close()


@pytest.fixture(params=["keyed", "keyless"])
def world(request):
    return request.getfixturevalue(request.param)


@pytest.mark.parametrize("cap", [0, 64])
def test_masks_and_limits(world, cap):
    snap, rows, keys = world
    snap.tune("query_cap", cap)
    try:
        qs = cases(rows)
        for limit in LIMITS:
            check_call(snap, rows, keys, qs, 0, limit)
        mid = int(keys[len(keys) // 2])  # and from the middle of the key range
        check_call(snap, rows, keys, qs, mid, 7)
    finally:
        snap.tune("query_cap", 0)


@pytest.mark.parametrize("cap", [0, 64])
def test_paging(world, cap):
    snap, rows, keys = world
    snap.tune("query_cap", cap)
    try:
        qs = cases(rows)
        page_walk(snap, rows, keys, qs[::3])
    finally:
        snap.tune("query_cap", 0)


def test_selection_passes(world):
    """An unfiltered first page of 7 out of ~3,000 matches.  The default list holds them all: one scan.  A
    list of 64 does not: the scan, one histogram pass and the compaction -- 11 bits split the range the
    matching keys differ in (64 bits of uniform keys; 12 bits of the keys i + 1) into 2,048 buckets of 1.5
    keys on average (2 for i + 1), so the bucket in which the count reaches 7 leaves fewer than 64 at or
    below it and no second histogram runs."""
    snap, rows, keys = world
    one = row_queries([0], np.zeros((1, 6), np.uint32), 0, 7)
    *ans, st = run(snap, one, with_stats=True)
    assert st["passes"] == 1 and st["rows_scanned"] == len(rows)
    snap.tune("query_cap", 64)
    try:
        *ans64, st64 = run(snap, one, with_stats=True)
        assert st64["passes"] == 3 and st64["rows_scanned"] == 3 * len(rows)
        for a, b in zip(ans, ans64):
            assert np.array_equal(a, b)
        # limit above / equal to the matches of a (ns, rel) query: one page, next 0, whatever the list
        t = np.asarray([[1, 0, 2, 0, 0, 0]], np.uint32)
        wm = expect(rows, keys, NS | REL, t[0], 0, 1)[3]
        assert wm > 64
        for limit in (wm, wm + 1, wm - 1):
            r, k, off, nxt, matched = run(snap, row_queries([NS | REL], t, 0, limit))
            wr, wk, wn, _ = expect(rows, keys, NS | REL, t[0], 0, limit)
            assert int(matched[0]) == wm and int(nxt[0]) == wn and (wn == 0) == (limit >= wm)
            assert np.array_equal(r, wr) and np.array_equal(k, wk)
    finally:
        snap.tune("query_cap", 0)


def test_keyless_order_is_export_order(keyless):
    snap, ex, keys = keyless
    r, k, off, nxt, matched = run(snap, row_queries([0], np.zeros((1, 6), np.uint32), 0, len(ex) + 5))
    assert np.array_equal(r, ex) and np.array_equal(k, keys) and int(nxt[0]) == 0 and int(matched[0]) == len(ex)


def test_equal_keys_come_in_position_order():
    """Keys with long runs of equal values (15 values over ~3,000 rows): equal keys come in kg_snapshot_export's
    order and a page that ends inside a run skips its rest.  With a list of 64 the key bits run out with ~200
    matches in the bucket, so the narrowing goes on over the position bits: at least two histogram passes."""
    rows, _ = graph()
    key_of = lambda r: (r[:, 1] // 10 + 1).astype(np.uint64)  # noqa: E731  (derived from the row: known after export)
    rows = rows[np.argsort(key_of(rows), kind="stable")]
    snap = Snapshot(rows, interner(), keys=key_of(rows))
    try:
        ex = snap.export()
        keys = key_of(ex)
        qs = cases(ex)[::4] + [(0, np.zeros(6, np.uint32))]
        for cap in (0, 64):
            snap.tune("query_cap", cap)
            for limit in (7, 100, 5000):
                check_call(snap, ex, keys, qs, 0, limit)
            check_call(snap, ex, keys, qs, 7, 7)
        *_, st = run(snap, row_queries([0], np.zeros((1, 6), np.uint32), 0, 7), with_stats=True)
        assert st["passes"] >= 4  # scan, a histogram over the key, one over the position, compaction
    finally:
        snap.close()


def test_fast_path_enters_the_hub_row_at_the_token(keyed):
    snap, rows, keys = keyed
    t = np.asarray([[*HUB, 0, 0, 0]], np.uint32)
    hub_keys = np.sort(keys[(rows[:, :3] == HUB).all(axis=1)])
    n_hub = len(hub_keys)
    assert n_hub >= 705
    *_, st = run(snap, row_queries([NS | OBJ | REL], t, 0, 7), with_stats=True)
    assert st["rows_scanned"] == n_hub and st["passes"] == 1
    after = int(hub_keys[400])
    r, k, off, nxt, matched, st = run(snap, row_queries([NS | OBJ | REL], t, after, 7), with_stats=True)
    # the entries after the token, not the row from its top
    assert st["rows_scanned"] == n_hub - 401 == int(matched[0])
    assert np.array_equal(k, hub_keys[401:408]) and int(nxt[0]) == int(hub_keys[407])
    # with a subject the same entries are tested
    ts = np.asarray([[*HUB, SUBJECT_ID, 1003, 0]], np.uint32)
    *_, st = run(snap, row_queries([NS | OBJ | REL | SUBJ], ts, after, 7), with_stats=True)
    assert st["rows_scanned"] == n_hub - 401


def test_refresh_merges_in_key_order():
    rows, keys = graph()
    rng = np.random.default_rng(11)
    base = Snapshot(rows, interner(), keys=keys)
    # deletes: 40 random tuples (every row equal to one goes) and every row of one small node
    node = rows[np.nonzero((rows[:, :3] != HUB).any(axis=1))[0][0], :3]
    dels = np.concatenate([rows[rng.integers(len(rows), size=40)], rows[(rows[:, :3] == node).all(axis=1)]])
    ins = rows[rng.integers(len(rows), size=120)].copy()
    ins[:60, 1] = rng.integers(N_OBJ, N_OBJ + 20, size=60)  # new objects: new nodes
    ins[60:, 4] = np.where(ins[60:, 3] == SUBJECT_ID, 3000 + np.arange(60), ins[60:, 4])
    ins = ins[~(ins[:, None, :] == dels[None, :, :]).all(axis=2).any(axis=1)]
    ins_keys = np.sort(np.setdiff1d(np.unique(rng.integers(1, 2**64 - 1, size=len(ins) + 8, dtype=np.uint64)), keys)[:len(ins)])
    new = base.apply(ins, dels, ins_keys)
    try:
        keep = ~(rows[:, None, :] == dels[None, :, :]).all(axis=2).any(axis=1)
        rows2, keys2 = np.concatenate([rows[keep], ins]), np.concatenate([keys[keep], ins_keys])
        assert not (rows2[:, :3] == node).all(axis=1).any()  # the node is empty now
        qs = cases(rows2) + [(NS | OBJ | REL, np.asarray([*node, 0, 0, 0], np.uint32)), (NS | OBJ, np.asarray([*node, 0, 0, 0], np.uint32))]
        for cap in (0, 64):
            new.tune("query_cap", cap)
            check_call(new, rows2, keys2, qs, 0, 100)
            check_call(new, rows2, keys2, qs, int(np.sort(keys2)[len(keys2) // 3]), 7)
        page_walk(new, rows2, keys2, qs[::7])
        check_call(base, rows, keys, cases(rows)[::5], 0, 100)  # the base still answers from its own rows
    finally:
        new.close()
        base.close()


@pytest.mark.parametrize("mat", [None, "0"])
def test_union_relation_lists_raw_tuples_only(mat, monkeypatch):
    """Namespace programs whose unions are materialised: the merged check rows of a union node are not
    tuples of its relation.  The same answers with materialisation off."""
    if mat is None:
        monkeypatch.delenv("KG_MATERIALIZE", raising=False)
    else:
        monkeypatch.setenv("KG_MATERIALIZE", mat)
    unions = 0
    for case in load("rewrites_test.json"):
        c = Case(case)
        reg = Registry(c.tuples, c.namespaces, interner=c.it)
        snap = reg.snapshot
        unions += snap.materialized()["union_nodes"]
        arr = c.arr
        ex = snap.export()
        assert sorted(map(tuple, ex.tolist())) == sorted(map(tuple, arr.tolist()))
        keys = np.arange(1, len(ex) + 1, dtype=np.uint64)
        qs = []
        for n in c.namespaces:
            for r in n.relations:
                t = np.asarray([c.it.ns_id(n.name), 0, c.it.rel_id(r.name), 0, 0, 0], np.uint32)
                qs.append((NS | REL, t))
                for o in sorted({x.object for x in c.tuples}):
                    t2 = t.copy()
                    t2[1] = c.it.obj_id(o)
                    qs.append((NS | OBJ | REL, t2))
        qs.append((0, np.zeros(6, np.uint32)))
        check_call(snap, ex, keys, qs, 0, 1000)
        # the raw tuples, whatever the order of the nodes: the multiset the program's tuples give
        for mask, t in qs:
            r = run(snap, row_queries([mask], t[None, :], 0, 1000))[0]
            assert sorted(map(tuple, r.tolist())) == sorted(map(tuple, expect(arr, keys, mask, t, 0, 1000)[0].tolist()))
    assert (unions > 0) == (mat is None)


def test_edge_cases(keyed):
    snap, rows, keys = keyed
    empty = Snapshot(np.zeros((0, 6), np.uint32), interner())
    try:
        for mask in (0, NS, NS | OBJ | REL, SUBJ, 15):
            r, k, off, nxt, matched = run(empty, row_queries([mask], np.zeros((1, 6), np.uint32), 0, 10))
            assert len(r) == 0 and off.tolist() == [0, 0] and nxt.tolist() == [0] and matched.tolist() == [0]
    finally:
        empty.close()
    r, k, off, nxt, matched = run(snap, np.zeros(0, _lib.ROW_QUERY_DTYPE))
    assert len(r) == 0 and off.tolist() == [0] and len(nxt) == 0 and len(matched) == 0
    with pytest.raises(_lib.KetoGPUError, match=r"\(-2\)"):
        run(snap, row_queries([0, 0], np.zeros((2, 6), np.uint32), 0, [5, 0]))
    qs = cases(rows)[10:18]  # 8 requests in one call
    assert len(qs) == 8
    check_call(snap, rows, keys, qs, 0, 7)


def test_concurrent_calls(keyed):
    snap, rows, keys = keyed
    qs = cases(rows)
    rng = np.random.default_rng(3)
    work = []
    for _ in range(4):
        pick = rng.integers(len(qs), size=50)
        work.append([row_queries([qs[i][0]], qs[i][1][None, :], int(keys[rng.integers(len(keys))]) if i % 2 else 0,
                                 int(rng.choice(LIMITS))) for i in pick])
    serial = [[run(snap, q) for q in w] for w in work]
    got = [None] * 4

    def worker(k):
        got[k] = [run(snap, q) for q in work[k]]
    ts = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for k in range(4):
        assert got[k] is not None
        for a, b in zip(got[k], serial[k]):
            for x, y in zip(a, b):
                assert np.array_equal(x, y)


# ------------------------------------------------------------------ persister and handler
def _twin_persisters():
    """A host-mode and a device-mode persister with the same seed (the same shard ids) and the same writes:
    a first build, then an incremental refresh with deletes, one of which empties an object."""
    from keto_amd.ketoapi import RelationTuple, SubjectSet
    from keto_amd.persister import SnapshotPersister
    rng = np.random.default_rng(77)

    def tup():
        ns, obj, rel = f"n{rng.integers(2)}", f"o{rng.integers(12)}", f"r{rng.integers(3)}"
        if rng.random() < 0.4:
            return RelationTuple(ns, obj, rel, subject_set=SubjectSet(f"n{rng.integers(2)}", f"o{rng.integers(12)}",
                                                                      "..." if rng.random() < 0.3 else f"r{rng.integers(3)}"))
        return RelationTuple(ns, obj, rel, subject_id=f"u{rng.integers(15)}")
    first = [tup() for _ in range(130)]
    second = [tup() for _ in range(40)] + first[:3]  # duplicates
    gone = [first[i] for i in rng.integers(len(first), size=25)] + [t for t in first if t.object == "o3"]
    ps = []
    for device_reads in (False, True):
        p = SnapshotPersister(seed=9, device_reads=device_reads)
        p.write_relation_tuples(*first)
        if device_reads:
            p.snapshot()  # the first build; what follows is applied to it
        p.transact_relation_tuples(second, gone)
        ps.append(p)
    return ps


def _persister_queries():
    from keto_amd.ketoapi import SubjectSet
    from keto_amd.persister import RelationQuery as Q
    return [Q(), Q("n0"), Q("n1", object="o1"), Q("n0", relation="r0"), Q("n0", object="o2", relation="r1"),
            Q(subject_id="u3"), Q("n0", subject_id="u3"), Q("n1", object="o4", subject_id="u1"), Q(relation="r2", subject_id="u0"),
            Q("n0", "o1", "r0", "u2"), Q(subject_set=SubjectSet("n0", "o1", "r1")), Q(subject_set=SubjectSet("n1", "o2", "...")),
            Q("n0", subject_set=SubjectSet("n0", "o5", "r0")), Q(object="o3"), Q("other"), Q(object="never"),
            Q(subject_id="nobody"), Q(subject_set=SubjectSet("n0", "o1", "unknown")), Q(subject_id="o1")]


def test_persister_device_reads_match_host_reads():
    from keto_amd.persister import MalformedPageToken, RelationQuery
    host, dev = _twin_persisters()
    n_names = len(dev.interner._obj_names), len(dev.interner._rel_names), len(dev.interner._ns_names)
    for q in _persister_queries():
        for size in (1, 3, 0):
            tok_h = tok_d = ""
            while True:
                rh, tok_h = host.get_relation_tuples(q, tok_h, size)
                rd, tok_d = dev.get_relation_tuples(q, tok_d, size)
                assert rd == rh and tok_d == tok_h, (q, size)
                if not tok_h:
                    break
    assert dev.rebuilds == 1 and dev.applies == 1 and host.rebuilds == 0  # the refreshed snapshot answered
    assert n_names == (len(dev.interner._obj_names), len(dev.interner._rel_names), len(dev.interner._ns_names))
    with pytest.raises(MalformedPageToken):
        dev.get_relation_tuples(_persister_queries()[0], page_token="not-a-uuid")
    # a read sees every committed write
    from keto_amd.ketoapi import RelationTuple
    t = RelationTuple("n0", "fresh", "r0", subject_id="u1")
    for p in (host, dev):
        p.write_relation_tuples(t)
    q = RelationQuery(object="fresh")
    assert dev.get_relation_tuples(q) == host.get_relation_tuples(q) == ([t], "")


def test_handler_over_device_reads_returns_the_same_json():
    from keto_amd.handlers import RelationTuplesHandler
    host, dev = _twin_persisters()
    hh, hd = RelationTuplesHandler(host, host.mapper), RelationTuplesHandler(dev, dev.mapper)
    for query in ("", "namespace=n0", "namespace=n1&object=o1", "subject_id=u3", "relation=r2&subject_id=u0",
                  "subject_set.namespace=n0&subject_set.object=o1&subject_set.relation=r1", "object=never",
                  "page_size=foo", "page_token=zzz", "subject=u1"):
        for size in ("", "&page_size=4"):
            token = ""
            while True:
                url = query + size + (f"&page_token={token}" if token else "")
                a, b = hh.get_relations(url), hd.get_relations(url)
                assert a == b, url
                token = a[1].get("next_page_token", "") if a[0] == 200 else ""
                if not token:
                    break
    for req in ({"relation_query": {"namespace": "n0", "subject": {"id": "u3"}}, "page_size": 2},
                {"query": {"namespace": "n1", "object": ""}}, {"relation_query": {}}):
        assert hh.grpc_list_relation_tuples(req) == hd.grpc_list_relation_tuples(req)
