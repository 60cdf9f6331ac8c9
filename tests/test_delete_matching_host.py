"""Delete by query (kg_snapshot_delete_matching, DELETE /admin/relation-tuples, DeleteRelationTuples), the parts
that need no GPU: the ABI (exports, struct layout against the header, refusals before any launch),
tests/delete_ref.py against RelationQuery.matches and the host persister's delete_all_relation_tuples, and the
handlers over the host-mode persister (a restatement of the two REST delete cases of the reference's
internal/relationtuple/transact_server_test.go, their inputs in tests/golden/transact_server_cases.json)."""
import ctypes as C
import os

import numpy as np
import pytest

from delete_ref import Q_NS, Q_OBJ, Q_REL, Q_SUBJECT, delete_ref
from golden_cases import load
from keto_amd.handlers import HandlerError, RelationTuplesHandler
from keto_amd.ketoapi import RelationTuple, SubjectSet
from keto_amd.namespace import Namespace
from keto_amd.persister import RelationQuery, SnapshotPersister

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = load("transact_server_cases.json")


# ------------------------------------------------------------------ ABI
def test_delete_symbols_exported():
    from keto_amd import _lib
    with open(os.path.join(ROOT, "include", "ketogpu.h")) as f:
        hdr = f.read()
    L = _lib.load()
    for name in ("kg_snapshot_delete_matching", "kg_delete_free"):
        assert name in _lib.EXPORTS and name + "(" in hdr
        assert hasattr(L, name), name
    assert L.kg_snapshot_delete_matching.argtypes is not None and len(L.kg_snapshot_delete_matching.argtypes) == 8
    assert L.kg_snapshot_delete_matching.restype is C.c_int and L.kg_delete_free.restype is None
    assert "relationtuples.go:146-162,187-201" in hdr  # the reference lines, as the other entries name theirs


def test_delete_struct_layout_matches_header():
    from header_probe import probe
    from keto_amd import _lib
    fields = ("matched", "keys", "n_queries", "n_deleted", "rows_scanned", "kernel_ms", "pinned")
    got = probe(["sizeof(kg_delete_buf)", "KG_DELETE_MAX_QUERIES", "KG_DELETE_KEYS"] +
                [f"offsetof(kg_delete_buf, {f})" for f in fields])
    B = _lib.kg_delete_buf
    want = [C.sizeof(B), _lib.KG_DELETE_MAX_QUERIES, _lib.KG_DELETE_KEYS] + [getattr(B, f).offset for f in fields]
    assert got == want
    assert got[:3] == [56, 64, 1]


def test_delete_refusals_need_no_gpu():
    """Every refusal comes before the handle is looked at (a fake one is never dereferenced) and before any
    launch: -2 and a message."""
    from keto_amd import _lib
    L = _lib.load()
    buf = _lib.kg_delete_buf()
    reqs = (_lib.kg_row_query * 65)()
    out = C.c_void_p()
    fake = C.c_void_p(0x1000)
    q, o, b = C.byref(reqs), C.byref(out), C.byref(buf)
    for args, word in (((None, q, 1, 0, None, None, o, b), "NULL"),
                       ((fake, q, 1, 0, None, None, None, b), "NULL"),
                       ((fake, q, 1, 0, None, None, o, None), "NULL"),
                       ((fake, None, 1, 0, None, None, o, b), "NULL"),
                       ((fake, q, 65, 0, None, None, o, b), "at most 64"),
                       ((fake, q, 1, 2, None, None, o, b), "flag"),
                       ((fake, q, 1, 0x80000001, None, None, o, b), "flag")):
        out.value = 0x2000
        assert L.kg_snapshot_delete_matching(*args) == -2, word
        assert word in _lib.last_error(), (word, _lib.last_error())
        if args[6] is not None and args[0] is not None and args[7] is not None:
            assert out.value is None  # *out is NULL after a refusal
    L.kg_delete_free(None)
    L.kg_delete_free(C.byref(_lib.kg_delete_buf()))  # an empty buffer: nothing to return


# ------------------------------------------------------------------ delete_ref against the host persister
def _random_tuples(rng, n):
    out = []
    for _ in range(n):
        ns, obj, rel = f"n{rng.integers(2)}", f"o{rng.integers(6)}", f"r{rng.integers(3)}"
        if rng.random() < 0.45:
            srel = "..." if rng.random() < 0.3 else f"r{rng.integers(3)}"
            out.append(RelationTuple(ns, obj, rel, subject_set=SubjectSet(f"n{rng.integers(2)}", f"o{rng.integers(6)}", srel)))
        else:  # u* and o* subject ids: an id spelled like an object is still a subject id
            out.append(RelationTuple(ns, obj, rel, subject_id=f"u{rng.integers(5)}" if rng.random() < 0.8 else f"o{rng.integers(6)}"))
    return out + [out[i] for i in rng.integers(n, size=n // 4)]  # duplicates


def _persister(tuples):
    p = SnapshotPersister(seed=11)
    p.write_relation_tuples(*tuples)
    return p


def _rows_keys(p):
    rows = p.interner.tuples_array(t for _, t in p._rows)
    keys = np.fromiter((p._key(sid.int) for sid, _ in p._rows), np.uint64, len(p._rows))
    return rows, keys


def _query_for(mask, t: RelationTuple, subject_set):
    sid = sset = None
    if mask & Q_SUBJECT:
        if subject_set is not None:
            sset = subject_set
        else:
            sid = t.subject_id if t.subject_id is not None else t.subject_set.object
    return RelationQuery(t.namespace if mask & Q_NS else None, t.object if mask & Q_OBJ else None,
                         t.relation if mask & Q_REL else None, sid, sset)


@pytest.mark.parametrize("mask", range(16))
def test_delete_ref_equals_matches_and_host_delete_all(mask):
    """All 16 field combinations, with the fields of a subject-id row, of a subject-set row, of a `...`-set row
    and of two rows mixed: delete_ref's kept rows, keys, deleted keys and count equal what RelationQuery.matches
    says row by row and what the host persister is left with."""
    rng = np.random.default_rng(300 + mask)
    tuples = _random_tuples(rng, 90)
    ids = [t for t in tuples if t.subject_id is not None]
    sets = [t for t in tuples if t.subject_set is not None and t.subject_set.relation != "..."]
    wild = [t for t in tuples if t.subject_set is not None and t.subject_set.relation == "..."]
    a, b, w = ids[0], sets[0], wild[0]
    mixed = RelationTuple(a.namespace, b.object, a.relation, subject_id=ids[-1].subject_id)
    picks = [(a, None), (b, b.subject_set), (w, w.subject_set), (mixed, None), (mixed, sets[-1].subject_set),
             (b, None)]  # (b, None): a subject-set row's object name asked for as a subject id
    hits = 0
    for t, sset in picks:
        p = _persister(tuples)
        rows, keys = _rows_keys(p)
        q = _query_for(mask, t, sset)
        want_gone = np.asarray([q.matches(x) for _, x in p._rows], bool)
        got = p._query_ids(q)
        assert got is not None  # every string here is one some tuple has
        assert got[0] == mask
        kept, kept_keys, dead_keys, matched = delete_ref(rows, keys, [got])
        assert int(matched[0]) == int(want_gone.sum())
        assert np.array_equal(kept, rows[~want_gone]) and np.array_equal(kept_keys, keys[~want_gone])
        assert np.array_equal(dead_keys, np.sort(keys[want_gone]))
        p.delete_all_relation_tuples(q)
        left, left_keys = _rows_keys(p)
        assert np.array_equal(left, kept) and np.array_equal(left_keys, kept_keys) and len(p) == len(kept)
        # the same rows without keys: the deleted keys are positions + 1
        kept2, none, dead_pos, matched2 = delete_ref(rows, None, [got])
        assert none is None and np.array_equal(kept2, kept) and np.array_equal(dead_pos, np.nonzero(want_gone)[0] + 1)
        assert matched2[0] == matched[0]
        hits += int(want_gone.sum())
    assert hits > 0
    if mask == 0:
        assert len(kept) == 0  # no field: every row


def test_delete_ref_counts_rows_once_and_queries_each():
    rows = np.asarray([[0, 1, 1, 0xFFFFFFFF, 7, 0], [0, 1, 1, 0xFFFFFFFF, 7, 0], [0, 2, 1, 0, 1, 1], [1, 1, 2, 0, 1, 0],
                       [0, 7, 1, 0xFFFFFFFF, 1, 0]], np.uint32)
    keys = np.asarray([5, 5, 9, 11, 30], np.uint64)
    qs = [(Q_NS, (0, 0, 0, 0, 0, 0)), (Q_SUBJECT, (0, 0, 0, 0xFFFFFFFF, 7, 0)), (Q_SUBJECT, (9, 9, 9, 0, 1, 1)),
          (Q_SUBJECT, (0, 0, 0, 0xFFFFFFFF, 1, 0)), (Q_OBJ | Q_REL, (5, 1, 2, 0, 0, 0)), (Q_SUBJECT, (0, 0, 0, 0, 7, 0))]
    kept, kk, dead, matched = delete_ref(rows, keys, qs[:2])
    assert matched.tolist() == [4, 2] and dead.tolist() == [5, 5, 9, 30] and kk.tolist() == [11]
    assert delete_ref(rows, keys, qs[2:3])[3].tolist() == [1]      # the set (0, 1, 1), not the id 1
    assert delete_ref(rows, keys, qs[3:4])[2].tolist() == [30]     # the id 1, not the sets naming object 1
    assert delete_ref(rows, keys, qs[4:5])[2].tolist() == [11]
    assert delete_ref(rows, keys, qs[5:6])[3].tolist() == [0]      # a set (0, 7, 0): no such row, the id 7 rows stay
    assert delete_ref(rows, keys, [])[0].shape == (5, 6)


# ------------------------------------------------------------------ handlers over the host-mode persister
def handler(tuples=(), namespaces=("ns",), **kw):
    p = SnapshotPersister([Namespace(n) for n in namespaces], seed=5, **kw)
    p.write_relation_tuples(*[RelationTuple.from_json(t) if isinstance(t, dict) else t for t in tuples])
    return RelationTuplesHandler(p, p.mapper), p


@pytest.mark.parametrize("case", GOLDEN["delete"], ids=lambda c: c["name"])
def test_rest_delete_cases_of_the_reference(case):
    h, p = handler(case["tuples"])
    assert len(p) == len(case["tuples"])
    assert h.delete_relations(case["query"]) == (case["status"], None)
    left, token = p.get_relation_tuples(RelationQuery(**case["list"]), page_size=case["page_size"])
    assert [t.to_json() for t in left] == case["left"] and token == ""
    assert len(p) == 0


def test_rest_delete_queries_and_errors():
    a = RelationTuple("ns", "o", "r", subject_id="x")
    b = RelationTuple("ns", "o", "r", subject_set=SubjectSet("ns", "x", "r"))
    c = RelationTuple("ns", "o2", "r2", subject_id="y")
    s = "subject_set.namespace=ns&subject_set.object=x&subject_set.relation=r"
    h, p = handler([a, a, b, c])
    # request errors change nothing: 400 on a bad subject form, 404 for a namespace that is not configured
    for q in ("subject_id=x&" + s, "subject_set.namespace=ns", "subject=x"):
        status, body = h.delete_relations(q)
        assert status == 400 and body["error"]["code"] == 400, q
    for q in ("namespace=unknown", "subject_set.namespace=unknown&subject_set.object=x&subject_set.relation=r"):
        status, body = h.delete_relations(q)
        assert status == 404 and body["error"]["code"] == 404, q
    assert len(p) == 4
    assert h.delete_relations("object=none") == (204, None) and len(p) == 4  # nothing matches: still 204
    assert h.delete_relations("subject_id=x") == (204, None)  # both copies of a, not the set naming x
    assert sorted(map(str, p.get_relation_tuples(RelationQuery())[0])) == sorted(map(str, [b, c]))
    assert h.delete_relations(s) == (204, None) and p.get_relation_tuples(RelationQuery())[0] == [c]
    assert h.delete_relations({"relation": "r"}) == (204, None) and len(p) == 1  # a mapping as url.Values
    h2, p2 = handler([a, a, b, c])
    assert h2.delete_relations("") == (204, None)  # an empty query: everything
    assert len(p2) == 0 and h2.get_relations("")[1] == {"relation_tuples": [], "next_page_token": ""}


@pytest.mark.parametrize("form", ["relation_query", "query"])
def test_grpc_delete_request_forms(form):
    a = RelationTuple("ns", "o1", "r1", subject_id="s1")
    b = RelationTuple("ns", "o2", "r1", subject_set=SubjectSet("ns", "o1", "r1"))
    c = RelationTuple("ns", "o3", "r2", subject_id="s1")
    h, p = handler([a, b, c])
    assert h.grpc_delete_relation_tuples({form: {"object": "nope"}}) == {} and len(p) == 3
    assert h.grpc_delete_relation_tuples({form: {"subject": {"set": {"namespace": "ns", "object": "o1", "relation": "r1"}}}}) == {}
    assert sorted(map(str, p.get_relation_tuples(RelationQuery())[0])) == sorted(map(str, [a, c]))
    # the deprecated query's empty strings mean unset; the relation query's are filters
    assert h.grpc_delete_relation_tuples({form: {"namespace": "ns", "object": "", "relation": "r2"}}) == {}
    assert len(p) == (1 if form == "query" else 2)
    assert h.grpc_delete_relation_tuples({form: {"subject": {"id": "s1"}}}) == {} and len(p) == 0
    with pytest.raises(HandlerError) as e:
        h.grpc_delete_relation_tuples({form: {"namespace": "unknown"}})
    assert e.value.status == 404 and e.value.grpc_code == 5


def test_grpc_delete_needs_a_query():
    h, p = handler([RelationTuple("ns", "o", "r", subject_id="x")])
    with pytest.raises(HandlerError) as e:
        h.grpc_delete_relation_tuples({})
    assert e.value.status == 400 and e.value.message == "invalid request" and e.value.grpc_code == 3
    assert len(p) == 1


def test_device_deletes_is_off_by_default_and_a_host_delete_builds_no_snapshot():
    h, p = handler([RelationTuple("ns", "o", "r", subject_id="x"), RelationTuple("ns", "o2", "r", subject_id="x")])
    assert p.device_deletes is False and SnapshotPersister().device_deletes is False
    assert h.delete_relations("object=o")[0] == 204 and len(p) == 1
    p.delete_all_relation_tuples(RelationQuery(subject_id="x"))
    assert len(p) == 0
    assert p._snap is None and p.rebuilds == 0 and p.applies == 0 and p.device_deletes_done == 0
