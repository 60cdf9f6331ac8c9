"""Tuple listing (kg_snapshot_query, GET /relation-tuples, ListRelationTuples), the parts that need no GPU:
RelationTuplesHandler over the host-mode persister (a restatement of the reference's
internal/relationtuple/read_server_test.go, its concrete cases in tests/golden/read_server_cases.json), the
ABI struct layout against the header, and the exports."""
import ctypes as C
import json
import os
import uuid

import pytest

from golden_cases import load
from keto_amd.handlers import HandlerError, RelationTuplesHandler
from keto_amd.ketoapi import RelationTuple, SubjectSet
from keto_amd.namespace import Namespace
from keto_amd.persister import RelationQuery, SnapshotPersister

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = load("read_server_cases.json")


def handler(tuples=(), namespaces=("ns",), **kw):
    p = SnapshotPersister([Namespace(n) for n in namespaces], seed=5, **kw)
    p.write_relation_tuples(*[RelationTuple.from_json(t) if isinstance(t, dict) else t for t in tuples])
    return RelationTuplesHandler(p, p.mapper), p


def as_set(body):
    return sorted(json.dumps(t, sort_keys=True) for t in body["relation_tuples"])


@pytest.mark.parametrize("case", GOLDEN["rest"], ids=lambda c: c["name"])
def test_rest_cases_of_the_reference(case):
    h, _ = handler(case["tuples"])
    status, body = h.get_relations(case["query"])
    assert status == case["status"]
    if "body" in case:
        assert body == case["body"]
    if case.get("all"):
        assert as_set(body) == sorted(json.dumps(t, sort_keys=True) for t in case["tuples"])
        assert body["next_page_token"] == case["next_page_token"]
    if "contains" in case:
        assert case["contains"] in json.dumps(body)
    if status != 200:
        assert body["error"]["code"] == status


def test_rest_paginates():
    g = GOLDEN["paginates"]
    h, _ = handler(g["tuples"])
    seen, token = [], ""
    for want in g["pages"]:
        q = f"namespace={g['query']['namespace']}&page_size={g['page_size']}" + (f"&page_token={token}" if token else "")
        status, body = h.get_relations(q)
        assert status == 200 and len(body["relation_tuples"]) == want
        seen += body["relation_tuples"]
        token = body["next_page_token"]
        if token:
            uuid.UUID(token)
    assert token == ""
    assert sorted(json.dumps(t, sort_keys=True) for t in seen) == sorted(json.dumps(t, sort_keys=True) for t in g["tuples"])


def test_query_parsing_and_both_subject_forms():
    a = RelationTuple("ns", "o", "r", subject_id="x")
    b = RelationTuple("ns", "o", "r", subject_set=SubjectSet("ns", "x", "r"))
    c = RelationTuple("ns", "o2", "r2", subject_id="y")
    h, _ = handler([a, a, b, c])
    get = lambda q: h.get_relations(q)  # noqa: E731
    assert get("")[1]["relation_tuples"] == [t.to_json() for t in h.manager.get_relation_tuples(RelationQuery())[0]]
    assert len(get("")[1]["relation_tuples"]) == 4
    assert get("subject_id=x")[1]["relation_tuples"] == [a.to_json(), a.to_json()]  # subject-id rows only
    s = "subject_set.namespace=ns&subject_set.object=x&subject_set.relation=r"
    assert get(s)[1]["relation_tuples"] == [b.to_json()]  # subject-set rows only
    assert get("namespace=ns&object=o2&relation=r2&subject_id=y")[1]["relation_tuples"] == [c.to_json()]
    assert get({"relation": "r2"})[1]["relation_tuples"] == [c.to_json()]  # a mapping as url.Values
    assert get("relation=")[1] == {"relation_tuples": [], "next_page_token": ""}  # present and empty: a filter
    assert get("object=none")[1] == {"relation_tuples": [], "next_page_token": ""}
    # request errors: 400 with the messages of the check handler's subject decoding
    assert get("subject_id=x&" + s)[0] == 400
    assert get("subject_set.namespace=ns")[0] == 400
    assert get("subject=x")[0] == 400
    # namespaces as Mapper.FromQuery: one that is named must be configured
    assert get("namespace=unknown")[0] == 404
    assert get("subject_set.namespace=unknown&subject_set.object=x&subject_set.relation=r")[0] == 404


def test_page_size_and_token_errors():
    h, _ = handler([RelationTuple("ns", "o", "r", subject_id=f"u{i}") for i in range(5)])
    for bad in ("foo", "1.5", "1_0"):
        status, body = h.get_relations(f"page_size={bad}")
        assert status == 400 and "invalid syntax" in body["error"]["message"] and bad in body["error"]["message"]
    status, body = h.get_relations("page_size=0x2")  # strconv.ParseInt base 0
    assert status == 200 and len(body["relation_tuples"]) == 2 and body["next_page_token"]
    status, body = h.get_relations("page_size=")  # empty: the default size
    assert status == 200 and len(body["relation_tuples"]) == 5
    status, body = h.get_relations("page_token=not-a-uuid")
    assert status == 500 and body["error"]["message"] == "malformed page token"
    with pytest.raises(HandlerError) as e:
        h.grpc_list_relation_tuples({"relation_query": {}, "page_token": "zzz"})
    assert e.value.status == 500


@pytest.mark.parametrize("form", ["relation_query", "query"])
def test_grpc_request_forms(form):
    g = GOLDEN["grpc_gets"]
    h, _ = handler(g["tuples"])
    assert h.grpc_list_relation_tuples({form: {"object": "nope"}}) == {"relation_tuples": [], "next_page_token": ""}
    resp = h.grpc_list_relation_tuples({form: dict(g["query"])})
    want = [{"namespace": t["namespace"], "object": t["object"], "relation": t["relation"],
             "subject": {"id": t["subject_id"]} if "subject_id" in t else {"set": t["subject_set"]}} for t in g["tuples"]]
    key = lambda d: json.dumps(d, sort_keys=True)  # noqa: E731
    assert sorted(map(key, resp["relation_tuples"])) == sorted(map(key, want)) and resp["next_page_token"] == ""
    # a subject in the query, both kinds
    r = h.grpc_list_relation_tuples({form: {"subject": {"id": "s1"}}})
    assert [t["object"] for t in r["relation_tuples"]] == ["o1"]
    r = h.grpc_list_relation_tuples({form: {"subject": {"set": {"namespace": "ns", "object": "o1", "relation": "r1"}}}})
    assert [t["object"] for t in r["relation_tuples"]] == ["o2"]
    # the deprecated query's empty strings mean unset; the relation query's are filters
    r = h.grpc_list_relation_tuples({form: {"namespace": "ns", "object": "", "relation": ""}})
    assert len(r["relation_tuples"]) == (2 if form == "query" else 0)
    # paging
    p = GOLDEN["paginates"]
    h2, _ = handler(p["tuples"])
    first = h2.grpc_list_relation_tuples({form: dict(p["query"]), "page_size": p["page_size"]})
    second = h2.grpc_list_relation_tuples({form: dict(p["query"]), "page_size": p["page_size"],
                                           "page_token": first["next_page_token"]})
    assert [len(first["relation_tuples"]), len(second["relation_tuples"])] == p["pages"]
    assert first["next_page_token"] and second["next_page_token"] == ""
    with pytest.raises(HandlerError) as e:
        h.grpc_list_relation_tuples({form: {"namespace": "unknown"}})
    assert e.value.status == 404 and e.value.grpc_code == 5


def test_grpc_needs_a_query():
    h, _ = handler()
    with pytest.raises(HandlerError) as e:
        h.grpc_list_relation_tuples({"page_size": 3})
    assert e.value.status == 400 and e.value.message == "you must provide a query" and e.value.grpc_code == 3


def test_device_reads_is_off_by_default_and_host_reads_build_no_snapshot():
    h, p = handler([RelationTuple("ns", "o", "r", subject_id="x")])
    assert p.device_reads is False
    assert h.get_relations("namespace=ns")[0] == 200
    assert p._snap is None and p.rebuilds == 0  # the host path never touches the device


def test_query_struct_layout_matches_header():
    from header_probe import probe
    from keto_amd import _lib
    fields_q = ("mask", "t", "after", "limit")
    fields_b = ("req_off", "rows", "keys", "next", "matched", "n_reqs", "n_rows", "rows_scanned", "passes", "kernel_ms",
                "pinned")
    got = probe(["sizeof(kg_row_query)", "sizeof(kg_query_buf)", "KG_Q_NS", "KG_Q_OBJ", "KG_Q_REL", "KG_Q_SUBJECT"] +
                [f"offsetof(kg_row_query, {f})" for f in fields_q] + [f"offsetof(kg_query_buf, {f})" for f in fields_b])
    Q, B = _lib.kg_row_query, _lib.kg_query_buf
    want = [C.sizeof(Q), C.sizeof(B), _lib.KG_Q_NS, _lib.KG_Q_OBJ, _lib.KG_Q_REL, _lib.KG_Q_SUBJECT] + \
        [getattr(Q, f).offset for f in fields_q] + [getattr(B, f).offset for f in fields_b]
    assert got == want
    assert got[0] == 48 and got[1] == 88
    # the numpy record the Python callers fill is the same struct
    D = _lib.ROW_QUERY_DTYPE
    assert D.itemsize == 48 and [D.fields[f][1] for f in fields_q] == [getattr(Q, f).offset for f in fields_q]


def test_query_symbols_exported():
    from keto_amd import _lib
    with open(os.path.join(ROOT, "include", "ketogpu.h")) as f:
        hdr = f.read()
    L = _lib.load()
    for name in ("kg_snapshot_query", "kg_query_free"):
        assert name in _lib.EXPORTS and name + "(" in hdr
        assert hasattr(L, name), name
    assert L.kg_snapshot_query.argtypes is not None and L.kg_query_free.restype is None


def test_query_null_arguments():
    from keto_amd import _lib
    L = _lib.load()
    buf = _lib.kg_query_buf()
    req = _lib.kg_row_query()
    fake = C.c_void_p(0x1000)  # never dereferenced: the arguments are checked first
    for args in ((None, C.byref(req), 1, C.byref(buf)), (fake, C.byref(req), 1, None), (fake, None, 1, C.byref(buf))):
        assert L.kg_snapshot_query(*args) == -2
        assert "NULL" in _lib.last_error()
    L.kg_query_free(None)
    L.kg_query_free(C.byref(buf))  # an empty buffer: nothing to return
