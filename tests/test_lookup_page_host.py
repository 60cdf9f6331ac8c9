"""Host tests of the paged lookups (no GPU): the ctypes structs against include/ketogpu.h, the argument
checks the C ABI makes before it touches a snapshot, and the handlers' order=id page parsing."""
import ctypes as C
import os

import numpy as np
import pytest

from header_probe import probe
from keto_amd import _lib
from keto_amd.handlers import HandlerError, ListObjectsHandler, ListSubjectsHandler, parse_id_page

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_page_struct_layout_matches_header():
    fields_p = ("list", "next", "rounds", "pinned")
    got = probe(["sizeof(kg_lookup_page)", "sizeof(kg_lookup_pages)", "sizeof(kg_lookup_buf)", "KG_LOOKUP_END"] +
                [f"offsetof(kg_lookup_pages, {f})" for f in fields_p] +
                ["offsetof(kg_lookup_page, from)", "offsetof(kg_lookup_page, limit)"])
    P, S = _lib.kg_lookup_page, _lib.kg_lookup_pages
    want = [C.sizeof(P), C.sizeof(S), C.sizeof(_lib.kg_lookup_buf), _lib.KG_LOOKUP_END] + \
        [getattr(S, f).offset for f in fields_p] + [P.from_.offset, P.limit.offset]
    assert got == want
    assert got[0] == 8 and got[1] == got[2] + 24 and got[3] == 0xFFFFFFFF
    # the (n, 2) uint32 array the Python callers pass is an array of kg_lookup_page
    assert np.dtype(np.uint32).itemsize * 2 == C.sizeof(P)


def test_page_symbols_exported():
    with open(os.path.join(ROOT, "include", "ketogpu.h")) as f:
        hdr = f.read()
    L = _lib.load()
    for name in ("kg_lookup_objects_page", "kg_lookup_subjects_page", "kg_lookup_pages_free"):
        assert name in hdr and name in _lib.EXPORTS
        assert getattr(L, name) is not None


@pytest.mark.parametrize("call,width", [("kg_lookup_objects_page", 6), ("kg_lookup_subjects_page", 4)])
def test_argument_checks_come_before_the_snapshot(call, width):
    """limit == 0 is -2, whichever request has it; so are a missing pages array and a missing snapshot."""
    L = _lib.load()
    fn = getattr(L, call)
    reqs = np.zeros((3, width), np.uint32)
    out = _lib.kg_lookup_pages()
    for bad in range(3):
        pages = np.asarray([[0, 5], [7, 1], [0, 0xFFFFFFFF]], np.uint32)
        pages[bad, 1] = 0
        assert fn(None, reqs.ctypes.data, pages.ctypes.data, 3, 5, C.byref(out)) == -2
        assert f"page {bad} has limit 0" in _lib.last_error()
        assert not out.next and not out.list.req_off and out.rounds == 0
    pages = np.asarray([[0, 5], [7, 1], [0, 0xFFFFFFFF]], np.uint32)
    assert fn(None, reqs.ctypes.data, None, 3, 5, C.byref(out)) == -2 and "pages is NULL" in _lib.last_error()
    assert fn(None, reqs.ctypes.data, pages.ctypes.data, 3, 5, C.byref(out)) == -2  # no snapshot
    assert fn(None, reqs.ctypes.data, pages.ctypes.data, 3, 5, None) == -2
    L.kg_lookup_pages_free(C.byref(out))  # an empty buffer may be freed
    L.kg_lookup_pages_free(None)


def test_parse_id_page():
    assert parse_id_page("", "garbage", 0) is None  # no order: the name-ordered paging parses its own token
    assert parse_id_page("id", "", 100) == (0, 100)
    assert parse_id_page("id", "0", 1) == (0, 1)
    assert parse_id_page("id", "4294967295", 4294967295) == (0xFFFFFFFF, 0xFFFFFFFF)
    for order, token, size in (("id", "-1", 5), ("id", "1.5", 5), ("id", "x", 5), ("id", "4294967296", 5), ("id", "+3", 5),
                               ("id", " 3", 5), ("id", "3", 0), ("id", "3", -1), ("id", "3", 4294967296),
                               ("name", "", 5), ("ID", "", 5), ("id", "٣", 5)):
        with pytest.raises(HandlerError) as e:
            parse_id_page(order, token, size)
        assert e.value.status == 400 and e.value.message == "malformed page_token or page_size", (order, token, size)


class _Mapper:
    def check_namespace(self, name):
        pass


class _Engine:
    """Records the paged calls; the unpaged methods must not be reached with order=id."""

    def __init__(self):
        self.calls = []

    def lookup_objects_page(self, *a):
        self.calls.append(("objects",) + a)
        return ["b", "a"], 17

    def lookup_subjects_page(self, *a):
        self.calls.append(("subjects",) + a)
        return ["z"], None


def test_handlers_pass_the_page_through():
    e = _Engine()
    ho, hs = ListObjectsHandler(e, _Mapper()), ListSubjectsHandler(e, _Mapper())
    status, body = ho.get_list_objects("namespace=n&relation=r&subject_id=u&order=id&page_size=2&page_token=9&max-depth=3")
    assert status == 200 and body == {"objects": ["b", "a"], "next_page_token": "17"}  # id order: not sorted by name
    assert e.calls[-1] == ("objects", "n", "r", "u", 3, 9, 2)
    assert ho.grpc_list_objects({"namespace": "n", "relation": "r", "subject": {"id": "u"}, "order": "id"}) == \
        {"objects": ["b", "a"], "next_page_token": "17"}
    assert e.calls[-1] == ("objects", "n", "r", "u", 0, 0, ListObjectsHandler.DEFAULT_PAGE_SIZE)
    status, body = hs.get_list_subjects("namespace=n&object=o&relation=r&order=id")
    assert status == 200 and body == {"subject_ids": ["z"], "next_page_token": ""}
    assert e.calls[-1] == ("subjects", "n", "o", "r", 0, 0, ListSubjectsHandler.DEFAULT_PAGE_SIZE)
    assert hs.grpc_list_subjects({"namespace": "n", "object": "o", "relation": "r", "order": "id", "page_token": "4",
                                  "page_size": 3}) == {"subject_ids": ["z"], "next_page_token": ""}
    assert e.calls[-1] == ("subjects", "n", "o", "r", 0, 4, 3)
    n = len(e.calls)
    for q in ("order=id&page_token=x", "order=id&page_token=-2", "order=id&page_size=0", "order=id&page_size=q",
              "order=name"):
        status, body = ho.get_list_objects("namespace=n&relation=r&subject_id=u&" + q)
        assert status == 400 and body["error"]["code"] == 400, q
        status, body = hs.get_list_subjects("namespace=n&object=o&relation=r&" + q)
        assert status == 400 and body["error"]["code"] == 400, q
    with pytest.raises(HandlerError) as x:
        ho.grpc_list_objects({"namespace": "n", "relation": "r", "subject": {"id": "u"}, "order": "id", "page_token": "zz"})
    assert x.value.status == 400
    assert len(e.calls) == n  # a malformed page never reaches the engine
