"""Subject-set lookup (kg_lookup_subject_sets, kg_lookup_subject_sets_page), the parts that need no GPU: the
exports, argument checks that fail before a device is touched, the ABI struct layout against the header, and
the handler's decoding of the subject-set filter."""
import ctypes as C

import pytest


def test_symbols_exported():
    from keto_amd import _lib
    L = _lib.load()
    for name in ("kg_lookup_subject_sets", "kg_lookup_subject_sets_page"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name)


def test_null_arguments():
    from keto_amd import _lib
    L = _lib.load()
    req = (C.c_uint32 * 6)(0, 0, 0, 0, 0, 0)
    fake = C.c_void_p(0x1000)  # never dereferenced: the arguments are checked first
    buf = _lib.kg_lookup_buf()
    want = []
    for args in ((None, req, 1, 5, C.byref(buf)), (fake, req, 1, 5, None), (fake, None, 1, 5, C.byref(buf))):
        rc = L.kg_lookup_subject_sets(*args)
        assert rc != 0 and "NULL" in _lib.last_error()
        want.append(rc)
        four = None if args[1] is None else (C.c_uint32 * 4)(0, 0, 0, 0)
        assert L.kg_lookup_subjects(args[0], four, *args[2:]) == rc  # the code kg_lookup_subjects uses
    L.kg_lookup_free(C.byref(buf))  # an empty buffer: nothing to return
    out = _lib.kg_lookup_pages()
    page = (C.c_uint32 * 2)(0, 1)
    for args in ((None, req, page, 1, 5, C.byref(out)), (fake, req, page, 1, 5, None), (fake, None, page, 1, 5, C.byref(out)),
                 (fake, req, None, 1, 5, C.byref(out))):
        assert L.kg_lookup_subject_sets_page(*args) == want[0]
        assert "NULL" in _lib.last_error()
    assert L.kg_lookup_subject_sets_page(fake, req, (C.c_uint32 * 2)(0, 0), 1, 5, C.byref(out)) == -2
    assert "limit 0" in _lib.last_error()
    L.kg_lookup_pages_free(C.byref(out))


def test_struct_layout_matches_header():
    from header_probe import probe
    from keto_amd import _lib
    S = _lib.kg_lookup_subj_set
    fields = [f for f, _ in S._fields_]
    assert fields == ["ns", "obj", "rel", "sns", "srel", "max_depth"]
    got = probe(["sizeof(kg_lookup_subj_set)", "sizeof(kg_lookup_buf)", "sizeof(kg_lookup_pages)", "KG_SUBJECT_ID"] +
                [f"offsetof(kg_lookup_subj_set, {f})" for f in fields])
    assert C.sizeof(S) == 24
    assert got == [24, C.sizeof(_lib.kg_lookup_buf), C.sizeof(_lib.kg_lookup_pages), _lib.KG_SUBJECT_ID] + \
        [getattr(S, f).offset for f in fields]


class _NoEngine:
    """The request is rejected before the engine is asked."""

    def __getattr__(self, name):
        raise AssertionError("engine reached")


class _Recorder:
    """An engine that records the call and answers with two names."""

    def __init__(self):
        self.calls = []

    def lookup_subjects(self, *a):
        self.calls.append(("lookup_subjects",) + a)
        return ["a", "b"]

    def lookup_subjects_page(self, *a):
        self.calls.append(("lookup_subjects_page",) + a)
        return ["a", "b"], 7


def _handler(engine):
    from keto_amd.handlers import ListSubjectsHandler
    from keto_amd.mapper import Interner, Mapper
    return ListSubjectsHandler(engine, Mapper(Interner()))


@pytest.mark.parametrize("query", [
    "namespace=n&object=o&relation=r&subject_set.namespace=g",                                    # a lone namespace
    "namespace=n&object=o&relation=r&subject_set.relation=m",                                     # a lone relation
    "namespace=n&object=o&relation=r&subject_set.namespace=g&subject_set.relation=",
    "namespace=n&object=o&relation=r&subject_set.namespace=g&subject_set.relation=m&subject_set.object=x",
    "namespace=n&object=o&relation=r&subject_set.object=x",
    "namespace=n&object=o&relation=r&subject_set.namespace=g&subject_set.relation=m&page_size=0",
    "namespace=n&object=o&relation=r&subject_set.namespace=g&subject_set.relation=m&page_size=x",
    "namespace=n&object=o&relation=r&subject_set.namespace=g&subject_set.relation=m&page_token=-1",
    "namespace=n&object=o&relation=r&subject_set.namespace=g&subject_set.relation=m&order=id&page_size=0",
    "namespace=n&relation=r&subject_set.namespace=g&subject_set.relation=m",
])
def test_filter_rejected_before_the_engine(query):
    status, body = _handler(_NoEngine()).get_list_subjects(query)
    assert status == 400, body


def test_grpc_filter_rejected_before_the_engine():
    from keto_amd.handlers import HandlerError
    h = _handler(_NoEngine())
    base = {"namespace": "n", "object": "o", "relation": "r"}
    for f in ({"namespace": "g"}, {"relation": "m"}, {}, {"namespace": "g", "relation": "m", "object": "x"}):
        with pytest.raises(HandlerError) as e:
            h.grpc_list_subjects(dict(base, subject_set=f))
        assert e.value.status == 400
    with pytest.raises(HandlerError) as e:
        h.grpc_list_subjects(dict(base, subject_set={"namespace": "g", "relation": "m"}, page_size=-1))
    assert e.value.status == 400


def test_requests_without_the_filter_keep_their_shape():
    eng = _Recorder()
    h = _handler(eng)
    assert h.get_list_subjects("namespace=n&object=o&relation=r&max-depth=3") == \
        (200, {"subject_ids": ["a", "b"], "next_page_token": ""})
    assert h.get_list_subjects("namespace=n&object=o&relation=r&page_size=1") == \
        (200, {"subject_ids": ["a"], "next_page_token": "1"})
    assert h.get_list_subjects("namespace=n&object=o&relation=r&order=id&page_size=2&page_token=4") == \
        (200, {"subject_ids": ["a", "b"], "next_page_token": "7"})
    assert h.grpc_list_subjects({"namespace": "n", "object": "o", "relation": "r", "max_depth": 3}) == \
        {"subject_ids": ["a", "b"], "next_page_token": ""}
    assert eng.calls == [("lookup_subjects", "n", "o", "r", 3), ("lookup_subjects", "n", "o", "r", 0),
                         ("lookup_subjects_page", "n", "o", "r", 0, 4, 2), ("lookup_subjects", "n", "o", "r", 3)]
