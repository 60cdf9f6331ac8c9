"""Subject lookup (kg_lookup_subjects), the parts that need no GPU: the export, argument checks that fail
before a device is touched, the ABI struct layout against the header, and the handler's request decoding."""
import ctypes as C

import pytest


def test_lookup_subjects_symbol_exported():
    from keto_amd import _lib
    L = _lib.load()
    assert "kg_lookup_subjects" in _lib.EXPORTS
    assert hasattr(L, "kg_lookup_subjects")


def test_lookup_subjects_null_arguments():
    from keto_amd import _lib
    L = _lib.load()
    buf = _lib.kg_lookup_buf()
    req = (C.c_uint32 * 4)(0, 0, 0, 0)
    fake = C.c_void_p(0x1000)  # never dereferenced: the arguments are checked first
    for args in ((None, req, 1, 5, C.byref(buf)), (fake, req, 1, 5, None), (fake, None, 1, 5, C.byref(buf))):
        assert L.kg_lookup_subjects(*args) != 0
        assert "NULL" in _lib.last_error()
    L.kg_lookup_free(C.byref(buf))  # an empty buffer: nothing to return


def test_lookup_subjects_struct_sizes_match_header():
    from header_probe import probe
    from keto_amd import _lib
    got = probe(["sizeof(kg_lookup_subj)", "sizeof(kg_lookup_buf)", "offsetof(kg_lookup_subj, rel)",
                 "offsetof(kg_lookup_subj, max_depth)", "offsetof(kg_lookup_buf, n_reqs)",
                 "offsetof(kg_lookup_buf, pinned)"])
    B = _lib.kg_lookup_buf
    assert C.sizeof(B) == 104  # 4 pointers, 7 counters, kernel_ms, pinned: as before this call existed
    assert got == [16, C.sizeof(B), 8, 12, B.n_reqs.offset, B.pinned.offset]


class _NoEngine:
    """The request is rejected before the engine is asked."""

    def lookup_subjects(self, *a):
        raise AssertionError("engine reached")


@pytest.mark.parametrize("query", [
    "namespace=n&object=o&relation=r&max-depth=abc",
    "namespace=n&object=o&relation=r&page_size=0",
    "namespace=n&object=o&relation=r&page_size=x",
    "namespace=n&object=o&relation=r&page_token=x",
    "namespace=n&object=o&relation=r&page_token=-1",
    "namespace=n&relation=r",
    "object=o&relation=r",
    "namespace=n&object=o",
])
def test_list_subjects_rejects_before_the_engine(query):
    from keto_amd.handlers import ListSubjectsHandler
    from keto_amd.mapper import Interner, Mapper
    status, body = ListSubjectsHandler(_NoEngine(), Mapper(Interner())).get_list_subjects(query)
    assert status == 400, body


def test_list_subjects_grpc_incomplete_and_export():
    import keto_amd
    from keto_amd.handlers import HandlerError, ListSubjectsHandler
    from keto_amd.mapper import Interner, Mapper
    assert keto_amd.ListSubjectsHandler is ListSubjectsHandler
    h = ListSubjectsHandler(_NoEngine(), Mapper(Interner()))
    for req in ({"namespace": "n", "relation": "r"}, {"object": "o", "relation": "r"}, {"namespace": "n", "object": "o"},
                {"namespace": "n", "object": "o", "relation": "r", "page_size": -1}):
        with pytest.raises(HandlerError) as e:
            h.grpc_list_subjects(req)
        assert e.value.status == 400
