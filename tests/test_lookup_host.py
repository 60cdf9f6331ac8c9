"""Reverse lookup (kg_lookup_objects), the parts that need no GPU: the exports, argument checks that
fail before a device is touched, the ABI struct layout against the header, and the handler's request
decoding."""
import ctypes as C

import pytest


def test_lookup_symbols_exported():
    from keto_amd import _lib
    L = _lib.load()
    for name in ("kg_lookup_objects", "kg_lookup_free"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name), name


def test_lookup_null_arguments():
    from keto_amd import _lib
    L = _lib.load()
    buf = _lib.kg_lookup_buf()
    req = (C.c_uint32 * 6)(0, 0, 0xFFFFFFFF, 0, 0, 0)
    fake = C.c_void_p(0x1000)  # never dereferenced: the arguments are checked first
    for args in ((None, req, 1, 5, C.byref(buf)), (fake, req, 1, 5, None), (fake, None, 1, 5, C.byref(buf))):
        assert L.kg_lookup_objects(*args) != 0
        assert "NULL" in _lib.last_error()
    L.kg_lookup_free(None)
    L.kg_lookup_free(C.byref(buf))  # an empty buffer: nothing to return


def test_lookup_struct_sizes_match_header():
    from header_probe import probe
    from keto_amd import _lib
    got = probe(["sizeof(kg_lookup)", "sizeof(kg_lookup_buf)", "offsetof(kg_lookup_buf, n_reqs)",
                 "offsetof(kg_lookup_buf, kernel_ms)", "offsetof(kg_lookup_buf, pinned)"])
    B = _lib.kg_lookup_buf
    assert got == [24, C.sizeof(B), B.n_reqs.offset, B.kernel_ms.offset, B.pinned.offset]


class _NoEngine:
    """The request is rejected before the engine is asked."""

    def lookup_objects(self, *a):
        raise AssertionError("engine reached")

    def check_is_member(self, *a):
        raise AssertionError("engine reached")


@pytest.mark.parametrize("query", [
    "namespace=n&relation=r&subject_id=u&subject_set.namespace=n&subject_set.object=o&subject_set.relation=r",
    "namespace=n&relation=r&subject_id=u&max-depth=abc",
    "namespace=n&relation=r&subject_set.namespace=n",
    "namespace=n&relation=r",
    "namespace=n&relation=r&subject=u",
])
def test_list_objects_rejects_like_check(query):
    from keto_amd.handlers import CheckHandler, ListObjectsHandler
    from keto_amd.mapper import Interner, Mapper
    m = Mapper(Interner())
    want = CheckHandler(_NoEngine(), m).get_check(query + "&object=o")
    got = ListObjectsHandler(_NoEngine(), m).get_list_objects(query)
    assert want[0] == 400 and got == want


def test_list_objects_bad_paging_and_grpc_subject():
    from keto_amd.handlers import HandlerError, ListObjectsHandler
    from keto_amd.mapper import Interner, Mapper
    h = ListObjectsHandler(_NoEngine(), Mapper(Interner()))
    assert h.get_list_objects("namespace=n&relation=r&subject_id=u&page_size=0")[0] == 400
    assert h.get_list_objects("namespace=n&relation=r&subject_id=u&page_token=x")[0] == 400
    assert h.get_list_objects("relation=r&subject_id=u")[0] == 400
    with pytest.raises(HandlerError) as e:
        h.grpc_list_objects({"namespace": "n", "relation": "r"})
    assert e.value.status == 400
