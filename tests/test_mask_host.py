"""Host tests of the access masks (kg_lookup_objects_mask_device, kg_lookup_subject_sets_mask_device,
kg_mask_select_device): the symbols, every argument the library refuses before it looks at the snapshot or
launches anything, and the numpy restatements of the two definitions that the GPU tests compare against."""
import ctypes as C

import numpy as np
import pytest

from keto_amd import _lib

END = _lib.KG_LOOKUP_END
MASK_BUF = _lib.kg_lookup_mask_buf  # what the mask calls return on the host
MASK_CALLS = ["kg_lookup_objects_mask_device", "kg_lookup_subject_sets_mask_device"]
NEW = MASK_CALLS + ["kg_lookup_mask_free", "kg_mask_select_device"]


# ---------------------------------------------------------------- the definitions, restated
def mask_ref(ids_per_request, base, n_bits, row_words):
    """uint32 [n, row_words]: bit (o - base) & 31 of word (o - base) >> 5 of row i for every o of request i's
    ids with base <= o < base + n_bits, every other bit 0."""
    assert n_bits > 0 and row_words >= (n_bits + 31) // 32
    out = np.zeros((len(ids_per_request), row_words), np.uint32)
    for i, ids in enumerate(ids_per_request):
        for o in set(int(x) for x in ids):
            if base <= o < base + n_bits:
                out[i, (o - base) >> 5] |= np.uint32(1 << ((o - base) & 31))
    return out


def popcounts(mask):
    """The bits set in every row."""
    m = np.ascontiguousarray(mask, np.uint32)
    return np.unpackbits(m.view(np.uint8), axis=1).sum(axis=1).astype(np.uint64) if m.size else \
        np.zeros(m.shape[0], np.uint64)


def select_ref(mask, cand, limit, base, n_bits):
    """(out uint32 [n, limit], count uint32 [n]): per row the first `limit` allowed candidates in their order,
    then END; count is every allowed entry of the row.  Allowed: base <= id < base + n_bits and the bit set."""
    mask, cand = np.asarray(mask, np.uint32), np.asarray(cand, np.uint32)
    n = cand.shape[0]
    out = np.full((n, limit), END, np.uint32)
    count = np.zeros(n, np.uint32)
    for i in range(n):
        kept = []
        for c in cand[i].tolist():
            d = c - base
            if base <= c < base + n_bits and (int(mask[i, d >> 5]) >> (d & 31)) & 1:
                kept.append(c)
        count[i] = len(kept)
        out[i, :min(limit, len(kept))] = kept[:limit]
    return out, count


def test_mask_ref_on_hand_cases():
    m = mask_ref([[5, 6, 36, 37, 81], [4, 82, 5000], [], [5, 5, 5]], 5, 77, 5)
    # row 0: ids 5, 6 -> bits 0, 1 of word 0; 36 -> bit 31; 37 -> bit 0 of word 1; 81 -> bit 76: bit 12 of word 2
    assert m.tolist() == [[0x80000003, 1, 1 << 12, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0]]
    assert popcounts(m).tolist() == [5, 0, 0, 1]
    assert mask_ref([[0, 31, 32]], 0, 33, 2).tolist() == [[0x80000001, 1]]
    assert mask_ref([], 0, 1, 1).shape == (0, 1) and popcounts(mask_ref([], 0, 1, 1)).tolist() == []


def test_select_ref_on_hand_cases():
    mask = mask_ref([[5, 7, 9, 81], []], 5, 77, 3)
    mask[0, 2] |= np.uint32(1 << 20)  # a padding bit (bit 84 >= n_bits) allows nothing
    cand = np.asarray([[9, 4, 7, 7, END, 82, 89, 81, 6, 5], [5, 7, 9, 81, 0, 1, 2, 3, 4, END]], np.uint32)
    out, count = select_ref(mask, cand, 3, 5, 77)
    assert out.tolist() == [[9, 7, 7], [END, END, END]] and count.tolist() == [5, 0]
    out, count = select_ref(mask, cand, 7, 5, 77)
    assert out.tolist() == [[9, 7, 7, 81, 5, END, END], [END] * 7] and count.tolist() == [5, 0]
    out, count = select_ref(mask, cand[:, :0], 2, 5, 77)
    assert out.tolist() == [[END, END], [END, END]] and count.tolist() == [0, 0]


# ---------------------------------------------------------------- the library, without a GPU
def test_new_symbols_are_exported_and_bound():
    L = _lib.load()
    header = open(_lib.os.path.join(_lib.HERE, "..", "include", "ketogpu.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name) and name + "(" in header, name
        assert getattr(L, name).argtypes is not None, name
    assert len(L.kg_lookup_objects_mask_device.argtypes) == 10 and len(L.kg_mask_select_device.argtypes) == 12
    assert C.sizeof(MASK_BUF) == 11 * 8


FAKE = 0x1000  # a non-NULL pointer the library must never follow: every case below fails before that


def _mask_call(name, n=1, base=0, n_bits=64, row_words=2, reqs=FAKE, d_mask=FAKE, out=True):
    buf = MASK_BUF()
    rc = getattr(_lib.load(), name)(None, reqs, n, 5, base, n_bits, d_mask, row_words, C.byref(buf) if out else None,
                                    None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("name", MASK_CALLS)
@pytest.mark.parametrize("bad, word", [
    (dict(n_bits=0), "n_bits"),
    (dict(n_bits=65, row_words=2), "row_words"),
    (dict(n_bits=1, row_words=0), "row_words"),
    (dict(base=0xFFFFFFFF, n_bits=1), "base + n_bits"),
    (dict(base=0x80000000, n_bits=0x80000000, row_words=1 << 26), "base + n_bits"),
    (dict(n=1 << 62, row_words=8), "overflows"),
    (dict(d_mask=None), "d_mask"),
    (dict(out=False), "out"),
    (dict(reqs=None), "reqs"),
])
def test_mask_calls_refuse_bad_arguments_before_any_launch(name, bad, word):
    rc, text = _mask_call(name, **bad)
    assert rc == -2 and word in text and name in text, (rc, text)


@pytest.mark.parametrize("name", MASK_CALLS)
def test_mask_calls_with_good_arguments_reach_the_snapshot_check(name):
    rc, text = _mask_call(name)
    assert rc == -2 and "NULL snapshot" in text
    rc, text = _mask_call(name, base=0xFFFFFFFE, n_bits=1, row_words=1)  # base + n_bits == 0xFFFFFFFF is the top
    assert rc == -2 and "NULL snapshot" in text
    rc, text = _mask_call(name, n=0, reqs=None, d_mask=None, out=False)  # nothing is needed for no request
    assert rc == -2 and "NULL snapshot" in text
    rc, text = _mask_call(name, n=0, n_bits=0)  # the geometry is checked whatever n is
    assert rc == -2 and "n_bits" in text


def _select_call(n=1, row_words=2, base=0, n_bits=64, k_in=4, limit=3, d_mask=FAKE, d_cand=FAKE, d_out=FAKE,
                 d_count=FAKE):
    rc = _lib.load().kg_mask_select_device(None, d_mask, row_words, base, n_bits, d_cand, n, k_in, limit, d_out, d_count,
                                           None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("bad, word", [
    (dict(limit=0), "limit"),
    (dict(n_bits=65, row_words=2), "row_words"),
    (dict(d_mask=None), "NULL pointer"),
    (dict(d_cand=None), "NULL pointer"),
    (dict(d_out=None), "NULL pointer"),
    (dict(d_count=None), "NULL pointer"),
])
def test_select_refuses_bad_arguments_before_any_launch(bad, word):
    rc, text = _select_call(**bad)
    assert rc == -2 and word in text and "kg_mask_select_device" in text, (rc, text)


def test_select_with_good_arguments_reaches_the_snapshot_check():
    for ok in (dict(), dict(k_in=0, d_cand=None), dict(n=0, d_mask=None, d_cand=None, d_out=None, d_count=None)):
        rc, text = _select_call(**ok)
        assert rc == -2 and "NULL snapshot" in text, (ok, rc, text)


def test_mask_free_takes_an_empty_buffer():
    buf = MASK_BUF()
    _lib.load().kg_lookup_mask_free(C.byref(buf))
    _lib.load().kg_lookup_mask_free(None)
    assert buf.pinned == 0 and not buf.n_set
