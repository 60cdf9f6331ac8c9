"""GPU tests of the ranked select (kg_mask_select_device), compared with select_ref: the first `limit` allowed
ids of every ranked row in their order, then KG_LOOKUP_END, and the count of every allowed entry.  The library
call is driven directly so that the output buffers start full of garbage; Engine.mask_select is held against
it, and against a Python loop over lookup_objects end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from keto_amd import _lib
from keto_amd.engine import Registry
from keto_amd.ketoapi import RelationTuple
from keto_amd.mapper import Interner
from test_mask_host import END, mask_ref, select_ref

pytestmark = pytest.mark.gpu

T = RelationTuple.from_string
DEV = torch.device("cuda", 0)
GARBAGE = 0x5A5A5A5A
BASE, N_BITS, ROW_WORDS = 5, 77, 5  # an unaligned base, a partial last word, two spare words


@pytest.fixture(scope="module")
def engine():
    reg = Registry([T("d:o1#view@alice")], [], interner=Interner())
    return reg.permission_engine()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(DEV)


def select(e, mask, cand, limit, base=BASE, n_bits=N_BITS):
    """kg_mask_select_device on a stream of the test's, into buffers full of garbage; the result on the host."""
    n, k_in = cand.shape
    d_mask, d_cand = dev(mask), dev(cand)
    out = torch.full((n, limit), GARBAGE, dtype=torch.int32, device=DEV)
    count = torch.full((n,), GARBAGE, dtype=torch.int32, device=DEV)
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    _lib.check(_lib.load().kg_mask_select_device(
        e.snapshot.handle, C.c_void_p(d_mask.data_ptr()), mask.shape[1], base, n_bits, C.c_void_p(d_cand.data_ptr()), n,
        k_in, limit, C.c_void_p(out.data_ptr()), C.c_void_p(count.data_ptr()), C.c_void_p(stream.cuda_stream)),
        "kg_mask_select_device")
    stream.synchronize()
    return out.cpu().numpy().view(np.uint32), count.cpu().numpy().view(np.uint32)


def agree(e, mask, cand, limit, base=BASE, n_bits=N_BITS):
    out, count = select(e, mask, cand, limit, base, n_bits)
    want_out, want_count = select_ref(mask, cand, limit, base, n_bits)
    assert np.array_equal(count, want_count), (count.tolist(), want_count.tolist())
    bad = np.nonzero((out != want_out).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5].tolist(), out[bad[:1]].tolist(), want_out[bad[:1]].tolist())
    return out, count


def random_mask(rng, n):
    """Rows with about half of the range allowed; the padding bits and the spare words hold noise, which allows
    nothing."""
    m = mask_ref([rng.choice(np.arange(BASE, BASE + N_BITS), N_BITS // 2, replace=False) for _ in range(n)],
                 BASE, N_BITS, ROW_WORDS)
    noise = rng.integers(0, 1 << 32, m.shape, dtype=np.uint64).astype(np.uint32)
    m[:, 2] |= noise[:, 2] & np.uint32(~((1 << (N_BITS - 64)) - 1) & 0xFFFFFFFF)
    m[:, 3:] = noise[:, 3:]
    return m


def random_cand(rng, n, k_in):
    """Ranked ids around the range: below the base, at base + n_bits and above, END, and duplicates."""
    pool = np.concatenate([np.arange(0, BASE + N_BITS + 40), [END, END, BASE + N_BITS, BASE - 1, 0x7FFFFFFE, 4000]])
    return rng.choice(pool, (n, k_in)).astype(np.uint32)


@pytest.mark.parametrize("n", [1, 5, 70])
@pytest.mark.parametrize("k_in", [0, 1, 63, 64, 65, 130])
def test_widths_and_row_counts(engine, k_in, n):
    """Rows of less than, exactly and more than one and two chunks; 5 and 70 rows leave a group with spare waves."""
    rng = np.random.default_rng(100 * k_in + n)
    mask, cand = random_mask(rng, n), random_cand(rng, n, k_in)
    _, want_count = select_ref(mask, cand, 1, BASE, N_BITS)
    top = int(want_count.max()) if n else 0
    assert k_in < 63 or top > 3  # not vacuous: some row keeps several ids
    for limit in sorted({1, 3, max(top - 1, 1), max(top, 1), top + 1, 200}):  # below, equal to and above the counts
        out, count = agree(engine, mask, cand, limit)
        assert k_in or ((out == END).all() and not count.any())
    out, count = engine.mask_select(dev(mask), dev(cand), 7, BASE, N_BITS)  # the engine's call, on the current stream
    want_out, want_count = select_ref(mask, cand, 7, BASE, N_BITS)
    assert out.dtype == count.dtype == torch.int32 and out.shape == (n, 7) and count.shape == (n,)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want_out)
    assert np.array_equal(count.cpu().numpy().view(np.uint32), want_count)
    assert (out.cpu().numpy()[want_out == END] == -1).all()  # END reads as -1


def test_limit_around_the_count_and_a_run_across_chunks(engine):
    allowed = [BASE + 3, BASE + 40, BASE + 76, BASE, BASE + 64]
    mask = mask_ref([allowed] * 3, BASE, N_BITS, ROW_WORDS)
    cand = np.full((3, 130), BASE + 1, np.uint32)  # BASE + 1 is not allowed
    cand[0, [0, 17, 63, 64, 129]] = allowed  # five allowed ids, the chunk edges among their places
    cand[1, 62:67] = allowed  # an allowed run at 62 .. 66 crosses the first chunk boundary
    cand[2, 126:130] = allowed[:4]  # and one at the end of the partial last chunk
    for limit in (4, 5, 6):
        out, count = agree(engine, mask, cand, limit)
        assert count.tolist() == [5, 5, 4]
    out, count = agree(engine, mask, cand, 3)
    assert out[1].tolist() == allowed[:3] and out[0].tolist() == allowed[:3] and count.tolist() == [5, 5, 4]


def test_rows_at_the_edges_of_the_range(engine):
    mask = mask_ref([list(range(BASE, BASE + N_BITS))] * 2 + [[]] + [[BASE, BASE + N_BITS - 1]], BASE, N_BITS, ROW_WORDS)
    mask[:, 2] |= np.uint32(0xFFFFE000)  # every padding bit
    mask[:, 3:] = 0xFFFFFFFF  # and every spare word
    k = 70
    cand = np.zeros((4, k), np.uint32)
    cand[0] = np.arange(BASE, BASE + k)  # everything is allowed
    cand[1] = np.resize(np.asarray([BASE - 1, BASE + N_BITS, END, 0, BASE + N_BITS + 31, BASE + 95, BASE + 159, 0x80000004],
                                   np.uint32), k)  # nothing is: below, at and above the range, in the padding, END
    cand[2] = np.arange(BASE, BASE + k)  # nothing is: an empty row
    cand[3] = np.resize(np.asarray([BASE, BASE, BASE + N_BITS - 1, BASE + 1, BASE, END], np.uint32), k)  # duplicates
    for limit in (1, 69, 70, 71):
        out, count = agree(engine, mask, cand, limit)
        assert count.tolist() == [k, 0, 0, int((cand[3] == BASE).sum() + (cand[3] == BASE + N_BITS - 1).sum())]
        assert (out[1] == END).all() and (out[2] == END).all() and out[0, :min(limit, k)].tolist() == cand[0, :limit].tolist()
    # base 0 and a range that ends at the top of the id space
    top = mask_ref([[0xFFFFFFFE, 0xFFFFFFFD]], 0xFFFFFFFD, 2, 1)
    c2 = np.asarray([[END, 0xFFFFFFFE, 0xFFFFFFFC, 0xFFFFFFFD, 0, END]], np.uint32)
    out, count = agree(engine, top, c2, 4, base=0xFFFFFFFD, n_bits=2)
    assert out.tolist() == [[0xFFFFFFFE, 0xFFFFFFFD, END, END]] and count.tolist() == [2]


def test_bad_arguments_are_refused_with_a_snapshot(engine):
    mask, cand = dev(np.zeros((2, 2), np.uint32)), dev(np.zeros((2, 4), np.uint32))
    with pytest.raises(_lib.KetoGPUError, match="limit"):
        engine.mask_select(mask, cand, 0, 0, 64)
    with pytest.raises(_lib.KetoGPUError, match="row_words"):
        engine.mask_select(mask, cand, 3, 0, 65)
    with pytest.raises(ValueError):
        engine.mask_select(mask[:1], cand, 3, 0, 64)


def test_object_mask_then_select_equals_a_loop_over_lookup_objects():
    it = Interner()
    tuples = [T(f"doc:d{i}#view@(group:g{i % 7}#member)") for i in range(200)]
    tuples += [T("group:g1#member@alice"), T("group:g4#member@alice"), T("group:g5#member@(group:g4#member)"),
               T("group:g2#member@bob"), T("doc:d3#view@alice"), T("folder:f#view@alice")]
    reg = Registry(tuples, [], interner=it)
    e = reg.permission_engine()
    rng = np.random.default_rng(5)
    ranked = [f"d{i}" for i in rng.permutation(200)[:150]] + ["f", "g1", "alice"]  # other namespaces' names too
    ranked = [ranked[i] for i in rng.permutation(len(ranked))] + ranked[:5]  # and some names twice
    cand = torch.tensor([[it.obj_id(name, create=False) for name in ranked]], dtype=torch.int32, device=DEV)
    for who in ("alice", "bob", "nobody"):
        allowed = set(e.lookup_objects("doc", "view", who, 5))
        want = [name for name in ranked if name in allowed]
        mask = e.object_mask("doc", "view", who, 5)
        assert mask.dim() == 1 and mask.dtype == torch.int32 and mask.shape[0] == (it.n_objects + 31) // 32
        for limit in (10, 500):
            out, count = e.mask_select(mask, cand, limit)
            assert int(count[0]) == len(want) and (who == "nobody" or len(want) > 10)
            got = [it.obj_name(i) for i in out[0].tolist() if i != -1]
            assert got == want[:limit] and out[0].tolist()[len(got):] == [-1] * (limit - len(got))
