"""GPU tests of the access masks (kg_lookup_objects_mask_device, kg_lookup_subject_sets_mask_device): every
row must equal mask_ref of the unpaged call's answer on the same requests -- every other bit of the caller's
buffer cleared -- with n_set the rows' popcounts and n_errors, err_code and the five counters those of the
unpaged call.  One family is compared with the CPU oracle directly."""
import threading

import numpy as np
import pytest
import torch

import test_gpu_lookup as lo
import test_gpu_lookup_subject_sets as lss
import test_gpu_lookup_subjects as ls
from keto_amd import _lib
from keto_amd.engine import Config, Engine, Registry, Snapshot
from keto_amd.ketoapi import RelationTuple
from keto_amd.mapper import Interner, SUBJECT_ID
from oracle.oracle import Oracle
from test_gpu_lookup_page import _mixed_case
from test_mask_host import mask_ref, popcounts

pytestmark = pytest.mark.gpu

T = RelationTuple.from_string
COUNTERS = ("exact", "candidates", "confirmed", "reverse_edges", "levels")
DEV = torch.device("cuda", 0)


def as_set_requests(four):
    """(n,4) kg_lookup_subj rows as (n,6) kg_lookup_subj_set rows that list subject ids."""
    four = np.asarray(four, np.uint32).reshape(-1, 4)
    six = np.zeros((len(four), 6), np.uint32)
    six[:, :3], six[:, 3], six[:, 5] = four[:, :3], SUBJECT_ID, four[:, 3]
    return six


def calls(e, kind):
    """(the unpaged call, the mask call) of the kind: objects, or subject sets / subject ids."""
    return (e.lookup_objects_ids, e.lookup_objects_mask_ids) if kind == "objects" else \
        (e.lookup_subject_sets_ids, e.lookup_subject_sets_mask_ids)


def split(off, ids):
    return [ids[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def host(mask):
    return mask.cpu().numpy().view(np.uint32)


def agree(e, kind, reqs, base, n_bits, row_words):
    """The mask call into a buffer of 0xFFFFFFFF words against the unpaged call on the same requests.  Returns
    (the unpaged answers, the mask on the host, the call's counters).  A lane keeps its grown key list between
    calls and a rerun after a regrowth counts its edges again, so a first call brings the list to its size: the
    two calls that are compared then start alike (with "lookup_cap" set every call starts at that size)."""
    unpaged, masked = calls(e, kind)
    unpaged(reqs)
    off, ids, err, nerr = unpaged(reqs, with_stats=True)
    want_stats = e.last_stats
    answers = split(off, ids)
    buf = torch.full((len(reqs), row_words), -1, dtype=torch.int32, device=DEV)
    mask, n_set, m_err, m_nerr = masked(reqs, base=base, n_bits=n_bits, out=buf, with_stats=True)
    stats = e.last_stats
    assert mask.data_ptr() == buf.data_ptr()
    got = host(mask)
    want = mask_ref(answers, base, n_bits, row_words)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5].tolist(), got[bad[:1]].tolist(), want[bad[:1]].tolist())
    assert np.array_equal(n_set, popcounts(got))
    assert np.array_equal(m_err, err) and np.array_equal(m_nerr, nerr)
    assert {k: stats[k] for k in COUNTERS} == {k: want_stats[k] for k in COUNTERS}
    return answers, got, stats


def geometries(it):
    """base 5 / 77 bits / 5 words: an unaligned base, a partial last word, two spare words, ids on both sides of
    the range; and the whole id space from 0."""
    return [(5, 77, 5), (0, it.n_objects, (it.n_objects + 31) // 32)]


# ---------------------------------------------------------------- random graphs
@pytest.mark.parametrize("seed", [1, 3])
def test_random_graphs_objects(seed):
    """150 requests: three walk groups.  The first geometry is also held against the oracle."""
    it, tuples, reqs = lo._case1(seed)
    reg = Registry(tuples, [], interner=it)
    e = Engine(reg.snapshot, Config(5))
    for base, n_bits, row_words in geometries(it):
        answers, got, st = agree(e, "objects", reqs, base, n_bits, row_words)
        assert st["levels"] > 0 and got.any()
        below = sum(int((a < base).sum()) for a in answers)
        above = sum(int((a >= base + n_bits).sum()) for a in answers)
        assert base == 0 or (below > 0 and above > 0)  # the range cuts answers on both sides
    t6 = it.tuples_array(tuples)
    ref = lo.reference(Oracle(t6, it.wildcard_rel), lo.domains(t6), reqs, 5)
    mask, n_set, err, nerr = e.lookup_objects_mask_ids(reqs, base=5, n_bits=77)
    assert mask.shape == (150, 3) and mask.dtype == torch.int32
    assert np.array_equal(host(mask), mask_ref([r[0] for r in ref], 5, 77, 3))
    assert nerr.tolist() == [r[1] for r in ref] and err.tolist() == [r[2] for r in ref]


@pytest.mark.parametrize("seed", [1, 3])
def test_random_graphs_subject_ids(seed):
    it, tuples, four = ls._case1(seed)
    reqs = as_set_requests(four)
    reg = Registry(tuples, [], interner=it)
    e = Engine(reg.snapshot, Config(5))
    off, ids, _, _ = e.lookup_subjects_ids(four)  # the id requests of the set call answer as kg_lookup_subjects
    for base, n_bits, row_words in geometries(it):
        answers, got, st = agree(e, "subjects", reqs, base, n_bits, row_words)
        assert all(np.array_equal(a, b) for a, b in zip(answers, split(off, ids)))
        assert st["levels"] > 0 and got.any()
        # the range cuts answers at its top (the subject ids were interned after the objects: none lies below 5)
        assert base == 0 or sum(int((a >= base + n_bits).sum()) for a in answers) > 0


# ---------------------------------------------------------------- duplicates, regrowth
def test_hub_and_cycle_give_one_bit_per_id():
    """A subject id reached through 5,000 nodes, a 40-cycle: the key list holds an id many times, the row one bit."""
    it, tuples, four = ls._hub_case()
    reg = Registry(tuples, [], interner=it)
    e = Engine(reg.snapshot, Config(6))
    answers, got, st = agree(e, "subjects", as_set_requests(four), 0, it.n_objects, (it.n_objects + 31) // 32)
    listed = sum(len(a) for a in answers)
    assert st["exact"] > listed > 10000 and int(popcounts(got).sum()) == listed
    g = lss._hub_graph()  # set requests (three filters) and an id request: 94 requests
    e = Engine(g.reg.snapshot, Config(41))
    answers, got, st = agree(e, "subjects", g.reqs, 0, g.it.n_objects, (g.it.n_objects + 31) // 32)
    listed = sum(len(a) for a in answers)
    assert st["exact"] > listed > 10000 and int(popcounts(got).sum()) == listed
    agree(e, "subjects", g.reqs, 5, 77, 5)


def test_key_list_regrows_before_the_mask_tail():
    it = Interner()
    tuples = [T(f"n:o{i}#r@big") for i in range(3000)]
    reg = Registry(tuples, [], interner=it)
    qs = [T("n:any#r@big")] + [T(f"n:any#r@nobody{i}") for i in range(63)]
    qs = qs[20:] + qs[:20]  # the big one in the middle of the group
    reqs = lo.requests_array(it, qs, [0] * len(qs))
    e = Engine(reg.snapshot, Config(5))
    n_bits = it.n_objects
    reg.snapshot.tune("lookup_cap", 16)  # the key list starts at 16 entries: the group is rerun with a larger one
    try:
        answers, got, _ = agree(e, "objects", reqs, 0, n_bits, (n_bits + 31) // 32 + 1)
        assert sum(len(a) for a in answers) == 3000 and int(popcounts(got).sum()) == 3000
        agree(e, "objects", reqs, 1000, 1001, 40)
    finally:
        reg.snapshot.tune("lookup_cap", 0)
    agree(e, "objects", reqs, 0, n_bits, (n_bits + 31) // 32)


# ---------------------------------------------------------------- every tail in one call
@pytest.fixture(scope="module")
def mixed():
    it, namespaces, prog, tuples, t6, (oreq, omodes), (sreq, smodes) = _mixed_case()
    reg = Registry(tuples, namespaces, interner=it)
    yield it, reg, oreq, as_set_requests(sreq)
    reg.snapshot.tune("lookup_cap", 0)


@pytest.mark.parametrize("kind", ["objects", "subjects"])
def test_every_tail_in_one_call(mixed, kind):
    """Walk, formula, confirm-nodes' candidates and confirm-all requests, an undeclared relation and errors in one
    call, with the lists at their default size and starting at 64 entries."""
    it, reg, oreq, sreq = mixed
    reqs = oreq if kind == "objects" else sreq
    e = Engine(reg.snapshot, Config(5))
    for cap in (0, 64):
        reg.snapshot.tune("lookup_cap", cap)
        for base, n_bits, row_words in geometries(it):
            answers, got, st = agree(e, kind, reqs, base, n_bits, row_words)
        assert st["candidates"] > 0 and st["confirmed"] > 0 and st["exact"] > 0, st
        _, masked = calls(e, kind)
        _, _, err, nerr = masked(reqs)
        assert nerr.any() and err[nerr > 0].all() and max(len(a) for a in answers) > 64


def test_id_and_set_requests_in_one_call():
    g = lss.random_case(2)
    f3 = lss.set_filters(g.t6)[:3]
    mixed_reqs = g.reqs.copy()
    for i in range(len(mixed_reqs)):
        k = i % 4
        mixed_reqs[i, 3], mixed_reqs[i, 4] = (SUBJECT_ID, 0) if k == 3 else f3[k]
    e = Engine(g.reg.snapshot, Config(5))
    for base, n_bits, row_words in geometries(g.it):
        answers, got, _ = agree(e, "subjects", mixed_reqs, base, n_bits, row_words)
    kinds = [sum(len(a) > 0 for a in answers[k::4]) for k in range(4)]
    assert kinds[3] > 0 and sum(kinds[:3]) > 0, kinds


# ---------------------------------------------------------------- the edges of the call
def test_no_request():
    it, tuples, reqs = lo._case1(1)
    e = Engine(Registry(tuples, [], interner=it).snapshot, Config(5))
    for call, width in ((e.lookup_objects_mask_ids, 6), (e.lookup_subject_sets_mask_ids, 6)):
        mask, n_set, err, nerr = call(np.zeros((0, width), np.uint32), base=5, n_bits=77)
        assert mask.shape == (0, 3) and len(n_set) == len(err) == len(nerr) == 0
        keep = torch.full((0, 5), -1, dtype=torch.int32, device=DEV)
        assert call(np.zeros((0, width), np.uint32), base=5, n_bits=77, out=keep)[0] is keep


def test_bad_geometry_is_refused_with_a_snapshot():
    it, tuples, reqs = lo._case1(1)
    e = Engine(Registry(tuples, [], interner=it).snapshot, Config(5))
    small = torch.zeros((len(reqs), 2), dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.KetoGPUError, match="row_words") as ex:
        e.lookup_objects_mask_ids(reqs, base=5, n_bits=77, out=small)
    assert "(-2)" in str(ex.value) and not small.any()  # nothing was written
    with pytest.raises(_lib.KetoGPUError, match="n_bits"):
        e.lookup_subject_sets_mask_ids(as_set_requests(ls._case1(1)[2]), n_bits=0)


def test_sharded_snapshot_is_refused():
    it, tuples, reqs = lo._case1(2)
    snap = Snapshot(it.tuples_array(tuples), it, shard=(0, 2))
    e = Engine(snap, Config(5))
    for call, r in ((e.lookup_objects_mask_ids, reqs), (e.lookup_subject_sets_mask_ids, as_set_requests(ls._case1(2)[2]))):
        with pytest.raises(_lib.KetoGPUError, match="not supported on hash-sharded snapshots") as ex:
            call(r, n_bits=64)
        assert "(-3)" in str(ex.value)


def test_mask_follows_the_rows_after_apply():
    it = Interner()
    tuples = [T(f"d:o{i}#view@alice") for i in range(40)] + [T("d:o7#view@(g:eng#m)"), T("g:eng#m@bob")]
    rows = it.tuples_array(tuples)
    snap = Snapshot(rows, it)
    reqs = lo.requests_array(it, [T("d:any#view@alice"), T("d:any#view@bob")], [0, 0])
    sreq = lss.requests_array(it, [("d", "o7", "view", None, None, 0), ("d", "o7", "view", "g", "m", 0)])
    bit = lambda m, r, name: (int(m[r, it.obj_id(name) >> 5]) >> (it.obj_id(name) & 31)) & 1  # noqa: E731
    n_bits = it.n_objects + 8  # room for the ids the delta brings
    words = (n_bits + 31) // 32
    e = Engine(snap, Config(5))
    _, got, _ = agree(e, "objects", reqs, 0, n_bits, words)
    assert bit(got, 0, "o3") and bit(got, 1, "o7") and popcounts(got).tolist() == [40, 1]
    _, got, _ = agree(e, "subjects", sreq, 0, n_bits, words)
    assert bit(got, 0, "alice") and bit(got, 0, "bob") and bit(got, 1, "eng")
    dels = it.tuples_array([T("d:o3#view@alice"), T("g:eng#m@bob")])
    ins = it.tuples_array([T("d:new#view@alice"), T("d:o9#view@(g:eng#m)"), T("g:eng#m@carol")])
    assert it.n_objects <= n_bits
    new = snap.apply(ins, dels)
    e2 = Engine(new, Config(5))
    _, got, _ = agree(e2, "objects", reqs, 0, n_bits, words)
    assert not bit(got, 0, "o3") and bit(got, 0, "new") and popcounts(got).tolist() == [40, 0]
    _, got, _ = agree(e2, "subjects", sreq, 0, n_bits, words)
    assert bit(got, 0, "alice") and not bit(got, 0, "bob") and bit(got, 0, "carol") and bit(got, 1, "eng")
    _, got, _ = agree(e, "objects", reqs, 0, n_bits, words)  # the old snapshot still answers from its own rows
    assert bit(got, 0, "o3") and not bit(got, 0, "new")
    for s in (snap, new):
        s.close()


def test_eight_threads_get_their_own_masks():
    it, tuples, reqs = lo._case1(2)
    reg = Registry(tuples, [], interner=it)
    it2, tuples2, sfour = ls._case1(2)
    reg2 = Registry(tuples2, [], interner=it2)
    sreq = as_set_requests(sfour)
    serial, serial2 = Engine(reg.snapshot, Config(5)), Engine(reg2.snapshot, Config(5))
    want = mask_ref(split(*serial.lookup_objects_ids(reqs)[:2]), 5, 77, 5)
    want2 = mask_ref(split(*serial2.lookup_subject_sets_ids(sreq)[:2]), 5, 77, 5)
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            mine = np.arange(k, 150, 8)
            for _ in range(3):
                buf = torch.full((len(mine), 5), -1, dtype=torch.int32, device=DEV)
                if k % 2:
                    got = Engine(reg.snapshot, Config(5)).lookup_objects_mask_ids(reqs[mine], 5, 77, out=buf)[0]
                    assert np.array_equal(host(got), want[mine])
                else:
                    got = Engine(reg2.snapshot, Config(5)).lookup_subject_sets_mask_ids(sreq[mine], 5, 77, out=buf)[0]
                    assert np.array_equal(host(got), want2[mine])
        except BaseException as x:  # noqa: BLE001
            errors.append(x)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert want.any() and want2.any()


@pytest.mark.parametrize("side", [False, True])
def test_the_call_waits_for_the_callers_stream(side):
    """A kernel that fills the buffer is enqueued on the current stream, behind enough work to still be pending,
    immediately before the call: the lane's clear and its bits must land after it."""
    it, tuples, reqs = lo._case1(0)
    reg = Registry(tuples, [], interner=it)
    e = Engine(reg.snapshot, Config(5))
    row_words = 4096
    want = mask_ref(split(*e.lookup_objects_ids(reqs)[:2]), 0, 32 * row_words, row_words)
    buf = torch.zeros((len(reqs), row_words), dtype=torch.int32, device=DEV)
    ballast = torch.zeros(1 << 26, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(DEV) if side else torch.cuda.current_stream(DEV)
    with torch.cuda.stream(stream):
        for _ in range(4):
            ballast.add_(1)
        buf.fill_(-1)
        mask, n_set, _, _ = e.lookup_objects_mask_ids(reqs, base=0, n_bits=32 * row_words, out=buf)
    got = host(mask)  # the call returned with the mask complete
    assert np.array_equal(got, want) and np.array_equal(n_set, popcounts(want)) and want.any()
    torch.cuda.synchronize()
    assert int(ballast[0]) == 4
