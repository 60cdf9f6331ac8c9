"""GPU parity tests for batched expand (BuildTree): HIP path vs the reference's golden trees and the
CPU oracle.  Trees are compared exactly (same pre-order, same child order) against the oracle --
stronger than the reference's order-insensitive AssertInternalTreesAreEqual."""
import numpy as np
import pytest

from golden_cases import Case, all_cases
from keto_amd.engine import ExpandEngine, Registry, records_to_tree
from keto_amd.ketoapi import RelationTuple, SubjectSet, trees_equal_unordered
from keto_amd.mapper import SUBJECT_ID
from oracle.oracle import Oracle, records_to_tree as oracle_tree

pytestmark = pytest.mark.gpu

EXPAND_CASES = all_cases("expands")


@pytest.mark.parametrize("fn,case", EXPAND_CASES, ids=[f"{f}:{c['name']}" for f, c in EXPAND_CASES])
def test_golden_expand(fn, case):
    c = Case(case)
    reg = Registry(c.tuples, c.namespaces, interner=c.it)
    ex = reg.expand_engine()
    for e in case["expands"]:
        ex.config.max_read_depth = e["global_max_depth"]
        if e.get("subject_id") is not None:
            subject = e["subject_id"]
        else:
            ss = e["subject_set"]
            subject = SubjectSet(ss["namespace"], ss["object"], ss["relation"])
        got = ex.build_tree(subject, e["max_depth"])
        exp = Case.expected_tree(e)
        if e.get("ordered"):
            assert got == exp
        else:
            assert trees_equal_unordered(got, exp), (got, exp)


def _records(rec):
    return None if rec is None else np.asarray(rec, np.int64)


# (expand_gw, expand_skip_lds): default (16-lane walkers, then the 64-lane pass, gather-walk, hash pass);
# gather-walk on every root; hash pass on every root; the 64-lane pass on every root
GW_MODES = [(1, 0), (1, 1), (0, 1), (1, 2)]


def _random_graph(seed):
    """(registry, oracle, roots) of test_random_expand_vs_oracle's seeded graph"""
    rng = np.random.default_rng(50 + seed)
    n_obj = 30 + 30 * seed
    tuples = []
    for _ in range(200 + 300 * seed):
        ns, obj, rel = rng.choice(["a", "b"]), f"o{rng.integers(n_obj)}", rng.choice(["r0", "r1", "r2"])
        if rng.random() < 0.55:
            srel = rng.choice(["r0", "r1", "r2", "..."])
            s = f"({rng.choice(['a', 'b'])}:o{rng.integers(n_obj)}#{srel})"
        else:
            s = f"u{rng.integers(30)}"
        tuples.append(RelationTuple.from_string(f"{ns}:{obj}#{rel}@{s}"))
    reg = Registry(tuples, [])
    it = reg.interner
    oracle = Oracle(it.tuples_array(tuples), it.wildcard_rel)
    roots = []
    for _ in range(400):
        if rng.random() < 0.05:
            roots.append([SUBJECT_ID, it.obj_id(f"u{rng.integers(30)}"), 0, 0])
        else:
            roots.append([it.ns_id(rng.choice(["a", "b"])), it.obj_id(f"o{rng.integers(n_obj + 2)}"),
                          it.rel_id(rng.choice(["r0", "r1", "r2"])), int(rng.integers(-1, 7))])
    return reg, oracle, roots


def _root_rows(roots):
    arr = np.asarray(roots, np.int64)
    arr[:, 3] = arr[:, 3].astype(np.int32).view(np.uint32)
    return arr.astype(np.uint32)


@pytest.mark.parametrize("gw,skip", GW_MODES, ids=["default", "gw-all", "hash-all", "lds64-all"])
@pytest.mark.parametrize("seed", range(5))
def test_random_expand_vs_oracle(seed, gw, skip):
    reg, oracle, roots = _random_graph(seed)
    reg.snapshot.tune("expand_gw", gw)
    reg.snapshot.tune("expand_skip_lds", skip)
    for gmax in (1, 2, 4, 7):
        ex = ExpandEngine(reg.snapshot)
        ex.config.max_read_depth = gmax
        got = ex.build_trees_ids(_root_rows(roots))
        for r, g in zip(roots, got):
            exp = oracle.expand(r[0], r[1], r[2], r[3], gmax)
            _cmp_records(exp, g, (r, gmax))


def _wide_rows_graph():
    """900 + 300 sets under one root, rows wider than a wave"""
    tuples = [RelationTuple.from_string(f"g:root#m@(g:c{i}#m)") for i in range(900)]
    tuples += [RelationTuple.from_string(f"g:c{i}#m@(g:d{i % 300}#m)") for i in range(900)]
    tuples += [RelationTuple.from_string(f"g:d{i}#m@u{i}") for i in range(300)]
    tuples += [RelationTuple.from_string(f"g:c{i}#m@x{i}") for i in range(0, 900, 7)]
    return tuples


@pytest.mark.parametrize("gw", [1, 0])
def test_expand_overflow_tier_and_wide_rows(gw):
    # a root whose visited set exceeds the LDS tier (pass 2: gather-walk or the HBM hash) and rows wider
    # than a wave
    tuples = _wide_rows_graph()
    reg = Registry(tuples, [])
    reg.snapshot.tune("expand_gw", gw)
    it = reg.interner
    oracle = Oracle(it.tuples_array(tuples), it.wildcard_rel)
    ex = reg.expand_engine()
    for gmax in (2, 3, 4):
        ex.config.max_read_depth = gmax
        got = ex.build_tree(SubjectSet("g", "root", "m"), 0)
        exp = oracle_tree(oracle.expand(it.ns_id("g"), it.obj_id("root"), it.rel_id("m"), 0, gmax), it)
        assert got == exp, gmax


HASH_CAP_DEFAULT = 1 << 18


def _marked_sets(oracle, exp, rows):
    """Sets BuildTree marks visited for the tree `exp` (oracle records): every set with rows is marked
    when it first appears, as a union or as a leaf.  rows caches which sets have rows."""
    if exp is None:
        return 0
    seen = set()
    for r in np.asarray(exp, np.int64):
        key = (int(r[2]), int(r[3]), int(r[4]))
        if not r[1] or key in seen:
            continue
        if key not in rows:
            rows[key] = oracle.expand(key[0], key[1], key[2], 0, 1) is not None
        if rows[key]:
            seen.add(key)
    return len(seen)


def _bitmap_pass_calls(snap, oracle, rows, gmax, caps=(16,)):
    """Expands `rows` (kg_set rows) at depth gmax with hash-pass lists of `caps` entries -- every root that
    marks more sets than that is answered by the whole-graph bitmap pass -- TWICE in a row, then twice at
    the default list size, all on one engine.  The library clears the visited tables and the bitmap when
    the list size changes (their layout moves), so it is the second call at each size that starts from
    what the call before left behind: a bit or a key that pass 3 or an overflowing hash slot does not
    remove shows there as a set wrongly taken for visited.  Every call must equal the oracle, so the
    small-list calls and the default calls give identical records.  Returns the largest number of sets a
    root marks (from the oracle's tree)."""
    ex = ExpandEngine(snap)
    ex.config.max_read_depth = gmax
    exp = [oracle.expand(int(r[0]), int(r[1]), int(r[2]), int(d), gmax)
           for r, d in zip(rows, rows[:, 3].astype(np.int32))]
    for cap in caps:
        calls = []
        for size in (cap, cap, HASH_CAP_DEFAULT, HASH_CAP_DEFAULT):
            snap.tune("expand_hash_cap", size)
            calls.append((size, ex.build_trees_ids(rows)))
        for k, (size, got) in enumerate(calls):
            for r, e, g in zip(rows, exp, got):
                _cmp_records(e, g, (r.tolist(), gmax, "list size", size, "call", k))
    has_rows = {}
    return max(_marked_sets(oracle, e, has_rows) for e in exp)


def test_expand_bitmap_pass_wide_rows():
    """Pass 3 (k_expand_hbm, the whole-graph bitmap): the wide-rows root outgrows the LDS store (512),
    then a 16-entry hash-pass list (expand_hash_cap), and is answered by the bitmap pass."""
    tuples = _wide_rows_graph()
    reg = Registry(tuples, [])
    reg.snapshot.tune("expand_gw", 0)
    it = reg.interner
    oracle = Oracle(it.tuples_array(tuples), it.wildcard_rel)
    root = np.asarray([[it.ns_id("g"), it.obj_id("root"), it.rel_id("m"), 0]], np.uint32)
    for gmax in (2, 3, 4):
        assert _bitmap_pass_calls(reg.snapshot, oracle, root, gmax) > 512, gmax


@pytest.mark.parametrize("seed", [1, 4])
def test_expand_bitmap_pass_random(seed):
    """Pass 3 on the random graphs: no LDS pass, no gather-walk, small hash-pass lists, so every root that
    marks more sets than a list holds is answered by the bitmap pass.

    These graphs are sparse: counted from the oracle's trees, the most sets with rows one root marks is
    4 / 7 / 9 (seed 1) and 4 / 11 / 14 (seed 4) at depths 2 / 4 / 7 -- never more than 16, so by that count
    the calls with 16-entry lists do not reach pass 3 on these graphs (they are kept: same trees).  Next to
    them the test runs 4-entry lists (the key's lower bound), and for those it asserts at depths 4 and 7
    that some root outgrows the list; at depth 2 none does."""
    reg, oracle, roots = _random_graph(seed)
    reg.snapshot.tune("expand_gw", 0)
    reg.snapshot.tune("expand_skip_lds", 1)
    rows = _root_rows(roots)
    for gmax in (2, 4, 7):
        most = _bitmap_pass_calls(reg.snapshot, oracle, rows, gmax, caps=(16, 4))
        print(f"seed {seed} depth {gmax}: a root marks up to {most} sets with rows")
        assert gmax == 2 or most > 4, gmax


def test_expand_gather_walk_large_slot_and_cycles():
    """A neighbourhood too large for a small gather-walk slot (96 k copied entries > 64 Ki): the root
    moves on to a large slot.  Shared grandchildren, back edges to the root and to a middle layer, and
    subject ids in every row make the visited order matter; depths 2..6 (the copy's reach D-2 and the
    local ids' reach D-1 both vary)."""
    tuples = [RelationTuple.from_string(f"g:root#m@(g:c{i}#m)") for i in range(320)]
    for i in range(320):
        for j in range(300):
            tuples.append(RelationTuple.from_string(f"g:c{i}#m@(g:d{(i * 7 + j * 13) % 2000}#m)"))
        tuples.append(RelationTuple.from_string(f"g:c{i}#m@u{i}"))
    for k in range(2000):
        tuples.append(RelationTuple.from_string(f"g:d{k}#m@(g:e{k % 50}#m)"))
        tuples.append(RelationTuple.from_string(f"g:d{k}#m@v{k}"))
        if k % 97 == 0:
            tuples.append(RelationTuple.from_string(f"g:d{k}#m@(g:root#m)"))
            tuples.append(RelationTuple.from_string(f"g:d{k}#m@(g:c{k % 320}#m)"))
    for k in range(50):
        tuples.append(RelationTuple.from_string(f"g:e{k}#m@(g:c{k}#m)"))
        tuples.append(RelationTuple.from_string(f"g:e{k}#m@w{k}"))
    reg = Registry(tuples, [])
    it = reg.interner
    oracle = Oracle(it.tuples_array(tuples), it.wildcard_rel)
    # (expand_gw, expand_gw_wait_us): default; large slots that never wait (their tickets are
    # abandoned and the roots go to the hash pass); no gather-walk
    for gw, wait in ((1, 100000), (1, 0), (0, 100000)):
        reg.snapshot.tune("expand_gw", gw)
        reg.snapshot.tune("expand_gw_wait_us", wait)
        ex = reg.expand_engine()
        for gmax in (2, 3, 4, 6):
            ex.config.max_read_depth = gmax
            got = ex.build_tree(SubjectSet("g", "root", "m"), 0)
            exp = oracle_tree(oracle.expand(it.ns_id("g"), it.obj_id("root"), it.rel_id("m"), 0, gmax), it)
            assert got == exp, (gw, wait, gmax)


def _cmp_records(exp, g, what):
    if exp is None:
        assert g is None, what
        return
    assert g is not None, what
    e2 = np.asarray(exp, np.int64).copy()
    g2 = np.asarray(g, np.int64).copy()
    ids = e2[:, 1] == 0  # SubjectIDs: oracle ns=rel=-1, GPU KG_SUBJECT_ID / 0
    e2[ids, 2] = 0
    e2[ids, 4] = 0
    g2[g2[:, 1] == 0, 2] = 0
    g2[g2[:, 1] == 0, 4] = 0
    assert e2.shape == g2.shape and (e2 == g2).all(), what


@pytest.mark.parametrize("n_tuples,gmax,gw,skip,wait", [(300_000, 5, 1, 0, 100000), (1_000_000, 3, 1, 0, 100000),
                                                         (300_000, 5, 1, 1, 100000), (300_000, 5, 0, 0, 100000),
                                                         (300_000, 5, 1, 0, 0), (300_000, 5, 1, 0, 50),
                                                         (300_000, 5, 1, 2, 100000)])
def test_c5_hot_group_roots_vs_oracle(n_tuples, gmax, gw, skip, wait):
    """Config C5's workload at reduced size: the generator's most popular group#member roots (the
    roots bench.py --mode expand times), expanded at the global depth, against the oracle's
    BuildTree on the snapshot's own rows -- same pre-order, same child order, every root."""
    from keto_amd.engine import Snapshot
    from keto_amd.synth import hot_group_roots
    snap = Snapshot.synthetic(n_tuples, seed=20250131)
    snap.tune("expand_gw", gw)
    snap.tune("expand_skip_lds", skip)
    snap.tune("expand_gw_wait_us", wait)  # 0 / 50 us: large slots give their tickets up
    roots = hot_group_roots(snap.synth_ids(), 1500)
    ex = ExpandEngine(snap)
    ex.config.max_read_depth = gmax
    got = ex.build_trees_ids(roots)
    oracle = Oracle(snap.export(), 0)
    big = 0
    for r, g in zip(roots, got):
        exp = oracle.expand(int(r[0]), int(r[1]), int(r[2]), 0, gmax)
        _cmp_records(exp, g, (r.tolist(), gmax))
        big += g is not None and len(g) > 512
    assert big > 0  # some trees outgrow the LDS pass (the hash / bitmap passes are exercised)


def test_expand_lane_memory_stays_flat():
    """A long-lived caller's lane keeps its device buffers, grown only when a call's output does not
    fit: 16 calls of the same batch on one thread allocate nothing after the first (the compacted-
    output buffer used to double on every call until hipMalloc failed, seen at C5 scale)."""
    import torch
    from keto_amd.engine import Snapshot
    from keto_amd.synth import hot_group_roots
    snap = Snapshot.synthetic(300_000, seed=20250131)
    roots = hot_group_roots(snap.synth_ids(), 2000)
    ex = ExpandEngine(snap)
    ex.config.max_read_depth = 5
    first = ex.build_trees_ids(roots)
    ex.build_trees_ids(roots)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(14):
        again = ex.build_trees_ids(roots)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < (64 << 20), (free0, free1)
    assert all((a is None and b is None) or (a == b).all() for a, b in zip(first, again))


@pytest.mark.parametrize("gw,skip", [(1, 0), (0, 1)], ids=["default", "hash-all"])
def test_expand_device_io_vs_oracle(gw, skip):
    """kg_expand_batch_device (roots and trees in HBM, offsets by a device scan): the same trees as the
    host-buffer call and the oracle's BuildTree, on C5 roots (giant trees included) and on random roots
    with nil trees and subject-id roots; an empty batch; the device output pool reused across calls."""
    import torch
    from keto_amd import _lib
    from keto_amd.engine import Snapshot
    from keto_amd.synth import hot_group_roots
    snap = Snapshot.synthetic(300_000, seed=20250131)
    snap.tune("expand_gw", gw)
    snap.tune("expand_skip_lds", skip)
    roots = hot_group_roots(snap.synth_ids(), 1500)
    rng = np.random.default_rng(7)
    extra = roots[rng.choice(len(roots), 64)].copy()
    extra[:16, 1] = 0x7FFFFFF0  # unknown objects: nil trees
    extra[16:24, 0] = SUBJECT_ID  # subject-id roots: a leaf each
    roots = np.concatenate([roots, extra])
    ex = ExpandEngine(snap)
    ex.config.max_read_depth = 5
    host = ex.build_trees_ids(roots)
    oracle = Oracle(snap.export(), 0)
    for k in range(2):  # the second call reuses the pool's buffers
        dev = ex.build_trees_ids(roots, device=True)
        for r, h, d in zip(roots, host, dev):
            assert (h is None) == (d is None) and (h is None or (h == d).all()), r.tolist()
    for r, d in zip(roots[:200], dev[:200]):
        if r[0] != SUBJECT_ID:
            _cmp_records(oracle.expand(int(r[0]), int(r[1]), int(r[2]), 0, 5), d, r.tolist())
    assert sum(d is not None and len(d) > 512 for d in dev) > 0
    # empty batch: root_off = [0]
    L = _lib.load()
    buf = _lib.kg_tree_buf()
    z = torch.zeros((1, 4), dtype=torch.int32, device="cuda:0")
    _lib.check(L.kg_expand_batch_device(snap.handle, z.data_ptr(), 0, 5, buf, None), "kg_expand_batch_device")
    off = np.ones(1, np.uint64)
    _lib.device_to_host(off, buf.root_off, 8)
    assert buf.n_nodes == 0 and off[0] == 0
    L.kg_tree_free(buf)


def test_expand_buffers_regrow_vs_oracle():
    """One engine's expand buffers (the lane's for host output, the stream workspace's for device output)
    sized for 200 roots, regrown for 2 000, then used for 200 again: host and device trees are equal on
    every call, and the first 100 roots of each equal the oracle's BuildTree."""
    from keto_amd.engine import Snapshot
    from keto_amd.synth import hot_group_roots
    snap = Snapshot.synthetic(300_000, seed=20250131)
    ids = snap.synth_ids()
    ex = ExpandEngine(snap)
    ex.config.max_read_depth = 5
    oracle = Oracle(snap.export(), 0)
    want = {}  # the oracle's tree per root, computed once
    for n in (200, 2000, 200):
        roots = hot_group_roots(ids, n)
        assert len(roots) == n
        host = ex.build_trees_ids(roots)
        dev = ex.build_trees_ids(roots, device=True)
        for r, h, d in zip(roots, host, dev):
            assert (h is None) == (d is None) and (h is None or (h.shape == d.shape and (h == d).all())), (n, r.tolist())
        for r, d in zip(roots[:100], dev[:100]):
            key = tuple(int(x) for x in r[:3])
            if key not in want:
                want[key] = oracle.expand(key[0], key[1], key[2], 0, 5)
            _cmp_records(want[key], d, (n, r.tolist()))
    snap.close()
