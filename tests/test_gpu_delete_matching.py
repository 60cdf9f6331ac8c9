"""GPU tests of the delete-by-query refresh (kg_snapshot_delete_matching, keto_amd/csrc/kg_delete.hip): what
the call reports and what the snapshot it returns holds and answers, against tests/delete_ref.py (rows, keys,
counts), kg_snapshot_query on the base (the deleted keys), the CPU oracle on the remaining rows and a full
build from them.  Bit-exact: ids, row order, keys, answers, codes.

   1  every filter, keyed and unkeyed          7  chains, and the base stays valid
   2  range edges (16-byte tail, wave edges)   8  namespace programs, materialised or not
   3  a 5 000-entry hub, the live marking      9  the grid-stride loops (10^6 rows)
   4  64 queries in one call                  10  replicas
   5  no match, n = 0                         11  SnapshotPersister(device_deletes=True)
   6  everything
"""
import numpy as np
import pytest

import test_gpu_lookup as lo
import test_gpu_lookup_subjects as ls
import test_gpu_query as tq
from delete_ref import Q_NS, Q_OBJ, Q_REL, Q_SUBJECT, delete_ref
from keto_amd import _lib
from keto_amd.engine import Config, Engine, ExpandEngine, Snapshot, queries_array, row_queries
from keto_amd.ketoapi import RelationTuple
from keto_amd.mapper import Interner, SUBJECT_ID
from keto_amd.namespace import (ComputedSubjectSet, InvertResult, Namespace, Relation, SubjectSetRewrite,
                                compile_program)
from keto_amd.persister import RelationQuery, SnapshotPersister
from oracle.oracle import POLICY_CANONICAL, POLICY_DFS, Oracle
from refresh_ref import apply_ref, node_rows, nodes_of
from test_gpu_check import random_graph, random_program, random_queries
from test_gpu_expand import _cmp_records
from test_gpu_persister import shard_rows
from test_gpu_refresh import (_formula_graph, _formula_namespaces, _keys, _live, _own_nodes, _same_as_full_build,
                              _same_export, _same_rows, _undeclared_graph)

pytestmark = pytest.mark.gpu

S = SUBJECT_ID
T = RelationTuple.from_string
NODE = Q_NS | Q_OBJ | Q_REL
EVERYTHING = 0xFFFFFFFF
NO_ROWS = np.zeros((0, 6), np.uint32)


def reqs_of(qs):
    """kg_row_query records of (mask, tuple ids) pairs; `after` and `limit` are ignored by the delete (a limit
    of 0 would be refused by the listing: it is left at 0 here on purpose)."""
    return row_queries([m for m, _ in qs], np.asarray([t for _, t in qs], np.uint32).reshape(-1, 6), after=12345, limit=0)


class World:
    """A base snapshot and its rows as the reference needs them: a keyed base in key order with its keys, an
    unkeyed one in export order with keys None (the order keys are then positions + 1)."""

    def __init__(self, rows, it, keys=None, program=None, **kw):
        self.it, self.program, self.kw = it, program, kw
        self.snap = Snapshot(rows, it, program, keys=keys, **kw)
        self.keys = None if keys is None else np.asarray(keys, np.uint64)
        self.rows = np.asarray(rows, np.uint32).reshape(-1, 6) if keys is not None else self.snap.export()
        self.export = self.snap.export()

    @classmethod
    def of(cls, snap, rows, keys, it, program=None):
        """The world of a snapshot some call returned, with the rows and keys the reference gives it."""
        w = cls.__new__(cls)
        w.it, w.program, w.kw, w.snap, w.keys, w.export = it, program, {}, snap, keys, snap.export()
        w.rows = rows if keys is not None else w.export
        return w


def delete_and_compare(w: World, qs, what, nodes=None):
    """One call on w.snap with keys: the report against delete_ref and against kg_snapshot_query on the base,
    the returned snapshot's export (exactly: the base's export without the matched rows), rows() of every
    node and a full build.  Returns (snapshot or None, rows, keys) of the result."""
    reqs = reqs_of(qs)
    new, matched, dkeys, stats = w.snap.delete_matching(reqs, want_keys=True, with_stats=True)
    rows, keys, want_dead, want_matched = delete_ref(w.rows, w.keys, qs)
    assert matched.tolist() == want_matched.tolist(), (what, matched.tolist(), want_matched.tolist())
    assert stats["n_deleted"] == len(w.rows) - len(rows) == len(dkeys), (what, stats, len(w.rows) - len(rows))
    assert np.array_equal(dkeys, want_dead), (what, dkeys[:8], want_dead[:8])
    assert stats["rows_scanned"] == len(w.rows)
    # the listing of the same filters on the base: its keys and its counts
    lreqs = reqs.copy()
    lreqs["after"], lreqs["limit"] = 0, EVERYTHING
    _, lkeys, off, _, lmatched = w.snap.query(lreqs)
    assert lmatched.tolist() == matched.tolist(), what
    assert np.array_equal(np.sort(np.unique(lkeys)), np.unique(dkeys)), what
    if len(qs) == 1:
        assert np.array_equal(lkeys, dkeys), what
    if len(rows) == len(w.rows):
        assert new is None, what
        return None, rows, keys
    assert new is not None, what
    assert np.array_equal(new.export(), delete_ref(w.export, None, qs)[0]), what  # order kept, node ids unchanged
    nodes = nodes_of(w.rows) if nodes is None else nodes
    _same_rows(new, rows, nodes, what)
    _same_export(new, rows, what)
    full = Snapshot(rows, w.it, w.program, keys=keys)  # (an unkeyed result's rows are its export)
    (a_off, a), (b_off, b) = new.rows(nodes), full.rows(nodes)
    assert np.array_equal(a_off, b_off) and np.array_equal(a, b), what
    full.close()
    return new, rows, keys


def listing_agrees(snap, rows, keys, qs, what):
    """kg_snapshot_query on a result: whole listings of the given filters (tq.expect is the reference)."""
    if keys is None:
        rows, keys = snap.export(), np.arange(1, len(rows) + 1, dtype=np.uint64)
    qs = [(m, np.asarray(t, np.uint32)) for m, t in qs]
    tq.check_call(snap, rows, keys, qs, np.zeros(len(qs), np.uint64), np.full(len(qs), 5000, np.uint32))


def checks_agree(snap, rows, it, q6, what, prog=None, depths=None):
    """Engine checks at depths 1..6 equal the oracle on the rows (canonical policy), and the Go-order DFS where
    that agrees with it."""
    depths = (np.arange(len(q6)) % 6) + 1 if depths is None else depths
    out, err = Engine(snap, Config(6)).batch_check_ids(queries_array(q6, depths))
    oracle = Oracle(rows, it.wildcard_rel, prog)
    exp, oerr, _ = oracle.check_batch(q6, depths, 6, POLICY_CANONICAL)
    bad = np.nonzero((out != exp) | (err.astype(np.int64) != oerr))[0]
    assert bad.size == 0, (what, bad[:8], out[bad[:8]], exp[bad[:8]])
    dfs, _, _ = oracle.check_batch(q6, depths, 6, POLICY_DFS)
    inv = dfs == exp
    assert (out[inv] == dfs[inv]).all(), what
    return out


# ---------------------------------------------------------------- 1. every filter, keyed and unkeyed
def _filter_world(keyed):
    rng = np.random.default_rng(41)
    it, tuples, nss, rels = random_graph(rng, n_obj=30, n_rows=330, p_wild=0.25)  # subject sets name objects
    tuples += [tuples[i] for i in rng.integers(len(tuples), size=40)]  # duplicate rows
    rows = it.tuples_array(tuples)
    rows = rows[rng.permutation(len(rows))]
    keys = np.sort(rng.integers(1, 2**63, len(rows)).astype(np.uint64)) if keyed else None
    qs = random_queries(rng, nss, rels, 400, n_obj=30)
    q6 = np.asarray([it.tuple_ids(t) for t in qs], np.uint32)
    absent = (it.ns_id(nss[0]), it.obj_id("nobody"), it.rel_id(rels[0]))  # interned, in no row
    return World(rows, it, keys), q6, absent


def _subject_kinds(rows, absent, rng):
    """kind -> a row whose (ns, obj, rel) the query names, and the subject it asks for."""
    sid = rows[rows[:, 3] == S]
    sset = rows[(rows[:, 3] != S) & (rows[:, 5] != 0)]
    wild = rows[(rows[:, 3] != S) & (rows[:, 5] == 0)]
    any_row = rows[rng.integers(len(rows))]
    pick = lambda a: a[rng.integers(len(a))].copy()  # noqa: E731
    out = {"subject id": pick(sid), "subject set": pick(sset), "... set": pick(wild)}
    for kind, subj in (("absent id", (S, absent[1], 0)), ("id >= 2^31", (S, 0x90000000, 0)),
                       ("unknown set", (absent[0], absent[1], absent[2]))):
        t = any_row.copy()
        t[3:] = subj
        out[kind] = t
    return out


KINDS = ["subject id", "subject set", "... set", "absent id", "id >= 2^31", "unknown set"]


@pytest.fixture(scope="module", params=["keyed", "unkeyed"])
def filter_world(request):
    w, q6, absent = _filter_world(request.param == "keyed")
    yield w, q6, absent
    w.snap.close()


@pytest.mark.parametrize("kind", KINDS)
def test_every_filter(filter_world, kind):
    """All 16 masks with each kind of subject, one query a call, on a graph of 370 rows with duplicates."""
    w, q6, absent = filter_world
    rng = np.random.default_rng(KINDS.index(kind))
    t = _subject_kinds(w.rows, absent, rng)[kind]
    some = 0
    for mask in range(16):
        what = (kind, mask, t.tolist())
        new, rows, keys = delete_and_compare(w, [(mask, t)], what)
        if new is None:
            assert (mask & Q_SUBJECT) and kind in KINDS[3:], what  # only a subject no row has matches nothing
            continue
        some += 1
        probe = w.rows[rng.integers(len(w.rows))]
        listing_agrees(new, rows, keys, [(0, t), (mask, t), (NODE, probe), (Q_SUBJECT, probe), (Q_NS | Q_REL, t)], what)
        checks_agree(new, rows, w.it, q6, what)
        new.close()
    assert some >= 8


# ---------------------------------------------------------------- 2. range edges
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257])
def test_range_edges(n):
    """Bases of n row entries on two nodes, position p holding the subject id 6000 + p (and, in a second base,
    every even position the id 5000): the first entry, the last, every one and every second go, by subject
    alone (no owner search) and by namespace + subject (an owner per lane item, walked over the node edge)."""
    it = Interner()
    it.ns_id("n0")
    it.rel_id("r1")
    cut = (n + 1) // 2 if n > 1 else 1
    rows = np.zeros((n, 6), np.uint32)
    rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = np.where(np.arange(n) < cut, 1, 2), 1, S, 6000 + np.arange(n)
    even = rows.copy()
    even[::2, 4] = 5000
    for base_rows, subjects in ((rows, (6000, 6000 + n - 1, None)), (even, (5000,))):
        w = World(base_rows, it)
        assert np.array_equal(w.export, base_rows)  # positions are what the test says they are
        for subj in subjects:
            for extra in (0, Q_NS):
                q = (0, np.zeros(6, np.uint32)) if subj is None else (extra | Q_SUBJECT, np.asarray((0, 0, 0, S, subj, 0), np.uint32))
                what = (n, subj, extra)
                new, left, _ = delete_and_compare(w, [q], what)
                want = n if subj is None else ((n + 1) // 2 if subj == 5000 else 1)
                assert len(left) == n - want and new is not None, what
                assert new.info()["rows"] == n - want
                new.close()
        w.snap.close()


# ---------------------------------------------------------------- 3. hub
def test_hub_and_live_marking():
    """A keyed base with a 5 000-entry node among small ones: one of its subjects, which occurs three times,
    goes; then the whole node by (ns, obj, rel), which leaves it empty and its object named nowhere.  Both
    lookups on the result equal the oracle's over the live rows and a full build's: `n = not r` does not list
    the emptied object and an undeclared relation does not count it."""
    rng = np.random.default_rng(8)
    it = Interner()
    not_r = SubjectSetRewrite([InvertResult(ComputedSubjectSet("r"))])
    namespaces = [Namespace("a", [Relation("r"), Relation("n", rewrite=not_r)])]
    prog = compile_program(namespaces, it, lower_ttu=False)
    tuples = [T(f"a:hub#r@u{i}") if i % 4 else T(f"a:hub#r@(a:o{(i // 4) % 600}#r)") for i in range(5000)]
    tuples += [T("a:hub#r@thrice")] * 3
    tuples += [T(f"a:o{rng.integers(40)}#r@u{rng.integers(60)}") for _ in range(200)]
    tuples += [T(f"a:o{rng.integers(40)}#r@(a:o{rng.integers(40)}#r)") for _ in range(60)]
    rows = it.tuples_array(tuples)
    rows = rows[rng.permutation(len(rows))]
    keys = np.sort(rng.integers(1, 2**62, len(rows)).astype(np.uint64))
    w = World(rows, it, keys, prog)
    hub = np.asarray(it.tuple_ids(T("a:hub#r@thrice")), np.uint32)
    oreq = lo.requests_array(it, [T("a:any#n@stranger"), T("a:any#nope@u3"), T("a:any#n@u3"), T("a:any#r@u3"),
                                  T("a:any#r@thrice")], [0, 0, 0, 0, 0])
    sreq = ls.requests_array(it, [("a", "hub", "r"), ("a", "o3", "r"), ("a", "o3", "n"), ("a", "hub", "n")], [0, 2, 0, 0])

    def lookups(snap, rows, keys, what):
        oracle = Oracle(rows, it.wildcard_rel, prog)
        oref = lo.reference(oracle, lo.domains(rows), oreq, 5)
        sref = ls.reference(oracle, ls.subject_domain(rows), sreq, 5)
        full = Snapshot(rows, it, prog, keys=keys)
        for who, s in ((what, snap), (what + ", full build", full)):
            try:
                lo.compare(Engine(s, Config(5)), oreq, oref)
                ls.compare(Engine(s, Config(5)), sreq, sref)
            except AssertionError as x:
                raise AssertionError(f"{who}: {x}") from x
        full.close()
        return oref, sref

    oref, _ = lookups(w.snap, w.rows, w.keys, "base")
    hub_id = it.obj_id("hub")
    assert hub_id in oref[4][0] and oref[1][1] > 0
    assert oref[1][1] == len(lo.domains(w.rows)[it.ns_id("a")])  # the undeclared relation errs on the whole domain
    a, rows_a, keys_a = delete_and_compare(w, [(NODE | Q_SUBJECT, hub)], "thrice")
    assert len(rows_a) == len(rows) - 3
    oref, sref = lookups(a, rows_a, keys_a, "thrice gone")
    assert oref[4][0] == [] and len(sref[0][0]) > 3000
    b, rows_b, keys_b = delete_and_compare(World.of(a, rows_a, keys_a, it, prog), [(NODE, hub)], "the hub's node")
    assert len(rows_b) < 300 and len(node_rows(rows_b, [hub[:3]])[1]) == 0
    oref, sref = lookups(b, rows_b, keys_b, "hub emptied")
    dom = lo.domains(rows_b)[it.ns_id("a")]
    assert hub_id not in dom and len(oref[0][0]) == len(dom) and hub_id not in oref[0][0]  # `not` lists the rest
    assert oref[1][1] == len(dom)  # ... and the undeclared relation counts the rest
    assert sref[0][0] == []
    for s in (w.snap, a, b):
        s.close()


# ---------------------------------------------------------------- 4. many queries
def test_64_queries_in_one_call():
    """64 overlapping queries -- namespaces, nodes, relations, subject ids, subject sets, unknown ones, the
    same query twice -- in one call: per-query counts as delete_ref, every row counted once in n_deleted; the
    same 64 as single calls in a chain end at the same rows."""
    rng = np.random.default_rng(64)
    it, tuples, nss, rels = random_graph(rng, n_obj=40, n_rows=900, n_ns=4, n_rel=4)
    rows = it.tuples_array(tuples)
    keys = np.sort(rng.integers(1, 2**40, len(rows)).astype(np.uint64))  # a few ties
    w = World(rows, it, keys)
    qs = []
    for k in range(64):
        t = rows[rng.integers(len(rows))].copy()
        mask = [NODE, Q_SUBJECT, Q_OBJ, Q_NS | Q_REL | Q_SUBJECT, Q_REL | Q_OBJ, NODE | Q_SUBJECT, Q_OBJ | Q_SUBJECT][k % 7]
        if k % 16 == 5:
            t[4] = 0x7FFFFFF0  # a subject no row has
        qs.append((mask, t))
    qs[40] = qs[3]
    qs[63] = (Q_NS | Q_REL, rows[0].copy())  # a large share of one namespace
    new, left, left_keys = delete_and_compare(w, qs, "64 at once")
    matched = delete_ref(rows, keys, qs)[3]
    assert int(matched.sum()) > len(rows) - len(left) > 100 and (matched == 0).any()  # overlap, and idle queries
    checks = np.asarray([it.tuple_ids(t) for t in random_queries(rng, nss, rels, 400, n_obj=40)], np.uint32)
    checks_agree(new, left, it, checks, "64 at once")
    cur, cur_rows, cur_keys, built = w.snap, rows, keys, 0
    for i, q in enumerate(qs):
        nxt, m, _ = cur.delete_matching(reqs_of([q]))
        cur_rows, cur_keys, _, want = delete_ref(cur_rows, cur_keys, [q])
        assert m.tolist() == want.tolist(), i
        if nxt is not None:
            if cur is not w.snap:
                cur.close()
            cur, built = nxt, built + 1
    assert 10 < built < 64  # later queries find their rows gone already
    assert np.array_equal(cur_rows, left) and np.array_equal(cur_keys, left_keys)
    assert np.array_equal(cur.export(), new.export())
    _same_rows(cur, left, nodes_of(rows), "64 in a chain")
    for s in (cur, new, w.snap):
        s.close()


# ---------------------------------------------------------------- 5. no match, n = 0
def test_no_match_and_no_queries_build_nothing():
    rng = np.random.default_rng(5)
    it, tuples, nss, rels = random_graph(rng, n_obj=30, n_rows=300)
    rows = it.tuples_array(tuples)
    keys = np.sort(rng.integers(1, 4000, len(rows)).astype(np.uint64))
    w = World(rows, it, keys)
    info = w.snap.info()
    q6 = np.asarray([it.tuple_ids(t) for t in random_queries(rng, nss, rels, 300, n_obj=30)], np.uint32)
    before = checks_agree(w.snap, rows, it, q6, "before")
    none = [(Q_OBJ, np.asarray((0, it.obj_id("nobody"), 0, 0, 0, 0), np.uint32)),
            (Q_SUBJECT, np.asarray((0, 0, 0, S, 0x80000001, 0), np.uint32)),
            (Q_NS, np.asarray((0xFFFF, 0, 0, 0, 0, 0), np.uint32)),
            (NODE | Q_SUBJECT, np.concatenate([rows[0, :3], [S, 0x7FFFFFF0, 0]]).astype(np.uint32))]
    for qs in (none, none[:1], []):
        new, matched, dkeys, stats = w.snap.delete_matching(reqs_of(qs) if qs else np.zeros(0, _lib.ROW_QUERY_DTYPE),
                                                            want_keys=True, with_stats=True)
        assert new is None and matched.tolist() == [0] * len(qs) and len(dkeys) == 0 and stats["n_deleted"] == 0
    new, matched, dkeys = w.snap.delete_matching(np.zeros(0, _lib.ROW_QUERY_DTYPE))
    assert new is None and len(matched) == 0 and dkeys is None
    assert w.snap.info() == info
    assert (checks_agree(w.snap, rows, it, q6, "after") == before).all()
    # the base kept its host node map: an apply on it is the ordinary one
    ins = it.tuples_array([T(f"{nss[0]}:fresh#{rels[0]}@u1"), tuples[5]])
    ik = np.asarray([17, 3999], np.uint64)
    dels = rows[rng.choice(len(rows), 30, replace=False)]
    new = w.snap.apply(ins, dels, ik)
    rows1, keys1 = apply_ref(rows, keys, ins, ik, dels)
    nodes = nodes_of(rows, ins)
    _same_rows(new, rows1, nodes, "apply on the base")
    _same_export(new, rows1, "apply on the base")
    _same_as_full_build(new, rows1, keys1, it, nodes, "apply on the base")
    checks_agree(new, rows1, it, q6, "apply on the base")
    new.close()
    w.snap.close()


# ---------------------------------------------------------------- 6. everything
@pytest.mark.parametrize("keyed", [True, False])
def test_mask_zero_empties_the_snapshot(keyed):
    rng = np.random.default_rng(6)
    it, tuples, nss, rels = random_graph(rng, n_obj=30, n_rows=300)
    rows = it.tuples_array(tuples)
    keys = np.sort(rng.integers(1, 4000, len(rows)).astype(np.uint64)) if keyed else None
    w = World(rows, it, keys)
    # the all-rows query among others: every row still counts once
    new, left, _ = delete_and_compare(w, [(Q_NS, rows[0]), (0, np.zeros(6, np.uint32)), (Q_SUBJECT, rows[1])], "everything")
    assert len(left) == 0 and len(new.export()) == 0 and new.info()["rows"] == 0
    assert new.info()["nodes"] == w.snap.info()["nodes"]  # the nodes stay behind, empty
    q6 = np.concatenate([rows, np.asarray([it.tuple_ids(t) for t in random_queries(rng, nss, rels, 300, n_obj=30)], np.uint32)])
    out, err = Engine(new, Config(6)).batch_check_ids(queries_array(q6, 0))
    assert (out == 0).all() and (err == 0).all()
    empty, matched, dkeys = new.delete_matching(reqs_of([(0, np.zeros(6, np.uint32))]), want_keys=True)
    assert empty is None and matched.tolist() == [0] and len(dkeys) == 0  # a base without rows
    fresh = it.tuples_array(tuples[:50] + [T(f"{nss[1]}:brand#{rels[1]}@({nss[0]}:new#{rels[0]})")])
    fk = np.sort(rng.integers(1, 4000, len(fresh)).astype(np.uint64)) if keyed else None
    again = new.apply(fresh, NO_ROWS, fk)
    nodes = nodes_of(rows, fresh)
    _same_rows(again, fresh, nodes, "inserts into the emptied snapshot")
    _same_export(again, fresh, "inserts into the emptied snapshot")
    _same_as_full_build(again, fresh, fk, it, nodes, "inserts into the emptied snapshot")
    checks_agree(again, fresh, it, q6, "inserts into the emptied snapshot")
    for s in (again, new, w.snap):
        s.close()


# ---------------------------------------------------------------- 7. chains and the base
def test_chain_and_base_stays_valid():
    """delete -> apply -> delete -> apply, each step against delete_ref / apply_ref in rows, checks and expand
    trees; the first base answers the same before, after, and after its children are closed."""
    rng = np.random.default_rng(71)
    it, tuples, nss, rels = random_graph(rng, n_obj=50, n_rows=900)
    arr = it.tuples_array(tuples)
    rows0, pool = arr[:600], arr[600:]
    keys0 = np.sort(rng.integers(1, 4000, 600)).astype(np.uint64)
    q6 = np.asarray([it.tuple_ids(t) for t in random_queries(rng, nss, rels, 1200, n_obj=50)], np.uint32)
    depths = rng.integers(0, 7, len(q6))
    roots = np.asarray([[it.ns_id(rng.choice(nss)), it.obj_id(f"o{rng.integers(52)}"), it.rel_id(rng.choice(rels)), 0]
                        for _ in range(100)], np.uint32)
    nodes = nodes_of(arr)

    def ask(snap, rows, what):
        out = checks_agree(snap, rows, it, q6, what, depths=depths)
        oracle = Oracle(rows, it.wildcard_rel)
        trees = ExpandEngine(snap, Config(5)).build_trees_ids(roots)
        for r, g in zip(roots.tolist(), trees):
            _cmp_records(oracle.expand(r[0], r[1], r[2], 0, 5), g, (what, r))
        _same_rows(snap, rows, nodes, what)
        _same_export(snap, rows, what)
        return out, trees, snap.rows(nodes)

    def same(x, y):
        assert (x[0] == y[0]).all() and np.array_equal(x[2][0], y[2][0]) and np.array_equal(x[2][1], y[2][1])
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(x[1], y[1]))

    base = World(rows0, it, keys0)
    before = ask(base.snap, rows0, "base before")
    w, made = base, []
    for lo_ in (0, 150):
        sid = w.rows[w.rows[:, 3] == S][rng.integers(50)]
        sset = w.rows[w.rows[:, 3] != S][rng.integers(50)]
        qs = [(Q_SUBJECT, sid), (Q_NS | Q_OBJ, w.rows[rng.integers(len(w.rows))]), (Q_SUBJECT, sset)]
        a, rows_a, keys_a = delete_and_compare(w, qs, ("delete", lo_), nodes)
        assert a is not None
        ask(a, rows_a, ("delete", lo_))
        ins, ik = pool[lo_:lo_ + 150], rng.integers(1, 4000, 150).astype(np.uint64)
        dels = rows_a[rng.choice(len(rows_a), 30, replace=False)]
        b = a.apply(ins, dels, ik)
        rows_b, keys_b = apply_ref(rows_a, keys_a, ins, ik, dels)
        ask(b, rows_b, ("apply", lo_))
        _same_as_full_build(b, rows_b, keys_b, it, nodes, ("apply", lo_))
        made += [a, b]
        w = World.of(b, rows_b, keys_b, it)
    same(ask(base.snap, rows0, "base after"), before)
    last = ask(made[-1], w.rows, "the last of the chain")
    for s in made[:-1]:
        s.close()
    same(ask(base.snap, rows0, "base after its children are closed"), before)
    same(ask(made[-1], w.rows, "the last, alone"), last)
    made[-1].close()
    base.snap.close()


# ---------------------------------------------------------------- 8. programs
@pytest.mark.parametrize("mat", [1, 0])
@pytest.mark.parametrize("program", ["random", "formula"])
def test_rewrites_after_delete(program, mat, monkeypatch):
    """The pattern of test_gpu_refresh.test_rewrites_after_refresh with deletes by query: every call takes the
    last own row of a rewritten relation from some objects (a node delete), every row of a subject id, and a
    whole relation of one namespace.  Answers, error codes and the number of queries left to the interpreter
    equal a full build's from delete_ref's rows, and the oracle's."""
    monkeypatch.setenv("KG_MATERIALIZE", str(mat))
    rng = np.random.default_rng(800 + (1 if program == "formula" else 0))
    it = Interner()
    n_obj, n_users = 50, 25
    if program == "formula":
        namespaces, nss = _formula_namespaces(), ["d"]
        tuples = _formula_graph(rng, n_obj, n_users, 750)
        qrels = ["a", "u1", "u2", "u3", "f1", "f2", "f3", "f4", "f5", "f6", "f7"]
        qs = [T(f"d:o{rng.integers(n_obj + 2)}#{rng.choice(qrels)}@u{rng.integers(n_users + 2)}") for _ in range(1500)]
    else:
        nss, rels = ["a", "b", "c"], ["r0", "r1", "r2", "r3"]
        namespaces = random_program(rng, nss, rels, unions_only=False)
        tuples = _undeclared_graph(rng, nss, rels, n_obj, n_users, 750)
        qs = random_queries(rng, nss, rels, 1500, n_obj=n_obj, n_users=n_users)
    prog = compile_program(namespaces, it, lower_ttu=False)  # the oracle: TTU leaves as written
    rewritten = sorted((n.name, r.name) for n in namespaces for r in n.relations if r.rewrite is not None)
    m = SnapshotPersister(namespaces=namespaces, interner=it, max_read_depth=5, seed=mat)  # the program, the shard ids
    m.write_relation_tuples(*tuples)
    rows, keys = shard_rows(m), _keys(m)
    q6 = np.asarray([it.tuple_ids(t) for t in qs], np.uint32)
    depths = rng.integers(-1, 7, len(qs))
    cur = Snapshot(rows, it, m.program, keys=keys)
    lost, general, errors = 0, 0, 0
    for step in range(4):
        live = [it.relation_tuple(r) for r in rows]
        own = sorted(_own_nodes(live, set(rewritten)))
        assert len(own) >= 3, step
        dq = [(NODE, np.asarray(it.tuple_ids(RelationTuple(*node, subject_id="x")), np.uint32))
              for node in own[::max(1, len(own) // 3)][:3]]
        ids = rows[rows[:, 3] == S]
        dq.append((Q_SUBJECT, ids[rng.integers(len(ids))]))
        if step == 2:
            dq.append((Q_NS | Q_REL, rows[rng.integers(len(rows))]))
        reqs = reqs_of(dq)
        nxt, matched, dkeys = cur.delete_matching(reqs, want_keys=True)
        rows, keys, want_dead, want_matched = delete_ref(rows, keys, dq)
        assert nxt is not None and matched.tolist() == want_matched.tolist() and np.array_equal(dkeys, want_dead)
        lost += len(own) - len(_own_nodes([it.relation_tuple(r) for r in rows], set(rewritten)))
        cur.close()
        cur = nxt
        _same_export(cur, rows, step)
        full = Snapshot(rows, it, m.program, keys=keys)
        e, ef = Engine(cur, m.config), Engine(full, m.config)
        out, err = e.batch_check_ids(queries_array(q6, depths), with_stats=True)
        fout, ferr = ef.batch_check_ids(queries_array(q6, depths), with_stats=True)
        assert (out == fout).all() and (err == ferr).all(), (step, np.nonzero(out != fout)[0][:8])
        assert e.last_stats["n_general"] == ef.last_stats["n_general"], (step, e.last_stats["n_general"],
                                                                         ef.last_stats["n_general"])
        general += e.last_stats["n_general"]
        exp, oerr, _ = Oracle(rows, it.wildcard_rel, prog).check_batch(q6, depths, 5, POLICY_CANONICAL)
        bad = np.nonzero((out != exp) | (err.astype(np.int64) != oerr))[0]
        assert bad.size == 0, (step, [(str(qs[i]), int(depths[i]), int(out[i]), int(err[i]), int(exp[i]), int(oerr[i]))
                                      for i in bad[:8]])
        errors += int((exp == 2).sum())
        if step == 3:
            trees = 0
            for t, d in zip(qs[:60], depths[:60].tolist()):
                ra, rb = e.check_relation_tuple(t, d), ef.check_relation_tuple(t, d)
                assert ra.membership == rb.membership and (ra.err and ra.err.code) == (rb.err and rb.err.code), str(t)
                assert ra.tree == rb.tree, str(t)
                trees += ra.tree is not None
            assert trees > 0
        full.close()
    cur.close()
    assert lost >= 9 and general > 0 and errors > 0, (lost, general, errors)


# ---------------------------------------------------------------- 9. stride loops
def test_stride_loops_synthetic_base():
    """An unkeyed device-generated base (Snapshot.synthetic(1_000_000): 821 312 rows on 187 496 nodes); one call
    deletes a hot user's subject id everywhere and the group namespace's member relation.  The launches are
    capped at two 256-thread workgroups per CU (one for the per-node kernels), so on the 256 CUs of an MI355X
    k_del_rows covers 2 * 256 * 256 * 4 = 524 288 entries a trip (2 trips), k_del_scatter and k_del_keys
    131 072 (7 trips), k_del_nodes and k_del_newoff 65 536 nodes (3 trips) -- asserted below from the device's
    CU count."""
    from test_gpu_check import _torch
    torch = _torch()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    base = Snapshot.synthetic(1_000_000, seed=20250131)
    rows0 = base.export()
    info = base.info()
    print("synthetic base:", info, "CUs:", n_cu)
    assert len(rows0) > 2 * n_cu * 256 * 4  # k_del_rows: a second trip (and the per-entry kernels' fourth)
    assert info["nodes"] > n_cu * 256  # k_del_nodes, k_del_newoff: a second trip
    ids, counts = np.unique(rows0[rows0[:, 3] == S, 4], return_counts=True)
    hot = int(ids[np.argmax(counts)])
    GROUP, MEMBER = 1, 2  # the generator's ids (include/ketogpu.h)
    qs = [(Q_SUBJECT, (0, 0, 0, S, hot, 0)), (Q_NS | Q_REL, (GROUP, 0, MEMBER, 0, 0, 0))]
    new, matched, dkeys, stats = base.delete_matching(reqs_of(qs), want_keys=True, with_stats=True)
    rows1, _, want_dead, want_matched = delete_ref(rows0, None, qs)
    print("deleted", stats, "matched", matched.tolist())
    assert matched.tolist() == want_matched.tolist() and int(counts.max()) > 100 and want_matched[1] > 10_000
    assert np.array_equal(dkeys, want_dead) and stats["n_deleted"] == len(rows0) - len(rows1)
    assert np.array_equal(new.export(), rows1)
    nodes = rows0[np.random.default_rng(9).choice(len(rows0), 3000, replace=False), :3]  # nodes may repeat
    _same_rows(new, rows1, nodes, "synthetic")
    n, gmax = 20000, 10
    dq = torch.empty((n, 7), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().kg_synth_queries(base.handle, 7, n, dq.data_ptr()), "kg_synth_queries")
    q = dq.cpu().numpy().view(np.uint32)
    out, err = Engine(new, Config(gmax)).batch_check_ids(q)
    exp, oerr, _ = Oracle(rows1, 0).check_batch(q[:, :6], q[:, 6].view(np.int32), gmax, POLICY_CANONICAL, nthreads=8)
    assert (err == 0).all() and (oerr == 0).all()
    assert (out == exp).all(), np.nonzero(out != exp)[0][:10]
    base0, _ = Engine(base, Config(gmax)).batch_check_ids(q)
    assert (base0 != exp).any() and (exp == 1).any()  # the delete changed answers, and members remain
    new.close()
    base.close()


# ---------------------------------------------------------------- 10. replicas
def test_delete_per_replica():
    """devices=[0, 0]: the match runs once for replica 0 and again on the second replica's own device copy.
    kg_snapshot_query rotates over the replicas, so two calls in a row read the rows of both; a host batch
    large enough to be split reads both too."""
    rng = np.random.default_rng(10)
    it, tuples, nss, rels = random_graph(rng, n_obj=60, n_rows=700)
    rows = it.tuples_array(tuples)
    keys = np.sort(rng.integers(1, 2**50, len(rows)).astype(np.uint64))
    w = World(rows, it, keys, devices=[0, 0])
    assert w.snap.replicas() == [0, 0]
    sid = rows[rows[:, 3] == S][3]
    qs = [(Q_SUBJECT, sid), (Q_NS | Q_REL, rows[7]), (NODE, rows[11])]
    new, left, left_keys = delete_and_compare(w, qs, "replicas")
    assert new.replicas() == [0, 0] and 0 < len(left) < len(rows) - 50
    nodes = nodes_of(rows)
    per_node = [(NODE, np.concatenate([nd, [0, 0, 0]]).astype(np.uint32)) for nd in nodes[:60]]
    for call in range(2):  # replica 0, replica 1
        listing_agrees(new, left, left_keys, [(0, rows[0])] + per_node, ("replica call", call))
    q6 = np.tile(np.asarray([it.tuple_ids(t) for t in random_queries(rng, nss, rels, 1000, n_obj=60)], np.uint32), (40, 1))
    depths = np.tile(rng.integers(0, 7, 1000), 40)
    out, err = Engine(new, Config(5)).batch_check_ids(queries_array(q6, depths))  # 40 000 queries: split over both
    exp, oerr, _ = Oracle(left, it.wildcard_rel).check_batch(q6, depths, 5, POLICY_CANONICAL)
    assert (out == exp).all() and (err == 0).all() and (oerr == 0).all(), np.nonzero(out != exp)[0][:8]
    old, _ = Engine(w.snap, Config(5)).batch_check_ids(queries_array(q6, depths))
    assert (old != out).any()
    new.close()
    w.snap.close()


# ---------------------------------------------------------------- 11. persister
def test_persister_device_deletes_match_host_deletes():
    """Two persisters with one seed (the same shard ids), one deleting on the device and reading from it, one
    in host mode, through the same writes, transactions and five delete_all calls: by namespace, by object, by
    subject id, by subject set, and by a string never seen.  After each: the same pages, the same length, and
    checks equal to the oracle."""
    rng = np.random.default_rng(111)
    _, tuples, nss, rels = random_graph(rng, n_obj=40, n_rows=700, n_ns=3)  # (each persister interns for itself)
    dev = SnapshotPersister(seed=21, device_deletes=True, device_reads=True)
    host = SnapshotPersister(seed=21)
    both = (dev, host)
    e = dev.permission_engine()
    qs = random_queries(rng, nss, rels, 800, n_obj=40)
    depths = rng.integers(0, 7, len(qs))

    def agree(what):
        for q in (RelationQuery(), RelationQuery(nss[0]), RelationQuery(object="o3"), RelationQuery(subject_id="u5")):
            for size in (7, 0):
                th = td = ""
                while True:
                    rh, th = host.get_relation_tuples(q, th, size)
                    rd, td = dev.get_relation_tuples(q, td, size)
                    assert rd == rh and td == th, (what, q, size)
                    if not th:
                        break
        assert len(dev) == len(host), what
        it = dev.interner
        q6 = np.asarray([it.tuple_ids(t) for t in qs], np.uint32)
        out, err = e.batch_check_ids(queries_array(q6, depths))
        rows = it.tuples_array(t for _, t in host._rows)  # the host persister's rows in shard order, as dev's ids
        exp, oerr, _ = Oracle(rows, it.wildcard_rel).check_batch(q6, depths, 5, POLICY_CANONICAL)
        assert (out == exp).all() and (err == 0).all() and (oerr == 0).all(), (what, np.nonzero(out != exp)[0][:8])
        return exp

    for p in both:
        p.write_relation_tuples(*tuples[:400])
    agree("first build")
    for p in both:
        p.transact_relation_tuples(tuples[400:550], [tuples[i] for i in range(0, 60, 2)])
    seen = [agree("transaction")]
    deletes = [lambda live: RelationQuery(namespace=nss[2]),
               lambda live: RelationQuery(object=live[len(live) // 2].object),
               lambda live: RelationQuery(subject_id=next(t.subject_id for t in live if t.subject_id is not None)),
               lambda live: RelationQuery(subject_set=next(t.subject_set for t in live if t.subject_set is not None)),
               lambda live: RelationQuery(namespace=nss[0], object="never seen")]
    n_names = None
    for k, make in enumerate(deletes):
        dq = make(_live(host))  # what it names is in a live row (but for the last)
        applies, length = dev.applies, len(host)
        if k == 4:
            n_names = len(dev.interner._obj_names)
        for p in both:
            p.delete_all_relation_tuples(dq)
        assert dev.applies == applies, dq  # no tuple delta: the delete itself built the snapshot
        assert dev.device_deletes_done == min(k + 1, 4) and not dev._p_del and not dev._p_ins
        assert (len(host) < length) == (k < 4), dq
        seen.append(agree(dq))
        if k == 1:  # writes between the deletes: the next delete first applies them
            for p in both:
                p.transact_relation_tuples(tuples[550:], [tuples[i] for i in range(100, 130)])
            seen.append(agree("transaction between deletes"))
    assert n_names == len(dev.interner._obj_names)  # the unknown string was not interned
    assert dev.device_deletes_done == 4 and host.device_deletes_done == 0 and host._snap is None
    assert dev.rebuilds == 1 and dev.applies == 2
    assert sum((a != b).any() for a, b in zip(seen, seen[1:])) >= 3  # the deletes changed answers
