"""GPU tests of the lookups' formula mode: a request on a boolean rewrite (and / or / not over plain and
union relations, kg_formula.hip) takes its candidates from a walk over the plan's walk leaves and from the
impure nodes of its relation and leaves, not from the whole domain.  The answers stay those of the check
(CPU oracle, and the same engine with kg_snapshot_tune "lookup_formula" 0); the counters say how many checks
they cost.

  1  a hand fixture whose counters follow from the walk leaves J = {u} of share = u & !blocked
  2  random formula graphs against the oracle, the key at 0 and a snapshot built without materialisation
  3  an object that is a candidate several times over is checked, and its error counted, once
  4  the candidate key list regrows
  5  after every transaction of a persister
  6  four threads
"""
import threading

import numpy as np
import pytest

import test_gpu_lookup as lo
import test_gpu_lookup_subjects as ls
from keto_amd.engine import Config, Engine, Registry, Snapshot
from keto_amd.ketoapi import RelationTuple
from keto_amd.mapper import Interner
from keto_amd.namespace import (ComputedSubjectSet, InvertResult, Namespace, Relation, SubjectSetRewrite,
                                compile_program)
from keto_amd.persister import RelationQuery, SnapshotPersister
from oracle.oracle import Oracle
from test_gpu_persister import shard_rows
from test_gpu_refresh import _formula_graph, _formula_namespaces, _keys

pytestmark = pytest.mark.gpu

T = RelationTuple.from_string
KEYS = ("n_objs", "exact", "candidates", "confirmed")


def stats(e, kind, reqs):
    (e.lookup_objects_ids if kind == "objects" else e.lookup_subjects_ids)(reqs, with_stats=True)
    return tuple(int(e.last_stats[k]) for k in KEYS)


# ---------------------------------------------------------------- 1. the hand fixture
def hand_namespaces():
    C, N, O = ComputedSubjectSet, InvertResult, SubjectSetRewrite
    d = Namespace("d", [Relation("a"), Relation("b"), Relation("blocked"),
                        Relation("u", rewrite=O([C("a"), C("b")])),
                        Relation("share", rewrite=O([C("u"), N(C("blocked"))], "and"))])
    return [d, Namespace("g", [Relation("m")])]


def hand_tuples(n_alice=5):
    """alice holds a on o0 .. o{n_alice-1} and reaches b on o5, o6, o7 through g:core -> g:team (two levels
    of subject sets, so from depth 3 on); filler holds a on 200 objects; alice is blocked on o0 and o5, which
    she would share, and on o100 .. o103, which she does not reach through u."""
    tuples = [T(f"d:o{i}#a@filler") for i in range(200)] + [T(f"d:o{i}#a@alice") for i in range(n_alice)]
    tuples += [T(f"d:o{i}#b@(g:team#m)") for i in (5, 6, 7)]
    tuples += [T("g:team#m@(g:core#m)"), T("g:core#m@alice")] + [T(f"g:other#m@x{k}") for k in range(50)]
    tuples += [T(f"d:o{i}#blocked@alice") for i in (0, 5, 100, 101, 102, 103)]
    return tuples


@pytest.fixture(scope="module")
def hand():
    it = Interner()
    namespaces, tuples = hand_namespaces(), hand_tuples()
    reg = Registry(tuples, namespaces, interner=it, max_read_depth=10)
    yield reg, it
    reg.snapshot.tune("lookup_formula", 1)


def names(it, ids):
    return sorted((it.obj_name(int(i)) for i in ids), key=lambda s: (len(s), s))


@pytest.mark.parametrize("through_global", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3, 5])
def test_hand_objects_alice(hand, d, through_global):
    """d:*#share@alice.  The walk listens to u alone: its candidates are the members of u -- o0 .. o4 at
    depth 1 and 2, o5, o6, o7 too from depth 3 -- and not o100 .. o103, where alice is only blocked.  The
    blocked o0 and o5 are checked and dropped; nothing is listed without a check."""
    reg, it = hand
    reg.snapshot.tune("lookup_formula", 1)
    e = Engine(reg.snapshot, Config(d if through_global else 10))
    reqs = lo.requests_array(it, [T("d:any#share@alice")], [0 if through_global else d])
    off, objs, err, nerr = e.lookup_objects_ids(reqs, with_stats=True)
    got = tuple(int(e.last_stats[k]) for k in KEYS)
    want = ["o1", "o2", "o3", "o4"] + (["o6", "o7"] if d >= 3 else [])
    print("objects alice", d, through_global, got)
    assert names(it, objs) == want and not nerr.any()
    assert got == ((4, 0, 5, 4) if d < 3 else (6, 0, 8, 6)), got
    reg.snapshot.tune("lookup_formula", 0)
    off0, objs0, err0, nerr0 = e.lookup_objects_ids(reqs, with_stats=True)
    assert np.array_equal(objs, objs0) and not nerr0.any()
    assert e.last_stats["candidates"] == 200, e.last_stats  # every object of d
    reg.snapshot.tune("lookup_formula", 1)


@pytest.mark.parametrize("subject,listed,candidates", [
    ("(g:team#m)", ["o5", "o6", "o7"], 3), ("(g:core#m)", ["o5", "o6", "o7"], 3),
    ("filler", [f"o{i}" for i in range(200)], 200), ("x3", [], 0)])
def test_hand_objects_other_subjects(hand, subject, listed, candidates):
    reg, it = hand
    reg.snapshot.tune("lookup_formula", 1)
    e = Engine(reg.snapshot, Config(10))
    reqs = lo.requests_array(it, [T(f"d:any#share@{subject}")], [5])
    off, objs, err, nerr = e.lookup_objects_ids(reqs, with_stats=True)
    got = tuple(int(e.last_stats[k]) for k in KEYS)
    print("objects", subject, got)
    assert names(it, objs) == listed and not nerr.any()
    assert got == (len(listed), 0, candidates, len(listed)), got


@pytest.mark.parametrize("obj,d,listed,candidates", [
    ("o0", 5, ["filler"], 2), ("o1", 5, ["alice", "filler"], 2), ("o5", 5, ["filler"], 2), ("o5", 1, ["filler"], 1),
    ("o5", 2, ["filler"], 1), ("o100", 5, ["filler"], 1), ("o150", 5, ["filler"], 1), ("o999", 5, [], 0)])
def test_hand_subjects(hand, obj, d, listed, candidates):
    """d:obj#share: the forward walk from the object's u node lists its candidates -- filler and, where she
    reaches u within the depth, alice -- and the check drops the blocked alice.  An object without a u node is
    empty without a check.  With the key at 0 every one of the 52 subject ids is checked."""
    reg, it = hand
    reg.snapshot.tune("lookup_formula", 1)
    e = Engine(reg.snapshot, Config(10))
    reqs = ls.requests_array(it, [("d", obj, "share")], [d])
    off, ids, err, nerr = e.lookup_subjects_ids(reqs, with_stats=True)
    got = tuple(int(e.last_stats[k]) for k in KEYS)
    print("subjects", obj, d, got)
    assert sorted(it.obj_name(int(i)) for i in ids) == listed and not nerr.any()
    assert got == (len(listed), 0, candidates, len(listed)), got
    reg.snapshot.tune("lookup_formula", 0)
    off0, ids0, err0, nerr0 = e.lookup_subjects_ids(reqs, with_stats=True)
    assert np.array_equal(ids, ids0) and not nerr0.any()
    assert e.last_stats["candidates"] == 52, e.last_stats
    reg.snapshot.tune("lookup_formula", 1)


def test_hand_against_oracle(hand):
    """Every request of the tables above in one call of each kind (formula bits beside reverse bits of u and
    a in one walk group), against the oracle."""
    reg, it = hand
    reg.snapshot.tune("lookup_formula", 1)
    t6 = it.tuples_array(hand_tuples())
    oracle = Oracle(t6, it.wildcard_rel, compile_program(hand_namespaces(), it))
    subs = ["alice", "filler", "x3", "nobody", "(g:team#m)", "(g:core#m)", "(d:o5#u)"]
    qs = [T(f"d:any#{r}@{s}") for r in ("share", "u", "a", "blocked") for s in subs for _ in range(4)]
    oreq = lo.requests_array(it, qs, [1, 2, 3, 5] * (len(qs) // 4))
    roots = [("d", o, r) for r in ("share", "u") for o in ("o0", "o1", "o5", "o100", "o150", "o999") for _ in range(4)]
    sreq = ls.requests_array(it, roots, [1, 2, 3, 5] * (len(roots) // 4))
    e = Engine(reg.snapshot, Config(10))
    lo.compare(e, oreq, lo.reference(oracle, lo.domains(t6), oreq, 10))
    ls.compare(e, sreq, ls.reference(oracle, ls.subject_domain(t6), sreq, 10))


# ---------------------------------------------------------------- 2. against the oracle
QRELS = ["a", "u1", "u2", "u3", "f1", "f3", "f4", "f6", "f7", "nope", "f2", "f5"]
DEPTHS = list(range(-1, 8))


@pytest.mark.parametrize("seed", range(6))
def test_formula_graphs_vs_oracle(seed, monkeypatch):
    rng = np.random.default_rng(4100 + seed)
    n_obj, n_users = 40, 30
    it, namespaces = Interner(), _formula_namespaces()
    prog = compile_program(namespaces, it, lower_ttu=False)
    tuples = _formula_graph(rng, n_obj, n_users, 600)
    t6 = it.tuples_array(tuples)
    subs = [f"u{k}" for k in (0, 7, 19, n_users + 1)] + [f"(d:o{o}#u2)" for o in (3, 11)]
    qs = [T(f"d:any#{r}@{s}") for r in QRELS for s in subs for _ in DEPTHS]
    oreq = lo.requests_array(it, qs, DEPTHS * (len(qs) // len(DEPTHS)))
    roots = [("d", f"o{o}", r) for r in QRELS for o in (1, 5, 17, n_obj + 1) for _ in DEPTHS]
    sreq = ls.requests_array(it, roots, DEPTHS * (len(roots) // len(DEPTHS)))
    oracle = Oracle(t6, it.wildcard_rel, prog)
    dom, sdom = lo.domains(t6), ls.subject_domain(t6)
    oref, sref = lo.reference(oracle, dom, oreq, 5), ls.reference(oracle, sdom, sreq, 5)

    snap = Snapshot(t6, it, prog)
    e = Engine(snap, Config(5))
    rel = {r: it.rel_id(r) for r in QRELS}
    of12 = oreq[np.isin(oreq[:, 1], [rel["f1"], rel["f2"]])]
    sf12 = sreq[np.isin(sreq[:, 2], [rel["f1"], rel["f2"]])]
    of37 = oreq[np.isin(oreq[:, 1], [rel["f3"], rel["f7"]])]
    cand = {}
    for key in (1, 0):
        snap.tune("lookup_formula", key)
        lo.compare(e, oreq, oref)
        ls.compare(e, sreq, sref)
        cand[key] = (stats(e, "objects", of12)[2], stats(e, "subjects", sf12)[2])
        # f(0) = true: every object of the namespace stays a candidate
        assert stats(e, "objects", of37)[2] == len(of37) * len(dom[it.ns_id("d")])
    print("candidates of f1 / f2, key on and off:", cand)
    assert cand[1][0] <= cand[0][0] and cand[1][1] <= cand[0][1], cand
    assert cand[0] == (len(of12) * len(dom[it.ns_id("d")]), len(sf12) * len(sdom)), cand
    snap.close()

    monkeypatch.setenv("KG_MATERIALIZE", "0")  # no unions, no plans: the interpreter answers every candidate
    plain = Snapshot(t6, it, prog)
    e0 = Engine(plain, Config(5))
    lo.compare(e0, oreq, oref)
    ls.compare(e0, sreq, sref)
    assert stats(e0, "objects", of12)[2] == cand[0][0]
    plain.close()


# ---------------------------------------------------------------- 3. duplicates and errors once
def test_candidate_once():
    """f2 = (u2 & !a) | blocked has the walk leaves {u2, blocked}.  p has an impure node on two leaves (a and
    blocked rows that name the undeclared d:x#und) and impure union nodes above the first; q is reached
    through both walk leaves; r and s through u2 alone.  x occurs only inside the subject sets.  Each of p, q,
    r, s is one candidate: the error of p is counted once, q is confirmed once."""
    it, namespaces = Interner(), _formula_namespaces()
    prog = compile_program(namespaces, it, lower_ttu=False)
    tuples = [T("d:p#a@(d:x#und)"), T("d:p#blocked@(d:x#und)"), T("d:q#b@bob"), T("d:q#blocked@bob"), T("d:r#a@bob"),
              T("d:s#b@bob"), T("d:s#b@carol")]
    t6 = it.tuples_array(tuples)
    oracle = Oracle(t6, it.wildcard_rel, prog)
    snap = Snapshot(t6, it, prog)
    e = Engine(snap, Config(5))
    oreq = lo.requests_array(it, [T("d:any#f2@bob")], [5])
    oref = lo.reference(oracle, lo.domains(t6), oreq, 5)
    assert oref[0][1] >= 1, oref  # p errs
    lo.compare(e, oreq, oref)
    got = tuple(int(e.last_stats[k]) for k in KEYS)
    print("f2@bob", got, oref)
    assert got == (len(oref[0][0]), 0, 4, len(oref[0][0])), got
    roots = [("d", o, "f2") for o in ("p", "q", "r", "s", "x")]
    sreq = ls.requests_array(it, roots, [5] * len(roots))
    sref = ls.reference(oracle, ls.subject_domain(t6), sreq, 5)
    ls.compare(e, sreq, sref)
    n_listed = sum(len(r[0]) for r in sref)
    got = tuple(int(e.last_stats[k]) for k in KEYS)
    print("f2 subjects", got, sref)
    # p is confirmed over the 2 subject ids (an impure leaf node); q, r and s walk: bob on q through both
    # walk leaves, one candidate; bob on r; bob and carol on s; x has no node
    assert got == (n_listed, 0, 2 + 1 + 1 + 2, n_listed), got
    snap.tune("lookup_formula", 0)
    lo.compare(e, oreq, oref)
    ls.compare(e, sreq, sref)
    snap.close()


# ---------------------------------------------------------------- 4. regrowth
def test_candidate_keys_regrow():
    it = Interner()
    namespaces, tuples = hand_namespaces(), hand_tuples(n_alice=3000)
    reg = Registry(tuples, namespaces, interner=it, max_read_depth=10)
    t6 = it.tuples_array(tuples)
    oracle = Oracle(t6, it.wildcard_rel, compile_program(namespaces, it))
    oreq = lo.requests_array(it, [T("d:any#share@alice"), T("d:any#share@(g:team#m)"), T("d:any#u@alice")], [5, 5, 5])
    oref = lo.reference(oracle, lo.domains(t6), oreq, 10)
    e = Engine(reg.snapshot, Config(10))
    reg.snapshot.tune("lookup_cap", 16)  # both key lists start at 16 entries
    lo.compare(e, oreq[:1], oref[:1])
    # alice reaches o0 .. o2999 through u and is blocked on six of them
    assert e.last_stats["candidates"] == 3000 and e.last_stats["n_objs"] == 3000 - 6, e.last_stats
    lo.compare(e, oreq, oref)
    assert e.last_stats["candidates"] == 3000 + 3, e.last_stats
    sreq = ls.requests_array(it, [("d", "o5", "share"), ("d", "o1", "share")], [5, 5])
    ls.compare(e, sreq, ls.reference(oracle, ls.subject_domain(t6), sreq, 10))
    reg.snapshot.tune("lookup_cap", 0)
    lo.compare(e, oreq, oref)


# ---------------------------------------------------------------- 5. refresh
def test_formula_lookups_after_refresh():
    it, namespaces = Interner(), hand_namespaces()
    prog = compile_program(namespaces, it)
    m = SnapshotPersister(namespaces=namespaces, interner=it, max_read_depth=10, seed=3)
    e = m.permission_engine()
    m.write_relation_tuples(*hand_tuples())
    subs = ["alice", "filler", "x3", "(g:team#m)"]
    oreq = lo.requests_array(it, [T(f"d:any#share@{s}") for s in subs for _ in range(3)], [1, 3, 5] * len(subs))
    roots = [("d", o, "share") for o in ("o0", "o1", "o2", "o5", "o6", "o8", "o100", "o210", "o999") for _ in range(3)]
    sreq = ls.requests_array(it, roots, [1, 3, 5] * (len(roots) // 3))

    def compare_all(step):
        rows = shard_rows(m)
        oracle = Oracle(rows, it.wildcard_rel, prog)
        full = Engine(Snapshot(rows, it, m.program, keys=_keys(m)), m.config)
        oref = lo.reference(oracle, lo.domains(rows), oreq, 10)
        sref = ls.reference(oracle, ls.subject_domain(rows), sreq, 10)
        counters = []
        for who, eng in (("refreshed", e), ("full build", full)):
            try:
                lo.compare(eng, oreq, oref)
                counters.append(tuple(int(eng.last_stats[k]) for k in KEYS))
                ls.compare(eng, sreq, sref)
                counters.append(tuple(int(eng.last_stats[k]) for k in KEYS))
            except AssertionError as x:
                raise AssertionError(f"step {step}, {who}: {x}") from x
        assert counters[:2] == counters[2:], (step, counters)  # dead nodes give no candidate
        full.snapshot.close()
        return oref

    compare_all(0)
    # new objects; o8 gets impure a and u nodes (a subject set of an undeclared relation) and alice through b
    m.write_relation_tuples(*[T(f"d:o{i}#a@alice") for i in range(205, 215)], T("d:o8#a@(g:zz#und)"), T("d:o8#b@alice"))
    oref = compare_all(1)
    assert it.obj_id("o210") in oref[2][0]
    for o in ("o2", "o6"):  # two listed objects lose every tuple
        m.delete_all_relation_tuples(RelationQuery(namespace="d", object=o))
    oref = compare_all(2)
    assert it.obj_id("o2") not in oref[2][0] and it.obj_id("o1") in oref[2][0]
    m.write_relation_tuples(T("d:o1#blocked@alice"))
    oref = compare_all(3)
    assert it.obj_id("o1") not in oref[2][0] and it.obj_id("o3") in oref[2][0]
    assert m.applies == 3


# ---------------------------------------------------------------- 6. concurrency
def test_formula_lookups_concurrent(hand):
    reg, it = hand
    reg.snapshot.tune("lookup_formula", 1)
    subs = ["alice", "filler", "x3", "(g:team#m)", "(g:core#m)"]
    oreq = lo.requests_array(it, [T(f"d:any#{r}@{s}") for r in ("share", "u") for s in subs], [5] * (2 * len(subs)))
    roots = [("d", o, r) for r in ("share", "u") for o in ("o0", "o1", "o5", "o100", "o999")]
    sreq = ls.requests_array(it, roots, [5] * len(roots))
    serial = Engine(reg.snapshot, Config(10))
    want_o = [a.tolist() for a in serial.lookup_objects_ids(oreq)]
    want_s = [a.tolist() for a in serial.lookup_subjects_ids(sreq)]
    errors = []

    def work(k):
        try:
            e = Engine(reg.snapshot, Config(10))
            for _ in range(5):
                if k % 2:
                    assert [a.tolist() for a in e.lookup_objects_ids(oreq)] == want_o
                    assert [a.tolist() for a in e.lookup_subjects_ids(sreq)] == want_s
                else:
                    assert [a.tolist() for a in e.lookup_subjects_ids(sreq)] == want_s
                    assert [a.tolist() for a in e.lookup_objects_ids(oreq)] == want_o
        except Exception as x:  # noqa: BLE001
            errors.append(x)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
