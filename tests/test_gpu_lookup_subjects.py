"""GPU tests of the subject lookup (kg_lookup_subjects): for every request the list must equal what the
CPU oracle's canonical check says over EVERY subject id of the domain (the ids that occur as the
SubjectID of a tuple), with the same error count and the code of the lowest erring id."""
import threading

import numpy as np
import pytest

from golden_cases import Case, load
from keto_amd.engine import CheckError, Config, Engine, Registry
from keto_amd.handlers import ListSubjectsHandler
from keto_amd.ketoapi import RelationTuple
from keto_amd.mapper import Interner, SUBJECT_ID
from oracle.oracle import POLICY_CANONICAL, Oracle
from test_gpu_check import random_graph, random_program, random_queries

pytestmark = pytest.mark.gpu

T = RelationTuple.from_string


def subject_domain(t6):
    """The ascending subject ids that occur as the SubjectID of a tuple."""
    t6 = np.asarray(t6, np.uint32).reshape(-1, 6)
    return np.unique(t6[t6[:, 3] == SUBJECT_ID, 4])


def reference(oracle, dom, reqs, gmax):
    """Per request: (ascending member subject ids, n_errors, err_code of the lowest erring id)."""
    n, m = len(reqs), len(dom)
    q = np.zeros((n, m, 6), np.uint32)
    for k in range(3):
        q[:, :, k] = reqs[:, k, None]
    q[:, :, 3], q[:, :, 4] = SUBJECT_ID, dom[None, :]
    depths = np.repeat(reqs[:, 3].copy().view(np.int32), m)
    res, err, _ = oracle.check_batch(q.reshape(-1, 6), depths, gmax, POLICY_CANONICAL, nthreads=8)
    res, err = res.reshape(n, m), np.asarray(err).reshape(n, m)
    out = []
    for i in range(n):
        bad = np.nonzero(res[i] == 2)[0]
        out.append((dom[res[i] == 1].tolist(), len(bad), int(err[i, bad[0]]) if len(bad) else 0))
    return out


def requests_array(it, roots, depths):
    """(namespace, object, relation) names -> (n,4) kg_lookup_subj rows."""
    r = np.zeros((len(roots), 4), np.uint32)
    for i, (ns, obj, rel) in enumerate(roots):
        r[i] = (it.ns_id(ns), it.obj_id(obj), it.rel_id(rel), np.int32(depths[i]).view(np.uint32))
    return r


def roots_of(qs):
    """Check-shaped query tuples with their subject dropped."""
    return [(t.namespace, t.object, t.relation) for t in qs]


def compare(e, reqs, ref, with_stats=True):
    off, ids, err, nerr = e.lookup_subjects_ids(reqs, with_stats=with_stats)
    assert off[0] == 0 and off[-1] == len(ids)
    for i, (want, n_bad, code) in enumerate(ref):
        got = ids[int(off[i]):int(off[i + 1])].tolist()
        assert got == want, (i, reqs[i].tolist(), got[:10], want[:10])
        assert (int(nerr[i]), int(err[i])) == (n_bad, code), (i, reqs[i].tolist())
    return off, ids


def _case1(seed):
    rng = np.random.default_rng(9000 + seed)
    n_obj = 40 + 15 * (seed % 4)
    it, tuples, nss, rels = random_graph(rng, n_obj=n_obj, n_rows=250 + 120 * (seed % 4))
    qs = random_queries(rng, nss, rels + ["..."], 150, n_obj=n_obj)  # n_obj + 3: some roots have no node
    reqs = requests_array(it, roots_of(qs), rng.integers(-1, 9, len(qs)))
    return it, tuples, reqs


@pytest.mark.parametrize("seed", range(8))
def test_random_graphs(seed):
    it, tuples, reqs = _case1(seed)
    reg = Registry(tuples, [], interner=it)
    t6 = it.tuples_array(tuples)
    oracle, dom = Oracle(t6, it.wildcard_rel), subject_domain(t6)
    for gmax in (1, 3, 5, 8):
        e = Engine(reg.snapshot, Config(gmax))
        _, ids = compare(e, reqs, reference(oracle, dom, reqs, gmax))
        st = e.last_stats
        assert st["candidates"] == 0 and st["exact"] >= st["n_objs"] == len(ids), st  # the walk alone answered
        assert gmax < 3 or (len(ids) > 0 and st["levels"] > 0)  # the requests reach something


def test_depth_boundary():
    it = Interner()
    tuples = [T(f"g:c{i}#m@(g:c{i - 1}#m)") for i in range(1, 7)] + [T(f"g:c{i}#m@u{i}") for i in range(7)]
    reg = Registry(tuples, [], interner=it, max_read_depth=10)
    e = reg.permission_engine()
    for d in range(1, 10):  # u{i} sits 6 - i levels below c6 and is probed at rest depth d - 1 - (6 - i) >= 0
        want = sorted(f"u{i}" for i in range(7) if 6 - i <= d - 1)
        assert e.lookup_subjects("g", "c6", "m", d) == want, d
        assert Engine(reg.snapshot, Config(d)).lookup_subjects("g", "c6", "m", 0) == want, d  # the global depth


def _hub_case():
    it = Interner()
    tuples = [T(f"g:big#m@ku{i}") for i in range(5000)]                 # 5,000 direct ids: two 4,096-entry passes
    tuples += [T(f"g:fan#m@(g:k{i}#m)") for i in range(5000)]           # 5,000 set children ...
    tuples += [T(f"g:k{i}#m@ku{i}") for i in range(5000)]               # ... one user each
    tuples += [T(f"g:k{i}#m@shared") for i in range(5000)]              # ... and one they all share
    tuples += [T(f"d:c{i}#v@(d:c{(i + 1) % 40}#v)") for i in range(40)]  # a 40-cycle
    tuples += [T("d:c0#v@cyc"), T("d:c20#w@cyc"), T("g:y#m@(g:big#...)"), T("g:y#m@yuser"), T("g:y#w@(d:c5#v)"),
               T("g:top#m@(g:k0#m)"), T("g:top#m@(g:big#m)"), T("g:top#m@(d:c7#v)"), T("g:top#w@deep"),
               T("g:top#m@shared"), T("d:c5#w@(g:top#m)")]
    tuples += [T("d:c0#v@cyc"), T("g:big#m@ku7"), T("d:c3#v@(d:c4#v)"), T("g:top#m@(g:big#m)")]  # duplicates
    named = ["g:big#m", "d:c5#v", "g:k0#m", "g:top#w", "d:c0#v", "g:y#m", "d:c20#w", "g:k4999#m", "d:c39#v", "g:missing#m",
             "g:fan#m", "d:c5#w", "g:y#w", "d:c7#v", "g:k2500#m", "d:c20#v", "g:big#...", "d:c1#v", "g:top#m", "d:c30#v",
             "g:k1#m", "d:c3#v", "d:c10#v", "d:c2#v"]
    roots = [(x.split(":")[0], x.split(":")[1].split("#")[0], x.split("#")[1]) for x in named for _ in range(3)]
    depths = [0, 2, 41] * len(named)
    return it, tuples, requests_array(it, roots, depths)  # 72 requests, 66 with a root node: two walk groups


def test_hub_cycle_duplicates():
    it, tuples, reqs = _hub_case()
    reg = Registry(tuples, [], interner=it)
    t6 = it.tuples_array(tuples)
    oracle, dom = Oracle(t6, it.wildcard_rel), subject_domain(t6)
    for gmax in (2, 3, 6, 12):
        e = Engine(reg.snapshot, Config(gmax))
        _, ids = compare(e, reqs, reference(oracle, dom, reqs, gmax))
        st = e.last_stats
        assert st["candidates"] == 0 and st["exact"] >= len(ids) > 10000, st


def test_output_regrowth():
    it = Interner()
    tuples = [T(f"n:big#r@s{i}") for i in range(20000)] + [T(f"n:o{i}#r@s{i}") for i in range(63)]
    reg = Registry(tuples, [], interner=it)
    t6 = it.tuples_array(tuples)
    oracle, dom = Oracle(t6, it.wildcard_rel), subject_domain(t6)
    roots = [("n", f"o{i}", "r") for i in range(63)]
    roots = roots[:30] + [("n", "big", "r")] + roots[30:]  # the big one in the middle of the group
    reqs = requests_array(it, roots, [0] * len(roots))
    ref = reference(oracle, dom, reqs, 5)
    assert sum(len(r[0]) for r in ref) == 20063
    e = Engine(reg.snapshot, Config(5))
    compare(e, reqs, ref)
    reg.snapshot.tune("lookup_cap", 16)  # the output list starts at 16 entries: the group is rerun with a larger one
    compare(e, reqs, ref)
    reg.snapshot.tune("lookup_cap", 0)
    compare(e, reqs, ref)
    compare(e, reqs[:40], ref[:40])


def test_golden_rewrites_programs():
    for case in load("rewrites_test.json"):
        c = Case(case)
        reg = Registry(c.tuples, c.namespaces, interner=c.it)
        oracle, dom = Oracle(c.arr, c.it.wildcard_rel, c.prog), subject_domain(c.arr)
        rels = sorted({r.name for n in c.namespaces for r in n.relations} | {"undeclared"})
        objects = sorted({t.object for t in c.tuples} | {t.subject_set.object for t in c.tuples if t.subject_set})
        roots = [(n.name, o, r) for n in c.namespaces for o in objects for r in rels]
        rng = np.random.default_rng(1)
        reqs = requests_array(c.it, roots, rng.integers(-1, 7, len(roots)))
        for gmax in (1, 3, 6):
            compare(Engine(reg.snapshot, Config(gmax)), reqs, reference(oracle, dom, reqs, gmax))
        reg.snapshot.tune("lookup_domain_rows", 1)  # the domain from the check rows, as without a holder bitmap
        compare(Engine(reg.snapshot, Config(6)), reqs, reference(oracle, dom, reqs, 6))


@pytest.mark.parametrize("mat", [1, 0])
@pytest.mark.parametrize("unions", [False, True])
def test_random_programs(unions, mat, monkeypatch):
    """The graph shape of test_gpu_lookup.test_random_programs, 4 seeds: every rewrite kind or unions only,
    undeclared relations in tuples and requests, materialisation on and off."""
    from keto_amd.namespace import compile_program
    monkeypatch.setenv("KG_MATERIALIZE", str(mat))
    exact = 0
    for seed in range(4):
        rng = np.random.default_rng(300 + seed + (1000 if unions else 0))
        nss, rels = ["a", "b", "c"], ["r0", "r1", "r2", "r3"]
        it = Interner()
        namespaces = random_program(rng, nss, rels, unions_only=unions)
        prog = compile_program(namespaces, it, lower_ttu=False)  # the oracle: TTU leaves as written
        n_obj, n_users = 30 + 10 * seed, 25
        tuples = []
        for _ in range(150 + 60 * seed):
            ns, obj = rng.choice(nss), f"o{rng.integers(n_obj)}"
            rel = rng.choice(rels) if rng.random() < 0.97 else "undeclared"
            if rng.random() < 0.5:
                srel = rng.choice(rels + ["..."]) if rng.random() < 0.98 else "undeclared"
                s = f"({rng.choice(nss)}:o{rng.integers(n_obj)}#{srel})"
            else:
                s = f"u{rng.integers(n_users)}"
            tuples.append(T(f"{ns}:{obj}#{rel}@{s}"))
        reg = Registry(tuples, namespaces, interner=it)
        qs = random_queries(rng, nss, rels + ["undeclared"], 100, n_obj=n_obj, n_users=n_users)
        reqs = requests_array(it, roots_of(qs), rng.integers(-1, 7, len(qs)))
        t6 = it.tuples_array(tuples)
        oracle, dom = Oracle(t6, it.wildcard_rel, prog), subject_domain(t6)
        for gmax in (1, 2, 4, 6):
            e = Engine(reg.snapshot, Config(gmax))
            compare(e, reqs, reference(oracle, dom, reqs, gmax))
            exact += e.last_stats["exact"]
    if unions and mat:  # the walk runs on materialised relations
        assert exact > 0


def test_undeclared_relation_reports_every_subject():
    from keto_amd.namespace import Namespace, Relation
    it = Interner()
    tuples = [T(f"a:o{i}#r@u{i % 3}") for i in range(5)] + [T("a:o0#r@(a:o1#r)")]
    reg = Registry(tuples, [Namespace("a", [Relation("r")])], interner=it)
    e = reg.permission_engine()
    reqs = requests_array(it, [("a", "o0", "nope")], [0])
    off, ids, err, nerr = e.lookup_subjects_ids(reqs, with_stats=True)
    assert len(ids) == 0 and int(nerr[0]) == 3 and int(err[0]) == 1  # KG_ERR_RELATION_NOT_FOUND
    assert e.last_stats["candidates"] == 3 and e.last_stats["confirmed"] == 0
    off, ids, err, nerr = e.lookup_subjects_ids(np.zeros((0, 4), np.uint32))
    assert off.tolist() == [0] and len(ids) == 0 and len(err) == 0 and len(nerr) == 0


def test_candidate_lists_regrow():
    """70,000 subject ids on one object: under an undeclared relation the domain outgrows its first 64 Ki
    entries and every id is reported with the relation-not-found code; the plain relation lists all of
    them by the walk."""
    from keto_amd.namespace import Namespace, Relation, compile_program
    it = Interner()
    namespaces = [Namespace("n", [Relation("r")])]
    prog = compile_program(namespaces, it, lower_ttu=False)
    tuples = [RelationTuple("n", "o", "r", subject_id=f"u{i}") for i in range(70000)]
    reg = Registry(tuples, namespaces, interner=it)
    t6 = it.tuples_array(tuples)
    oracle, dom = Oracle(t6, it.wildcard_rel, prog), subject_domain(t6)
    reqs = requests_array(it, [("n", "o", "nope"), ("n", "o", "r")], [0, 0])
    ref = reference(oracle, dom, reqs, 5)
    assert ref[0] == ([], 70000, 1) and len(ref[1][0]) == 70000
    e = Engine(reg.snapshot, Config(5))
    for _ in range(2):  # the second run reuses the grown lists
        compare(e, reqs, ref)
        assert e.last_stats["candidates"] == 70000 and e.last_stats["exact"] == 70000
    reg.snapshot.tune("lookup_domain_rows", 1)
    compare(e, reqs, ref)
    assert e.last_stats["candidates"] == 70000


def test_confirmation_in_chunks():
    """64 confirm-mode requests over 70,000 subject ids are 4,480,000 candidate checks: more than one 4 Mi
    chunk of them, with members (an `and` rewrite) and errors (an undeclared relation) in every chunk."""
    from keto_amd.namespace import ComputedSubjectSet, Namespace, Relation, SubjectSetRewrite, compile_program
    it = Interner()
    both = SubjectSetRewrite([ComputedSubjectSet("r"), ComputedSubjectSet("r")], "and")
    namespaces = [Namespace("n", [Relation("r"), Relation("both", rewrite=both)])]
    prog = compile_program(namespaces, it, lower_ttu=False)
    tuples = [RelationTuple("n", "o", "r", subject_id=f"u{i}") for i in range(70000)]
    reg = Registry(tuples, namespaces, interner=it)
    t6 = it.tuples_array(tuples)
    oracle, dom = Oracle(t6, it.wildcard_rel, prog), subject_domain(t6)
    two = requests_array(it, [("n", "o", "both"), ("n", "o", "nope")], [0, 0])
    ref = reference(oracle, dom, two, 5)
    assert len(ref[0][0]) == 70000 and ref[1] == ([], 70000, 1)
    e = Engine(reg.snapshot, Config(5))
    compare(e, np.tile(two, (32, 1)), ref * 32)  # identical requests have identical answers
    st = e.last_stats
    assert st["candidates"] == 64 * 70000 and st["confirmed"] == 32 * 70000 and st["exact"] == 0, st


def test_symmetry_with_reverse_lookup():
    """s in lookup_subjects(ns, o, rel)  <=>  o in lookup_objects(ns, rel, s), over a whole random graph."""
    rng = np.random.default_rng(77)
    n_obj = 50
    it, tuples, nss, rels = random_graph(rng, n_obj=n_obj, n_rows=350)
    reg = Registry(tuples, [], interner=it)
    e = Engine(reg.snapshot, Config(5))
    dom = subject_domain(it.tuples_array(tuples))
    roots = [(ns, f"o{o}", rel) for ns in nss for rel in rels for o in range(n_obj)]
    sreq = requests_array(it, roots, [0] * len(roots))
    off, ids, _, nerr = e.lookup_subjects_ids(sreq)
    assert not nerr.any()
    forward = {(int(sreq[i, 0]), int(sreq[i, 2]), int(sreq[i, 1]), int(s))
               for i in range(len(sreq)) for s in ids[int(off[i]):int(off[i + 1])]}
    oreq = np.asarray([(it.ns_id(ns), it.rel_id(rel), SUBJECT_ID, int(s), 0, 0) for ns in nss for rel in rels for s in dom],
                      np.uint32)
    off, objs, _, nerr = e.lookup_objects_ids(oreq)
    assert not nerr.any()
    backward = {(int(oreq[i, 0]), int(oreq[i, 1]), int(o), int(oreq[i, 3]))
                for i in range(len(oreq)) for o in objs[int(off[i]):int(off[i + 1])]}
    assert forward == backward and len(forward) > 100


def test_alternation_on_one_lane():
    """Both lookups share a lane's masks and lists: interleaved calls must each repeat their first answer."""
    it, tuples, sreq = _case1(3)
    rng = np.random.default_rng(5)
    reg = Registry(tuples, [], interner=it)
    e = Engine(reg.snapshot, Config(6))
    oreq = np.asarray([(it.ns_id(f"n{rng.integers(3)}"), it.rel_id(f"r{rng.integers(3)}"), SUBJECT_ID,
                        it.obj_id(f"u{rng.integers(40)}"), 0, 0) for _ in range(100)], np.uint32)
    first = {}
    for step in range(8):
        kind = ("subjects", "objects", "objects", "subjects")[step % 4]
        part = slice(0, None) if step < 4 else slice(step, 70 + step)  # other group boundaries later on
        got = e.lookup_subjects_ids(sreq[part]) if kind == "subjects" else e.lookup_objects_ids(oreq[part])
        key = (kind, part.start, part.stop)
        want = first.setdefault(key, got)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), step
        whole = first[(kind, 0, None)]  # a slice of the requests answers like the same requests in the whole
        lo = part.start
        for i in range(len(sreq[part]) if kind == "subjects" else len(oreq[part])):
            assert np.array_equal(got[1][int(got[0][i]):int(got[0][i + 1])],
                                  whole[1][int(whole[0][lo + i]):int(whole[0][lo + i + 1])]), (step, i)
    assert len(first[("subjects", 0, None)][1]) > 0 and len(first[("objects", 0, None)][1]) > 0


def test_replicas_rotate():
    it, tuples, reqs = _case1(1)
    reg = Registry(tuples, [], interner=it, devices=[0, 0])
    t6 = it.tuples_array(tuples)
    ref = reference(Oracle(t6, it.wildcard_rel), subject_domain(t6), reqs, 5)
    e = Engine(reg.snapshot, Config(5))
    for _ in range(3):  # successive calls land on different replicas
        compare(e, reqs, ref)


def test_sharded_snapshot_is_refused():
    from keto_amd import _lib
    from keto_amd.engine import Snapshot
    it, tuples, reqs = _case1(2)
    snap = Snapshot(it.tuples_array(tuples), it, shard=(0, 2))
    with pytest.raises(_lib.KetoGPUError, match="not supported on hash-sharded snapshots") as ex:
        Engine(snap, Config(5)).lookup_subjects_ids(reqs)
    assert "(-3)" in str(ex.value)


def test_concurrent_calls_match_serial():
    it, tuples, reqs = _case1(0)
    reg = Registry(tuples, [], interner=it)
    e = Engine(reg.snapshot, Config(5))
    off0, ids0, _, _ = e.lookup_subjects_ids(reqs)
    bad = []

    def work():
        for _ in range(4):
            off, ids, err, nerr = Engine(reg.snapshot, Config(5)).lookup_subjects_ids(reqs)
            if not (np.array_equal(off, off0) and np.array_equal(ids, ids0) and not nerr.any()):
                bad.append(1)

    th = [threading.Thread(target=work) for _ in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad


def test_engine_and_handler():
    from keto_amd.namespace import Namespace, Relation
    case = load("cat_videos.json")[0]
    c = Case(case)
    reg = Registry(c.tuples, c.namespaces, interner=c.it)
    e = reg.permission_engine()
    objects = sorted({t.object for t in c.tuples})
    subjects = sorted({t.subject_id for t in c.tuples if t.subject_id is not None})
    listed = 0
    for o in objects:
        for d in (1, 2, 3, 5):
            want = [s for s in subjects if e.check_is_member(RelationTuple("videos", o, "view", subject_id=s), d)]
            assert e.lookup_subjects("videos", o, "view", d) == want, (o, d)
            listed += len(want)
    assert listed > 0
    o = max(objects, key=lambda x: len(e.lookup_subjects("videos", x, "view", 5)))
    full = e.lookup_subjects("videos", o, "view", 5)
    assert len(full) >= 2
    h = ListSubjectsHandler(e, reg.mapper)
    got, token = [], ""
    for _ in range(len(full) + 1):
        status, body = h.get_list_subjects({"namespace": "videos", "object": o, "relation": "view", "max-depth": "5",
                                            "page_size": "1", "page_token": token})
        assert status == 200 and len(body["subject_ids"]) == 1
        got += body["subject_ids"]
        token = body["next_page_token"]
        if not token:
            break
    assert got == full
    assert h.get_list_subjects({"namespace": "videos", "object": o, "relation": "view"})[1]["subject_ids"] == \
        e.lookup_subjects("videos", o, "view", 0)
    assert h.grpc_list_subjects({"namespace": "videos", "object": o, "relation": "view", "max_depth": 5}) == \
        {"subject_ids": full, "next_page_token": ""}
    assert h.get_list_subjects("namespace=nope&object=o&relation=view")[0] == 404
    # an undeclared relation of a configured namespace: the checks end in errors
    it = Interner()
    reg2 = Registry([T("a:o#r@u")], [Namespace("a", [Relation("r")])], interner=it)
    e2 = reg2.permission_engine()
    with pytest.raises(CheckError) as ex:
        e2.lookup_subjects("a", "o", "nope", 0)
    assert ex.value.code == 1
    assert ListSubjectsHandler(e2, reg2.mapper).get_list_subjects("namespace=a&object=o&relation=nope")[0] == 500
