"""GPU tests of the reverse lookup (kg_lookup_objects): for every request the list must equal what the
CPU oracle's canonical check says over EVERY object of the request's namespace (the objects that occur
in a tuple of the namespace, as an object or in a subject set), with the same error count and code."""
import threading

import numpy as np
import pytest

from golden_cases import Case, load
from keto_amd.engine import CheckError, Config, Engine, Registry
from keto_amd.handlers import ListObjectsHandler
from keto_amd.ketoapi import RelationTuple, SubjectSet
from keto_amd.mapper import Interner, SUBJECT_ID
from oracle.oracle import POLICY_CANONICAL, Oracle
from test_gpu_check import random_graph, random_program, random_queries

pytestmark = pytest.mark.gpu


def domains(t6):
    """namespace id -> ascending object ids that occur in a tuple of the namespace."""
    t6 = np.asarray(t6, np.uint32).reshape(-1, 6)
    out = {}
    for ns in set(t6[:, 0].tolist()) | set(t6[t6[:, 3] != SUBJECT_ID, 3].tolist()):
        a = t6[t6[:, 0] == ns, 1]
        b = t6[(t6[:, 3] == ns) & (t6[:, 3] != SUBJECT_ID), 4]
        out[int(ns)] = np.unique(np.concatenate([a, b]))
    return out


def reference(oracle, dom, reqs, gmax):
    """Per request: (ascending member object ids, n_errors, err_code of the lowest erring object)."""
    rows, depths, owner = [], [], []
    for i, (ns, rel, sns, sobj, srel, d) in enumerate(reqs.tolist()):
        objs = dom.get(ns, np.zeros(0, np.uint32))
        q = np.zeros((len(objs), 6), np.uint32)
        q[:, 0], q[:, 1], q[:, 2], q[:, 3], q[:, 4], q[:, 5] = ns, objs, rel, sns, sobj, srel
        rows.append(q)
        depths.append(np.full(len(objs), np.uint32(d).view(np.int32), np.int64))
        owner.append(np.full(len(objs), i, np.int64))
    q6, dd, ow = np.concatenate(rows), np.concatenate(depths), np.concatenate(owner)
    res, err, _ = oracle.check_batch(q6, dd, gmax, POLICY_CANONICAL)
    out = []
    for i in range(len(reqs)):
        m = ow == i
        o, r, e = q6[m, 1], res[m], np.asarray(err)[m]
        bad = np.nonzero(r == 2)[0]
        out.append((o[r == 1].tolist(), len(bad), int(e[bad[0]]) if len(bad) else 0))
    return out


def requests_array(it, qs, depths):
    """Check-shaped query tuples -> (n,6) kg_lookup rows (the object is dropped)."""
    r = np.zeros((len(qs), 6), np.uint32)
    for i, t in enumerate(qs):
        ns, _, rel, sns, sobj, srel = it.tuple_ids(t)
        r[i] = (ns, rel, sns, sobj, srel, np.int32(depths[i]).view(np.uint32))
    return r


def compare(e, reqs, ref, with_stats=True):
    off, objs, err, nerr = e.lookup_objects_ids(reqs, with_stats=with_stats)
    assert off[0] == 0 and off[-1] == len(objs)
    for i, (want, n_bad, code) in enumerate(ref):
        got = objs[int(off[i]):int(off[i + 1])].tolist()
        assert got == want, (i, reqs[i].tolist(), got[:10], want[:10])
        assert (int(nerr[i]), int(err[i])) == (n_bad, code), (i, reqs[i].tolist())
    return off, objs


def _case1(seed):
    rng = np.random.default_rng(7000 + seed)
    n_obj = 40 + 15 * (seed % 4)
    it, tuples, nss, rels = random_graph(rng, n_obj=n_obj, n_rows=250 + 120 * (seed % 4))
    qs = random_queries(rng, nss, rels + ["..."], 150, n_obj=n_obj, p_setq=0.3)
    reqs = requests_array(it, qs, rng.integers(-1, 9, len(qs)))
    return it, tuples, reqs


@pytest.mark.parametrize("seed", range(8))
def test_random_graphs(seed):
    it, tuples, reqs = _case1(seed)
    reg = Registry(tuples, [], interner=it)
    t6 = it.tuples_array(tuples)
    oracle, dom = Oracle(t6, it.wildcard_rel), domains(t6)
    for gmax in (1, 3, 5, 8):
        e = Engine(reg.snapshot, Config(gmax))
        _, objs = compare(e, reqs, reference(oracle, dom, reqs, gmax))
        st = e.last_stats
        assert st["candidates"] == 0 and st["exact"] == st["n_objs"] == len(objs), st  # the walk alone answered
        assert gmax < 3 or (len(objs) > 0 and st["levels"] > 0)  # the requests reach something


def test_depth_boundary():
    it = Interner()
    tuples = [RelationTuple.from_string("g:c0#m@user")]
    tuples += [RelationTuple.from_string(f"g:c{i}#m@(g:c{i - 1}#m)") for i in range(1, 7)]
    reg = Registry(tuples, [], interner=it, max_read_depth=10)
    e = reg.permission_engine()
    for d in range(1, 9):
        assert e.lookup_objects("g", "m", "user", d) == [f"c{i}" for i in range(min(d, 7))]
    for g in range(1, 9):  # the same through the global depth
        assert Engine(reg.snapshot, Config(g)).lookup_objects("g", "m", "user", 0) == [f"c{i}" for i in range(min(g, 7))]


def test_hub_cycle_duplicates():
    it = Interner()
    T = RelationTuple.from_string
    tuples = [T(f"g:h{i}#m@hubuser") for i in range(5000)]            # a subject 5,000 nodes hold
    tuples += [T(f"g:top{i}#m@(g:hub#m)") for i in range(5000)]       # a node with 5,000 parents
    tuples += [T("g:hub#m@deep"), T("g:hub#m@(d:c7#v)"), T("g:hub#w@deep")]
    tuples += [T(f"d:c{i}#v@(d:c{(i + 1) % 40}#v)") for i in range(40)]  # a 40-cycle
    tuples += [T("d:c0#v@cyc"), T("d:c20#w@cyc"), T("d:x#v@(g:hub#m)"), T("g:y#m@(d:c5#v)"), T("g:y#w@(d:c5#v)"),
               T("d:z#w@(g:top17#m)"), T("g:top3#m@(g:h9#m)")]
    tuples += [T("d:c0#v@cyc"), T("g:hub#m@deep"), T("d:c3#v@(d:c4#v)"), T("g:h1#m@hubuser")]  # duplicates
    reg = Registry(tuples, [], interner=it)
    t6 = it.tuples_array(tuples)
    oracle, dom = Oracle(t6, it.wildcard_rel), domains(t6)
    subjects = ["hubuser", "deep", "cyc", "nobody", "(g:hub#m)", "(d:c3#v)"]
    qs, depths = [], []
    for s in subjects:
        for ns, rel in (("g", "m"), ("d", "v"), ("g", "w"), ("d", "w")):
            for d in (0, 2, 41):
                qs.append(T(f"{ns}:any#{rel}@{s}"))
                depths.append(d)
    reqs = requests_array(it, qs, depths)  # 72 requests: two walk groups, (ns, rel) mixed inside each
    for gmax in (2, 3, 6, 12):
        e = Engine(reg.snapshot, Config(gmax))
        compare(e, reqs, reference(oracle, dom, reqs, gmax))
        assert e.last_stats["candidates"] == 0


def test_output_regrowth():
    it = Interner()
    tuples = [RelationTuple.from_string(f"n:o{i}#r@big") for i in range(20000)]
    reg = Registry(tuples, [], interner=it)
    t6 = it.tuples_array(tuples)
    oracle, dom = Oracle(t6, it.wildcard_rel), domains(t6)
    qs = [RelationTuple.from_string("n:any#r@big")] + [RelationTuple.from_string(f"n:any#r@nobody{i}") for i in range(63)]
    qs = qs[20:] + qs[:20]  # the big one in the middle of the group
    reqs = requests_array(it, qs, [0] * len(qs))
    ref = reference(oracle, dom, reqs, 5)
    assert sum(len(r[0]) for r in ref) == 20000
    e = Engine(reg.snapshot, Config(5))
    compare(e, reqs, ref)
    reg.snapshot.tune("lookup_cap", 16)  # the output list starts at 16 entries: the group is rerun with a larger one
    compare(e, reqs, ref)
    compare(e, reqs[:30], ref[:30])
    reg.snapshot.tune("lookup_cap", 0)
    compare(e, reqs, ref)


def test_golden_rewrites_programs():
    for case in load("rewrites_test.json"):
        c = Case(case)
        reg = Registry(c.tuples, c.namespaces, interner=c.it)
        oracle, dom = Oracle(c.arr, c.it.wildcard_rel, c.prog), domains(c.arr)
        rels = sorted({r.name for n in c.namespaces for r in n.relations} | {"undeclared"})
        subs = sorted({t.subject_id for t in c.tuples if t.subject_id is not None}) + ["nobody"]
        sets = sorted({str(t.subject_set) for t in c.tuples if t.subject_set is not None})
        qs = [RelationTuple.from_string(f"{n.name}:any#{r}@{s}") for n in c.namespaces for r in rels for s in subs]
        qs += [RelationTuple.from_string(f"{n.name}:any#{r}@({s})") for n in c.namespaces for r in rels for s in sets[:6]]
        rng = np.random.default_rng(1)
        reqs = requests_array(c.it, qs, rng.integers(-1, 7, len(qs)))
        for gmax in (1, 3, 6):
            compare(Engine(reg.snapshot, Config(gmax)), reqs, reference(oracle, dom, reqs, gmax))


@pytest.mark.parametrize("mat", [1, 0])
@pytest.mark.parametrize("unions", [False, True])
def test_random_programs(unions, mat, monkeypatch):
    """The graph shape of test_gpu_check.test_random_rewrites_vs_oracle, 4 seeds: every rewrite kind or
    unions only, undeclared relations in tuples and requests, materialisation on and off."""
    from keto_amd.namespace import compile_program
    monkeypatch.setenv("KG_MATERIALIZE", str(mat))
    exact = 0
    for seed in range(4):
        rng = np.random.default_rng(100 + seed + (1000 if unions else 0))
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
            tuples.append(RelationTuple.from_string(f"{ns}:{obj}#{rel}@{s}"))
        reg = Registry(tuples, namespaces, interner=it)
        qs = random_queries(rng, nss, rels + ["undeclared"], 100, n_obj=n_obj, n_users=n_users, p_setq=0.3)
        reqs = requests_array(it, qs, rng.integers(-1, 7, len(qs)))
        t6 = it.tuples_array(tuples)
        oracle, dom = Oracle(t6, it.wildcard_rel, prog), domains(t6)
        for gmax in (1, 2, 4, 6):
            e = Engine(reg.snapshot, Config(gmax))
            compare(e, reqs, reference(oracle, dom, reqs, gmax))
            exact += e.last_stats["exact"]
    if unions and mat:  # the reverse path runs on materialised relations
        assert exact > 0


def test_undeclared_relation_reports_every_object():
    from keto_amd.namespace import Namespace, Relation
    it = Interner()
    tuples = [RelationTuple.from_string(f"a:o{i}#r@u") for i in range(5)]
    reg = Registry(tuples, [Namespace("a", [Relation("r")])], interner=it)
    e = reg.permission_engine()
    reqs = requests_array(it, [RelationTuple.from_string("a:any#nope@u")], [0])
    off, objs, err, nerr = e.lookup_objects_ids(reqs)
    assert len(objs) == 0 and int(nerr[0]) == 5 and int(err[0]) == 1  # KG_ERR_RELATION_NOT_FOUND
    off, objs, err, nerr = e.lookup_objects_ids(np.zeros((0, 6), np.uint32))
    assert off.tolist() == [0] and len(objs) == 0


def test_candidate_lists_regrow():
    """70,000 objects under an undeclared relation: the domain keys and the candidate checks both outgrow
    their first 64 Ki entries, and every object is reported with the relation-not-found code."""
    from keto_amd.namespace import Namespace, Relation, compile_program
    it = Interner()
    namespaces = [Namespace("n", [Relation("r")])]
    prog = compile_program(namespaces, it, lower_ttu=False)
    tuples = [RelationTuple("n", f"o{i}", "r", subject_id="u") for i in range(70000)]
    reg = Registry(tuples, namespaces, interner=it)
    t6 = it.tuples_array(tuples)
    oracle, dom = Oracle(t6, it.wildcard_rel, prog), domains(t6)
    reqs = requests_array(it, [RelationTuple.from_string("n:any#nope@u"), RelationTuple.from_string("n:any#r@u")], [0, 0])
    ref = reference(oracle, dom, reqs, 5)
    assert ref[0] == ([], 70000, 1) and len(ref[1][0]) == 70000
    e = Engine(reg.snapshot, Config(5))
    compare(e, reqs, ref)
    assert e.last_stats["candidates"] == 70000 and e.last_stats["exact"] == 70000
    compare(e, reqs, ref)  # the grown lists, reused


def test_replicas_rotate():
    it, tuples, reqs = _case1(1)
    reg = Registry(tuples, [], interner=it, devices=[0, 0])
    t6 = it.tuples_array(tuples)
    ref = reference(Oracle(t6, it.wildcard_rel), domains(t6), reqs, 5)
    e = Engine(reg.snapshot, Config(5))
    for _ in range(3):  # successive calls land on different replicas
        compare(e, reqs, ref)


def test_sharded_snapshot_is_refused():
    from keto_amd import _lib
    from keto_amd.engine import Snapshot
    it, tuples, reqs = _case1(2)
    snap = Snapshot(it.tuples_array(tuples), it, shard=(0, 2))
    with pytest.raises(_lib.KetoGPUError, match="not supported on hash-sharded snapshots") as ex:
        Engine(snap, Config(5)).lookup_objects_ids(reqs)
    assert "(-3)" in str(ex.value)


def test_concurrent_calls_match_serial():
    it, tuples, reqs = _case1(0)
    reg = Registry(tuples, [], interner=it)
    e = Engine(reg.snapshot, Config(5))
    off0, objs0, _, _ = e.lookup_objects_ids(reqs)
    bad = []

    def work():
        for _ in range(4):
            off, objs, err, nerr = Engine(reg.snapshot, Config(5)).lookup_objects_ids(reqs)
            if not (np.array_equal(off, off0) and np.array_equal(objs, objs0) and not nerr.any()):
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
    for subject in ("cat lady", "*", SubjectSet("videos", "/cats", "owner")):
        for d in (1, 2, 3, 5):
            want = []
            for o in objects:
                t = RelationTuple("videos", o, "view", subject_set=subject) if isinstance(subject, SubjectSet) \
                    else RelationTuple("videos", o, "view", subject_id=subject)
                if e.check_is_member(t, d):
                    want.append(o)
            assert e.lookup_objects("videos", "view", subject, d) == want, (subject, d)
    full = e.lookup_objects("videos", "view", "cat lady", 5)
    assert len(full) >= 2
    h = ListObjectsHandler(e, reg.mapper)
    got, token = [], ""
    for _ in range(len(full) + 1):
        status, body = h.get_list_objects({"namespace": "videos", "relation": "view", "subject_id": "cat lady",
                                           "max-depth": "5", "page_size": "1", "page_token": token})
        assert status == 200 and len(body["objects"]) == 1
        got += body["objects"]
        token = body["next_page_token"]
        if not token:
            break
    assert got == full
    assert h.get_list_objects("namespace=videos&relation=view&subject_id=cat%20lady")[1]["objects"] == \
        e.lookup_objects("videos", "view", "cat lady", 0)
    assert h.grpc_list_objects({"namespace": "videos", "relation": "view", "subject": {"id": "cat lady"},
                                "max_depth": 5})["objects"] == full
    assert h.get_list_objects("namespace=nope&relation=view&subject_id=x")[0] == 404
    # an undeclared relation of a configured namespace: the checks end in errors
    it = Interner()
    reg2 = Registry([RelationTuple.from_string("a:o#r@u")], [Namespace("a", [Relation("r")])], interner=it)
    e2 = reg2.permission_engine()
    with pytest.raises(CheckError) as ex:
        e2.lookup_objects("a", "nope", "u", 0)
    assert ex.value.code == 1
    assert ListObjectsHandler(e2, reg2.mapper).get_list_objects("namespace=a&relation=nope&subject_id=u")[0] == 500
