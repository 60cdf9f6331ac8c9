"""GPU tests of the paged lookups (kg_lookup_objects_page / kg_lookup_subjects_page).  The page is defined
through the unpaged call: with A the ascending answer of a request and E its ascending erring ids, the page
from `frm` is the first `limit` ids of {a in A : a >= frm}; next is END when A holds no further id, else the
page's last id + 1; n_errors / err_code are about the ids of E in [frm, next).

  1  pages against the oracle in the walk modes, both lookups
  2  programs and errors: golden and random programs, materialised or not, undeclared relations, formulas
  3  frm = 0, limit = 0xFFFFFFFF is the unpaged call
  4  the emission filter and the regrowth of the key list
  5  the early stop: checks <= sum of max(64, 4 c*) (derived in test_early_stop_*)
  6  walk keys and confirmed candidates interleaved
  7  refresh, threads, engine and handlers
  8  one call with requests of every mode, unpaged and paged, lists at their default size and at 64 entries
"""
import threading

import numpy as np
import pytest

import test_gpu_lookup as lo
import test_gpu_lookup_subjects as ls
from golden_cases import Case, load
from keto_amd.engine import CheckError, Config, Engine, Registry, Snapshot
from keto_amd.handlers import ListObjectsHandler, ListSubjectsHandler
from keto_amd.ketoapi import RelationTuple
from keto_amd.mapper import Interner, SUBJECT_ID
from keto_amd.namespace import (ComputedSubjectSet, InvertResult, Namespace, Relation, SubjectSetRewrite,
                                compile_program)
from keto_amd.persister import RelationQuery, SnapshotPersister
from oracle.oracle import POLICY_CANONICAL, Oracle
from test_gpu_check import random_program, random_queries
from test_gpu_lookup_formula import hand_namespaces
from test_gpu_refresh import _formula_graph, _formula_namespaces

pytestmark = pytest.mark.gpu

T = RelationTuple.from_string
END = 0xFFFFFFFF


# ---------------------------------------------------------------- the reference and its slices
def _split(ids, res, err):
    bad = np.nonzero(res == 2)[0]
    return ids[res == 1].tolist(), [(int(ids[j]), int(err[j])) for j in bad]


def full_objects(oracle, dom, reqs, gmax):
    """test_gpu_lookup.reference with every erring id kept: per request (ascending member object ids,
    ascending (erring object id, code))."""
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
    err = np.asarray(err)
    return [_split(q6[ow == i, 1], res[ow == i], err[ow == i]) for i in range(len(reqs))]


def full_subjects(oracle, dom, reqs, gmax):
    """test_gpu_lookup_subjects.reference with every erring id kept."""
    n, m = len(reqs), len(dom)
    q = np.zeros((n, m, 6), np.uint32)
    for k in range(3):
        q[:, :, k] = reqs[:, k, None]
    q[:, :, 3], q[:, :, 4] = SUBJECT_ID, dom[None, :]
    depths = np.repeat(reqs[:, 3].copy().view(np.int32), m)
    res, err, _ = oracle.check_batch(q.reshape(-1, 6), depths, gmax, POLICY_CANONICAL, nthreads=8)
    res, err = res.reshape(n, m), np.asarray(err).reshape(n, m)
    return [_split(dom, res[i], err[i]) for i in range(n)]


def slice_ref(members, errs, frm, limit):
    """The page by the definition: (ids, next, n_errors, err_code)."""
    a = [x for x in members if x >= frm]
    page = a[:limit]
    nxt = END if len(a) <= limit else page[-1] + 1
    e = [c for i, c in errs if i >= frm and (nxt == END or i < nxt)]
    return page, nxt, len(e), e[0] if e else 0


def page_through(call, reqs, limit, full, start=None, stats=None):
    """Calls with every unfinished request at its own cursor until every next is END; each page must be the
    slice.  Returns the number of calls.  stats(live requests): a check of every call's counters."""
    n = len(reqs)
    cur = np.zeros(n, np.uint32) if start is None else np.asarray(start, np.uint32).copy()
    live = np.arange(n)
    nerr_sum = np.zeros(n, np.int64)
    calls = 0
    while len(live):
        pages = np.stack([cur[live], np.full(len(live), limit, np.uint32)], 1)
        off, ids, err, nerr, nxt = call(reqs[live], pages)
        assert off[0] == 0 and off[-1] == len(ids) and len(off) == len(live) + 1
        for k, i in enumerate(live.tolist()):
            got = (ids[int(off[k]):int(off[k + 1])].tolist(), int(nxt[k]), int(nerr[k]), int(err[k]))
            want = slice_ref(*full[i], int(cur[i]), limit)
            assert got == want, (i, reqs[i].tolist(), int(cur[i]), limit, got, want)
            nerr_sum[i] += got[2]
        if stats is not None:
            stats(live)
        cur[live] = nxt
        live = live[nxt != END]
        calls += 1
        assert calls <= 100000
    if start is None:  # the pages' error counts sum to the unpaged count
        assert nerr_sum.tolist() == [len(f[1]) for f in full]
    return calls


def objects_call(e):
    return lambda reqs, pages: e.lookup_objects_page_ids(reqs, pages, with_stats=True)


def subjects_call(e):
    return lambda reqs, pages: e.lookup_subjects_page_ids(reqs, pages, with_stats=True)


# ---------------------------------------------------------------- 1. walk modes against the oracle
@pytest.mark.parametrize("seed", range(4))
def test_walk_pages_objects(seed):
    it, tuples, reqs = lo._case1(seed)  # 150 requests: three walk groups
    reg = Registry(tuples, [], interner=it)
    t6 = it.tuples_array(tuples)
    oracle, dom = Oracle(t6, it.wildcard_rel), lo.domains(t6)
    for gmax in (1, 5):
        e = Engine(reg.snapshot, Config(gmax))
        full = full_objects(oracle, dom, reqs, gmax)

        def no_checks(live):
            assert e.last_stats["candidates"] == 0 and e.last_stats["rounds"] == 0, e.last_stats

        for limit in (1, 3, 1000):
            calls = page_through(objects_call(e), reqs, limit, full, stats=no_checks)
            assert calls == max(max(1, -(-len(f[0]) // limit)) for f in full)
        assert gmax < 5 or sum(len(f[0]) for f in full) > 0


@pytest.mark.parametrize("seed", range(4))
def test_walk_pages_subjects(seed):
    it, tuples, reqs = ls._case1(seed)
    reg = Registry(tuples, [], interner=it)
    t6 = it.tuples_array(tuples)
    oracle, dom = Oracle(t6, it.wildcard_rel), ls.subject_domain(t6)
    for gmax in (1, 5):
        e = Engine(reg.snapshot, Config(gmax))
        full = full_subjects(oracle, dom, reqs, gmax)

        def no_checks(live):
            assert e.last_stats["candidates"] == 0 and e.last_stats["rounds"] == 0, e.last_stats

        for limit in (1, 3, 1000):
            page_through(subjects_call(e), reqs, limit, full, stats=no_checks)
        assert gmax < 5 or sum(len(f[0]) for f in full) > 0


# ---------------------------------------------------------------- 2. programs and errors
def _golden_requests(c):
    rels = sorted({r.name for n in c.namespaces for r in n.relations} | {"undeclared"})
    subs = sorted({t.subject_id for t in c.tuples if t.subject_id is not None}) + ["nobody"]
    sets = sorted({str(t.subject_set) for t in c.tuples if t.subject_set is not None})
    qs = [T(f"{n.name}:any#{r}@{s}") for n in c.namespaces for r in rels for s in subs]
    qs += [T(f"{n.name}:any#{r}@({s})") for n in c.namespaces for r in rels for s in sets[:6]]
    rng = np.random.default_rng(1)
    oreq = lo.requests_array(c.it, qs, rng.integers(-1, 7, len(qs)))
    objects = sorted({t.object for t in c.tuples} | {t.subject_set.object for t in c.tuples if t.subject_set})
    roots = [(n.name, o, r) for n in c.namespaces for o in objects for r in rels]
    sreq = ls.requests_array(c.it, roots, rng.integers(-1, 7, len(roots)))
    return oreq, sreq


@pytest.mark.parametrize("mat", [None, "0"])
def test_golden_programs(mat, monkeypatch):
    if mat is None:
        monkeypatch.delenv("KG_MATERIALIZE", raising=False)
    else:
        monkeypatch.setenv("KG_MATERIALIZE", mat)
    n_err = 0
    for case in load("rewrites_test.json"):
        c = Case(case)
        reg = Registry(c.tuples, c.namespaces, interner=c.it)
        oracle = Oracle(c.arr, c.it.wildcard_rel, c.prog)
        oreq, sreq = _golden_requests(c)
        e = Engine(reg.snapshot, Config(6))
        ofull = full_objects(oracle, lo.domains(c.arr), oreq, 6)
        sfull = full_subjects(oracle, ls.subject_domain(c.arr), sreq, 6)
        n_err += sum(len(f[1]) for f in ofull) + sum(len(f[1]) for f in sfull)
        for limit in (2, 7):
            page_through(objects_call(e), oreq, limit, ofull)
            page_through(subjects_call(e), sreq, limit, sfull)
    assert n_err > 0  # the undeclared relations err


@pytest.mark.parametrize("mat", [None, "0"])
@pytest.mark.parametrize("unions", [False, True])
def test_random_programs(unions, mat, monkeypatch):
    """The graphs of test_gpu_lookup.test_random_programs: every rewrite kind or unions only, undeclared
    relations in tuples and requests."""
    if mat is None:
        monkeypatch.delenv("KG_MATERIALIZE", raising=False)
    else:
        monkeypatch.setenv("KG_MATERIALIZE", mat)
    n_err, n_cand = 0, []
    for seed in range(2):
        rng = np.random.default_rng(100 + seed + (1000 if unions else 0))
        nss, rels = ["a", "b", "c"], ["r0", "r1", "r2", "r3"]
        it = Interner()
        namespaces = random_program(rng, nss, rels, unions_only=unions)
        prog = compile_program(namespaces, it, lower_ttu=False)
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
        qs = random_queries(rng, nss, rels + ["undeclared"], 100, n_obj=n_obj, n_users=n_users, p_setq=0.3)
        depths = rng.integers(-1, 7, len(qs))
        oreq = lo.requests_array(it, qs, depths)
        sreq = ls.requests_array(it, ls.roots_of(qs), depths)
        t6 = it.tuples_array(tuples)
        oracle = Oracle(t6, it.wildcard_rel, prog)
        for gmax in (2, 6):
            e = Engine(reg.snapshot, Config(gmax))
            ofull = full_objects(oracle, lo.domains(t6), oreq, gmax)
            sfull = full_subjects(oracle, ls.subject_domain(t6), sreq, gmax)
            n_err += sum(len(f[1]) for f in ofull) + sum(len(f[1]) for f in sfull)
            for limit in (2, 7):
                page_through(objects_call(e), oreq, limit, ofull, stats=lambda live: n_cand.append(e.last_stats["candidates"]))
                page_through(subjects_call(e), sreq, limit, sfull)
    assert n_err > 0 and sum(n_cand) > 0


@pytest.mark.parametrize("formula", [1, 0])
def test_formula_graphs(formula):
    rng = np.random.default_rng(4100)
    n_obj, n_users = 40, 30
    it, namespaces = Interner(), _formula_namespaces()
    prog = compile_program(namespaces, it, lower_ttu=False)
    tuples = _formula_graph(rng, n_obj, n_users, 600)
    t6 = it.tuples_array(tuples)
    qrels = ["a", "u1", "u2", "u3", "f1", "f3", "f4", "f6", "f7", "nope", "f2", "f5"]
    subs = [f"u{k}" for k in (0, 7, 19, n_users + 1)] + [f"(d:o{o}#u2)" for o in (3, 11)]
    qs = [T(f"d:any#{r}@{s}") for r in qrels for s in subs for _ in (2, 5)]
    oreq = lo.requests_array(it, qs, [2, 5] * (len(qs) // 2))
    roots = [("d", f"o{o}", r) for r in qrels for o in (1, 5, 17, n_obj + 1) for _ in (2, 5)]
    sreq = ls.requests_array(it, roots, [2, 5] * (len(roots) // 2))
    oracle = Oracle(t6, it.wildcard_rel, prog)
    ofull = full_objects(oracle, lo.domains(t6), oreq, 5)
    sfull = full_subjects(oracle, ls.subject_domain(t6), sreq, 5)
    snap = Snapshot(t6, it, prog)
    snap.tune("lookup_formula", formula)
    e = Engine(snap, Config(5))
    for limit in (2, 7):
        page_through(objects_call(e), oreq, limit, ofull)
        page_through(subjects_call(e), sreq, limit, sfull)
    snap.close()


# ---------------------------------------------------------------- 3. identity
def _identity(e, kind, reqs):
    unpaged = (e.lookup_objects_ids if kind == "objects" else e.lookup_subjects_ids)(reqs)
    pages = np.stack([np.zeros(len(reqs), np.uint32), np.full(len(reqs), END, np.uint32)], 1)
    paged = (e.lookup_objects_page_ids if kind == "objects" else e.lookup_subjects_page_ids)(reqs, pages)
    for a, b in zip(unpaged, paged[:4]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert (paged[4] == END).all() and len(paged[4]) == len(reqs)
    return unpaged


def test_identity_with_the_unpaged_call():
    it, tuples, reqs = lo._case1(3)  # walk mode
    off, _, _, _ = _identity(Engine(Registry(tuples, [], interner=it).snapshot, Config(5)), "objects", reqs)
    assert off[-1] > 0
    it, tuples, reqs = ls._case1(3)
    _identity(Engine(Registry(tuples, [], interner=it).snapshot, Config(5)), "subjects", reqs)
    c = Case(load("rewrites_test.json")[0])  # programs: confirm modes, undeclared relations
    oreq, sreq = _golden_requests(c)
    e = Engine(Registry(c.tuples, c.namespaces, interner=c.it).snapshot, Config(6))
    _, _, _, nerr = _identity(e, "objects", oreq)
    assert nerr.any()
    _identity(e, "subjects", sreq)
    rng = np.random.default_rng(4101)  # formula graphs, the key on and off
    it, namespaces = Interner(), _formula_namespaces()
    prog = compile_program(namespaces, it, lower_ttu=False)
    t6 = it.tuples_array(_formula_graph(rng, 40, 30, 600))
    qs = [T(f"d:any#{r}@u{k}") for r in ("f1", "f2", "f3", "u2", "nope") for k in (0, 7, 31)]
    oreq = lo.requests_array(it, qs, [5] * len(qs))
    sreq = ls.requests_array(it, [("d", f"o{o}", r) for r in ("f1", "f2", "f3", "u2", "nope") for o in (1, 5, 41)], [5] * 15)
    snap = Snapshot(t6, it, prog)
    for key in (1, 0):
        snap.tune("lookup_formula", key)
        _identity(Engine(snap, Config(5)), "objects", oreq)
        _identity(Engine(snap, Config(5)), "subjects", sreq)
    snap.close()


def test_no_request():
    it = Interner()
    reg = Registry([T("n:o#r@u")], [], interner=it)
    e = Engine(reg.snapshot, Config(5))
    for call, w in ((e.lookup_objects_page_ids, 6), (e.lookup_subjects_page_ids, 4)):
        off, ids, err, nerr, nxt = call(np.zeros((0, w), np.uint32), np.zeros((0, 2), np.uint32))
        assert off.tolist() == [0] and len(ids) == len(err) == len(nerr) == len(nxt) == 0


# ---------------------------------------------------------------- 4. the emission filter
def test_emission_filter_and_regrowth():
    it = Interner()
    tuples = [T(f"n:o{i}#r@big") for i in range(20000)]
    reg = Registry(tuples, [], interner=it)
    e = Engine(reg.snapshot, Config(5))
    reqs = lo.requests_array(it, [T("n:any#r@big")], [0])
    _, A, _, _ = e.lookup_objects_ids(reqs)
    assert len(A) == 20000
    reg.snapshot.tune("lookup_cap", 256)
    try:
        frm = int(A[-10])  # exactly 10 answer ids at or above it: they fit the 256 entries, nothing regrows
        off, ids, err, nerr, nxt = e.lookup_objects_page_ids(reqs, [[frm, 4]], with_stats=True)
        assert ids.tolist() == A[-10:-6].tolist() and int(nxt[0]) == int(A[-7]) + 1 and not nerr.any()
        assert e.last_stats["exact"] == 10 and e.last_stats["candidates"] == 0, e.last_stats
        off, ids, err, nerr, nxt = e.lookup_objects_page_ids(reqs, [[int(A[-1]) + 1, 4]], with_stats=True)
        assert len(ids) == 0 and off.tolist() == [0, 0] and int(nxt[0]) == END
        assert e.last_stats["exact"] == 0, e.last_stats
        off, ids, err, nerr, nxt = e.lookup_objects_page_ids(reqs, [[0, 5]], with_stats=True)  # the list regrows
        assert ids.tolist() == A[:5].tolist() and int(nxt[0]) == int(A[4]) + 1
        assert e.last_stats["exact"] == 20000, e.last_stats
        # the same for the forward walk: 20,000 subject ids of one object
        it2 = Interner()
        reg2 = Registry([T(f"n:big#r@s{i}") for i in range(20000)], [], interner=it2)
        e2 = Engine(reg2.snapshot, Config(5))
        sreq = ls.requests_array(it2, [("n", "big", "r")], [0])
        _, S, _, _ = e2.lookup_subjects_ids(sreq)
        assert len(S) == 20000
        reg2.snapshot.tune("lookup_cap", 256)
        off, ids, err, nerr, nxt = e2.lookup_subjects_page_ids(sreq, [[int(S[-10]), 4]], with_stats=True)
        assert ids.tolist() == S[-10:-6].tolist() and int(nxt[0]) == int(S[-7]) + 1
        assert e2.last_stats["exact"] == 10, e2.last_stats
        off, ids, err, nerr, nxt = e2.lookup_subjects_page_ids(sreq, [[0, 5]], with_stats=True)
        assert ids.tolist() == S[:5].tolist() and int(nxt[0]) == int(S[4]) + 1 and e2.last_stats["exact"] == 20000
    finally:
        reg.snapshot.tune("lookup_cap", 0)


# ---------------------------------------------------------------- 5. the early stop
# The cap.  c* of a request: the position, among its ascending candidates >= frm, of the one that completes
# limit + 1 members (the number of its candidates when none does).  The first round checks at most 64
# candidates and every later round at most doubles the request's total, so the total T when the request
# stops satisfies T <= 64 or T/2 < c* (the round before had not reached c*): T <= max(64, 2 c*), within the
# bound the issue states, max(64, 4 c*).  A call's checks are at most the sum over its requests.
N_DOCS = 4096


def _doc_namespaces():
    C, N, O = ComputedSubjectSet, InvertResult, SubjectSetRewrite
    return [Namespace("doc", [Relation("viewer"), Relation("blocked"),
                              Relation("share", rewrite=O([C("viewer"), N(C("blocked"))], "and"))])]


@pytest.fixture(scope="module")
def docs():
    """dense: viewer of every doc; sparse: of every 64th (the 64th, 128th, ...); bk: viewer of every doc and
    blocked on the first 20; ghost: named by no tuple."""
    it = Interner()
    tuples = [RelationTuple("doc", f"d{i}", "viewer", subject_id="dense") for i in range(N_DOCS)]
    tuples += [RelationTuple("doc", f"d{i}", "viewer", subject_id="sparse") for i in range(63, N_DOCS, 64)]
    tuples += [RelationTuple("doc", f"d{i}", "viewer", subject_id="bk") for i in range(N_DOCS)]
    tuples += [RelationTuple("doc", f"d{i}", "blocked", subject_id="bk") for i in range(20)]
    reg = Registry(tuples, _doc_namespaces(), interner=it)
    ids = np.asarray([it.obj_id(f"d{i}") for i in range(N_DOCS)], np.uint32)
    assert (np.diff(ids.astype(np.int64)) > 0).all()  # d0, d1, ... in id order
    yield reg, it, ids
    reg.snapshot.tune("lookup_formula", 1)


def _share(it, who):
    return lo.requests_array(it, [T(f"doc:any#share@{w}") for w in who], [0] * len(who))


@pytest.mark.parametrize("formula", [0, 1])
def test_early_stop_dense(docs, formula):
    reg, it, ids = docs
    reg.snapshot.tune("lookup_formula", formula)
    e = Engine(reg.snapshot, Config(5))
    reqs = _share(it, ["dense"])
    _, A, _, _ = e.lookup_objects_ids(reqs, with_stats=True)
    assert A.tolist() == ids.tolist() and e.last_stats["candidates"] == N_DOCS  # the unpaged call checks every doc
    for at in (0, 2000):  # from the start and from a cursor in the middle
        off, got, err, nerr, nxt = e.lookup_objects_page_ids(reqs, [[int(ids[at]), 8]], with_stats=True)
        print("dense", formula, at, e.last_stats)
        assert got.tolist() == ids[at:at + 8].tolist() and int(nxt[0]) == int(ids[at + 7]) + 1 and not nerr.any()
        assert 9 <= e.last_stats["candidates"] <= 64 and e.last_stats["rounds"] == 1, e.last_stats  # c* = 9


@pytest.mark.parametrize("formula", [0, 1])
def test_early_stop_sparse_empty_blocked(docs, formula):
    reg, it, ids = docs
    reg.snapshot.tune("lookup_formula", formula)
    e = Engine(reg.snapshot, Config(5))
    members = ids[63::64]
    # confirm-all: every doc is a candidate, the 9th member is the 576th; the formula mode's candidates are
    # the 64 docs the walk reaches, the 9th of them completes the page
    off, got, err, nerr, nxt = e.lookup_objects_page_ids(_share(it, ["sparse"]), [[0, 8]], with_stats=True)
    print("sparse", formula, e.last_stats)
    assert got.tolist() == members[:8].tolist() and int(nxt[0]) == int(members[7]) + 1
    assert e.last_stats["candidates"] <= (4 * 576 if formula == 0 else 64), e.last_stats
    assert e.last_stats["candidates"] >= (576 if formula == 0 else 9)
    # nobody names ghost: no member ends the rounds early
    off, got, err, nerr, nxt = e.lookup_objects_page_ids(_share(it, ["ghost"]), [[0, 8]], with_stats=True)
    assert len(got) == 0 and int(nxt[0]) == END and not nerr.any()
    assert e.last_stats["candidates"] == (N_DOCS if formula == 0 else 0), e.last_stats
    # blocked on the first 20 docs: the page starts at the 21st
    off, got, err, nerr, nxt = e.lookup_objects_page_ids(_share(it, ["bk"]), [[0, 8]], with_stats=True)
    assert got.tolist() == ids[20:28].tolist() and int(nxt[0]) == int(ids[27]) + 1
    assert 29 <= e.last_stats["candidates"] <= 4 * 29, e.last_stats  # c* = 29


def test_early_stop_mixed_call(docs):
    reg, it, ids = docs
    reg.snapshot.tune("lookup_formula", 0)
    e = Engine(reg.snapshot, Config(5))
    reqs = _share(it, ["dense", "sparse", "ghost"])
    off, got, err, nerr, nxt = e.lookup_objects_page_ids(reqs, [[0, 8]] * 3, with_stats=True)
    print("mixed", e.last_stats)
    assert got[int(off[0]):int(off[1])].tolist() == ids[:8].tolist()
    assert got[int(off[1]):int(off[2])].tolist() == ids[63::64][:8].tolist()
    assert off[2] == off[3] and nxt.tolist() == [int(ids[7]) + 1, int(ids[63::64][7]) + 1, END]
    assert e.last_stats["candidates"] <= 64 + 4 * 576 + 4 * N_DOCS, e.last_stats
    assert e.last_stats["candidates"] <= 64 + 1024 + N_DOCS, e.last_stats  # what the doubling gives here
    # every request at its own cursor until the end, against the unpaged answers
    unp = e.lookup_objects_ids(reqs)
    full = [(unp[1][int(unp[0][i]):int(unp[0][i + 1])].tolist(), []) for i in range(3)]
    page_through(objects_call(e), reqs, 1000, full)


def test_early_stop_subjects():
    it = Interner()
    tuples = [RelationTuple("doc", "d0", "viewer", subject_id=f"u{i}") for i in range(2048)]
    reg = Registry(tuples, _doc_namespaces(), interner=it)
    reg.snapshot.tune("lookup_formula", 0)
    e = Engine(reg.snapshot, Config(5))
    sreq = ls.requests_array(it, [("doc", "d0", "share")], [0])
    _, S, _, _ = e.lookup_subjects_ids(sreq, with_stats=True)
    assert len(S) == 2048 and e.last_stats["candidates"] == 2048
    for at in (0, 1000):
        off, got, err, nerr, nxt = e.lookup_subjects_page_ids(sreq, [[int(S[at]), 8]], with_stats=True)
        assert got.tolist() == S[at:at + 8].tolist() and int(nxt[0]) == int(S[at + 7]) + 1
        assert 9 <= e.last_stats["candidates"] <= 64 and e.last_stats["rounds"] == 1, e.last_stats
    full = [(S.tolist(), [])]
    assert page_through(subjects_call(e), sreq, 500, full) == 5
    reg.snapshot.tune("lookup_domain_rows", 1)  # the domain sorted out of the check rows
    page_through(subjects_call(e), sreq, 500, full)


def test_subject_domain_of_many_waves():
    """60,000 subject ids: the holder bitmap is listed by many waves in the order they reserve their entries;
    the paged call indexes the domain by id, so it must sort it.  Two confirm requests at different cursors."""
    it = Interner()
    tuples = [RelationTuple("doc", "d0", "viewer", subject_id=f"u{i}") for i in range(60000)]
    tuples += [RelationTuple("doc", "d1", "viewer", subject_id=f"u{i}") for i in range(0, 60000, 7)]
    reg = Registry(tuples, _doc_namespaces(), interner=it)
    reg.snapshot.tune("lookup_formula", 0)
    e = Engine(reg.snapshot, Config(5))
    sreq = ls.requests_array(it, [("doc", "d0", "share"), ("doc", "d1", "share")], [0, 0])
    off, S, err, nerr = e.lookup_subjects_ids(sreq)
    full = [(S[int(off[i]):int(off[i + 1])].tolist(), []) for i in range(2)]
    assert len(full[0][0]) == 60000 and len(full[1][0]) == 8572
    assert page_through(subjects_call(e), sreq, 9000, full) == 7
    off, got, err, nerr, nxt = e.lookup_subjects_page_ids(sreq, [[full[0][0][31000], 8], [full[1][0][5000], 8]],
                                                          with_stats=True)
    assert got.tolist() == full[0][0][31000:31008] + full[1][0][5000:5008]
    assert nxt.tolist() == [full[0][0][31007] + 1, full[1][0][5007] + 1]
    assert e.last_stats["candidates"] <= 64 + 4 * 57, e.last_stats  # c* = 9, and 57: every 7th id is a member


# ---------------------------------------------------------------- 6. walk keys between candidates
def test_exact_keys_and_candidates_interleave():
    """d:*#a@bob in reverse mode: the even objects' nodes are pure and listed by the walk; the odd ones hold a
    subject set that reaches a rewrite, so they are impure candidates -- every other of them a member.  A walk
    key must not be placed ahead of a candidate that has not been checked yet."""
    it = Interner()
    n = 300
    tuples = []
    for i in range(n):
        if i % 2 == 0 or i % 4 == 1:
            tuples.append(T(f"d:o{i}#a@bob"))
        if i % 2:
            tuples.append(T(f"d:o{i}#a@(d:z#share)"))
    tuples.append(T("d:z#b@carol"))
    reg = Registry(tuples, hand_namespaces(), interner=it)
    e = Engine(reg.snapshot, Config(5))
    reqs = lo.requests_array(it, [T("d:any#a@bob"), T("d:any#a@carol"), T("d:any#a@bob")], [0, 0, 3])
    off, A, err, nerr = e.lookup_objects_ids(reqs, with_stats=True)
    st = e.last_stats
    want = [it.obj_id(f"o{i}") for i in range(n) if i % 4 != 3]
    assert A[:int(off[1])].tolist() == want and not nerr.any()
    assert st["candidates"] == 3 * (n // 2) and 0 < st["exact"] < st["n_objs"] and st["confirmed"] > 0, st
    full = [(A[int(off[i]):int(off[i + 1])].tolist(), []) for i in range(3)]
    for limit in (1, 2, 3):
        page_through(objects_call(e), reqs, limit, full)
    off, got, err, nerr, nxt = e.lookup_objects_page_ids(reqs[:1], [[0, 5]], with_stats=True)
    assert got.tolist() == want[:5] and e.last_stats["candidates"] <= 64 and e.last_stats["exact"] == n // 2


# ---------------------------------------------------------------- 7. refresh, threads, engine, handlers
def test_pages_after_refresh():
    it, namespaces = Interner(), hand_namespaces()
    m = SnapshotPersister(namespaces=namespaces, interner=it, max_read_depth=10, seed=3)
    e = m.permission_engine()
    m.write_relation_tuples(*[T(f"d:o{i}#a@alice") for i in range(30)], *[T(f"d:o{i}#blocked@alice") for i in (3, 4)])
    reqs = lo.requests_array(it, [T("d:any#share@alice"), T("d:any#u@alice"), T("d:any#nope@alice")], [0, 0, 0])
    sreq = ls.requests_array(it, [("d", "o1", "share"), ("d", "o1", "u"), ("d", "o7", "a")], [0, 0, 0])

    def check(step):
        unp = e.lookup_objects_ids(reqs)
        full = [(unp[1][int(unp[0][i]):int(unp[0][i + 1])].tolist(), []) for i in range(2)]
        nope = full[1][0]  # alice reaches u on every live object of d: each errs on the undeclared relation
        for limit in (1, 4):
            page_through(objects_call(e), reqs[:2], limit, full)
            page_through(objects_call(e), reqs[2:], limit, [([], [(o, 1) for o in nope])])
        assert int(unp[3][2]) == len(nope)
        uns = e.lookup_subjects_ids(sreq)
        sfull = [(uns[1][int(uns[0][i]):int(uns[0][i + 1])].tolist(), []) for i in range(3)]
        page_through(subjects_call(e), sreq, 1, sfull)
        return full

    full = check(0)
    assert len(full[0][0]) == 28 and len(full[1][0]) == 30
    m.write_relation_tuples(*[T(f"d:o{i}#b@alice") for i in range(40, 45)], T("d:o1#a@bert"))
    full = check(1)
    assert it.obj_id("o42") in full[0][0]
    m.delete_all_relation_tuples(RelationQuery(namespace="d", object="o10"))  # must not reappear on any page
    full = check(2)
    assert it.obj_id("o10") not in full[0][0] and it.obj_id("o11") in full[0][0] and len(full[0][0]) == 32
    A = full[0][0]  # the name-level page from o9: o9 and the next id of the answer, never o10
    k = A.index(it.obj_id("o9"))
    assert k + 2 < len(A)
    names, nxt = e.lookup_objects_page("d", "share", "alice", 0, it.obj_id("o9"), 2)
    assert names == [it.obj_name(A[k]), it.obj_name(A[k + 1])] and nxt == A[k + 1] + 1 and "o10" not in names
    names, nxt = e.lookup_objects_page("d", "share", "alice", 0, 0, 1000)
    assert names == [it.obj_name(o) for o in A] and nxt is None and "o10" not in names
    assert m.applies == 2


def test_eight_threads_page_different_requests():
    it, tuples, reqs = lo._case1(2)
    reg = Registry(tuples, [], interner=it)
    serial = Engine(reg.snapshot, Config(5))
    off, A, _, _ = serial.lookup_objects_ids(reqs)
    full = [(A[int(off[i]):int(off[i + 1])].tolist(), []) for i in range(len(reqs))]
    c = Case(load("rewrites_test.json")[0])
    oreq, _ = _golden_requests(c)
    reg2 = Registry(c.tuples, c.namespaces, interner=c.it)
    oracle = Oracle(c.arr, c.it.wildcard_rel, c.prog)
    full2 = full_objects(oracle, lo.domains(c.arr), oreq, 6)
    errors = []

    def work(k):
        try:
            if k % 2:
                mine = np.arange(k, len(reqs), 8)
                page_through(objects_call(Engine(reg.snapshot, Config(5))), reqs[mine], 2, [full[i] for i in mine])
            else:
                mine = np.arange(k, len(oreq), 8)
                page_through(objects_call(Engine(reg2.snapshot, Config(6))), oreq[mine], 2, [full2[i] for i in mine])
        except BaseException as x:  # noqa: BLE001
            errors.append(x)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_engine_and_handlers_in_id_order():
    it, namespaces = Interner(), _formula_namespaces()
    # test_gpu_lookup_formula.test_candidate_once: p errs on f2, q, r and s are candidates; more objects behind
    tuples = [T("d:p#a@(d:x#und)"), T("d:p#blocked@(d:x#und)"), T("d:q#b@bob"), T("d:q#blocked@bob"), T("d:r#a@bob"),
              T("d:s#b@bob"), T("d:s#b@carol")] + [T(f"d:zz{i}#b@bob") for i in (5, 40, 3, 12, 7)]
    reg = Registry(tuples, namespaces, interner=it)
    e = reg.permission_engine()
    with pytest.raises(CheckError):
        e.lookup_objects("d", "f2", "bob", 0)
    reg.snapshot.tune("lookup_formula", 0)  # the unpaged ids without the error: the members of f2 for bob
    by_id = [it.obj_name(int(o)) for o in e.lookup_objects_ids(lo.requests_array(it, [T("d:any#f2@bob")], [0]))[1]]
    reg.snapshot.tune("lookup_formula", 1)
    assert sorted(by_id) == sorted(["q", "s", "zz5", "zz40", "zz3", "zz12", "zz7"])
    assert by_id != sorted(by_id)  # id order is not name order here
    p = it.obj_id("p")
    assert p < it.obj_id("q")
    with pytest.raises(CheckError) as ex:  # the first page covers p
        e.lookup_objects_page("d", "f2", "bob", 0, 0, 3)
    assert ex.value.code != 0
    assert e.lookup_objects_page("d", "f2", "bob", 0, p + 1, 3) == (by_id[:3], it.obj_id(by_id[2]) + 1)
    assert e.lookup_objects_page("d", "f2", "bob", 0, it.obj_id(by_id[2]) + 1, 100) == (by_id[3:], None)
    h = ListObjectsHandler(e, reg.mapper)
    base = "namespace=d&relation=f2&subject_id=bob&order=id&page_size=3"
    assert h.get_list_objects(base)[0] == 500  # an error inside the page: that page only
    got, token, pages = [], str(p + 1), 0
    while token:
        status, body = h.get_list_objects(base + "&page_token=" + token)
        assert status == 200 and 1 <= len(body["objects"]) <= 3
        got += body["objects"]
        token = body["next_page_token"]
        pages += 1
    assert got == by_id and pages == 3
    assert h.get_list_objects(base + "&page_token=zz")[0] == 400
    assert h.get_list_objects(base + "&page_token=-1")[0] == 400
    assert h.get_list_objects("namespace=nope&relation=f2&subject_id=bob&order=id")[0] == 404
    assert h.grpc_list_objects({"namespace": "d", "relation": "f2", "subject": {"id": "bob"}, "order": "id",
                                "page_token": str(p + 1), "page_size": 3}) == \
        {"objects": by_id[:3], "next_page_token": str(it.obj_id(by_id[2]) + 1)}
    # without order: the name-ordered responses, as before
    assert h.get_list_objects("namespace=d&relation=f2&subject_id=bob")[0] == 500
    plain = h.get_list_objects("namespace=d&relation=b&subject_id=bob&page_size=3&page_token=3")
    names = e.lookup_objects("d", "b", "bob", 0)
    assert plain == (200, {"objects": names[3:6], "next_page_token": "6"}) and names == sorted(names)
    # subjects
    hs = ListSubjectsHandler(e, reg.mapper)
    sub_by_id = [n for _, n in sorted((it.obj_id(n), n) for n in e.lookup_subjects("d", "s", "b", 0))]
    assert sub_by_id == ["bob", "carol"]
    assert e.lookup_subjects_page("d", "s", "b", 0, 0, 1) == (["bob"], it.obj_id("bob") + 1)
    status, body = hs.get_list_subjects("namespace=d&object=s&relation=b&order=id&page_size=1")
    assert (status, body) == (200, {"subject_ids": ["bob"], "next_page_token": str(it.obj_id("bob") + 1)})
    status, body = hs.get_list_subjects("namespace=d&object=s&relation=b&order=id&page_size=1&page_token=" +
                                        body["next_page_token"])
    assert (status, body) == (200, {"subject_ids": ["carol"], "next_page_token": ""})
    assert hs.get_list_subjects("namespace=d&object=s&relation=b&order=id&page_token=1x")[0] == 400
    assert hs.get_list_subjects("namespace=d&object=s&relation=b&page_size=1")[1] == \
        {"subject_ids": ["bob"], "next_page_token": "1"}
    assert hs.get_list_subjects("namespace=d&object=p&relation=f2&order=id")[0] == \
        hs.get_list_subjects("namespace=d&object=p&relation=f2")[0]


def test_sharded_snapshot_is_refused():
    from keto_amd import _lib
    it, tuples, reqs = lo._case1(2)
    snap = Snapshot(it.tuples_array(tuples), it, shard=(0, 2))
    pages = np.stack([np.zeros(len(reqs), np.uint32), np.full(len(reqs), 3, np.uint32)], 1)
    with pytest.raises(_lib.KetoGPUError, match="not supported on hash-sharded snapshots") as ex:
        Engine(snap, Config(5)).lookup_objects_page_ids(reqs, pages)
    assert "(-3)" in str(ex.value)
    with pytest.raises(_lib.KetoGPUError, match="limit 0"):
        Engine(snap, Config(5)).lookup_objects_page_ids(reqs[:1], [[0, 0]])


# ---------------------------------------------------------------- 8. every tail through the shared confirm step
def _mixed_case():
    """Two namespaces, about 320 objects.  d: a, b and blocked are plain (reverse mode / walk), share = a and not
    blocked is a formula over plain leaves, open = not blocked has f(0) = true (confirm-all, with members) and
    nope is undeclared (confirm-all, every id errs).  The nodes d:o250..o259#a hold a subject set that reaches
    the rewrite share, so they are impure: candidates of the reverse requests and confirm-mode roots.  Returns
    the requests with the mode each takes, interleaved, one of them twice."""
    it = Interner()
    C, N, O = ComputedSubjectSet, InvertResult, SubjectSetRewrite
    namespaces = [Namespace("d", [Relation("a"), Relation("b"), Relation("blocked"),
                                  Relation("share", rewrite=O([C("a"), N(C("blocked"))], "and")),
                                  Relation("open", rewrite=O([N(C("blocked"))]))]),
                  Namespace("g", [Relation("m")])]
    tuples = [T(f"d:o{i}#a@big") for i in range(200)] + [T(f"d:o{i}#a@alice") for i in range(30)]
    tuples += [T(f"d:o{i}#b@alice") for i in range(300, 310)]
    tuples += [T(f"d:o{i}#blocked@alice") for i in (3, 4, 100)] + [T(f"d:o{i}#blocked@big") for i in range(150, 160)]
    tuples += [T(f"d:o{i}#a@(d:z#share)") for i in range(250, 260)] + [T("d:z#a@carol"), T("d:z#a@big")]
    tuples += [T(f"d:hub#a@s{i}") for i in range(100)] + [T("d:hub#blocked@s5"), T("d:hub#blocked@s6")]
    tuples += [T(f"g:t{k}#m@alice") for k in range(10)] + [T(f"g:t{k}#m@(g:core#m)") for k in range(5, 90)]
    tuples += [T("g:core#m@big")]
    oq = [("reverse", "d:any#a@big"), ("formula", "d:any#share@alice"), ("all", "d:any#open@alice"),
          ("all", "d:any#nope@alice"), ("reverse", "d:any#a@carol"), ("formula", "d:any#share@big"),
          ("all", "d:any#open@big"), ("reverse", "g:any#m@big"), ("all", "d:any#nope@big"),
          ("reverse", "d:any#a@big"), ("formula", "d:any#share@carol"), ("reverse", "g:any#m@alice")]
    sq = [("walk", ("d", "hub", "a")), ("formula", ("d", "hub", "share")), ("confirm", ("d", "hub", "open")),
          ("confirm", ("d", "hub", "nope")), ("walk", ("d", "o1", "a")), ("formula", ("d", "o1", "share")),
          ("confirm", ("d", "o251", "a")), ("walk", ("g", "t7", "m")), ("confirm", ("d", "o1", "open")),
          ("walk", ("d", "hub", "a")), ("formula", ("d", "o150", "share")), ("confirm", ("d", "o1", "nope"))]
    prog = compile_program(namespaces, it, lower_ttu=False)
    t6 = it.tuples_array(tuples)
    oreq = lo.requests_array(it, [T(q) for _, q in oq], [0] * len(oq))
    sreq = ls.requests_array(it, [r for _, r in sq], [0] * len(sq))
    return it, namespaces, prog, tuples, t6, (oreq, [m for m, _ in oq]), (sreq, [m for m, _ in sq])


def _mixed_reference(prog, it, t6, oreq, omodes, sreq, smodes, gmax=5):
    """The oracle's members and erring ids per request, and the conditions that keep the test from passing
    vacuously: every mode lists something, some request errs, some answer is longer than the tuned lists."""
    oracle = Oracle(t6, it.wildcard_rel, prog)
    ofull = full_objects(oracle, lo.domains(t6), oreq, gmax)
    sfull = full_subjects(oracle, ls.subject_domain(t6), sreq, gmax)
    for full, modes in ((ofull, omodes), (sfull, smodes)):
        for mode in set(modes):
            assert sum(m == mode for m in modes) >= 2
            assert any(len(f[0]) for f, m in zip(full, modes) if m == mode), mode
        assert any(len(f[1]) for f in full)
        assert max(len(f[0]) for f in full) > 64
    return ofull, sfull


@pytest.fixture(scope="module")
def mixed():
    it, namespaces, prog, tuples, t6, (oreq, omodes), (sreq, smodes) = _mixed_case()
    ofull, sfull = _mixed_reference(prog, it, t6, oreq, omodes, sreq, smodes)
    reg = Registry(tuples, namespaces, interner=it)
    yield reg, (oreq, omodes, ofull), (sreq, smodes, sfull)
    reg.snapshot.tune("lookup_cap", 0)


@pytest.mark.parametrize("kind", ["objects", "subjects"])
def test_every_tail_in_one_call(mixed, kind):
    """One call holds requests of every mode, so the scan's rows, the domain pairs, the formula keys and the
    paged rounds all pass through the same confirmation: unpaged against the oracle, the full-limit paged call
    against the unpaged one, pages of 3 from 0 to END, with the lists at their default size and starting at 64
    entries (the output list, the candidate keys and the check buffers regrow).  No fixture builds a snapshot
    without reverse indexes (they are absent only above 2^32 check rows), so the confirm-nodes mode is not run."""
    reg, ocase, scase = mixed
    reqs, modes, full = ocase if kind == "objects" else scase
    e = Engine(reg.snapshot, Config(5))
    ref = [(f[0], len(f[1]), f[1][0][1] if f[1] else 0) for f in full]
    counters = []
    for cap in (0, 64):
        reg.snapshot.tune("lookup_cap", cap)
        seen = []

        def note(live=None):
            seen.append((e.last_stats["candidates"], e.last_stats["confirmed"]))

        (lo if kind == "objects" else ls).compare(e, reqs, ref)
        note()
        assert seen[0][0] > 0 and seen[0][1] > 0 and 0 < e.last_stats["exact"] < e.last_stats["n_objs"], e.last_stats
        _identity(e, kind, reqs)
        page_through(objects_call(e) if kind == "objects" else subjects_call(e), reqs, 3, full, stats=note)
        counters.append(seen)
    assert counters[0] == counters[1]
