"""GPU tests of the subject-set lookup (kg_lookup_subject_sets, kg_lookup_subject_sets_page): for every
request (ns, obj, rel, sns, srel, depth) the list must equal what the CPU oracle's canonical check says over
EVERY subject set sns:o#srel of the domain (the sets that occur as the subject of a tuple), with the same
error count and the code of the lowest erring set.  A request with sns = KG_SUBJECT_ID lists subject ids
and must equal kg_lookup_subjects.

  1  random graphs, walk mode                      6  refresh (kg_snapshot_apply)
  2  id equivalence, mixed calls                   7  handler, threads, sharded snapshots
  3  the depth boundary                            8  the paged call over the cases of 1, 4 and 5
  4  shapes: hub row, cycle, `...`, duplicates
  5  rewrites: formula / confirm / interpreter / undeclared, random programs
"""
import threading

import numpy as np
import pytest

import test_gpu_lookup_subjects as ls
from keto_amd.engine import CheckError, Config, Engine, Registry, Snapshot
from keto_amd.handlers import ListSubjectsHandler
from keto_amd.ketoapi import RelationTuple, SubjectSet
from keto_amd.mapper import Interner, SUBJECT_ID
from keto_amd.namespace import (ComputedSubjectSet, InvertResult, Namespace, Relation, SubjectSetRewrite,
                                TupleToSubjectSet, compile_program)
from oracle.oracle import POLICY_CANONICAL, Oracle
from refresh_ref import apply_ref
from test_gpu_check import random_graph, random_program, random_queries
from test_gpu_lookup_page import END, page_through

pytestmark = pytest.mark.gpu

T = RelationTuple.from_string
NOT_FOUND = 1  # KG_ERR_RELATION_NOT_FOUND


# ---------------------------------------------------------------- the reference
def set_domain(t6, sns, srel):
    """The ascending object ids o such that sns:o#srel is the subject of a tuple."""
    t6 = np.asarray(t6, np.uint32).reshape(-1, 6)
    return np.unique(t6[(t6[:, 3] == sns) & (t6[:, 5] == srel) & (t6[:, 3] != SUBJECT_ID), 4])


def set_filters(t6):
    """The (namespace, relation) pairs that occur as subject sets."""
    t6 = np.asarray(t6, np.uint32).reshape(-1, 6)
    s = t6[t6[:, 3] != SUBJECT_ID]
    return sorted({(int(a), int(b)) for a, b in zip(s[:, 3], s[:, 5])})


def full_reference(oracle, t6, reqs, gmax):
    """Per request (ascending member ids, ascending (erring id, code)): the oracle's check of the request's
    object and relation on every subject of its domain -- the sets of its filter, or the subject ids."""
    rows, depths, owner, doms = [], [], [], {}
    for i, (ns, obj, rel, sns, srel, d) in enumerate(np.asarray(reqs, np.uint32).reshape(-1, 6).tolist()):
        ids = sns == SUBJECT_ID
        key = None if ids else (sns, srel)
        if key not in doms:
            doms[key] = ls.subject_domain(t6) if ids else set_domain(t6, sns, srel)
        dom = doms[key]
        q = np.zeros((len(dom), 6), np.uint32)
        q[:, 0], q[:, 1], q[:, 2], q[:, 3], q[:, 4], q[:, 5] = ns, obj, rel, sns, dom, 0 if ids else srel
        rows.append(q)
        depths.append(np.full(len(dom), np.uint32(d).view(np.int32), np.int64))
        owner.append(np.full(len(dom), i, np.int64))
    q6, dd, ow = np.concatenate(rows), np.concatenate(depths), np.concatenate(owner)
    res, err, _ = oracle.check_batch(q6, dd, gmax, POLICY_CANONICAL, nthreads=8)
    err = np.asarray(err)
    out = []
    for i in range(len(rows)):
        sel = ow == i
        ids_i, r, e = q6[sel, 4], res[sel], err[sel]
        out.append((ids_i[r == 1].tolist(), [(int(ids_i[j]), int(e[j])) for j in np.nonzero(r == 2)[0]]))
    return out


def brief(full):
    """(members, n_errors, err_code of the lowest erring id) per request."""
    return [(m, len(e), e[0][1] if e else 0) for m, e in full]


def requests_array(it, rows):
    """(namespace, object, relation, subject namespace | None, subject relation, depth) -> (n,6) rows; a
    subject namespace None asks for subject ids."""
    r = np.zeros((len(rows), 6), np.uint32)
    for i, (ns, obj, rel, sns, srel, d) in enumerate(rows):
        r[i] = (it.ns_id(ns), it.obj_id(obj), it.rel_id(rel), SUBJECT_ID if sns is None else it.ns_id(sns),
                0 if sns is None else it.rel_id(srel), np.int32(d).view(np.uint32))
    return r


def compare(e, reqs, ref):
    off, ids, err, nerr = e.lookup_subject_sets_ids(reqs, with_stats=True)
    assert off[0] == 0 and off[-1] == len(ids) and len(off) == len(reqs) + 1
    for i, (want, n_bad, code) in enumerate(ref):
        got = ids[int(off[i]):int(off[i + 1])].tolist()
        assert got == want, (i, reqs[i].tolist(), got[:10], want[:10])
        assert (int(nerr[i]), int(err[i])) == (n_bad, code), (i, reqs[i].tolist(), int(nerr[i]), int(err[i]), n_bad, code)
    return off, ids


def sets_call(e):
    return lambda reqs, pages: e.lookup_subject_sets_page_ids(reqs, pages, with_stats=True)


def page_all(e, reqs, full, limits=(1, 7, 100)):
    """Pages of every limit from 0 to END are the slices of the unpaged answer (page_through: the ids
    concatenate, the n_errors sum, every page's err_code is that of its range's lowest erring id); a `from` above
    every id is an empty page and END; limit 0xFFFFFFFF is the unpaged call."""
    for limit in limits:
        page_through(sets_call(e), reqs, limit, full)
    n = len(reqs)
    off, ids, err, nerr, nxt = e.lookup_subject_sets_page_ids(reqs, np.tile(np.asarray([0x7FFFFFFF, 5], np.uint32), (n, 1)))
    assert len(ids) == 0 and (nxt == END).all() and not nerr.any() and not off.any()
    off, ids, err, nerr, nxt = e.lookup_subject_sets_page_ids(reqs, np.tile(np.asarray([0, 0xFFFFFFFF], np.uint32), (n, 1)))
    u = e.lookup_subject_sets_ids(reqs)
    assert all(np.array_equal(a, b) for a, b in zip((off, ids, err, nerr), u)) and (nxt == END).all()
    first = [next((c for _, c in f[1]), 0) for f in full]
    assert err.tolist() == first  # the first non-zero err_code is the unpaged one


# ---------------------------------------------------------------- 1. random graphs, walk mode
class Graph:
    """A snapshot, its rows and oracle, and the references computed so far (one per request set and depth)."""

    def __init__(self, it, tuples, namespaces=(), reqs=None):
        self.it, self.tuples, self.reqs = it, tuples, reqs
        self.prog = compile_program(list(namespaces), it, lower_ttu=False) if namespaces else None
        self.reg = Registry(tuples, list(namespaces), interner=it, max_read_depth=10)
        self.t6 = it.tuples_array(tuples)
        self.oracle = Oracle(self.t6, it.wildcard_rel, self.prog) if self.prog is not None else \
            Oracle(self.t6, it.wildcard_rel)
        self._full = {}

    def full(self, gmax, reqs=None, tag="reqs"):
        key = (tag, gmax)
        if key not in self._full:
            self._full[key] = full_reference(self.oracle, self.t6, self.reqs if reqs is None else reqs, gmax)
        return self._full[key]


def _random_case(seed):
    rng = np.random.default_rng(9100 + seed)
    n_obj = 40 + 15 * (seed % 4)
    it, tuples, nss, rels = random_graph(rng, n_obj=n_obj, n_rows=250 + 120 * (seed % 4))
    qs = random_queries(rng, nss, rels + ["..."], 150, n_obj=n_obj)  # n_obj + 3: some roots have no node
    t6 = it.tuples_array(tuples)
    never = (it.ns_id("n1"), it.rel_id("never"))  # a pair no subject set has
    filters = set_filters(t6)
    assert never not in filters and any(f[1] == it.wildcard_rel for f in filters)
    filters.append(never)
    # The graph is sparse (a node has a third of a set child on average), so roots and filters drawn freely
    # rarely meet a set.  Every second request takes a root with a set two hops below it, and two requests in
    # three the filter of a set within three hops of their root (any level), where there is one.
    rows_of = {}
    for ns, obj, rel, sns, sobj, srel in t6.tolist():
        if sns != SUBJECT_ID:
            rows_of.setdefault((ns, obj, rel), []).append((sns, sobj, srel))
    chains = sorted(v for v in rows_of if any(c in rows_of for c in rows_of[v]))
    assert len(chains) > 3
    reqs = np.zeros((len(qs), 6), np.uint32)
    for i, t in enumerate(qs):
        root = (it.ns_id(t.namespace), it.obj_id(t.object), it.rel_id(t.relation))
        if i % 2 == 0:
            root = chains[rng.integers(len(chains))]
        levels, level = [], [root]
        for _ in range(3):
            level = [x for v in level for x in rows_of.get(v, [])]
            if level:
                levels.append(level)
        f = filters[rng.integers(len(filters))]
        if levels and rng.random() < 2 / 3:
            level = levels[rng.integers(len(levels))]
            x = level[rng.integers(len(level))]
            f = (x[0], x[2])
        reqs[i] = root + (f[0], f[1], np.int32(rng.integers(-1, 9)).view(np.uint32))
    return it, tuples, reqs


_GRAPHS = {}


def random_case(seed) -> Graph:
    """Built once per seed; the unpaged and the paged test share its snapshot and references."""
    if seed not in _GRAPHS:
        it, tuples, reqs = _random_case(seed)
        _GRAPHS[seed] = Graph(it, tuples, reqs=reqs)
    return _GRAPHS[seed]


@pytest.mark.parametrize("seed", range(8))
def test_random_graphs(seed):
    g = random_case(seed)
    # the generator, on the CPU: every filter that occurs has a domain, and some set is listed only from two
    # hops below its root on (at depth 8, not at depth 2)
    assert all(len(set_domain(g.t6, *f)) > 0 for f in set_filters(g.t6))
    deep, near = g.reqs.copy(), g.reqs.copy()
    deep[:, 5], near[:, 5] = 8, 2
    far = [set(a[0]) - set(b[0]) for a, b in zip(g.full(8, deep, "deep"), g.full(8, near, "near"))]
    assert sum(len(x) for x in far) > 0
    for gmax in (1, 3, 5, 8):
        e = Engine(g.reg.snapshot, Config(gmax))
        _, ids = compare(e, g.reqs, brief(g.full(gmax)))
        st = e.last_stats
        assert st["candidates"] == 0 and st["exact"] >= st["n_objs"] == len(ids), st  # the walk alone answered
        assert gmax < 3 or (len(ids) > 0 and st["levels"] > 0)  # not vacuous


# ---------------------------------------------------------------- 2. id equivalence, mixed calls
def test_ids_through_the_set_call_equal_lookup_subjects():
    g = random_case(1)
    as_ids = g.reqs.copy()
    as_ids[:, 3], as_ids[:, 4] = SUBJECT_ID, 77  # srel is ignored
    four = np.ascontiguousarray(g.reqs[:, [0, 1, 2, 5]])
    for gmax in (1, 5):
        e = Engine(g.reg.snapshot, Config(gmax))
        want = e.lookup_subjects_ids(four)
        got = e.lookup_subject_sets_ids(as_ids)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)) and (gmax < 5 or len(got[1]) > 0)
        compare(e, as_ids, brief(g.full(gmax, as_ids, "ids")))
        pages = np.tile(np.asarray([3, 4], np.uint32), (len(four), 1))
        assert all(np.array_equal(a, b) for a, b in zip(e.lookup_subject_sets_page_ids(as_ids, pages),
                                                        e.lookup_subjects_page_ids(four, pages)))


def test_mixed_kinds_in_one_call():
    """Id requests and set requests with three filters interleaved, 150 requests: every walk group mixes the
    kinds.  Each request answers as in a call of its own kind."""
    g = random_case(2)
    f3 = set_filters(g.t6)[:3]
    mixed = g.reqs.copy()
    for i in range(len(mixed)):
        k = i % 4
        mixed[i, 3], mixed[i, 4] = (SUBJECT_ID, 0) if k == 3 else f3[k]
    e = Engine(g.reg.snapshot, Config(5))
    off, ids = compare(e, mixed, brief(g.full(5, mixed, "mixed")))
    parts = [np.nonzero(np.arange(len(mixed)) % 4 == k)[0] for k in range(4)]
    seen = 0
    for k, part in enumerate(parts):
        if k == 3:
            o2, i2, _, _ = e.lookup_subjects_ids(np.ascontiguousarray(mixed[part][:, [0, 1, 2, 5]]))
        else:
            o2, i2, _, _ = e.lookup_subject_sets_ids(mixed[part])
        for j, r in enumerate(part.tolist()):
            a = ids[int(off[r]):int(off[r + 1])]
            assert np.array_equal(a, i2[int(o2[j]):int(o2[j + 1])]), (k, r)
            seen += len(a) > 0
    assert seen > 20
    page_all(e, mixed, g.full(5, mixed, "mixed"), limits=(7,))


# ---------------------------------------------------------------- 3. the depth boundary
def test_depth_boundary():
    it = Interner()
    tuples = [T(f"g:c{i}#m@(g:c{i - 1}#m)") for i in range(1, 7)] + [T(f"g:c{i}#m@u{i}") for i in range(7)]
    reg = Registry(tuples, [], interner=it, max_read_depth=10)
    e = reg.permission_engine()
    for d in range(1, 10):  # the set c{i} sits in the row of c{i+1}, 5 - i hops below the root c6
        want = [SubjectSet("g", f"c{i}", "m") for i in range(6) if 5 - i <= d - 1]
        assert e.lookup_subject_sets("g", "c6", "m", "g", "m", d) == want, d
        assert Engine(reg.snapshot, Config(d)).lookup_subject_sets("g", "c6", "m", "g", "m", 0) == want, d  # the global depth
    assert e.lookup_subject_sets("g", "c6", "m", "g", "...", 9) == []
    assert e.lookup_subject_sets("g", "c6", "m", "unknown", "m", 9) == []  # nothing is interned for the filter
    assert e.lookup_subject_sets("g", "c6", "m", "g", "unknown", 9) == []
    assert "unknown" not in it._ns and "unknown" not in it._rel


# ---------------------------------------------------------------- 4. shapes
def _hub_graph() -> Graph:
    if "hub" not in _GRAPHS:
        it, tuples, _ = ls._hub_case()
        named = ["g:fan#m", "g:big#m", "d:c5#v", "g:k0#m", "g:top#w", "d:c0#v", "g:y#m", "d:c20#w", "g:missing#m",
                 "d:c5#w", "g:y#w", "d:c7#v", "g:big#...", "g:top#m", "d:c39#v"]
        rows = []
        for x in named:
            ns, obj, rel = x.split(":")[0], x.split(":")[1].split("#")[0], x.split("#")[1]
            for sns, srel in (("g", "m"), ("d", "v"), ("g", "...")):
                rows += [(ns, obj, rel, sns, srel, d) for d in (2, 41)]
        rows += [("d", "c0", "v", "d", "v", d) for d in (1, 39, 40)]  # the cycle closes at depth 40
        rows.append(("g", "fan", "m", None, None, 3))  # an id request beside the fan's set request
        _GRAPHS["hub"] = Graph(it, tuples, reqs=requests_array(it, rows))  # 94 requests: two walk groups
    return _GRAPHS["hub"]


def test_hub_cycle_wildcard_duplicates():
    g = _hub_graph()
    it = g.it
    full = g.full(41)
    by = {tuple(r): f for r, f in zip(g.reqs.tolist(), full)}
    req = lambda *row: tuple(requests_array(it, [row])[0].tolist())  # noqa: E731
    assert len(by[req("g", "fan", "m", "g", "m", 2)][0]) == 5000  # a row of 5,000 set children
    cyc = by[req("d", "c0", "v", "d", "v", 41)][0]
    assert sorted(cyc) == sorted(it.obj_id(f"c{i}") for i in range(40))  # all 40, the root's own set among them
    assert by[req("d", "c0", "v", "d", "v", 39)][0] != cyc and by[req("d", "c0", "v", "d", "v", 40)][0] == cyc
    assert by[req("g", "y", "m", "g", "...", 2)][0] == [it.obj_id("big")]
    assert by[req("g", "missing", "m", "g", "m", 41)] == ([], [])
    for gmax in (41, 3):
        e = Engine(g.reg.snapshot, Config(gmax))
        _, ids = compare(e, g.reqs, brief(g.full(gmax)))
        assert e.last_stats["candidates"] == 0 and e.last_stats["exact"] >= len(ids) > 10000, e.last_stats
    g.reg.snapshot.tune("lookup_cap", 16)  # the output list starts at 16 entries: the groups are rerun with a larger one
    try:
        compare(e, g.reqs, brief(g.full(3)))
    finally:
        g.reg.snapshot.tune("lookup_cap", 0)
    compare(e, g.reqs, brief(g.full(3)))


# ---------------------------------------------------------------- 5. rewrites
def drive_namespaces():
    C, N, O, TT = ComputedSubjectSet, InvertResult, SubjectSetRewrite, TupleToSubjectSet
    view = lambda: O([C("viewer"), TT("parents", "view")])  # noqa: E731
    return [Namespace("group", [Relation("member")]),
            Namespace("folder", [Relation("viewer"), Relation("parents"), Relation("view", rewrite=view())]),
            Namespace("doc", [Relation("viewer"), Relation("parents"), Relation("blocked"),
                              Relation("view", rewrite=view()),
                              Relation("share", rewrite=O([C("view"), N(C("blocked"))], "and")),
                              Relation("nobody", rewrite=O([N(C("blocked"))])),  # the interpreter's
                              Relation("both", rewrite=O([C("viewer"), TT("parents", "view")], "and"))])]


DRIVE = """group:eng#member@alice  group:eng#member@(group:core#member)  group:core#member@bob
group:all#member@(group:eng#member)  group:ops#member@carol  group:lone#member@dave
folder:root#viewer@(group:all#member)  folder:sub#parents@(folder:root#...)  folder:sub#viewer@(group:ops#member)
doc:d1#parents@(folder:sub#...)  doc:d1#viewer@(group:lone#member)  doc:d1#blocked@(group:core#member)  doc:d1#viewer@u1
doc:d2#viewer@(group:eng#member)  doc:d2#blocked@(doc:d3#nobody)  doc:d2#parents@(folder:sub#...)
doc:d3#share@(group:ops#member)  doc:d3#viewer@(group:eng#member)  doc:d3#blocked@(group:ops#member)
doc:d4#parents@(folder:root#...)  doc:d4#viewer@(group:core#member)"""


def _drive_graph() -> Graph:
    if "drive" not in _GRAPHS:
        it = Interner()
        tuples = [T(x) for x in DRIVE.split()]
        rows = [("doc", o, rel, sns, srel, d)
                for o in ("d1", "d2", "d3", "d4", "d5")
                for rel in ("share", "view", "viewer", "parents", "blocked", "nobody", "both", "nope")
                for sns, srel in (("group", "member"), ("folder", "..."))
                for d in (0, 2)]
        rows += [("folder", o, rel, sns, srel, 0) for o in ("root", "sub") for rel in ("view", "parents", "nope")
                 for sns, srel in (("group", "member"), ("folder", "..."))]
        rows += [("doc", "d1", "share", None, None, 0), ("doc", "d2", "share", None, None, 0)]
        _GRAPHS["drive"] = Graph(it, tuples, drive_namespaces(), requests_array(it, rows))
    return _GRAPHS["drive"]


def test_rewrites_hand_graph():
    g = _drive_graph()
    it, snap = g.it, g.reg.snapshot
    groups = set_domain(g.t6, it.ns_id("group"), it.rel_id("member"))
    assert sorted(it.obj_name(int(o)) for o in groups) == ["all", "core", "eng", "lone", "ops"]
    one = lambda *row: requests_array(it, [row])  # noqa: E731
    try:
        for formula in (1, 0):
            snap.tune("lookup_formula", formula)
            for gmax in (2, 6):
                compare(Engine(snap, Config(gmax)), g.reqs, brief(g.full(gmax)))
        snap.tune("lookup_formula", 1)
        e = Engine(snap, Config(6))
        names = lambda ids: sorted(it.obj_name(int(i)) for i in ids)  # noqa: E731
        # share on d1 -- no share row, pure leaves -- walks from its view node: the sets it lists are checked once
        _, ids, _, nerr = e.lookup_subject_sets_ids(one("doc", "d1", "share", "group", "member", 0), with_stats=True)
        st = e.last_stats
        assert st["candidates"] > 0 and st["exact"] == 0 and st["candidates"] <= len(groups), st
        assert names(ids) == ["all", "eng", "lone", "ops"] and not nerr.any()  # core is blocked
        # d2's blocked leaf reaches a rewrite (doc:d3#nobody): every set of the filter's domain is checked
        _, ids, _, nerr = e.lookup_subject_sets_ids(one("doc", "d2", "share", "group", "member", 0), with_stats=True)
        st = e.last_stats
        assert st["candidates"] == len(groups) and st["exact"] == 0 and st["confirmed"] == len(ids) > 0, st
        # an undeclared relation reports every set of the domain
        _, ids, err, nerr = e.lookup_subject_sets_ids(one("doc", "d1", "nope", "group", "member", 0), with_stats=True)
        assert len(ids) == 0 and int(nerr[0]) == len(groups) and int(err[0]) == NOT_FOUND
        assert e.last_stats["candidates"] == len(groups)
        with pytest.raises(CheckError) as ex:
            e.lookup_subject_sets("doc", "d1", "nope", "group", "member", 0)
        assert ex.value.code == NOT_FOUND
        # two filters of confirm requests in one call: each request is paired with its own filter's sets only
        two = np.concatenate([one("doc", "d1", "nope", "group", "member", 0), one("doc", "d1", "nope", "folder", "...", 0)])
        _, ids, err, nerr = e.lookup_subject_sets_ids(two, with_stats=True)
        assert nerr.tolist() == [len(groups), 2] and e.last_stats["candidates"] == len(groups) + 2
    finally:
        snap.tune("lookup_formula", 1)


def _program_case(seed):
    key = ("program", seed)
    if key not in _GRAPHS:
        rng = np.random.default_rng(700 + seed)
        nss, rels = ["a", "b", "c"], ["r0", "r1", "r2", "r3"]
        it = Interner()
        namespaces = random_program(rng, nss, rels, unions_only=seed % 2 == 1)
        n_obj, n_users = 30 + 10 * seed, 25
        tuples = []
        for _ in range(150 + 60 * seed):
            ns, obj = rng.choice(nss), f"o{rng.integers(n_obj)}"
            rel = rng.choice(rels) if rng.random() < 0.97 else "undeclared"
            if rng.random() < 0.6:
                srel = rng.choice(rels + ["..."]) if rng.random() < 0.98 else "undeclared"
                s = f"({rng.choice(nss)}:o{rng.integers(n_obj)}#{srel})"
            else:
                s = f"u{rng.integers(n_users)}"
            tuples.append(T(f"{ns}:{obj}#{rel}@{s}"))
        qs = random_queries(rng, nss, rels + ["undeclared"], 100, n_obj=n_obj, n_users=n_users)
        filters = set_filters(it.tuples_array(tuples))
        reqs = np.zeros((len(qs), 6), np.uint32)
        for i, t in enumerate(qs):
            f = filters[rng.integers(len(filters))] if i % 10 else (SUBJECT_ID, 0)
            reqs[i] = (it.ns_id(t.namespace), it.obj_id(t.object), it.rel_id(t.relation), f[0], f[1],
                       np.int32(rng.integers(-1, 7)).view(np.uint32))
        _GRAPHS[key] = Graph(it, tuples, namespaces, reqs)
    return _GRAPHS[key]


@pytest.mark.parametrize("seed", range(4))
def test_random_programs(seed):
    g = _program_case(seed)
    listed = 0
    for gmax in (1, 3, 6):
        e = Engine(g.reg.snapshot, Config(gmax))
        _, ids = compare(e, g.reqs, brief(g.full(gmax)))
        listed += len(ids)
    assert listed > 0


# ---------------------------------------------------------------- 6. refresh
def test_refresh_follows_the_rows():
    it = Interner()
    namespaces = [Namespace("a", [Relation("r")])]
    prog = compile_program(namespaces, it, lower_ttu=False)
    tuples = [T("a:o0#r@(a:g1#r)"), T("a:o0#r@(a:g2#r)"), T("a:g2#r@(a:g3#r)"), T("a:o1#r@(a:g1#r)"), T("a:g3#r@u")]
    rows = it.tuples_array(tuples)
    reqs = requests_array(it, [("a", "o0", "r", "a", "r", 0), ("a", "o0", "nope", "a", "r", 0), ("a", "g3", "r", "a", "r", 0)])
    snap = Snapshot(rows, it, prog)
    names = lambda ids: sorted(it.obj_name(int(i)) for i in ids)  # noqa: E731

    def agree(s, rows):
        full = full_reference(Oracle(rows, it.wildcard_rel, prog), rows, reqs, 5)
        compare(Engine(s, Config(5)), reqs, brief(full))
        page_all(Engine(s, Config(5)), reqs, full, limits=(1,))
        return brief(full)

    ref = agree(snap, rows)
    assert names(ref[0][0]) == ["g1", "g2", "g3"] and ref[1] == ([], 3, NOT_FOUND)
    # the last tuple that holds a:g3#r goes, one with the new set a:g4#r comes: g3 stays behind as an object node
    dels, ins = it.tuples_array([tuples[2]]), it.tuples_array([T("a:g1#r@(a:g4#r)")])
    new = snap.apply(ins, dels)
    rows2, _ = apply_ref(rows, None, ins, None, dels)
    ref = agree(new, rows2)
    assert names(ref[0][0]) == ["g1", "g2", "g4"] and ref[1] == ([], 3, NOT_FOUND)
    only = new.apply(np.zeros((0, 6), np.uint32), ins)  # and the new one leaves again: two sets are left
    rows3, _ = apply_ref(rows2, None, np.zeros((0, 6), np.uint32), None, ins)
    ref = agree(only, rows3)
    assert names(ref[0][0]) == ["g1", "g2"] and ref[1] == ([], 2, NOT_FOUND)
    for s in (snap, new, only):
        s.close()


# ---------------------------------------------------------------- 7. handler, threads, sharded snapshots
def test_handler_lists_subject_sets():
    g = _drive_graph()
    e = g.reg.permission_engine()
    h = ListSubjectsHandler(e, g.reg.mapper)
    full = e.lookup_subject_sets("doc", "d1", "view", "group", "member", 6)
    assert [s.object for s in full] == ["all", "core", "eng", "lone", "ops"]
    as_json = [{"namespace": "group", "object": s.object, "relation": "member"} for s in full]
    base = {"namespace": "doc", "object": "d1", "relation": "view", "max-depth": "6",
            "subject_set.namespace": "group", "subject_set.relation": "member"}
    assert h.get_list_subjects(base) == (200, {"subject_sets": as_json, "next_page_token": ""})
    got, token = [], ""
    for _ in range(4):  # name order, by position
        status, body = h.get_list_subjects(dict(base, page_size="2", page_token=token))
        assert status == 200 and set(body) == {"subject_sets", "next_page_token"}
        got += body["subject_sets"]
        token = body["next_page_token"]
        if not token:
            break
    assert got == as_json
    by_id, token = [], ""
    for _ in range(4):  # id order, by cursor
        status, body = h.get_list_subjects(dict(base, page_size="2", page_token=token, order="id"))
        assert status == 200 and len(body["subject_sets"]) <= 2
        by_id += body["subject_sets"]
        token = body["next_page_token"]
        if not token:
            break
    assert sorted(x["object"] for x in by_id) == [x["object"] for x in as_json] and len(by_id) == 5
    assert [g.it.obj_id(x["object"]) for x in by_id] == sorted(g.it.obj_id(x["object"]) for x in by_id)
    assert h.grpc_list_subjects({"namespace": "doc", "object": "d1", "relation": "view", "max_depth": 6,
                                 "subject_set": {"namespace": "group", "relation": "member"}}) == \
        {"subject_sets": as_json, "next_page_token": ""}
    assert h.get_list_subjects(dict(base, namespace="nope"))[0] == 404
    assert h.get_list_subjects(dict(base, relation="nope"))[0] == 500  # the checks end in errors
    assert h.get_list_subjects(dict(base, **{"subject_set.namespace": "nowhere"})) == \
        (200, {"subject_sets": [], "next_page_token": ""})
    ids = h.get_list_subjects({"namespace": "doc", "object": "d1", "relation": "view", "max-depth": "6"})
    assert ids == (200, {"subject_ids": ["alice", "bob", "carol", "dave", "u1"], "next_page_token": ""})


def test_eight_threads_get_their_own_answers():
    g = random_case(0)
    full = brief(g.full(5))
    parts = [np.arange(k, len(g.reqs), 8) for k in range(8)]
    bad = []

    def work(k):
        e = Engine(g.reg.snapshot, Config(5))
        for _ in range(3):
            off, ids, err, nerr = e.lookup_subject_sets_ids(g.reqs[parts[k]])
            for j, r in enumerate(parts[k].tolist()):
                if ids[int(off[j]):int(off[j + 1])].tolist() != full[r][0] or int(nerr[j]):
                    bad.append((k, r))

    th = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad and sum(len(f[0]) for f in full) > 0


def test_sharded_snapshot_is_refused():
    from keto_amd import _lib
    it, tuples, reqs = _random_case(2)
    snap = Snapshot(it.tuples_array(tuples), it, shard=(0, 2))
    for call in (lambda e: e.lookup_subject_sets_ids(reqs),
                 lambda e: e.lookup_subject_sets_page_ids(reqs, np.tile(np.asarray([0, 5], np.uint32), (len(reqs), 1)))):
        with pytest.raises(_lib.KetoGPUError, match="not supported on hash-sharded snapshots") as ex:
            call(Engine(snap, Config(5)))
        assert "(-3)" in str(ex.value)
    snap.close()


# ---------------------------------------------------------------- 8. the paged call
@pytest.mark.parametrize("seed", range(8))
def test_pages_random_graphs(seed):
    g = random_case(seed)
    e = Engine(g.reg.snapshot, Config(5))
    page_all(e, g.reqs, g.full(5))


@pytest.mark.parametrize("limit", [1, 7, 100])
def test_pages_shapes(limit):
    g = _hub_graph()
    e = Engine(g.reg.snapshot, Config(3))
    page_all(e, g.reqs, g.full(3), limits=(limit,))
    if limit == 7:
        g.reg.snapshot.tune("lookup_cap", 16)
        try:
            page_through(sets_call(e), g.reqs, 100, g.full(3), start=np.full(len(g.reqs), 4000, np.uint32))
        finally:
            g.reg.snapshot.tune("lookup_cap", 0)


@pytest.mark.parametrize("formula", [1, 0])
def test_pages_rewrites(formula):
    g = _drive_graph()
    g.reg.snapshot.tune("lookup_formula", formula)
    try:
        for gmax in (2, 6):
            page_all(Engine(g.reg.snapshot, Config(gmax)), g.reqs, g.full(gmax))
    finally:
        g.reg.snapshot.tune("lookup_formula", 1)


@pytest.mark.parametrize("seed", range(4))
def test_pages_random_programs(seed):
    g = _program_case(seed)
    page_all(Engine(g.reg.snapshot, Config(6)), g.reqs, g.full(6))
