"""GPU tests at the depth limits: walks of up to 301 hops under request and global depths of up to 65535, across
the thresholds the code has -- the stream tier's 7-bit rest depth (127), the MS-BFS tier's 32 depth masks, the
16-bit packed depth field, the interpreter's 1,024 frames.  Every answer is compared exactly with the CPU oracle.

The graph: a chain g:c0 .. g:c300, c_i#m holding (g:c_{i+1}#m) and (g:x_i#m) -- two set edges a row, so a
one-edge stream budget hands every walk on -- with `end` on c300#m and a dummy user on every x_i#m; and a
40-cycle h:k0 .. h:k39 with `cyc` on k39.  c_j@end is a member exactly when the depth is at least 301 - j.
The oracle's canonical policy recurses once per depth level around a cycle (its C stack ends somewhere between
32,768 and 65,535 levels), so a query that can enter the cycle keeps a request depth of at most 302, and the cycle
has a namespace of its own so that no lookup of the chain's namespace checks it at 65535."""
import numpy as np
import pytest

import test_gpu_lookup as lo
import test_gpu_lookup_page as lp
import test_gpu_lookup_subject_sets as lss
import test_gpu_lookup_subjects as ls
from keto_amd import _lib
from keto_amd.engine import Config, Engine, ExpandEngine, Registry, queries_array
from keto_amd.ketoapi import RelationTuple
from keto_amd.mapper import Interner, SUBJECT_ID
from keto_amd.namespace import (ComputedSubjectSet, InvertResult, Namespace, Relation, SubjectSetRewrite,
                                TupleToSubjectSet, compile_program)
from oracle.oracle import POLICY_CANONICAL, Oracle
from test_gpu_expand import GW_MODES, _cmp_records
from sparse_ids import KNOBS, device_packed, tune as _tune

pytestmark = pytest.mark.gpu

T = RelationTuple.from_string
CHAIN = 300
DEPTHS = (31, 32, 33, 127, 128, 129, 301, 302)
CHECK_KNOBS = dict(KNOBS, **{"no-budget": dict(stream_ecap=0, back_edges=0, grid_ms=1)})
_g = {}


class Chain:
    def __init__(self):
        tuples = []
        for i in range(CHAIN):
            tuples += [T(f"g:c{i}#m@(g:c{i + 1}#m)"), T(f"g:c{i}#m@(g:x{i}#m)"), T(f"g:x{i}#m@dummy")]
        tuples += [T(f"g:c{CHAIN}#m@end")]
        tuples += [T(f"h:k{i}#m@(h:k{(i + 1) % 40}#m)") for i in range(40)] + [T("h:k39#m@cyc")]
        self.it = Interner()
        self.reg = Registry(tuples, [], interner=self.it)
        self.snap = self.reg.snapshot
        self.t6 = self.it.tuples_array(tuples)
        self.oracle = Oracle(self.t6, self.it.wildcard_rel)

    def q6(self, strings):
        return np.asarray([self.it.tuple_ids(T(s)) for s in strings], np.uint32)


def chain():
    if "chain" not in _g:
        _g["chain"] = Chain()
    return _g["chain"]


def boundary_queries(D):
    """(query strings, expected members): the roots D - 2, D - 1 and D hops from `end`'s holder (member, member,
    not a member; the chain has 300 hops), the same roots for an unknown subject, and the cycle."""
    qs, want = [], []
    for hops in (D - 2, D - 1, D):
        if 0 <= hops <= CHAIN:
            qs += [f"g:c{CHAIN - hops}#m@end", f"g:c{CHAIN - hops}#m@nobody", f"g:c{CHAIN - hops}#m@(g:c{CHAIN}#m)"]
            want += [hops <= D - 1, False, None]  # None: whatever the oracle says
    qs += ["h:k0#m@cyc", "h:k1#m@cyc", "h:k0#m@end", "h:k39#m@cyc"]
    want += [D >= 40, D >= 39, False, True]
    return qs, want


def _agrees(out, want):
    return all(w is None or int(o) == int(w) for o, w in zip(out.tolist(), want))


def _check(g, q7, gmax, name):
    e = Engine(g.snap, Config(gmax))
    out, err = e.batch_check_ids(q7, with_stats=True)
    exp, oerr, _ = g.oracle.check_batch(q7[:, :6], q7[:, 6].copy().view(np.int32), gmax, POLICY_CANONICAL)
    assert not err.any() and not oerr.any()
    assert (out == exp).all(), (name, gmax, np.nonzero(out != exp)[0][:8], q7[out != exp][:4].tolist())
    return out, e.last_stats


@pytest.mark.parametrize("name", list(CHECK_KNOBS))
def test_checks_across_the_depth_thresholds(name):
    g = chain()
    _tune(g.snap, CHECK_KNOBS[name])
    g.snap.tune("level_events", 1)  # kg_stats.tail_kind is recorded with the level events
    for D in DEPTHS:
        qs, want = boundary_queries(D)
        assert D > 129 or len(qs) == 13
        q6 = g.q6(qs)
        # through the request's depth under the largest global depth, then through the global depth
        out, st = _check(g, queries_array(q6, D), 65535, name)
        assert _agrees(out, want), (D, qs, out)
        out, st = _check(g, queries_array(q6, 0), D, name)
        assert _agrees(out, want), (D, qs, out)
        print(name, D, {k: st[k] for k in ("n_light", "n_heavy", "n_back", "n_grid", "n_no_holder", "tail_kind")})
        if name == "default" and D >= 129:  # the stream tier keeps 7 bits of rest depth: deeper queries are handed on
            assert st["n_heavy"] + st["n_back"] > 0, (D, st)
        if name == "tail-ms" and D in (32, 33):  # the MS-BFS tier has 32 depth masks: deeper batches take the grid rounds
            assert st["n_heavy"] + st["n_back"] > 0 and st["tail_kind"] == (2 if D == 32 else 1), (D, st)
    g.snap.tune("level_events", 0)
    _tune(g.snap, CHECK_KNOBS["default"])


@pytest.mark.parametrize("name", list(CHECK_KNOBS))
def test_checks_at_depth_65535_through_every_boundary(name):
    """Request depth 65535 under global depth 65535 (the packed depth field's largest value), on the chain: host
    buffers, the packed host boundary and the packed device call."""
    g = chain()
    _tune(g.snap, CHECK_KNOBS[name])
    qs = [f"g:c{j}#m@{s}" for j in (0, 1, 150, 172, 299, 300) for s in ("end", "nobody", "dummy", f"(g:c{CHAIN}#m)")]
    q7 = queries_array(g.q6(qs), 65535)
    out, _ = _check(g, q7, 65535, name)
    assert 0.05 < out.mean() < 0.95 and out[0] == 1 and out[1] == 0
    pout, pairs, n_err = Engine(g.snap, Config(65535)).batch_check_packed(q7)
    assert (pout == out).all() and n_err == 0
    assert (_lib.pack_queries(q7)[:, 3] >> 16 == 65535).all()
    rc, dout, derr = device_packed(g.snap, q7, 65535)
    assert rc == 0 and (dout == out).all() and not derr.any()
    _tune(g.snap, CHECK_KNOBS["default"])


# ---------------------------------------------------------------- expand
@pytest.mark.parametrize("mode", GW_MODES + ["device"], ids=["default", "gw-all", "hash-all", "lds64-all", "device"])
def test_expand_deep_chain(mode):
    g = chain()
    gw, skip = (1, 0) if mode == "device" else mode
    g.snap.tune("expand_gw", gw)
    g.snap.tune("expand_skip_lds", skip)
    it = g.it
    sets = [("g", "c0"), ("g", "c172"), ("g", "c299"), ("h", "k0")]
    for d in (31, 33, 127, 129, 302, 65535):
        for gmax, rd in ((65535, d), (d, 0)):
            roots = np.asarray([[it.ns_id(ns), it.obj_id(o), it.rel_id("m"), rd] for ns, o in sets] +
                               [[SUBJECT_ID, it.obj_id("end"), 0, rd]], np.uint32)
            got = ExpandEngine(g.snap, Config(gmax)).build_trees_ids(roots, device=mode == "device")
            for r, t in zip(roots, got):
                _cmp_records(g.oracle.expand(int(r[0]), int(r[1]), int(r[2]), int(r[3]), gmax), t, (r.tolist(), gmax))
            # c0's whole tree: 300 levels of (c_i, x_i, x_i's dummy), then c300 and `end`
            assert (d < 302 or len(got[0]) == 3 * CHAIN + 2) and len(got[4]) == 1
    g.snap.tune("expand_gw", 1)
    g.snap.tune("expand_skip_lds", 0)


# ---------------------------------------------------------------- lookups
@pytest.mark.parametrize("D", [128, 129, 301, 302, 65535])
def test_lookups_deep_chain(D):
    g = chain()
    it = g.it
    ns, m, c0 = it.ns_id("g"), it.rel_id("m"), it.obj_id("c0")
    e = Engine(g.snap, Config(65535))
    want_objs = sorted(it.obj_id(f"c{j}") for j in range(CHAIN + 1) if CHAIN - j <= D - 1)
    # the objects of g on which `end` has m
    reqs = np.asarray([[ns, m, SUBJECT_ID, it.obj_id("end"), 0, D]], np.uint32)
    full = lp.full_objects(g.oracle, lo.domains(g.t6), reqs, 65535)
    assert full[0] == (want_objs, [])
    off, ids, err, nerr = e.lookup_objects_ids(reqs, with_stats=True)
    assert ids.tolist() == want_objs and not nerr.any() and e.last_stats["levels"] <= CHAIN + 2, e.last_stats
    lp.page_through(lp.objects_call(e), reqs, 100, full)
    assert e.last_stats["levels"] <= CHAIN + 2, e.last_stats
    # the subject ids, and the sets g:*#m, that have m on c0
    reqs = np.asarray([[ns, c0, m, D]], np.uint32)
    full = lp.full_subjects(g.oracle, ls.subject_domain(g.t6), reqs, 65535)
    assert full[0][0] == sorted([it.obj_id("dummy")] + ([it.obj_id("end")] if D >= 301 else []))
    off, ids, err, nerr = e.lookup_subjects_ids(reqs, with_stats=True)
    assert ids.tolist() == full[0][0] and not nerr.any() and e.last_stats["levels"] <= CHAIN + 2, e.last_stats
    lp.page_through(lp.subjects_call(e), reqs, 100, full)
    reqs = np.asarray([[ns, c0, m, ns, m, D], [ns, c0, m, SUBJECT_ID, 0, D], [ns, c0, m, it.ns_id("h"), m, D]], np.uint32)
    full = lss.full_reference(g.oracle, g.t6, reqs, 65535)
    assert len(full[0][0]) == 2 * min(D, CHAIN) and full[2] == ([], [])  # c_1 .. c_D and x_0 .. x_(D-1)
    off, ids, err, nerr = e.lookup_subject_sets_ids(reqs, with_stats=True)
    assert [ids[int(off[i]):int(off[i + 1])].tolist() for i in range(3)] == [f[0] for f in full] and not nerr.any()
    assert e.last_stats["levels"] <= CHAIN + 2, e.last_stats
    lp.page_through(lss.sets_call(e), reqs, 100, full)
    # the same through the global depth
    if D <= 302:
        e = Engine(g.snap, Config(D))
        off, ids, err, nerr = e.lookup_objects_ids(np.asarray([[ns, m, SUBJECT_ID, it.obj_id("end"), 0, 0]], np.uint32))
        assert ids.tolist() == want_objs


# ---------------------------------------------------------------- the interpreter
FOLDERS = 100


def _folders(monkeypatch):
    """A folder chain of 100 levels under view = viewer | parents->view and share = view & !blocked, with
    KG_MATERIALIZE=0 so that the union runs in the interpreter too."""
    if "folders" not in _g:
        monkeypatch.setenv("KG_MATERIALIZE", "0")
        C, TT, N, O = ComputedSubjectSet, TupleToSubjectSet, InvertResult, SubjectSetRewrite
        nss = [Namespace("folder", [Relation("viewer"), Relation("parents"), Relation("blocked"),
                                    Relation("view", rewrite=O([C("viewer"), TT("parents", "view")])),
                                    Relation("share", rewrite=O([C("view"), N(C("blocked"))], "and"))])]
        tuples = [T(f"folder:f{i}#parents@(folder:f{i + 1}#...)") for i in range(FOLDERS)]
        tuples += [T(f"folder:f{FOLDERS}#viewer@alice"), T(f"folder:f{FOLDERS}#viewer@mallory"), T("folder:f0#blocked@mallory"),
                   T("folder:f1#blocked@mallory"), T("folder:f2#blocked@mallory"), T("folder:f50#viewer@bob")]
        it = Interner()
        prog = compile_program(nss, it, lower_ttu=False)
        reg = Registry(tuples, nss, interner=it)
        assert reg.snapshot.materialized()["union_nodes"] == 0
        _g["folders"] = (reg, it, Oracle(it.tuples_array(tuples), it.wildcard_rel, prog))
    return _g["folders"]


@pytest.mark.parametrize("cap2", [0, 32])
def test_interpreter_deep_folder_chain(cap2, monkeypatch):
    """The interpreter keeps 1,024 frames per slot; a 100-level chain of parents->view must fit them: the answers
    and error codes are the oracle's, and KG_ERR_RESOURCE is never returned."""
    reg, it, oracle = _folders(monkeypatch)
    reg.snapshot.tune("interp_cap2", cap2)
    roots = sorted({FOLDERS - h for D in (99, 100, 101, 102, 128) for h in (D - 2, D - 1, D) if 0 <= h <= FOLDERS} | {50, 60})
    qs = [f"folder:f{j}#{rel}@{s}" for j in roots for rel in ("view", "share") for s in ("alice", "mallory", "bob", "nobody")]
    q6 = np.asarray([it.tuple_ids(T(s)) for s in qs], np.uint32)
    seen = set()
    for D in (99, 100, 101, 102, 128):
        for gmax, rd in ((65535, D), (D, 0)):
            q7 = queries_array(q6, rd)
            e = Engine(reg.snapshot, Config(gmax))
            out, err = e.batch_check_ids(q7, with_stats=True)
            assert (err != _lib.KG_ERR_RESOURCE).all(), (D, gmax, [qs[i] for i in np.nonzero(err == _lib.KG_ERR_RESOURCE)[0][:8]])
            exp, oerr, _ = oracle.check_batch(q6, q7[:, 6].copy().view(np.int32), gmax, POLICY_CANONICAL)
            bad = np.nonzero((out != exp) | (err.astype(np.int64) != oerr))[0]
            assert bad.size == 0, (D, gmax, [(qs[i], int(out[i]), int(exp[i]), int(err[i]), int(oerr[i])) for i in bad[:8]])
            assert e.last_stats["n_general"] == len(qs)
            seen.add((D, tuple(out.tolist())))
            assert 0 < (out == 1).sum() < len(out)
    assert len({o for _, o in seen}) > 1  # the depths between them move the boundary
    reg.snapshot.tune("interp_cap2", 0)
