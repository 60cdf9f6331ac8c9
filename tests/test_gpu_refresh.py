"""GPU tests of the incremental refresh (kg_snapshot_apply, keto_amd/csrc/kg_delta.hip): what a refreshed
snapshot holds and answers, against tests/refresh_ref.py (the rows), the CPU oracle on those rows (checks,
expand trees, both lookups) and a full build from the same rows.  Bit-exact: ids, row order, answers, codes.

  1  the merged rows of direct Snapshot.apply calls on a keyed base with a 5 000-entry hub
  2  the grid-stride loops of the merge kernels (more than 2048 x 256 elements), on an unkeyed synthetic base
     whose host node map is rebuilt from the device
  3  two applies on one base and a chain; the base keeps answering as before
  4  kg_lookup_objects / kg_lookup_subjects after every transaction of a SnapshotPersister
  5  every rewrite kind (interpreter, formula split, unions, error answers) after a refresh
  6  the backward, grid and MS-BFS tiers on refreshed snapshots
"""
import numpy as np
import pytest

import test_gpu_lookup as lo
import test_gpu_lookup_subjects as ls
from keto_amd.engine import Config, Engine, ExpandEngine, Snapshot, queries_array
from keto_amd.ketoapi import RelationTuple
from keto_amd.mapper import Interner, SUBJECT_ID
from keto_amd.namespace import (ComputedSubjectSet, InvertResult, Namespace, Relation, SubjectSetRewrite,
                                TupleToSubjectSet, compile_program)
from keto_amd.persister import RelationQuery, SnapshotPersister
from oracle.oracle import POLICY_CANONICAL, Oracle
from refresh_ref import apply_ref, multiset, node_rows, nodes_of
from test_gpu_check import random_graph, random_program, random_queries
from test_gpu_expand import _cmp_records
from test_gpu_persister import shard_rows

pytestmark = pytest.mark.gpu

S = SUBJECT_ID
T = RelationTuple.from_string
STRIDE = 2048 * 256  # threads of the widest launch of k_delta_keep / _scatter_old / _copy / _isadj / _adjfill
NO_ROWS = np.zeros((0, 6), np.uint32)


def _same_rows(snap, rows, nodes, what):
    off, got = snap.rows(nodes)
    woff, want = node_rows(rows, nodes)
    bad = np.nonzero(off != woff)[0]
    assert bad.size == 0, (what, "row lengths", bad[:5], off[bad[:5]], woff[bad[:5]])
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (what, "rows", bad[:5], got[bad[:3]].tolist(), want[bad[:3]].tolist())


def _same_export(snap, rows, what):
    got, want = multiset(snap.export()), multiset(rows)
    assert got.shape == want.shape and np.array_equal(got, want), (what, got.shape, want.shape)


def _same_as_full_build(snap, rows, keys, it, nodes, what):
    full = Snapshot(rows, it, keys=keys)
    (a_off, a), (b_off, b) = snap.rows(nodes), full.rows(nodes)
    assert np.array_equal(a_off, b_off) and np.array_equal(a, b), what
    full.close()


# ---------------------------------------------------------------- 1. the merged rows
HUB = (0, 1, 1)
DUP = (0, 2, 1, S, 777, 0)
GONE = (0, 3, 2)  # the node whose every row is deleted


def _ids_interner():
    it = Interner()  # relation 0 = "..."
    for i in range(4):
        it.ns_id(f"n{i}")
    for i in range(1, 4):
        it.rel_id(f"r{i}")
    return it


def _hub_entry(i):
    return HUB + ((1, 100 + (i // 4) % 600, 1) if i % 4 == 0 else (S, 10000 + i, 0))


def _hub_base(rng):
    """A keyed base: the hub (keys 10, 20, ...), 320 ordinary nodes, three equal rows on one node."""
    rows = [_hub_entry(i) for i in range(5000)]
    keys = [10 * (i + 1) for i in range(5000)]
    for j in range(300):
        for _ in range(int(rng.integers(1, 7))):
            k = rng.integers(10)
            sub = (S, 30000 + int(rng.integers(200)), 0) if k < 6 else \
                ((1, 100 + int(rng.integers(300)), 1) if k < 9 else (2, 700 + int(rng.integers(20)), 0))
            rows.append((1, 100 + j, 1) + sub)
            keys.append(int(rng.integers(1, 60000)))
    for j in range(20):
        rows.append((2, 700 + j, 2, S, 31000 + j, 0))
        keys.append(int(rng.integers(1, 60000)))
    rows += [DUP, (0, 2, 1, S, 779, 0), DUP, DUP, (0, 2, 1, S, 778, 0)]
    keys += [15, 20, 25, 25, 25]
    rows += [GONE + (S, 40000 + j, 0) for j in range(3)] + [GONE + (1, 105, 1)]
    keys += [7, 30007, 30007, 59999]
    rows, keys = np.asarray(rows, np.uint32), np.asarray(keys, np.uint64)
    order = np.argsort(keys, kind="stable")
    return rows[order], keys[order]


def _hub_delta(rng):
    ins, ik = [], []
    hub_keys = np.concatenate([10 * rng.choice(np.arange(1, 5000), 300, replace=False) + 5,  # between old keys
                               10 * rng.choice(np.arange(1, 5001), 200, replace=False),      # equal to old keys
                               rng.integers(1, 10, 100),                                     # below the smallest
                               50001 + rng.integers(0, 50, 100)])                            # above the largest
    for j, k in enumerate(hub_keys.tolist()):
        ins.append(HUB + ((1, 100 + int(rng.integers(700)), 1) if j % 3 == 0 else (S, 50000 + j, 0)))
        ik.append(k)
    ins += [_hub_entry(1), _hub_entry(2), _hub_entry(4)]  # copies of kept entries
    ik += [12345, 20, 50]
    ins += [(2, 500 + j, 1, S, 60000 + j, 0) for j in range(20)]  # new nodes
    ik += rng.integers(1, 60000, 20).tolist()
    ins += [HUB + (2, 9999, 3), HUB + (2, 9998, 0)]  # subject sets (one "...") naming nodes that exist nowhere else
    ik += [123, 124]
    ins += [_hub_entry(3), _hub_entry(6), DUP]  # deleted below and inserted here: the inserts stay
    ik += [35, 70, 25]
    order = rng.permutation(len(ins))  # argument order is not key order
    ins, ik = np.asarray(ins, np.uint32)[order], np.asarray(ik, np.uint64)[order]
    dels = [_hub_entry(i) for i in range(0, 5000, 3)]  # every third entry: 1 667 deletes on one node
    dels += [DUP] + [GONE + (S, 40000 + j, 0) for j in range(3)] + [GONE + (1, 105, 1)]
    unknown = [HUB + (S, 999999, 0), (0, 4242, 1, S, 1, 0), HUB + (2, 8888, 1), (1, 100, 1, S, 10001, 0)]
    out_of_range = [(0xFFFF, 1, 1, S, 1, 0), (0, 0x7FFFFFFF, 1, S, 1, 0), HUB + (S, 0x7FFFFFFF, 0), HUB + (0xFFFF, 1, 1),
                    (0, 1, 0xFFFF, S, 1, 0)]
    return ins, ik, np.asarray(dels + unknown, np.uint32), np.asarray(out_of_range, np.uint32)


def test_merged_rows_keyed_hub():
    """Snapshot.apply called directly on a keyed base: a hub row of 5 000 entries (subject ids and subject sets)
    that loses every third entry and gains 700 with keys between, equal to, below and above the old ones; three
    equal rows deleted by one tuple; a node emptied completely; new nodes, one of them only named by a subject
    set; deletes of tuples the delta inserts, of unknown tuples and of out-of-range ids.  rows() of every node
    of base and delta and export() equal apply_ref and a full ordered build from apply_ref's output; then a
    second delta on the result, an empty one, one that deletes everything, and one into the emptied snapshot."""
    rng = np.random.default_rng(2024)
    it = _ids_interner()
    rows, keys = _hub_base(rng)
    ins, ik, dels, bad = _hub_delta(rng)
    nodes = nodes_of(rows, ins, dels)
    assert len(nodes) > 300
    snaps = [Snapshot(rows, it, keys=keys)]
    _same_rows(snaps[0], rows, nodes, "base")

    def step(ins, ik, dels, what):
        nonlocal rows, keys, nodes
        nodes = np.unique(np.concatenate([nodes, nodes_of(ins)]), axis=0)
        snaps.append(snaps[-1].apply(ins, dels, ik))
        rows, keys = apply_ref(rows, keys, ins, ik, dels)
        _same_rows(snaps[-1], rows, nodes, what)
        _same_export(snaps[-1], rows, what)
        _same_as_full_build(snaps[-1], rows, keys, it, nodes, what)

    n_before = len(rows)
    step(ins, ik, np.concatenate([dels, bad]), "first delta")
    hub = node_rows(rows, [HUB])[1]
    assert len(hub) < 5000 - 1600 + 710 and len(node_rows(rows, [GONE])[1]) == 0 and len(rows) < n_before
    assert (hub == np.asarray(_hub_entry(3), np.uint32)).all(1).sum() == 1  # deleted from the base, inserted once
    # the second delta: rows the first one inserted are base rows now; keys tie with old and inserted ones
    d2 = np.concatenate([ins[rng.choice(len(ins), 200, replace=False)],
                         np.asarray([_hub_entry(i) for i in range(1, 600, 3)], np.uint32)])
    i2 = np.asarray([HUB + (S, 70000 + j, 0) for j in range(60)] + [GONE + (S, 1, 0), DUP, DUP], np.uint32)
    k2 = np.concatenate([10 * rng.integers(1, 5000, 30) + 5, 10 * rng.integers(1, 5000, 30), [7, 25, 15]])
    k2 = k2.astype(np.uint64)
    step(i2, k2, d2, "second delta")
    step(NO_ROWS, np.zeros(0, np.uint64), NO_ROWS, "empty delta")
    assert len(rows) > 4000
    i3 = np.asarray([_hub_entry(i) for i in range(40)] + [(2, 500, 1, S, 5, 0), DUP], np.uint32)
    k3 = np.asarray([100 - i // 2 for i in range(40)] + [3, 3], np.uint64)
    step(i3, k3, np.unique(rows, axis=0), "everything deleted")
    assert len(rows) == 42
    step(np.asarray([HUB + (S, 5, 0), DUP, (3, 1, 1, 3, 2, 2)], np.uint32), np.asarray([90, 1, 2], np.uint64), NO_ROWS,
         "into the emptied snapshot")
    assert len(rows) == 45
    for s in snaps:
        s.close()


# ---------------------------------------------------------------- 2. the stride loops
def test_stride_loops_unkeyed_synthetic_base():
    """A delta whose touched nodes hold more than 2048 x 256 old entries, on a device-generated base of 10^6
    tuples: every grid-stride loop of the merge takes a second trip (k_delta_keep / k_delta_scatter_old over the
    touched entries, k_delta_copy / k_delta_isadj / k_delta_adjfill over all rows).  The base has no order keys
    (inserts go to the end of their rows) and no host node map (it is rebuilt from the device triples)."""
    from keto_amd import _lib
    from test_gpu_check import _torch
    torch = _torch()
    rng = np.random.default_rng(5)
    base = Snapshot.synthetic(1_000_000, seed=20250131)
    rows0 = base.export()
    old_rows = len(rows0)
    r64 = rows0.astype(np.uint64)
    node_key = (r64[:, 0] << np.uint64(48)) | (r64[:, 2] << np.uint64(32)) | r64[:, 1]
    uniq, first, inv, counts = np.unique(node_key, return_index=True, return_inverse=True, return_counts=True)
    by_len = np.argsort(-counts, kind="stable")
    n_touch = int(np.searchsorted(np.cumsum(counts[by_len]), STRIDE + 1)) + 1
    touched = by_len[:n_touch]
    assert old_rows >= STRIDE + 1 and int(counts[touched].sum()) >= STRIDE + 1, (old_rows, int(counts[touched].sum()))
    is_touched = np.zeros(len(uniq), bool)
    is_touched[touched] = True
    # export() lists node after node: a row's position in its node's row is its distance from the node's first
    assert int((np.diff(node_key) != 0).sum()) + 1 == len(uniq)
    pos = np.arange(old_rows) - first[inv]
    dels = rows0[is_touched[inv] & (pos % 5 == 0)]  # a spread: every fifth entry of every touched node
    assert len(np.unique(inv[is_touched[inv] & (pos % 5 == 0)])) == n_touch  # every touched node loses its first entry
    n_ins = 4000
    ins = rows0[first[rng.choice(touched, n_ins)]].copy()  # (ns, obj, rel) of touched nodes
    ids, sets = rows0[rows0[:, 3] == S], rows0[rows0[:, 3] != S]
    ins[:, 3:] = ids[rng.integers(0, len(ids), n_ins), 3:]
    to_set = rng.random(n_ins) < 0.3
    ins[to_set, 3:] = sets[rng.integers(0, len(sets), int(to_set.sum())), 3:]
    new_nodes = np.zeros((50, 6), np.uint32)  # nodes the base does not have
    new_nodes[:, 1], new_nodes[:, 2] = int(rows0[:, [1, 4]].max()) + 1 + np.arange(50), 1
    new_nodes[:, 3:] = ids[rng.integers(0, len(ids), 50), 3:]
    ins = np.concatenate([ins, new_nodes])
    new = base.apply(ins, dels)
    rows1, _ = apply_ref(rows0, None, ins, None, dels)
    assert len(rows1) < old_rows - STRIDE // 6
    _same_export(new, rows1, "refreshed")
    untouched = rng.choice(np.nonzero(~is_touched)[0], 1000, replace=False)
    nodes = np.concatenate([rows0[first[touched], :3], rows0[first[untouched], :3], new_nodes[:, :3]])
    _same_rows(new, rows1, nodes, "refreshed")
    n, gmax = 20000, 10
    dq = torch.empty((n, 7), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().kg_synth_queries(base.handle, 7, n, dq.data_ptr()), "kg_synth_queries")
    q = dq.cpu().numpy().view(np.uint32)
    out, err = Engine(new, Config(gmax)).batch_check_ids(q)
    exp, oerr, _ = Oracle(rows1, 0).check_batch(q[:, :6], q[:, 6].view(np.int32), gmax, POLICY_CANONICAL, nthreads=8)
    assert (err == 0).all() and (oerr == 0).all()
    assert (out == exp).all(), np.nonzero(out != exp)[0][:10]
    assert 0.01 < (exp == 1).mean() < 0.99
    base0, _ = Engine(base, Config(gmax)).batch_check_ids(q)
    assert (base0 != exp).any()  # the delta changed answers: the comparison is not one of two copies of the base
    new.close()
    base.close()


# ---------------------------------------------------------------- 3. fork and base validity
def test_fork_chain_and_base_stays_valid():
    """a = base.apply(d1), b = base.apply(d2) (the second apply on one base: its host node map has gone to a,
    so b's is rebuilt from the device triples), c = a.apply(d3).  Each equals apply_ref of its own history in
    rows, checks and expand trees; the base answers the same before the applies, after them and after a is
    closed, and c outlives a."""
    rng = np.random.default_rng(31)
    it, tuples, nss, rels = random_graph(rng, n_obj=50, n_rows=900)
    arr = it.tuples_array(tuples)
    rows0, pool = arr[:600], arr[600:]
    keys0 = np.sort(rng.integers(1, 4000, 600)).astype(np.uint64)  # ties
    qs = random_queries(rng, nss, rels, 1500, n_obj=50)
    q6 = np.asarray([it.tuple_ids(t) for t in qs], np.uint32)
    depths = rng.integers(0, 7, len(qs))
    roots = np.asarray([[it.ns_id(rng.choice(nss)), it.obj_id(f"o{rng.integers(52)}"), it.rel_id(rng.choice(rels)), 0]
                        for _ in range(120)], np.uint32)
    nodes = nodes_of(arr)

    def delta(rows, lo_, hi_):
        new_node = np.asarray([[it.ns_id(nss[0]), it.obj_id(f"fresh{lo_}"), it.rel_id(rels[0]), S, it.obj_id("u1"), 0]],
                              np.uint32)
        ins = np.concatenate([pool[lo_:hi_], new_node])
        return ins, rng.integers(1, 4000, len(ins)).astype(np.uint64), rows[rng.choice(len(rows), 40, replace=False)]

    def ask(snap, rows, what):
        out, err = Engine(snap, Config(5)).batch_check_ids(queries_array(q6, depths))
        oracle = Oracle(rows, it.wildcard_rel)
        exp, oerr, _ = oracle.check_batch(q6, depths, 5, POLICY_CANONICAL)
        assert (out == exp).all() and (err == 0).all() and (oerr == 0).all(), (what, np.nonzero(out != exp)[0][:8])
        trees = ExpandEngine(snap, Config(5)).build_trees_ids(roots)
        for r, g in zip(roots.tolist(), trees):
            _cmp_records(oracle.expand(r[0], r[1], r[2], 0, 5), g, (what, r))
        _same_rows(snap, rows, nodes, what)
        _same_export(snap, rows, what)
        return out, trees, snap.rows(nodes)

    def same(x, y):
        assert (x[0] == y[0]).all() and np.array_equal(x[2][0], y[2][0]) and np.array_equal(x[2][1], y[2][1])
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(x[1], y[1]))

    base = Snapshot(rows0, it, keys=keys0)
    before = ask(base, rows0, "base before")
    d1, d2 = delta(rows0, 0, 100), delta(rows0, 100, 200)
    a = base.apply(d1[0], d1[2], d1[1])
    b = base.apply(d2[0], d2[2], d2[1])
    rows_a, keys_a = apply_ref(rows0, keys0, d1[0], d1[1], d1[2])
    rows_b, keys_b = apply_ref(rows0, keys0, d2[0], d2[1], d2[2])
    d3 = delta(rows_a, 200, 300)
    c = a.apply(d3[0], d3[2], d3[1])
    rows_c, keys_c = apply_ref(rows_a, keys_a, d3[0], d3[1], d3[2])
    ask(a, rows_a, "a")
    ask(b, rows_b, "b")
    in_c = ask(c, rows_c, "c")
    assert (in_c[0] != before[0]).any()
    same(ask(base, rows0, "base after the applies"), before)
    a.close()
    same(ask(base, rows0, "base after a is closed"), before)
    same(ask(c, rows_c, "c after a is closed"), in_c)
    for s in (b, c, base):
        s.close()


# ---------------------------------------------------------------- programs and graphs of 4 and 5
def _formula_namespaces():
    """The program of test_gpu_check.test_formula_rewrites_vs_oracle: unions (u1, u2), formulas that split
    (f1, f2, f3 = not u1, f7), formulas that stay with the interpreter (f4: a tuple-to-subject-set leaf, f5: a
    non-union rewrite leaf, f6: an undeclared leaf) and a union that reaches an undeclared relation (u3)."""
    C, TT, N, O = ComputedSubjectSet, TupleToSubjectSet, InvertResult, SubjectSetRewrite
    rels = [Relation("a"), Relation("b"), Relation("blocked"), Relation("parent"),
            Relation("u1", rewrite=O([C("a"), TT("parent", "u1")])),
            Relation("u2", rewrite=O([C("b"), C("u1")])),
            Relation("f1", rewrite=O([C("u1"), N(C("blocked"))], "and")),
            Relation("f2", rewrite=O([O([C("u2"), N(C("a"))], "and"), C("blocked")])),
            Relation("f3", rewrite=O([N(C("u1"))])),
            Relation("f4", rewrite=O([C("u1"), TT("parent", "f1")], "and")),
            Relation("f5", rewrite=O([C("a"), C("f1")], "and")),
            Relation("f6", rewrite=O([C("u2"), C("und")], "and")),
            Relation("f7", rewrite=O([N(O([C("a"), C("b")], "and")), N(C("u2"))], "and")),
            Relation("u3", rewrite=O([C("a"), TT("parent", "zz")]))]
    return [Namespace("d", rels)]


def _formula_graph(rng, n_obj, n_users, n_rows):
    tuples = []
    for _ in range(n_rows):
        x = f"d:o{rng.integers(n_obj)}"
        k = rng.integers(10)
        if k < 3 or k == 9:
            tuples.append(f"{x}#parent@(d:o{rng.integers(n_obj)}#...)")
        elif k < 8:
            r = ["a", "b", "blocked", "a", "b"][k - 3]
            subj = f"u{rng.integers(n_users)}" if rng.random() < 0.7 else f"(d:o{rng.integers(n_obj)}#u2)"
            tuples.append(f"{x}#{r}@{subj}")
        elif rng.random() < 0.85:
            tuples.append(f"{x}#{rng.choice(['f1', 'f3', 'f7'])}@u{rng.integers(n_users)}")  # own rows: not split
        else:  # an undeclared relation, as an object's and inside a subject set
            tuples.append(f"{x}#undeclared@u{rng.integers(n_users)}" if rng.random() < 0.5
                          else f"{x}#a@(d:o{rng.integers(n_obj)}#undeclared)")
    return [T(t) for t in tuples]


def _undeclared_graph(rng, nss, rels, n_obj, n_users, n_rows):
    """The graph of test_gpu_check.test_random_rewrites_vs_oracle: a few undeclared relations."""
    tuples = []
    for _ in range(n_rows):
        ns, obj = rng.choice(nss), f"o{rng.integers(n_obj)}"
        rel = rng.choice(rels) if rng.random() < 0.97 else "undeclared"
        if rng.random() < 0.5:
            srel = rng.choice(rels + ["..."]) if rng.random() < 0.98 else "undeclared"
            s = f"({rng.choice(nss)}:o{rng.integers(n_obj)}#{srel})"
        else:
            s = f"u{rng.integers(n_users)}"
        tuples.append(T(f"{ns}:{obj}#{rel}@{s}"))
    return tuples


def _live(m):
    return [t for _, t in m._rows]


def _keys(m):
    return np.fromiter((m._key(sid.int) for sid, _ in m._rows), np.uint64, len(m._rows))


# ---------------------------------------------------------------- 4. lookups after a refresh
def _drop_objects(m, ns, objs):
    """Every tuple of the objects goes: the rows of their nodes and the rows that name them in a subject set."""
    for o in objs:
        m.delete_all_relation_tuples(RelationQuery(namespace=ns, object=o))
    named = {t for t in _live(m)
             if t.subject_set is not None and t.subject_set.namespace == ns and t.subject_set.object in objs}
    if named:
        m.delete_relation_tuples(*named)


@pytest.mark.parametrize("program", ["none", "unions", "random", "formula"])
def test_lookups_after_refresh(program):
    """Both lookups after every transaction of a persister: equal to the oracle's check over the domain of the
    LIVE rows (objects of the namespace that occur in a tuple / subject ids of a tuple) and to a full build
    from the same rows and keys.  One transaction removes every tuple of several objects, one every tuple of
    several subject ids: they leave the domains, so a `not` relation must not list them and an undeclared
    relation must not count them -- the refreshed snapshot keeps their (empty) nodes."""
    rng = np.random.default_rng({"none": 11, "unions": 12, "random": 13, "formula": 14}[program])
    n_obj, n_users = 40, 30
    if program == "formula":
        it, namespaces, nss = Interner(), _formula_namespaces(), ["d"]
        prog = compile_program(namespaces, it, lower_ttu=False)
        tuples = _formula_graph(rng, n_obj, n_users, 600)
        qrels = ["a", "u1", "u2", "u3", "f1", "f3", "f4", "f6", "f7", "nope"]
        qs = [T(f"d:any#{r}@u{k}") for r in qrels for k in (0, 7, 19, n_users + 1)] + \
             [T(f"d:any#{r}@(d:o{o}#u2)") for r in ("u1", "f3", "f2") for o in (3, 11)]
        roots = [("d", f"o{o}", r) for r in qrels for o in (1, 5, 17, n_obj + 1)]
    else:
        it, tuples, nss, rels = random_graph(rng, n_obj=n_obj, n_rows=600, n_users=n_users)
        namespaces = [] if program == "none" else random_program(rng, nss, rels, unions_only=program == "unions")
        prog = compile_program(namespaces, it, lower_ttu=False) if namespaces else None
        qrels = rels + (["..."] if program == "none" else ["undeclared"])
        qs = random_queries(rng, nss, qrels, 80, n_obj=n_obj, n_users=n_users, p_setq=0.3)
        roots = ls.roots_of(random_queries(rng, nss, qrels, 80, n_obj=n_obj, n_users=n_users))
    oreq = lo.requests_array(it, qs, rng.integers(-1, 8, len(qs)))
    sreq = ls.requests_array(it, roots, rng.integers(-1, 8, len(roots)))
    m = SnapshotPersister(namespaces=namespaces, interner=it, max_read_depth=5, seed=3)
    e = m.permission_engine()
    base, rest = tuples[:450], tuples[450:]
    m.write_relation_tuples(*base)
    ns0 = nss[0]
    left_objs = left_ids = not_members = candidates = 0

    def compare_all(step):
        nonlocal not_members, candidates
        rows = shard_rows(m)
        oracle = Oracle(rows, it.wildcard_rel, prog)
        full = Engine(Snapshot(rows, it, m.program, keys=_keys(m)), m.config)
        oref = lo.reference(oracle, lo.domains(rows), oreq, 5)
        sref = ls.reference(oracle, ls.subject_domain(rows), sreq, 5)
        for who, eng in (("refreshed", e), ("full build", full)):
            try:
                lo.compare(eng, oreq, oref)
                if who == "refreshed":
                    candidates += eng.last_stats["candidates"]
                assert program != "none" or eng.last_stats["candidates"] == 0  # the walk alone answers
                ls.compare(eng, sreq, sref)
                assert program != "none" or eng.last_stats["candidates"] == 0
            except AssertionError as x:
                raise AssertionError(f"step {step}, {who}: {x}") from x
        if program == "formula":
            f3 = it.rel_id("f3")
            not_members += sum(len(r[0]) for r, q in zip(oref, oreq.tolist()) if q[1] == f3)
        full.snapshot.close()
        return rows

    rows = compare_all(0)  # the first snapshot is a full build
    # 1: ordinary inserts (new objects, a subject set on one) and deletes
    ins = rest[:80] + [T(f"{ns0}:born{k}#{'a' if program == 'formula' else 'r0'}@u{k}") for k in range(3)]
    live = _live(m)
    m.transact_relation_tuples(ins, [live[i] for i in rng.choice(len(live), 15, replace=False)])
    rows = compare_all(1)
    # 2: six objects lose every tuple, as objects and inside subject sets
    dom = lo.domains(rows)[it.ns_id(ns0)]
    victims = [it.obj_name(int(o)) for o in rng.choice(dom, 6, replace=False)]
    _drop_objects(m, ns0, set(victims))
    rows = compare_all(2)
    left_objs = len(np.setdiff1d(dom, lo.domains(rows).get(it.ns_id(ns0), np.zeros(0, np.uint32))))
    assert left_objs >= 5, left_objs
    # 3: six subject ids lose every tuple
    sdom = ls.subject_domain(rows)
    gone = {it.obj_name(int(u)) for u in rng.choice(sdom, 6, replace=False)}
    for u in sorted(gone):
        m.delete_all_relation_tuples(RelationQuery(subject_id=u))
    m.write_relation_tuples(*[t for t in rest[80:120] if t.subject_id not in gone])
    rows = compare_all(3)
    left_ids = len(np.setdiff1d(sdom, ls.subject_domain(rows)))
    assert left_ids >= 5, left_ids
    # 4: one of the objects comes back, named only by a subject set
    live = _live(m)
    r_own, r_set = ("a", "u2") if program == "formula" else ("r0", "r1")
    back = T(f"{ns0}:born0#{r_own}@({ns0}:{victims[0]}#{r_set})")
    m.transact_relation_tuples([back] + rest[120:], [live[i] for i in rng.choice(len(live), 10, replace=False)])
    rows = compare_all(4)
    assert it.obj_id(victims[0]) in lo.domains(rows)[it.ns_id(ns0)]
    # 5: a whole namespace goes (the formula graph has one: five more objects instead)
    if len(nss) > 1:
        dom = lo.domains(rows)[it.ns_id(nss[2])]
        _drop_objects(m, nss[2], {it.obj_name(int(o)) for o in dom})
        rows = compare_all(5)
        assert it.ns_id(nss[2]) not in lo.domains(rows) and len(dom) >= 5
    else:
        dom = lo.domains(rows)[it.ns_id(ns0)]
        _drop_objects(m, ns0, {it.obj_name(int(o)) for o in rng.choice(dom, 5, replace=False)})
        rows = compare_all(5)
        assert len(np.setdiff1d(dom, lo.domains(rows)[it.ns_id(ns0)])) >= 5
    assert m.rebuilds == 1 and m.applies == 5
    if program == "formula":
        assert not_members > 0  # the `not` relation lists objects that are still in the domain
    if program != "none":
        assert candidates > 0  # confirm-mode requests ran on the refreshed snapshots


def test_lookup_domain_after_last_tuple_deleted():
    """The smallest case of the above, by hand: deletes take the last tuple of o1 (an object), of o5 and o6 (a
    row and the subject set it names) and of o7 and o8 (the same through a "..." set).  Their nodes stay in the
    refreshed snapshot, but the objects no longer occur: `n = not r` lists only o0, o2, o3, o4 for a stranger
    and an undeclared relation reports those four.  A "..." subject set then brings o6 back."""
    it = Interner()
    not_r = SubjectSetRewrite([InvertResult(ComputedSubjectSet("r"))])
    namespaces = [Namespace("a", [Relation("r"), Relation("n", rewrite=not_r)])]
    prog = compile_program(namespaces, it, lower_ttu=False)
    tuples = [T(f"a:o{i}#r@u") for i in range(5)] + [T("a:o5#r@(a:o6#r)"), T("a:o7#r@(a:o8#...)")]
    rows = it.tuples_array(tuples)
    reqs = lo.requests_array(it, [T("a:any#n@stranger"), T("a:any#nope@u"), T("a:any#n@u"), T("a:any#r@u")], [0, 0, 0, 0])
    snap = Snapshot(rows, it, prog)
    names = lambda ids: sorted(it.obj_name(i) for i in ids)  # noqa: E731

    def agree(snap, rows):
        oracle = Oracle(rows, it.wildcard_rel, prog)
        ref = lo.reference(oracle, lo.domains(rows), reqs, 5)
        lo.compare(Engine(snap, Config(5)), reqs, ref)
        full = Snapshot(rows, it, prog)
        lo.compare(Engine(full, Config(5)), reqs, ref)
        full.close()
        return ref

    ref = agree(snap, rows)
    assert len(ref[0][0]) == 9 and ref[1][1:] == (9, 1)
    dels = it.tuples_array([tuples[1], tuples[5], tuples[6]])
    a = snap.apply(NO_ROWS, dels)
    rows, _ = apply_ref(rows, None, NO_ROWS, None, dels)
    ref = agree(a, rows)
    assert names(ref[0][0]) == ["o0", "o2", "o3", "o4"] and ref[1] == ([], 4, 1) and ref[2][0] == []
    ins = it.tuples_array([T("a:o0#r@(a:o6#...)")])
    b = a.apply(ins, NO_ROWS)
    rows, _ = apply_ref(rows, None, ins, None, NO_ROWS)
    ref = agree(b, rows)
    assert names(ref[0][0]) == ["o0", "o2", "o3", "o4", "o6"] and ref[1] == ([], 5, 1)
    for s in (snap, a, b):
        s.close()


# ---------------------------------------------------------------- 5. every rewrite kind after a refresh
def _own_nodes(tuples, rewritten):
    """(namespace, object, relation) of the rows of relations with a rewrite: an object whose own node holds
    rows is not split by kg_formula.hip."""
    return {(t.namespace, t.object, t.relation) for t in tuples if (t.namespace, t.relation) in rewritten}


@pytest.mark.parametrize("mat", [1, 0])
@pytest.mark.parametrize("program", ["random", "formula"])
def test_rewrites_after_refresh(program, mat, monkeypatch):
    """The loop of test_gpu_persister.test_incremental_refresh_matches_full_build with every rewrite kind:
    the interpreter and the formula split run on refreshed snapshots, on graphs with undeclared relations.
    Every delta gives objects their first own row of a rewritten relation and takes the last one from others
    (what decides whether a formula query is split).  Answers and error codes equal the oracle and a full
    build; check trees equal the full build's."""
    monkeypatch.setenv("KG_MATERIALIZE", str(mat))
    rng = np.random.default_rng(600 + (1 if program == "formula" else 0))
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
    assert rewritten
    m = SnapshotPersister(namespaces=namespaces, interner=it, max_read_depth=5, seed=mat)
    base, rest = tuples[:450], tuples[450:]
    m.write_relation_tuples(*base)
    e = m.permission_engine()
    m.snapshot()  # the full build: every transaction below is a refresh
    q6 = np.asarray([it.tuple_ids(t) for t in qs], np.uint32)
    depths = rng.integers(-1, 7, len(qs))
    gained, lost, general, errors = set(), set(), 0, 0
    for step in range(6):
        live = _live(m)
        own = _own_nodes(live, set(rewritten))
        ins = [rest.pop() for _ in range(min(len(rest), 50))]
        free = [(ns, f"o{o}", rel) for ns, rel in rewritten for o in range(n_obj) if (ns, f"o{o}", rel) not in own]
        for k in rng.choice(len(free), 3, replace=False):  # a first own row
            ins.append(RelationTuple(*free[k], subject_id=f"u{rng.integers(n_users)}"))
        dels = [live[i] for i in rng.choice(len(live), 12, replace=False)]
        for node in sorted(own)[::max(1, len(own) // 3)][:3]:  # the last own row (every row of the node)
            dels += [t for t in live if (t.namespace, t.object, t.relation) == node]
        m.transact_relation_tuples(ins, dels)
        after = _own_nodes(_live(m), set(rewritten))
        gained |= after - own
        lost |= own - after
        out, err = e.batch_check_ids(queries_array(q6, depths), with_stats=True)
        general += e.last_stats["n_general"]
        rows = shard_rows(m)
        full = Snapshot(rows, it, m.program, keys=_keys(m))
        ef = Engine(full, m.config)
        fout, ferr = ef.batch_check_ids(queries_array(q6, depths), with_stats=True)
        assert (out == fout).all() and (err == ferr).all(), (step, np.nonzero(out != fout)[0][:8])
        # the same queries are split into leaf checks (own rows and purity decide): the interpreter gets the rest
        assert e.last_stats["n_general"] == ef.last_stats["n_general"], (step, e.last_stats["n_general"],
                                                                         ef.last_stats["n_general"])
        exp, oerr, _ = Oracle(rows, it.wildcard_rel, prog).check_batch(q6, depths, 5, POLICY_CANONICAL)
        bad = np.nonzero((out != exp) | (err.astype(np.int64) != oerr))[0]
        assert bad.size == 0, (step, [(str(qs[i]), int(depths[i]), int(out[i]), int(err[i]), int(exp[i]), int(oerr[i]))
                                      for i in bad[:8]])
        errors += int((exp == 2).sum())
        if step == 5:
            ea, eb = Engine(m.snapshot(), m.config), Engine(full, m.config)
            trees = 0
            for t, d in zip(qs[:100], depths[:100].tolist()):
                ra, rb = ea.check_relation_tuple(t, d), eb.check_relation_tuple(t, d)
                assert ra.membership == rb.membership and (ra.err and ra.err.code) == (rb.err and rb.err.code), str(t)
                assert ra.tree == rb.tree, str(t)
                trees += ra.tree is not None
            assert trees > 0
        full.close()
    assert m.applies == 6
    assert gained and lost, (len(gained), len(lost))  # both flips of the formula-split condition occurred
    assert general > 0 and errors > 0, (general, errors)


# ---------------------------------------------------------------- 6. the tail tiers after a refresh
def _dense_graph(rng, n_obj=120, n_users=60):
    """The graph of test_gpu_check.test_grid_dense_vs_oracle: dense set edges with cycles, and 40 docs nothing
    points at that hold the w* subjects."""
    tuples = []
    for i in range(n_obj):
        for _ in range(int(rng.integers(1, 14))):
            tuples.append(f"g:o{i}#m@(g:o{int(rng.integers(n_obj))}#m)")
        if rng.random() < 0.3:
            tuples.append(f"g:o{i}#m@u{int(rng.integers(n_users))}")
    for i in range(40):
        for _ in range(int(rng.integers(1, 8))):
            tuples.append(f"d:x{i}#v@(g:o{int(rng.integers(n_obj))}#m)")
        tuples.append(f"d:x{i}#v@w{int(rng.integers(20))}")
    return [T(t) for t in tuples]


@pytest.mark.parametrize("back_edges,ms", [(1, 0), (0, 0), (1, 1), (1, 8), (0, 8)])
def test_tail_tiers_after_refresh(back_edges, ms):
    """Three refreshes of the dense graph (the w* subjects move to other docs, cycle edges come and go); on
    each refreshed snapshot a tiny stream-tier budget sends the queries on to the backward tier (back_edges 0:
    its default budget answers them there) and, with a one-edge backward budget, to the grid tier: the
    per-query rounds (ms 0) or MS-BFS with ms words per mask.  These read adjx, the reverse index, the holder
    hash and bitmap and the node map that every refresh rebuilds.  Depths 2..9 against the oracle."""
    rng = np.random.default_rng(950)
    n_obj, n_users = 120, 60
    it = Interner()
    tuples = _dense_graph(rng, n_obj, n_users)
    rows = it.tuples_array(tuples)
    qs = []
    for _ in range(1500):
        root = f"d:x{int(rng.integers(40))}#v" if rng.random() < 0.6 else f"g:o{int(rng.integers(n_obj))}#m"
        r = rng.random()
        subj = f"u{int(rng.integers(n_users))}" if r < 0.7 else (f"w{int(rng.integers(20))}" if r < 0.9
                                                                  else f"(g:o{int(rng.integers(n_obj))}#m)")
        qs.append(T(f"{root}@{subj}"))
    q6 = np.asarray([it.tuple_ids(t) for t in qs], np.uint32)
    depths = rng.integers(0, 10, len(qs))
    snap = Snapshot(rows, it)  # no order keys: inserted rows go to the end of their node's row
    for refresh in range(3):
        held = rows[(rows[:, 3] == S) & (rows[:, 0] == it.ns_id("d"))]
        edges = rows[(rows[:, 3] != S) & (rows[:, 0] == it.ns_id("g"))]
        dels = np.concatenate([held[rng.choice(len(held), 12, replace=False)],
                               edges[rng.choice(len(edges), 60, replace=False)]])
        ins = [T(f"d:x{int(rng.integers(40))}#v@w{int(rng.integers(20))}") for _ in range(12)]
        ins += [T(f"g:o{int(rng.integers(n_obj))}#m@(g:o{int(rng.integers(n_obj))}#m)") for _ in range(60)]
        ins += [T(f"g:o{i}#m@(g:o{(i + 1) % 30}#m)") for i in range(30)] if refresh == 1 else []  # a 30-cycle
        ins = it.tuples_array(ins)
        new = snap.apply(ins, dels)
        rows, _ = apply_ref(rows, None, ins, None, dels)
        snap.close()
        snap = new
        snap.tune("stream_ecap", 3)
        snap.tune("back_edges", back_edges)
        snap.tune("grid_ms", 1 if ms else 0)
        if ms:
            snap.tune("grid_ms_words", ms)
        oracle = Oracle(rows, it.wildcard_rel)
        n_grid = n_back = 0
        members = []
        for gmax in range(2, 10):
            e = Engine(snap, Config(gmax))
            out, err = e.batch_check_ids(queries_array(q6, depths), with_stats=True)
            exp, _, _ = oracle.check_batch(q6, depths, gmax, POLICY_CANONICAL)
            bad = np.nonzero(out != exp)[0]
            assert bad.size == 0 and (err == 0).all(), (refresh, gmax, [(str(qs[i]), int(depths[i]), int(out[i]),
                                                                          int(exp[i])) for i in bad[:8]])
            n_grid += e.last_stats["n_grid"]
            n_back += e.last_stats["n_back"]
            members.append(exp == 1)
        print(f"refresh {refresh}: n_grid {n_grid}, n_back {n_back}, members {np.concatenate(members).mean():.3f}")
        if back_edges == 0:
            assert n_back > 0, (refresh, n_back)
        else:
            assert n_grid > 0, (refresh, n_grid)
        assert 0.01 < np.concatenate(members).mean() < 0.99  # both answers occur, by the oracle
    snap.close()


# ---------------------------------------------------------------- replicas
def test_refresh_per_replica():
    """SnapshotPersister(devices=[0, 0]): kg_snapshot_apply refreshes replica by replica, and a host batch
    large enough to be split over the two reads both."""
    rng = np.random.default_rng(77)
    it, tuples, nss, rels = random_graph(rng, n_obj=60, n_rows=700)
    m = SnapshotPersister(interner=it, max_read_depth=5, devices=[0, 0])
    m.write_relation_tuples(*tuples[:500])
    e = m.permission_engine()
    qs = random_queries(rng, nss, rels, 1000, n_obj=60)
    q6 = np.tile(np.asarray([it.tuple_ids(t) for t in qs], np.uint32), (40, 1))  # 40 000 queries
    depths = np.tile(rng.integers(0, 7, len(qs)), 40)
    changed = []
    for step in range(3):
        if step:
            live = _live(m)
            m.transact_relation_tuples(tuples[400 + 100 * step:500 + 100 * step],
                                       [live[i] for i in rng.choice(len(live), 60, replace=False)])
        out, err = e.batch_check_ids(queries_array(q6, depths))
        assert m.snapshot().replicas() == [0, 0]
        exp, oerr, _ = Oracle(shard_rows(m), it.wildcard_rel).check_batch(q6, depths, 5, POLICY_CANONICAL)
        assert (out == exp).all() and (err == 0).all() and (oerr == 0).all(), (step, np.nonzero(out != exp)[0][:8])
        changed.append(exp)
    assert m.rebuilds == 1 and m.applies == 2
    assert (changed[0] != changed[1]).any() and (changed[1] != changed[2]).any()
