"""The CPU oracle on chosen ids (tests/sparse_ids.py): its check answers and error codes, expand records
and the lookup references are the dense case's, mapped through the id maps -- the reference the GPU tests of
test_gpu_id_limits.py lean on is pinned here first.  Also the helper's own promises: strictly increasing
maps, and the ids each layout puts where.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sparse_ids as sp
import test_gpu_lookup as lo
import test_gpu_lookup_subject_sets as lss
import test_gpu_lookup_subjects as ls
from keto_amd.ketoapi import RelationTuple
from keto_amd.namespace import compile_program
from oracle.oracle import POLICY_CANONICAL, Oracle
from sparse_ids import SUBJECT_ID, TOP
from test_gpu_check import random_graph, random_program, random_queries

T = RelationTuple.from_string
N_NS, N_REL = 6, 6  # enough ids for every edge value of a pool (0, 255, 256, 4094, 4095, 65534)


class Case:
    """One dense case: rows, check queries, lookup requests of the three kinds, expand roots, the program as
    the library (TTU leaves lowered) and as the oracle compiles it.  Every id is interned before the maps are
    built.  arrange(): which ids the increasing object map puts at 0 and at 0x7FFFFFFE -- "top-subject": 0 = the
    object with the most set rows, top = the most held subject id; "top-object": swapped."""

    def __init__(self, seed, program=False, wild=True, n_obj=80, n_rows=600, n_users=40, n_q=2500, n_req=64):
        rng = np.random.default_rng(4100 + seed)
        it, tuples, nss, rels = random_graph(rng, n_obj=n_obj, n_rows=n_rows, n_ns=N_NS, n_rel=N_REL,
                                             p_wild=0.1 if wild else 0.0, n_users=n_users)
        self.namespaces = random_program(rng, nss, rels) if program else []
        qrels = list(rels)
        if program:  # undeclared relations, as rows, as subject sets and in queries: error codes cross the tables
            for _ in range(n_rows // 25):
                ns, o = rng.choice(nss), f"o{rng.integers(n_obj)}"
                s = f"({rng.choice(nss)}:o{rng.integers(n_obj)}#undeclared)" if rng.random() < 0.5 else f"u{rng.integers(n_users)}"
                tuples.append(T(f"{ns}:{o}#{'undeclared' if rng.random() < 0.5 else rng.choice(rels)}@{s}"))
            qrels.append("undeclared")
        self.prog_oracle = compile_program(self.namespaces, it, lower_ttu=False) if program else None
        self.n_rel_named = it.n_relations  # the ids from here on are the lowering's hidden relations: no query names one
        self.prog = compile_program(self.namespaces, it) if program else None
        qs = random_queries(rng, nss, qrels + (["..."] if wild else []), n_q, n_obj=n_obj, n_users=n_users)
        self.t6 = it.tuples_array(tuples)
        q6 = np.asarray([it.tuple_ids(t) for t in qs], np.uint32)
        # six namespaces x six relations x 80 objects thin the graph: random_queries alone finds under 1 % members.
        # Every second query is therefore a row's object with, three times in five, another row's subject.
        rows, other = self.t6[rng.integers(len(self.t6), size=n_q)], self.t6[rng.integers(len(self.t6), size=n_q)]
        swap = rng.random(n_q) < 0.6
        rows[swap, 3:] = other[swap, 3:]
        q6[1::2] = rows[1::2]
        self.depths = rng.integers(-1, 9, n_q)
        self.q7 = np.concatenate([q6, self.depths.astype(np.int32).view(np.uint32)[:, None]], 1)
        r, d = q6[:n_req], self.q7[:n_req, 6]
        self.lo_reqs = np.stack([r[:, 0], r[:, 2], r[:, 3], r[:, 4], r[:, 5], d], 1)
        self.ls_reqs = np.stack([r[:, 0], r[:, 1], r[:, 2], d], 1)
        filt = lss.set_filters(self.t6)
        f = np.asarray([filt[i % len(filt)] if i % 4 else (SUBJECT_ID, 0) for i in range(n_req)], np.uint32)
        self.lss_reqs = np.stack([r[:, 0], r[:, 1], r[:, 2], f[:, 0], f[:, 1], d], 1)
        # expand roots: the queries' objects and, every eighth, their subject ids
        self.roots = np.stack([np.where(np.arange(300) % 8 == 7, SUBJECT_ID, q6[:300, 0]),
                               np.where(np.arange(300) % 8 == 7, q6[:300, 4], q6[:300, 1]),
                               np.where(np.arange(300) % 8 == 7, 0, q6[:300, 2]), self.q7[:300, 6]], 1).astype(np.uint32)
        self.n_ns, self.n_rel, self.n_obj = it.n_namespaces, it.n_relations, len(it._obj_names)
        sets, ids = self.t6[self.t6[:, 3] != SUBJECT_ID], self.t6[self.t6[:, 3] == SUBJECT_ID]
        self.set_obj = int(np.bincount(sets[:, 1]).argmax())   # the object with the most set rows
        self.held = int(np.bincount(ids[:, 4]).argmax())       # the subject id the most rows hold
        self.arrange("top-subject")
        self.wild = wild
        # requests that list the two extremes whatever the seed: the set object through a direct holder of
        # one of its rows, the held subject through an object that holds it
        row = ids[ids[:, 1] == self.set_obj][0] if (ids[:, 1] == self.set_obj).any() else None
        hrow = ids[ids[:, 4] == self.held][0]
        if row is not None:
            self.lo_reqs = np.concatenate([self.lo_reqs, [[row[0], row[2], SUBJECT_ID, row[4], 0, 0]]]).astype(np.uint32)
        self.ls_reqs = np.concatenate([self.ls_reqs, [[hrow[0], hrow[1], hrow[2], 0]]]).astype(np.uint32)
        self.lss_reqs = np.concatenate([self.lss_reqs, [[hrow[0], hrow[1], hrow[2], SUBJECT_ID, 0, 0]]]).astype(np.uint32)

    def arrange(self, how):
        first, last = (self.set_obj, self.held) if how != "top-object" else (self.held, self.set_obj)
        self.perm = sp.order_objects(self.n_obj, first, last)

    def maps(self, layout, wildcard="zero", seed=0):
        assert wildcard != "none" or not self.wild
        return sp.IdMaps(layout, self.n_ns, self.n_rel, self.n_obj, seed, wildcard, self.perm)


def oracle_of(case, m):
    return Oracle(m.tuples(case.t6), m.wildcard, m.program(case.prog_oracle))


def answers(case, m, gmax=5):
    """Everything the GPU tests take from the oracle, on the ids of `m`."""
    o = oracle_of(case, m)
    t6 = m.tuples(case.t6)
    q = m.tuples(case.q7)
    out, err, _ = o.check_batch(q[:, :6], case.depths, gmax, POLICY_CANONICAL, nthreads=4)
    roots = m.roots(case.roots)
    trees = [o.expand(int(r[0]), int(r[1]), int(r[2]), int(np.uint32(r[3]).view(np.int32)), gmax) for r in roots]
    return dict(out=out, err=np.asarray(err), trees=trees,
                lo=lo.reference(o, lo.domains(t6), m.lookup_objects(case.lo_reqs), gmax),
                ls=ls.reference(o, ls.subject_domain(t6), m.lookup_subjects(case.ls_reqs), gmax),
                lss=lss.brief(lss.full_reference(o, t6, m.lookup_subject_sets(case.lss_reqs), gmax)))


def lifted(dense, up):
    """The dense answers on the chosen ids: ids through the increasing maps, everything else as it is."""
    ids = lambda ref: [(up.obj[np.asarray(a, np.int64)].tolist(), n, c) for a, n, c in ref]
    return dict(out=dense["out"], err=dense["err"], trees=[up.records(t) for t in dense["trees"]],
                lo=ids(dense["lo"]), ls=ids(dense["ls"]), lss=ids(dense["lss"]))


def same(a, b):
    assert (a["out"] == b["out"]).all() and (a["err"] == b["err"]).all()
    for k in ("lo", "ls", "lss"):
        assert a[k] == b[k], k
    for x, y in zip(a["trees"], b["trees"]):
        assert (x is None) == (y is None) and (x is None or np.array_equal(np.asarray(x, np.int64), np.asarray(y, np.int64)))


FREE = [("top-subject", w) for w in sp.WILDCARDS] + [("top-object", w) for w in sp.WILDCARDS] + [("packed", "top")]


@pytest.mark.parametrize("seed", range(4))
def test_oracle_invariant_rewrite_free(seed):
    for wild in (True, False):
        case = Case(seed, wild=wild, n_q=600)
        for layout, w in FREE:
            if (w == "none") == wild:
                continue
            case.arrange(layout)
            dense = answers(case, case.maps("dense", w))
            m = case.maps(layout, w, seed)
            same(lifted(dense, m.lift()), answers(case, m))
            assert 0.05 < (dense["out"] == 1).mean() < 0.95
            assert any(a for a, _, _ in dense["lo"]) and any(a for a, _, _ in dense["ls"]) and any(a for a, _, _ in dense["lss"])
            assert sum(t is not None for t in dense["trees"]) > 30


@pytest.mark.parametrize("seed", range(4))
def test_oracle_invariant_programs(seed):
    case = Case(seed, program=True, n_q=600)
    dense = answers(case, case.maps("dense"))
    assert (dense["out"] == 2).any() and 0.05 < (dense["out"] == 1).mean() < 0.95
    for layout in sp.PROGRAM_LAYOUTS:
        for w in ("zero", "top"):
            m = case.maps(layout, w, seed)
            same(lifted(answers(case, case.maps("dense", w)), m.lift()), answers(case, m))


@pytest.mark.parametrize("layout", [k for k in sp.LAYOUTS if k != "dense"])
@pytest.mark.parametrize("wildcard", sp.WILDCARDS)
def test_maps_increasing_and_edges(layout, wildcard):
    case = Case(1, program=layout in sp.PROGRAM_LAYOUTS, wild=wildcard != "none", n_q=300)
    m = case.maps(layout, wildcard, 3)
    for a in (m.ns, m.rel_pool, m.obj_pool):
        assert (np.diff(a.astype(np.int64)) > 0).all()
    ordinary = m.rel[1:].astype(np.int64)  # every relation but "..."
    assert (np.diff(ordinary) > 0).all() and set(m.obj_pool.tolist()) >= set(sp.OBJ_FIXED)
    pn, pr = sp.LAYOUTS[layout]
    assert set(m.ns.tolist()) >= set(pn["fixed"]) and set(m.rel_pool.tolist()) >= set(pr["fixed"])
    assert m.ns.max() == pn["top"] and m.rel_pool.max() == pr["top"]
    if layout in sp.PROGRAM_LAYOUTS:
        assert (int(m.ns.max()) + 1) * (int(m.rel.max()) + 1) <= 8 << 20
    it = m.interner()
    assert it.wildcard_rel == {"zero": 0, "top": pr["top"], "none": sp.NONE}[wildcard]
    t6 = m.tuples(case.t6)
    if wildcard == "none":  # relation 0 is an ordinary relation that set edges follow
        assert ((t6[:, 5] == 0) & (t6[:, 3] != SUBJECT_ID)).any() and (t6[:, 2] == 0).any()
    else:
        assert ((t6[:, 5] == it.wildcard_rel) & (t6[:, 3] != SUBJECT_ID)).any()
    sets, ids = t6[t6[:, 3] != SUBJECT_ID], t6[t6[:, 3] == SUBJECT_ID]
    assert (sets[:, 1] == 0).any() and (ids[:, 4] == TOP).any()  # the arrangement "top-subject"
    case.arrange("top-object")
    t6 = case.maps(layout, wildcard, 3).tuples(case.t6)
    assert (t6[(t6[:, 3] != SUBJECT_ID), 1] == TOP).any() and (t6[t6[:, 3] == SUBJECT_ID, 4] == 0).any()
    # the program's tables are re-indexed by the chosen ids
    if case.prog is not None:
        p = m.program(case.prog)
        assert len(p.ns_has_rel) == int(m.ns.max()) + 1 and p.ns_has_rel.sum() == case.prog.ns_has_rel.sum()
        assert (p.ns_has_rel[m.ns[:len(case.prog.ns_has_rel)]] == case.prog.ns_has_rel).all()
        assert (p.rel_rel == m.rel[case.prog.rel_rel]).all() and (p.rw[:, 3:] == case.prog.rw[:, 3:]).all()


def test_header_packer_at_the_field_limits(tmp_path):
    """kg_pack_query of include/ketogpu.h, compiled: every field packs at 0, 255, 256 and 4094 exactly as
    keto_amd._lib.pack_queries does, depths 65535 and 65536 pack as 65535, and 4095 is refused in every field --
    in the subject namespace too, where it would read back as the subject-id marker."""
    from keto_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "pack.c"
    src.write_text('#include "ketogpu.h"\nint pack_one(const kg_query* q, kg_query_packed* p) { return kg_pack_query(q, p); }\n')
    so = tmp_path / "pack.so"
    subprocess.run(["gcc", "-O1", "-shared", "-fPIC", "-I", os.path.join(root, "include"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))

    def header(q):
        out = np.zeros(4, np.uint32)
        return lib.pack_one(np.ascontiguousarray(q).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)), out

    base = np.asarray([7, 0x7FFFFFFE, 9, 11, 0, 13, 5], np.uint32)
    for col in (0, 2, 3, 5):
        for v in (0, 255, 256, 4094):
            for depth in (0, 1, 65535, 65536):
                q = base.copy()
                q[col], q[6] = v, depth
                rc, got = header(q)
                assert rc == 0 and (got == _lib.pack_queries(q[None])[0]).all(), (col, v, depth)
                assert got[3] >> 16 == min(depth, 65535)
        q = base.copy()
        q[col] = 4095
        assert header(q)[0] == -2, col
        with pytest.raises(ValueError):
            _lib.pack_queries(q[None])
    q = base.copy()
    q[3], q[5] = SUBJECT_ID, 4095  # a subject id: its relation is ignored
    rc, got = header(q)
    assert rc == 0 and (got == _lib.pack_queries(q[None])[0]).all() and (got[2] >> 24) | ((got[3] & 0xF) << 8) == 4095
