"""GPU tests at the id limits of include/ketogpu.h: namespace and relation ids up to 65534, object and subject
ids up to 0x7FFFFFFE, sparse, with the wildcard relation at 0, at the highest relation id and absent
(tests/sparse_ids.py puts the dense cases of the existing generators on such ids).  Every answer is compared
exactly with the CPU oracle on the same id arrays, and with the dense case's answer mapped through the
(strictly increasing) id maps.

  1  checks, rewrite-free: tiers and knobs          5  expand
  2  checks with programs: tables, error codes      6  lookups, unpaged and paged
  3  the packed boundary (three unpackers)          7  listing, rows, export
  4  the table limit                                8  apply: the extremes arrive in a delta
"""
import time

import numpy as np
import pytest

import sparse_ids as sp
import test_gpu_lookup as lo
import test_gpu_lookup_page as lp
import test_gpu_lookup_subject_sets as lss
import test_gpu_lookup_subjects as ls
from keto_amd import _lib
from keto_amd.engine import Config, Engine, ExpandEngine, Snapshot, queries_array
from oracle.oracle import POLICY_CANONICAL, Oracle
from refresh_ref import apply_ref, multiset
from sparse_ids import KNOBS, SUBJECT_ID, TOP, device_packed, tune as _tune
from test_gpu_expand import GW_MODES, _cmp_records
from test_gpu_query import check_call
from test_id_limits_host import Case, oracle_of

pytestmark = pytest.mark.gpu

END = _lib.KG_LOOKUP_END
GMAX = 5
_worlds = {}


@pytest.fixture(scope="module", autouse=True)
def _free_worlds():
    """The module's snapshots (six of them with a 256 MiB holder bitmap) go when its last test has run."""
    yield
    for w in _worlds.values():
        w.snap.close()
    _worlds.clear()


class World:
    """One case on one layout: the rows on the chosen ids, their snapshot and oracle, and the same for the dense
    ids (`dense`, a World of layout "dense" with the same object order)."""

    def __init__(self, case, m, monkeypatch=None, mat=1):
        self.case, self.m = case, m
        self.t6 = m.tuples(case.t6)
        self.q7 = m.tuples(case.q7)
        if monkeypatch is not None:
            monkeypatch.setenv("KG_MATERIALIZE", str(mat))
        t0 = time.perf_counter()
        self.snap = Snapshot(self.t6, m.interner(), m.program(case.prog))
        self.build_s = time.perf_counter() - t0
        self.oracle = oracle_of(case, m)

    def engine(self, gmax=GMAX):
        return Engine(self.snap, Config(gmax))


def world(layout, wildcard="zero", seed=0, program=False, mat=1, monkeypatch=None, arrange=None):
    """Module-scoped: one snapshot per (layout, wildcard, seed, program, materialisation, object order).  arrange:
    which ids are first and last ("top-subject" / "top-object"; default: the layout's, "top-object" with a program)."""
    arrange = arrange or ("top-object" if layout == "top-object" or program else "top-subject")
    key = (layout, wildcard, seed, program, mat, arrange)
    if key not in _worlds:
        case = Case(seed, program=program, wild=wildcard != "none")
        case.arrange(arrange)
        _worlds[key] = World(case, case.maps(layout, wildcard, seed), monkeypatch, mat)
        print(f"snapshot {key}: built in {_worlds[key].build_s * 1e3:.1f} ms")
    return _worlds[key]


def check_vs_oracle(w, q7, gmax=GMAX, with_stats=True):
    e = w.engine(gmax)
    out, err = e.batch_check_ids(q7, with_stats=with_stats)
    exp, oerr, _ = w.oracle.check_batch(q7[:, :6], q7[:, 6].copy().view(np.int32), gmax, POLICY_CANONICAL, nthreads=4)
    bad = np.nonzero((out != exp) | (err.astype(np.int64) != oerr))[0]
    assert bad.size == 0, (bad.size, [(q7[i].tolist(), int(out[i]), int(exp[i]), int(err[i]), int(oerr[i])) for i in bad[:8]])
    return out, err, e.last_stats


# ---------------------------------------------------------------- 1. checks, rewrite-free
def _out_of_space_queries(w):
    """Queries whose object or subject id is past the id space (0x7FFFFFFF, 0xFFFFFFFE), on rows that exist
    otherwise, and subject-set queries naming node triples that do not exist: all NotMember, no error."""
    rows = w.t6[w.t6[:, 3] == SUBJECT_ID][:8]
    extra = []
    for big in (0x7FFFFFFF, 0xFFFFFFFE):
        a, b = rows.copy(), rows.copy()
        a[:, 1], b[:, 4] = big, big
        extra += [a, b]
    sets = w.t6[w.t6[:, 3] != SUBJECT_ID][:8].copy()
    nowhere, far = sets.copy(), sets.copy()
    nowhere[:, 4] = 0x7FFFFFFC             # an object no row names
    far[:, 3], far[:, 5] = 65534, 65533    # a namespace / relation pair no row has
    nodes = {tuple(x) for x in np.concatenate([w.t6[:, :3], w.t6[:, 3:]])[:, [0, 2, 1]].tolist()}
    assert not any(tuple(x) in nodes for x in np.concatenate([nowhere, far])[:, [3, 5, 4]].tolist())
    return queries_array(np.concatenate(extra + [nowhere, far]), 0)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("wildcard", sp.WILDCARDS)
@pytest.mark.parametrize("layout", ["top-subject", "top-object"])
def test_checks_rewrite_free(layout, wildcard, seed):
    w = world(layout, wildcard, seed)
    d = world("dense", wildcard, seed, arrange=layout)
    sets, ids = w.t6[w.t6[:, 3] != SUBJECT_ID], w.t6[w.t6[:, 3] == SUBJECT_ID]
    if layout == "top-subject":  # 0x7FFFFFFE is a held subject id (the holder bitmap spans the id space), 0 a set row's object
        assert (ids[:, 4] == TOP).any() and (sets[:, 1] == 0).any()
    else:
        assert (sets[:, 1] == TOP).any() and (ids[:, 4] == 0).any()
    assert w.t6[:, [0, 3]][w.t6[:, [0, 3]] != SUBJECT_ID].max() == 65534 and max(w.t6[:, 2].max(), sets[:, 5].max()) == 65534
    for v in sp.EDGE:  # every edge value is a row's namespace, and a row's relation -- but for the id that "none" gives "..."
        assert (w.t6[:, 0] == v).any(), v
        assert (w.t6[:, 2] == v).any() or (sets[:, 5] == v).any() or (wildcard == "none" and v == w.m.rel[0]), v
    assert wildcard != "none" or not ((w.t6[:, 2] == w.m.rel[0]).any() or (sets[:, 5] == w.m.rel[0]).any())
    assert w.snap.interner.wildcard_rel == {"zero": 0, "top": 65534, "none": sp.NONE}[wildcard]
    if wildcard == "none":  # relation 0 is an ordinary relation that set edges follow
        assert (sets[:, 5] == 0).any() and (w.t6[:, 2] == 0).any()
    else:
        assert (sets[:, 5] == w.snap.interner.wildcard_rel).any()
    far = _out_of_space_queries(w)
    q7 = np.concatenate([w.q7, far])
    for name, knobs in KNOBS.items():
        _tune(w.snap, knobs)
        out, err, st = check_vs_oracle(w, q7)
        assert not out[len(w.q7):].any() and not err.any(), name
        assert 0.05 < (out[:len(w.q7)] == 1).mean() < 0.95
        if name == "default":
            assert st["n_light"] > 0 and st["n_no_holder"] > 0, st
        else:
            assert st["n_back"] + st["n_heavy"] > 0, (name, st)
        if name == "default":  # the dense case answers the same
            dout, derr = d.engine().batch_check_ids(d.q7)
            assert (dout == out[:len(w.q7)]).all() and not derr.any()
    _tune(w.snap, KNOBS["default"])


def test_inlined_subjects_compare_every_bit():
    """Rows of one or two subjects are inlined in the node's slot and compared there: a query whose subject id
    differs from a held one only above bit 15, 23 or 29 is not a member, on the root and one set edge away, under
    every knob set.  (The random cases hold few id pairs that share their low bits.)"""
    rows, qs = [], []
    for i, (a, b) in enumerate([(0x1000005, 5), (5 + 0x10000, 5 + 0x20000), (0x7FFFFFFE, 0x3FFFFFFE), (0x7F000000, 0x3F000000),
                                (0xFFFFFF, 0x1FFFFFF), (0, 0x1000000), (0x40000000, 0), (0x12345678, 0x02345678)]):
        one, two, up = [7, 100 + i, 9], [7, 200 + i, 9], [65534, 0x7FFFFF00 + i, 65534]
        rows += [one + [SUBJECT_ID, a, 0], two + [SUBJECT_ID, a, 0], two + [SUBJECT_ID, a ^ 0x00800000, 0], up + one, up + two]
        for node in (one, two, up):
            qs += [node + [SUBJECT_ID, x, 0] for x in (a, b, a ^ 0x00800000, b ^ 0x00800000, a ^ 0x01000000)]
    t6, q7 = np.asarray(rows, np.uint32), queries_array(np.asarray(qs, np.uint32), 0)
    snap = Snapshot(t6, sp.SimpleNamespace(n_namespaces=65535, n_relations=65535, wildcard_rel=0), None)
    exp, oerr, _ = Oracle(t6, 0).check_batch(q7[:, :6], np.zeros(len(q7), np.int32), 3, POLICY_CANONICAL)
    assert 0.2 < exp.mean() < 0.8 and not oerr.any()
    for name, knobs in KNOBS.items():
        _tune(snap, knobs)
        out, err = Engine(snap, Config(3)).batch_check_ids(q7)
        assert (out == exp).all() and not err.any(), (name, q7[out != exp][:6].tolist())
    snap.close()


# ---------------------------------------------------------------- 2. checks with programs
@pytest.mark.parametrize("mat", [1, 0])
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("layout", sp.PROGRAM_LAYOUTS)
def test_checks_with_programs(layout, seed, mat, monkeypatch):
    w = world(layout, "zero" if seed else "top", seed, True, mat, monkeypatch)
    d = world("dense", "zero" if seed else "top", seed, True, mat, monkeypatch)
    m = w.m
    assert (int(m.ns.max()) + 1) * (int(m.rel.max()) + 1) <= 8 << 20
    assert mat or w.snap.materialized()["union_nodes"] == 0
    # a relation id past the snapshot's table (what a fresh Interner id is): error 1 in a configured namespace,
    # no error in an unconfigured one, inside the table and past it
    n_ns, n_rel, has = int(m.ns.max()) + 1, int(m.rel.max()) + 1, m.program(w.case.prog).ns_has_rel
    conf, free = int(np.nonzero(has)[0][-1]), int(np.nonzero(has == 0)[0][-1])
    obj, sub = int(w.t6[0, 1]), int(w.t6[w.t6[:, 3] == SUBJECT_ID][0, 4])
    beyond = queries_array(np.asarray([[conf, obj, n_rel, SUBJECT_ID, sub, 0], [int(m.ns[0]), obj, n_rel + 7, SUBJECT_ID, TOP, 0],
                                       [free, obj, n_rel, SUBJECT_ID, sub, 0], [min(n_ns, 65534), obj, n_rel, SUBJECT_ID, sub, 0]],
                                      np.uint32), 0)
    assert has[conf] and has[int(m.ns[0])] and not has[free] and (n_ns == 65535 or min(n_ns, 65534) >= len(has))
    out, err, st = check_vs_oracle(w, np.concatenate([w.q7, beyond]))
    n = len(w.q7)
    last = 1 if n_ns == 65535 and has[65534] else 0  # namespace 65534 is the layout's own, configured one
    assert out[n:].tolist() == [2, 2, 0, 2 * last] and err[n:].tolist() == [1, 1, 0, last]
    assert (out[:n] == 2).any() and 0.05 < (out[:n] == 1).mean() < 0.95
    assert mat or st["n_general"] > 0
    dout, derr = d.engine().batch_check_ids(d.q7)
    assert (dout == out[:n]).all() and (derr == err[:n]).all()


# ---------------------------------------------------------------- 3. the packed boundary
PACK_IDS = (0, 255, 256, 4094)


def _packed_batch(w, program):
    """The case's queries plus, for every field of ns / rel / sns / srel and every id of 0, 255, 256 and 4094, a
    query with that field at that id (on a row that exists where the layout has the id), at request depths 0,
    1, 65535 and 65536 (which packs as 65535)."""
    rng = np.random.default_rng(11)
    base = w.t6[w.t6[:, 3] != SUBJECT_ID]
    # the lowering's hidden relations (declared for the library only): as a query's relation such an id is sent in
    # an unconfigured namespace, where any relation is accepted
    hidden = set(w.m.rel[w.case.n_rel_named:].tolist()) if program else set()
    free = int(np.nonzero(w.m.program(w.case.prog).ns_has_rel == 0)[0][0]) if program else 0
    extra = []
    for col in (0, 2, 3, 5):
        for v in PACK_IDS:
            hit = base[base[:, col] == v]
            for k in range(4):
                q = (hit if len(hit) else base)[rng.integers(len(hit) if len(hit) else len(base))].copy()
                q[col] = v
                if col == 2 and v in hidden:  # no caller can name a hidden relation where it is declared
                    q[0] = free
                extra.append(q)
    extra = np.asarray(extra, np.uint32)
    depths = np.tile(np.asarray([0, 1, 65535, 65536]), len(extra) // 4)
    q7 = np.concatenate([w.q7, queries_array(extra, depths)])
    for col in (0, 2, 3, 5):
        for v in PACK_IDS:
            assert (q7[:, col] == v).any(), (col, v)
    for dep in (0, 1, 65535, 65536):
        assert (q7[:, 6] == dep).any()
    return q7


@pytest.mark.parametrize("layout,program", [("packed", False), ("packed-ns", True), ("packed-rel", True),
                                            ("packed-ns", False), ("packed-rel", False)])
@pytest.mark.parametrize("seed", [0, 1])
def test_packed_boundary_at_the_field_limits(layout, program, seed):
    w = world(layout, "top", seed, program)
    q7 = _packed_batch(w, program)
    out, err, _ = check_vs_oracle(w, q7, GMAX, with_stats=False)
    pout, pairs, n_err = w.engine().batch_check_packed(q7)
    perr = np.zeros(len(q7), np.uint32)
    perr[pairs[:, 0]] = pairs[:, 1]
    assert (pout == out).all() and (perr == err).all() and n_err == (out == 2).sum()
    rc, dout, derr = device_packed(w.snap, q7, GMAX)
    assert rc == 0 and (dout == out).all() and (derr == err).all()
    assert 0.05 < (out[:len(w.q7)] == 1).mean() < 0.95
    for col in (0, 2, 3, 5):  # 4095 does not fit any field
        bad = q7[:4].copy()
        bad[:, 3], bad[:, col] = 7, 4095
        with pytest.raises(ValueError):
            _lib.pack_queries(bad)
        assert device_packed(w.snap, bad, GMAX)[0] == -2


def test_packed_host_unpack_on_a_sharded_snapshot():
    """kg_check_batch_packed on a hash-sharded snapshot unpacks on the host (kg_abi.cpp), the third unpacker beside
    k_resolve's and the device unpack kernel: one rank, the library's own stream, the batch of the test above."""
    from keto_amd.sharded import LibShardedChecker
    w = world("packed", "top", 0)
    q7 = _packed_batch(w, False)
    snap = Snapshot(w.t6, w.m.interner(), None, 0, shard=(0, 1))
    chk = LibShardedChecker(snap, 0, 1, None, snapshot_stream=True)
    try:
        e = Engine(snap, Config(GMAX))
        out, err = e.batch_check_ids(q7)
        exp, oerr, _ = w.oracle.check_batch(q7[:, :6], q7[:, 6].copy().view(np.int32), GMAX, POLICY_CANONICAL, nthreads=4)
        assert (out == exp).all() and not err.any() and not oerr.any()
        pout, pairs, n_err = e.batch_check_packed(q7)
        bad = np.nonzero(pout != exp)[0]
        assert bad.size == 0 and n_err == 0, (bad.size, q7[bad[:8]].tolist())
    finally:
        chk.close()


# ---------------------------------------------------------------- 4. the table limit
def test_program_table_limit():
    """A program on namespace 65534 x relation 65534 needs a table past 64 Mi entries: refused with the resource
    error and its message.  The same ids without a program build and answer."""
    from keto_amd.namespace import Program
    t6 = np.asarray([[65534, 5, 65534, SUBJECT_ID, 9, 0], [0, 5, 1, 65534, 5, 65534]], np.uint32)
    it = sp.SimpleNamespace(n_namespaces=65535, n_relations=65535, wildcard_rel=0)
    has = np.zeros(65535, np.uint8)
    has[65534] = 1
    prog = Program(has, np.asarray([65534], np.uint32), np.asarray([65534], np.uint32), np.asarray([-1], np.int32),
                   np.zeros((0, 5), np.int32), np.zeros(0, np.int32))
    assert _lib.KG_ERR_RESOURCE == 4
    with pytest.raises(_lib.KetoGPUError, match=r"\(-4\): .*namespace x relation table too large \(65535 x 65535\)"):
        Snapshot(t6, it, prog)
    snap = Snapshot(t6, it, None)
    q = queries_array(np.asarray([[65534, 5, 65534, SUBJECT_ID, 9, 0], [0, 5, 1, SUBJECT_ID, 9, 0],
                                  [0, 5, 1, SUBJECT_ID, 8, 0]], np.uint32), 0)
    out, err = Engine(snap, Config(3)).batch_check_ids(q)
    exp, _, _ = Oracle(t6, 0).check_batch(q[:, :6], np.zeros(3, np.int32), 3)
    assert out.tolist() == exp.tolist() == [1, 1, 0] and not err.any()


# ---------------------------------------------------------------- 5. expand
def _expand_roots(w):
    """The case's 300 roots and the extremes: set roots at object 0 and 0x7FFFFFFE, subject-id roots at 0 and
    0x7FFFFFFE."""
    sets = w.t6[w.t6[:, 3] != SUBJECT_ID]
    ext = [[SUBJECT_ID, TOP, 0, 0], [SUBJECT_ID, 0, 0, 0]]
    for edge in (0, TOP):  # the rows of the object at the edge, and a set that holds it
        ext += [[r[0], r[1], r[2], 0] for r in w.t6[w.t6[:, 1] == edge][:2]]
        ext += [[r[0], r[1], r[2], 0] for r in sets[sets[:, 4] == edge][:2]]
    ext = np.asarray(ext, np.uint32)
    return np.concatenate([w.m.roots(w.case.roots), ext])


@pytest.mark.parametrize("mode", GW_MODES + ["device"], ids=["default", "gw-all", "hash-all", "lds64-all", "device"])
@pytest.mark.parametrize("layout", ["top-subject", "top-object"])
@pytest.mark.parametrize("seed", [0, 1])
def test_expand(layout, mode, seed):
    w, d = world(layout, "zero", seed), world("dense", "zero", seed, arrange=layout)
    gw, skip = (1, 0) if mode == "device" else mode
    w.snap.tune("expand_gw", gw)
    w.snap.tune("expand_skip_lds", skip)
    roots = _expand_roots(w)
    assert (roots[:, 1] == 0).any() and (roots[:, 1] == TOP).any() and ((roots[:, 0] == SUBJECT_ID) & (roots[:, 1] == TOP)).any()
    ex = ExpandEngine(w.snap, Config(GMAX))
    got = ex.build_trees_ids(roots, device=mode == "device")
    trees = 0
    for r, g in zip(roots, got):
        exp = w.oracle.expand(int(r[0]), int(r[1]), int(r[2]), int(np.uint32(r[3]).view(np.int32)), GMAX)
        _cmp_records(exp, g, r.tolist())
        trees += g is not None and len(g) > 1
    assert trees > 30
    if layout == "top-object":  # the top object's own tree was walked, and it appears inside others
        assert sum(g is not None and (g[:, 3] == TOP).any() for g in got) > 1
    up, n = w.m.lift(), len(w.case.roots)  # the dense case's trees, through the maps
    dgot = ExpandEngine(d.snap, Config(GMAX)).build_trees_ids(d.m.roots(d.case.roots), device=mode == "device")
    for a, b in zip(dgot, got[:n]):
        _cmp_records(up.records(a) if a is not None else None, b, "dense")
    # a subject-id root past the id space: one Leaf naming 2^31-1 (ketogpu.h, kg_set)
    far = np.asarray([[SUBJECT_ID, 0x7FFFFFFF, 0, 0], [SUBJECT_ID, 0xFFFFFFFE, 0, 2], [SUBJECT_ID, 0x80000000, 0, 0]], np.uint32)
    for r, g in zip(far, ex.build_trees_ids(far, device=mode == "device")):
        assert g is not None and g.shape == (1, 6) and g[0, [0, 1, 3, 5]].tolist() == [2, 0, 0x7FFFFFFF, 0], (r, g)
        _cmp_records(w.oracle.expand(int(r[0]), int(r[1]), int(r[2]), int(r[3]), GMAX), g, r.tolist())
    w.snap.tune("expand_gw", 1)
    w.snap.tune("expand_skip_lds", 0)


# ---------------------------------------------------------------- 6. lookups
CALLS = {
    "objects": (lambda e: e.lookup_objects_ids, lambda e: e.lookup_objects_page_ids, "lo_reqs", "lookup_objects"),
    "subjects": (lambda e: e.lookup_subjects_ids, lambda e: e.lookup_subjects_page_ids, "ls_reqs", "lookup_subjects"),
    "sets": (lambda e: e.lookup_subject_sets_ids, lambda e: e.lookup_subject_sets_page_ids, "lss_reqs", "lookup_subject_sets"),
}


def _full_ref(w, kind, reqs):
    """Per request (ascending member ids, ascending (erring id, code)) from the oracle."""
    if kind == "objects":
        return lp.full_objects(w.oracle, lo.domains(w.t6), reqs, GMAX)
    if kind == "subjects":
        return lp.full_subjects(w.oracle, ls.subject_domain(w.t6), reqs, GMAX)
    return lss.full_reference(w.oracle, w.t6, reqs, GMAX)


def _reqs(w, kind):
    reqs = getattr(w.m, CALLS[kind][3])(getattr(w.case, CALLS[kind][2]))
    if kind == "sets":  # filters at 65534 (no row has the pair) and out of range: the empty answer
        far = reqs[:4].copy()
        far[:, 3], far[:, 4] = [65534, 65534, 65535, 0x10000], [65533, 65534, 3, 0xFFFFFFFE]
        reqs = np.concatenate([reqs, far])
    return np.ascontiguousarray(reqs)


def _refs(w, kind):
    key = ("ref", kind)
    if key not in w.__dict__:
        reqs = _reqs(w, kind)
        w.__dict__[key] = (reqs, _full_ref(w, kind, reqs))
    return w.__dict__[key]


LOOKUP_WORLDS = [("top-subject", "zero", False), ("top-object", "none", False), ("wide-rel", "top", True)]
# object ids are listed by the object lookup, subject ids by the subject lookup and by the id requests of the
# subject-set lookup: between them every layout lists both 0 and 0x7FFFFFFE
EDGE_LISTED = {("top-subject", "objects"): 0, ("top-subject", "subjects"): TOP, ("top-subject", "sets"): TOP,
               ("top-object", "objects"): TOP, ("top-object", "subjects"): 0, ("top-object", "sets"): 0}
LOOKUP_KNOBS = [(1, 0, 0), (0, 64, 1), (1, 64, 0), (0, 0, 1)]  # lookup_formula, lookup_cap, lookup_domain_rows


@pytest.mark.parametrize("formula,cap,dom_rows", LOOKUP_KNOBS)
@pytest.mark.parametrize("kind", list(CALLS))
@pytest.mark.parametrize("layout,wildcard,program", LOOKUP_WORLDS)
@pytest.mark.parametrize("seed", [0, 1])
def test_lookups(layout, wildcard, program, kind, formula, cap, dom_rows, seed):
    w = world(layout, wildcard, seed, program)
    reqs, full = _refs(w, kind)
    assert 64 <= len(reqs) <= 150
    _tune(w.snap, dict(lookup_formula=formula, lookup_cap=cap, lookup_domain_rows=dom_rows))
    e = w.engine()
    t0 = time.perf_counter()
    off, ids, err, nerr = CALLS[kind][0](e)(reqs, with_stats=True)
    print(f"{kind} lookup on {layout}: {len(reqs)} requests in {(time.perf_counter() - t0) * 1e3:.1f} ms")
    assert off[0] == 0 and off[-1] == len(ids)
    for i, (mem, bad) in enumerate(full):
        assert ids[int(off[i]):int(off[i + 1])].tolist() == mem, (i, reqs[i].tolist())
        assert (int(nerr[i]), int(err[i])) == (len(bad), bad[0][1] if bad else 0), (i, reqs[i].tolist())
    assert len(ids) > 0
    if not program:  # the layout's extreme of this kind of id is listed, and the dense case lists the same through the maps
        assert (ids == EDGE_LISTED[layout, kind]).any(), kind
        d = world("dense", wildcard, seed, arrange=layout)
        doff, dids, derr, dnerr = CALLS[kind][0](d.engine())(getattr(d.m, CALLS[kind][3])(getattr(d.case, CALLS[kind][2])))
        n = len(doff) - 1
        assert (doff == off[:n + 1]).all() and (w.m.lift().obj[dids] == ids[:int(off[n])]).all()
        assert (derr == err[:n]).all() and (dnerr == nerr[:n]).all()
    if kind == "sets":
        assert all(f == ([], []) for f in full[-4:]) and not nerr[-4:].any()
    # pages of 1 and 3 from 0 to END: the slices of the unpaged answer, the error counts sum, the codes agree
    page = CALLS[kind][1](e)
    for limit in (1, 3):
        lp.page_through(lambda r, p: page(r, p, with_stats=True), reqs, limit, full)
    _tune(w.snap, dict(lookup_formula=1, lookup_cap=0, lookup_domain_rows=0))


@pytest.mark.parametrize("layout,wildcard,kind", [("top-subject", "zero", "subjects"), ("top-subject", "zero", "sets"),
                                                  ("top-object", "none", "objects")])
@pytest.mark.parametrize("seed", [0, 1])
def test_lookup_pages_at_the_top_of_the_id_space(layout, wildcard, kind, seed):
    w = world(layout, wildcard, seed)
    reqs, full = _refs(w, kind)
    top = [i for i, (mem, _) in enumerate(full) if mem and mem[-1] == TOP]
    assert top, "a request lists 0x7FFFFFFE"
    reqs, full = reqs[top], [full[i] for i in top]
    n = len(reqs)
    page = CALLS[kind][1](w.engine())
    for frm, want in ((TOP, [TOP]), (0x7FFFFFFF, []), (0xFFFFFFFE, [])):
        off, ids, err, nerr, nxt = page(reqs, np.tile(np.asarray([frm, 5], np.uint32), (n, 1)))
        assert ids.tolist() == want * n and (nxt == END).all() and off.tolist() == [len(want) * i for i in range(n + 1)]
    # the page that ends exactly at 0x7FFFFFFE: by the header's definition its next is END when the answer holds
    # no further id, and a call from 0x7FFFFFFF (last id + 1) is the empty END page
    for i, (mem, bad) in enumerate(full):
        k = min(3, len(mem))
        frm = mem[-k]
        off, ids, err, nerr, nxt = page(reqs[i:i + 1], np.asarray([[frm, k]], np.uint32))
        assert ids.tolist() == mem[-k:] and int(nxt[0]) == END
        if len(mem) > 1:  # one id short: the cursor is the last id + 1, at most 0x7FFFFFFE
            off, ids, err, nerr, nxt = page(reqs[i:i + 1], np.asarray([[mem[-2], 1]], np.uint32))
            assert ids.tolist() == [mem[-2]] and int(nxt[0]) == mem[-2] + 1 <= TOP
            off, ids, err, nerr, nxt = page(reqs[i:i + 1], np.asarray([[int(nxt[0]), 1]], np.uint32))
            assert ids.tolist() == [TOP] and int(nxt[0]) == END


# ---------------------------------------------------------------- 7. listing, rows, export
def test_listing_rows_export_at_the_limits():
    """Snapshot.query with every mask on tuples whose fields sit at the limits, KG_Q_SUBJECT for a subject id and
    for a set; export() and rows() hand the ids back unchanged."""
    rng = np.random.default_rng(3)
    nsr, objs = [0, 255, 256, 4095, 65534], [0, 1, 31, 32, 0xFFFF, 0x10000, 0x7FFFFFFD, TOP]
    rows = []
    for _ in range(400):
        ns, obj, rel = rng.choice(nsr), rng.choice(objs), rng.choice(nsr)
        if rng.random() < 0.5:
            rows.append([ns, obj, rel, SUBJECT_ID, rng.choice(objs), 0])
        else:
            rows.append([ns, obj, rel, rng.choice(nsr), rng.choice(objs), rng.choice(nsr)])
    rows = np.asarray(rows, np.uint32)
    keys = np.sort(rng.choice(np.arange(1, 1 << 20, dtype=np.uint64), len(rows), replace=False))
    it = sp.SimpleNamespace(n_namespaces=65535, n_relations=65535, wildcard_rel=65534)
    snap = Snapshot(rows, it, None, keys=keys)
    sid, sset = rows[rows[:, 3] == SUBJECT_ID], rows[rows[:, 3] != SUBJECT_ID]
    top_s, top_o = sid[sid[:, 4] == TOP][0], sset[sset[:, 1] == TOP][0]
    edge = sset[(sset[:, 3] == 65534) | (sset[:, 5] == 65534)][0]
    absent = top_o.copy()
    absent[0], absent[4] = 4094, 0x7FFFFFFC
    qs = [(mask, t) for mask in range(16) for t in (top_s, top_o, edge, sid[0], sset[0], absent)]
    for limit in (1, 1000):
        check_call(snap, rows, keys, qs, 0, limit)
    assert np.array_equal(multiset(snap.export()), multiset(rows))
    nodes = np.unique(rows[:, :3], axis=0)
    off, got = snap.rows(nodes)
    assert off[-1] == len(rows)
    for i, nd in enumerate(nodes):
        want = rows[(rows[:, :3] == nd).all(axis=1)]
        assert np.array_equal(got[off[i]:off[i + 1]], want), nd


# ---------------------------------------------------------------- 8. apply
def _verify_after_apply(snap, rows, prog):
    """export() is the reference's rows; checks and one lookup of each kind equal the oracle's on those rows."""
    assert np.array_equal(multiset(snap.export()), multiset(rows))
    oracle = Oracle(rows, 0, prog)
    rng = np.random.default_rng(len(rows))
    q = rows[rng.integers(len(rows), size=600)].copy()
    other = rows[rng.integers(len(rows), size=600)]
    swap = rng.random(600) < 0.6
    q[swap, 3:] = other[swap, 3:]
    q7 = queries_array(q, 0)
    e = Engine(snap, Config(GMAX))
    out, err = e.batch_check_ids(q7)
    exp, oerr, _ = oracle.check_batch(q, np.zeros(len(q), np.int32), GMAX, POLICY_CANONICAL)
    assert (out == exp).all() and (err.astype(np.int64) == oerr).all() and 0.05 < (out == 1).mean() < 0.95
    assert prog is not None or not err.any()
    lo_reqs = np.ascontiguousarray(np.stack([q[:64, 0], q[:64, 2], q[:64, 3], q[:64, 4], q[:64, 5], q7[:64, 6]], 1))
    lo.compare(e, lo_reqs, lo.reference(oracle, lo.domains(rows), lo_reqs, GMAX), with_stats=False)
    ls_reqs = np.ascontiguousarray(np.stack([q[:64, 0], q[:64, 1], q[:64, 2], q7[:64, 6]], 1))
    ls.compare(e, ls_reqs, ls.reference(oracle, ls.subject_domain(rows), ls_reqs, GMAX), with_stats=False)
    f = lss.set_filters(rows)
    flt = np.asarray([f[i % len(f)] for i in range(64)], np.uint32)
    ss_reqs = np.ascontiguousarray(np.stack([q[:64, 0], q[:64, 1], q[:64, 2], flt[:, 0], flt[:, 1], q7[:64, 6]], 1))
    lss.compare(e, ss_reqs, lss.brief(lss.full_reference(oracle, rows, ss_reqs, GMAX)))
    return oracle


@pytest.mark.parametrize("program", [False, True])
def test_apply_brings_the_extremes(program):
    """A dense base, then one delta with subject id 0x7FFFFFFE (the holder bitmap grows from a few bytes to 2^31
    bits), namespace 65534 and a relation id above the base's (with a program: its tables grow), then a delta that
    deletes the top id again (the bitmap's top bit goes).  After each step export() equals the reference rows and
    checks and lookups equal the oracle's."""
    case = Case(2, program=program)
    m = case.maps("dense")
    base, prog, oprog = m.tuples(case.t6), m.program(case.prog), m.program(case.prog_oracle)
    it = sp.SimpleNamespace(n_namespaces=case.n_ns, n_relations=case.n_rel, wildcard_rel=0)
    snap = Snapshot(base, it, prog)
    _verify_after_apply(snap, base, oprog)
    holder = base[base[:, 3] != SUBJECT_ID][0]
    new_rel = case.n_rel + (5 if program else 40000)  # with a program the table stays below 64 Mi entries
    ins = np.asarray([[holder[3], holder[4], holder[5], SUBJECT_ID, TOP, 0],       # the top subject id, reachable
                      [base[0, 0], base[0, 1], base[0, 2], SUBJECT_ID, TOP, 0],
                      [65534, TOP, new_rel, SUBJECT_ID, TOP, 0],                    # a new namespace and relation
                      [base[1, 0], base[1, 1], base[1, 2], 65534, TOP, new_rel],    # ... that a base row now points at
                      [65534, 0, new_rel, SUBJECT_ID, 0x7FFFFFFD, 0]], np.uint32)
    none = np.zeros((0, 6), np.uint32)
    it.n_namespaces, it.n_relations = 65535, new_rel + 1
    snap2 = snap.apply(ins, none)
    rows2, _ = apply_ref(base, None, ins, None, none)
    _verify_after_apply(snap2, rows2, oprog)
    probe = np.asarray([[65534, TOP, new_rel, 0], [65534, 0, new_rel, 0]], np.uint32)
    off, ids, _, nerr = Engine(snap2, Config(GMAX)).lookup_subjects_ids(probe)
    assert ids.tolist() == [TOP, 0x7FFFFFFD] and not nerr.any()
    dels = ins[[0, 1, 2]]  # every row that holds the top id
    snap3 = snap2.apply(none, dels)
    rows3, _ = apply_ref(rows2, None, none, None, dels)
    assert not (rows3[rows3[:, 3] == SUBJECT_ID, 4] == TOP).any() and len(rows3) == len(base) + 2
    oracle3 = _verify_after_apply(snap3, rows3, oprog)
    e3 = Engine(snap3, Config(GMAX))
    off, ids, _, nerr = e3.lookup_subjects_ids(probe)
    assert ids.tolist() == [0x7FFFFFFD] and off.tolist() == [0, 0, 1] and not nerr.any()
    out, err = e3.batch_check_ids(queries_array(ins, 0))
    exp, oerr, _ = oracle3.check_batch(ins, np.zeros(len(ins), np.int32), GMAX, POLICY_CANONICAL)
    assert (out == exp).all() and (err.astype(np.int64) == oerr).all() and out[4] == 1
    assert program or out[:3].tolist() == [0, 0, 0]  # nothing holds the top id any more (a `not` rewrite may still say member)
    _verify_after_apply(snap2, rows2, oprog)  # the older snapshot still answers as before


# ---------------------------------------------------------------- the header's knob list
KNOB_DEFAULTS = {
    "stream_ecap": 512, "stream_steal": 4, "stream_wgs": 2, "back_wgs": 3, "grid_wgs": 2, "back_edges": 0,
    "interp_cap2": 0, "grid_reserve": 0, "grid_cap": 0, "max_lanes": 32, "grid_ms": 1, "grid_ms_words": 8,
    "grid_ms_bytes": 1 << 30, "grid_ms_tg_cap": 256, "grid_ms_cap": 0, "level_events": 0, "holder_sig": 1, "expand_gw": 1,
    "expand_gw_wait_us": 100000, "expand_skip_lds": 0, "expand_hash_cap": 1 << 18, "lookup_cap": 0,
    "lookup_domain_rows": 0, "lookup_formula": 1, "query_cap": 0, "shard_vis": 23, "shard_heavy": 64,
    "shard_budget": 0, "shard_back_budget": 1 << 14, "shard_bucket": 0, "shard_local": 1, "shard_force_exchange": 0,
    "shard_remote_meta": 1, "shard_max_reruns": 0, "shard_max_bytes": 0, "shard_force_overflow": 0,
}
# the range the header's comment gives each key (None: no bound on that side; "grid_reserve" takes any value)
KNOB_RANGES = {
    "stream_ecap": (0, 2 ** 32 - 1), "stream_steal": (1, 8), "stream_wgs": (0, 8), "back_wgs": (1, 3), "grid_wgs": (1, 64),
    "back_edges": (0, 2 ** 20), "interp_cap2": (0, 4194304), "grid_reserve": (None, None), "grid_cap": (0, 2 ** 34),
    "max_lanes": (1, 1024), "grid_ms": (0, 1), "grid_ms_words": (1, 16), "grid_ms_bytes": (2 ** 20, 2 ** 40),
    "grid_ms_tg_cap": (0, 2 ** 31 - 1), "grid_ms_cap": (0, 2 ** 28), "level_events": (0, 1), "holder_sig": (0, 1),
    "expand_gw": (0, 1), "expand_gw_wait_us": (0, 10 ** 7), "expand_skip_lds": (0, 2), "expand_hash_cap": (4, 2 ** 18),
    "lookup_cap": (0, 2 ** 32), "lookup_domain_rows": (0, 1), "lookup_formula": (0, 1), "query_cap": (0, 2 ** 32),
    "shard_vis": (10, 34), "shard_heavy": (0, 2 ** 32 - 1), "shard_budget": (0, 2 ** 32 - 1),
    "shard_back_budget": (0, 2 ** 32 - 1), "shard_bucket": (0, 2 ** 26), "shard_local": (0, 1),
    "shard_force_exchange": (0, 1), "shard_remote_meta": (0, 1), "shard_max_reruns": (0, 64),
    "shard_max_bytes": (0, None), "shard_force_overflow": (0, 1),
}
REMOVED_KNOBS = ["back", "resolve_unheld", "device_sync", "host_sync", "stream_chunk", "interp_wgs", "grid_bidir",
                 "shard_wgs", "shard_vis_mode", "shard_pack", "shard_level_occ"]


def test_knob_list_of_the_header():
    """Every key the kg_snapshot_tune comment of include/ketogpu.h names is accepted at its documented default;
    the values just outside its documented range are refused with -2 and an error that names the key; an unknown
    key and every key removed since are refused with -2 and "unknown knob".  Checks answer as before afterwards."""
    t6 = np.asarray([[0, i, 1, SUBJECT_ID, 20 + i, 0] for i in range(10)], np.uint32)
    snap = Snapshot(t6, sp.SimpleNamespace(n_namespaces=1, n_relations=2, wildcard_rel=0), None)
    L = _lib.load()
    assert set(KNOB_RANGES) == set(KNOB_DEFAULTS)
    for key, value in KNOB_DEFAULTS.items():
        assert L.kg_snapshot_tune(snap.handle, key.encode(), value) == 0, (key, _lib.last_error())
    for key, (lo, hi) in KNOB_RANGES.items():
        outside = ([] if lo is None else [lo - 1]) + ([] if hi is None else [hi + 1])
        if key == "grid_ms_words":
            outside += [3, 32]
        for value in outside:
            assert L.kg_snapshot_tune(snap.handle, key.encode(), value) == -2, (key, value)
            assert key in _lib.last_error() and "unknown knob" not in _lib.last_error(), (key, value, _lib.last_error())
        assert L.kg_snapshot_tune(snap.handle, key.encode(), KNOB_DEFAULTS[key]) == 0, (key, _lib.last_error())
    for key in ["no_such_knob"] + REMOVED_KNOBS:
        assert L.kg_snapshot_tune(snap.handle, key.encode(), 0) == -2, key
        assert "unknown knob" in _lib.last_error(), key
    out, err = Engine(snap, Config(2)).batch_check_ids(queries_array(t6, 0))
    assert out.all() and not err.any()
