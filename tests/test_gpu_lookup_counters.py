"""The counters of both lookups, pinned: (n_objs, exact, candidates, confirmed, reverse_edges, levels) of
last_stats for the depth-boundary chains, the hub graphs and the output-regrowth graphs of
test_gpu_lookup.py / test_gpu_lookup_subjects.py.  The walks are level-synchronous, so the counters are
deterministic; the answers themselves are compared with the oracle in those two files."""
import pytest

import test_gpu_lookup as lo
import test_gpu_lookup_subjects as ls
from keto_amd.engine import Config, Engine, Registry
from keto_amd.ketoapi import RelationTuple
from keto_amd.mapper import Interner

pytestmark = pytest.mark.gpu

T = RelationTuple.from_string
KEYS = ("n_objs", "exact", "candidates", "confirmed", "reverse_edges", "levels")


def stats(e, kind, reqs):
    (e.lookup_objects_ids if kind == "objects" else e.lookup_subjects_ids)(reqs, with_stats=True)
    return tuple(int(e.last_stats[k]) for k in KEYS)


# ---------------------------------------------------------------- the chains: derived by hand
@pytest.fixture(scope="module")
def reverse_chain():
    it = Interner()
    tuples = [T("g:c0#m@user")] + [T(f"g:c{i}#m@(g:c{i - 1}#m)") for i in range(1, 7)]
    reg = Registry(tuples, [], interner=it, max_read_depth=10)
    return reg, lambda d: lo.requests_array(it, [T("g:any#m@user")], [d])


@pytest.fixture(scope="module")
def forward_chain():
    it = Interner()
    tuples = [T(f"g:c{i}#m@(g:c{i - 1}#m)") for i in range(1, 7)] + [T(f"g:c{i}#m@u{i}") for i in range(7)]
    reg = Registry(tuples, [], interner=it, max_read_depth=10)
    return reg, lambda d: ls.requests_array(it, [("g", "c6", "m")], [d])


@pytest.mark.parametrize("through_global", [False, True])
@pytest.mark.parametrize("d", range(1, 10))
def test_reverse_chain(reverse_chain, d, through_global):
    """c0 holds the user and c{i} is the only parent of c{i-1}.  The seed lists c0; level j = 1 .. d-1
    reads the one reverse edge of c{j-1} and lists c{j}.  c6 has no parent: level 7 runs on the frontier
    {c6}, reads no edge and leaves no frontier, so levels == min(d-1, 7), reverse_edges == min(d-1, 6) and
    min(d, 7) objects are listed, all by the walk."""
    reg, reqs = reverse_chain
    e = Engine(reg.snapshot, Config(d if through_global else 10))
    got = stats(e, "objects", reqs(0 if through_global else d))
    assert got == (min(d, 7), min(d, 7), 0, 0, min(d - 1, 6), min(d - 1, 7)), (d, got)


@pytest.mark.parametrize("through_global", [False, True])
@pytest.mark.parametrize("d", range(1, 10))
def test_forward_chain(forward_chain, d, through_global):
    """The root is c6; level j = 0 .. d-1 has the frontier {c{6-j}} and ends with c0 (j == 6), so
    levels == min(d, 7).  A level's emit reads the node's whole check row: u{k} and the set c{k-1}, 2
    entries, for c0 the 1 entry u0 -- 2 * min(d, 6) entries plus 1 when d >= 7.  The expansion of level
    j runs when d-1 >= j+1 and reads the node's adj row: 1 edge, none for c0 -- min(d-1, 6) edges.
    reverse_edges counts both.  One id per level is listed, all by the walk."""
    reg, reqs = forward_chain
    e = Engine(reg.snapshot, Config(d if through_global else 10))
    got = stats(e, "subjects", reqs(0 if through_global else d))
    edges = 2 * min(d, 6) + (1 if d >= 7 else 0) + min(d - 1, 6)
    assert got == (min(d, 7), min(d, 7), 0, 0, edges, min(d, 7)), (d, got)


# ---------------------------------------------------------------- hubs and regrowth: as recorded
# What the commit before the two walks were folded into one returns.
HUB = {
    ("objects", 3): (45039, 45039, 0, 0, 5008, 2),
    ("objects", 12): (45075, 45075, 0, 0, 5026, 11),
    ("subjects", 3): (55048, 70069, 0, 0, 70206, 9),  # a group outgrows the first 64 Ki keys and is rerun
    ("subjects", 12): (55050, 70073, 0, 0, 70652, 36),
}
REGROWTH = {
    ("objects", 0): (20000, 20000, 0, 0, 0, 1),
    ("objects", 16): (20000, 20000, 0, 0, 0, 2),
    ("subjects", 0): (20063, 20063, 0, 0, 20063, 1),
    ("subjects", 16): (20063, 20063, 0, 0, 40126, 2),
}


def _hub_objects():
    """The graph and the 72 requests of test_gpu_lookup.test_hub_cycle_duplicates."""
    it = Interner()
    tuples = [T(f"g:h{i}#m@hubuser") for i in range(5000)]
    tuples += [T(f"g:top{i}#m@(g:hub#m)") for i in range(5000)]
    tuples += [T("g:hub#m@deep"), T("g:hub#m@(d:c7#v)"), T("g:hub#w@deep")]
    tuples += [T(f"d:c{i}#v@(d:c{(i + 1) % 40}#v)") for i in range(40)]
    tuples += [T("d:c0#v@cyc"), T("d:c20#w@cyc"), T("d:x#v@(g:hub#m)"), T("g:y#m@(d:c5#v)"), T("g:y#w@(d:c5#v)"),
               T("d:z#w@(g:top17#m)"), T("g:top3#m@(g:h9#m)")]
    tuples += [T("d:c0#v@cyc"), T("g:hub#m@deep"), T("d:c3#v@(d:c4#v)"), T("g:h1#m@hubuser")]
    qs, depths = [], []
    for s in ["hubuser", "deep", "cyc", "nobody", "(g:hub#m)", "(d:c3#v)"]:
        for ns, rel in (("g", "m"), ("d", "v"), ("g", "w"), ("d", "w")):
            for d in (0, 2, 41):
                qs.append(T(f"{ns}:any#{rel}@{s}"))
                depths.append(d)
    return it, tuples, lo.requests_array(it, qs, depths)


def _regrowth_objects():
    """test_gpu_lookup.test_output_regrowth: 20,000 objects of one subject, in the middle of a group."""
    it = Interner()
    tuples = [T(f"n:o{i}#r@big") for i in range(20000)]
    qs = [T("n:any#r@big")] + [T(f"n:any#r@nobody{i}") for i in range(63)]
    qs = qs[20:] + qs[:20]
    return it, tuples, lo.requests_array(it, qs, [0] * len(qs))


def _regrowth_subjects():
    """test_gpu_lookup_subjects.test_output_regrowth: 20,000 ids on one object, in the middle of a group."""
    it = Interner()
    tuples = [T(f"n:big#r@s{i}") for i in range(20000)] + [T(f"n:o{i}#r@s{i}") for i in range(63)]
    roots = [("n", f"o{i}", "r") for i in range(63)]
    roots = roots[:30] + [("n", "big", "r")] + roots[30:]
    return it, tuples, ls.requests_array(it, roots, [0] * len(roots))


GRAPHS = {"hub_objects": _hub_objects, "hub_subjects": ls._hub_case, "regrowth_objects": _regrowth_objects,
          "regrowth_subjects": _regrowth_subjects}


def fresh(name):
    """A new snapshot per case: a lane keeps its grown output list between calls, and a rerun counts."""
    it, tuples, reqs = GRAPHS[name]()
    return Registry(tuples, [], interner=it), reqs


@pytest.mark.parametrize("kind,gmax", sorted(HUB))
def test_hub(kind, gmax):
    reg, reqs = fresh("hub_" + kind)
    got = stats(Engine(reg.snapshot, Config(gmax)), kind, reqs)
    assert got == HUB[kind, gmax], got


@pytest.mark.parametrize("kind,cap", sorted(REGROWTH))
def test_output_regrowth(kind, cap):
    reg, reqs = fresh("regrowth_" + kind)
    reg.snapshot.tune("lookup_cap", cap)
    got = stats(Engine(reg.snapshot, Config(5)), kind, reqs)
    assert got == REGROWTH[kind, cap], got
