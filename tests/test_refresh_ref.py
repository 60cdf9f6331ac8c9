"""CPU tests of tests/refresh_ref.py (the reference the GPU refresh tests compare kg_snapshot_apply
with): apply_ref against a from-scratch np.lexsort over (node, key, origin, sequence) on random
deltas with tied keys and duplicate rows, and the corner cases of the contract by hand."""
import numpy as np
import pytest

from refresh_ref import SUBJECT_ID, apply_ref, multiset, node_rows, nodes_of


def _random_rows(rng, n, n_obj, key_hi):
    r = np.zeros((n, 6), np.uint32)
    r[:, 0], r[:, 1], r[:, 2] = rng.integers(0, 2, n), rng.integers(0, n_obj, n), rng.integers(1, 3, n)
    sets = rng.random(n) < 0.4
    r[:, 3] = np.where(sets, rng.integers(0, 2, n), SUBJECT_ID)
    r[:, 4] = rng.integers(0, n_obj, n)
    r[:, 5] = np.where(sets, rng.integers(0, 3, n), 0)
    return r, np.sort(rng.integers(0, key_hi, n).astype(np.uint64))


def _lexsort_ref(rows, keys, ins, ins_keys, dels):
    """Per node, the row indexes (into base ++ ins) in the contract's order, by one lexsort."""
    alive = np.asarray([not (dels == r).all(1).any() for r in rows], bool) if len(dels) else np.ones(len(rows), bool)
    allr = np.concatenate([rows, ins])
    use = np.concatenate([alive, np.ones(len(ins), bool)])
    _, node = np.unique(allr[:, :3], axis=0, return_inverse=True)
    node = node.ravel()
    key = np.concatenate([keys, ins_keys]) if keys is not None else np.zeros(len(allr), np.uint64)
    origin = np.concatenate([np.zeros(len(rows), np.int64), np.ones(len(ins), np.int64)])
    seq = np.concatenate([np.arange(len(rows)), np.arange(len(ins))])
    order = np.lexsort((seq, origin, key, node))
    order = order[use[order]]
    return allr[order], node[order]


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("seed", range(6))
def test_apply_ref_vs_lexsort(seed, keyed):
    rng = np.random.default_rng(40 + seed)
    rows, keys = _random_rows(rng, 300, 12, 60)  # 300 keys below 60: many ties
    rows = np.concatenate([rows, rows[:20]])  # duplicate rows
    keys = np.sort(np.concatenate([keys, keys[:20]]))
    ins, ins_keys = _random_rows(rng, 120, 14, 70)
    ins_keys = rng.permutation(ins_keys)  # inserts arrive in any key order
    ins[:10] = rows[:10]  # inserts equal to base rows, some of them deleted below
    dels = np.concatenate([rows[rng.choice(len(rows), 60, replace=False)], ins[:5], _random_rows(rng, 10, 40, 1)[0]])
    got, gk = apply_ref(rows, keys if keyed else None, ins, ins_keys if keyed else None, dels)
    want, wnode = _lexsort_ref(rows, keys if keyed else None, ins, ins_keys, dels)
    assert len(got) == len(want) and np.array_equal(multiset(got), multiset(want))
    nodes = nodes_of(rows, ins, dels)
    off, per_node = node_rows(got, nodes)
    woff, wper = node_rows(want, nodes)  # want is grouped by node already: node_rows keeps each group's order
    assert np.array_equal(off, woff) and np.array_equal(per_node, wper)
    if keyed:
        assert (gk[1:] >= gk[:-1]).all() and len(gk) == len(got)
    else:
        assert gk is None
    assert len(got) < len(rows) + len(ins)  # something was deleted
    assert any((got == r).all(1).any() for r in ins[:5])  # a deleted tuple that is also inserted stays, once per insert


def test_contract_by_hand():
    S = SUBJECT_ID
    base = np.asarray([[0, 1, 1, S, 7, 0], [0, 1, 1, S, 8, 0], [0, 1, 1, S, 7, 0], [0, 2, 1, 0, 1, 1],
                       [0, 1, 1, S, 9, 0]], np.uint32)
    keys = np.asarray([10, 20, 20, 25, 30], np.uint64)
    ins = np.asarray([[0, 1, 1, S, 5, 0], [0, 1, 1, S, 6, 0], [0, 1, 1, S, 7, 0], [0, 1, 1, S, 4, 0], [0, 3, 1, S, 1, 0]],
                     np.uint32)
    ins_keys = np.asarray([20, 5, 20, 99, 1], np.uint64)
    dels = np.asarray([[0, 1, 1, S, 7, 0], [0, 9, 9, S, 7, 0], [0xFFFF, 1, 1, S, 7, 0]], np.uint32)
    rows, k = apply_ref(base, keys, ins, ins_keys, dels)
    off, r = node_rows(rows, [[0, 1, 1], [0, 2, 1], [0, 3, 1], [0, 4, 4]])
    # both base copies of subject 7 go; the inserted 7 stays; key 20: the base row (8), then inserts 5, 7 in
    # argument order
    assert r[off[0]:off[1], 4].tolist() == [6, 8, 5, 7, 9, 4]
    assert off.tolist() == [0, 6, 7, 8, 8]
    assert k.tolist() == sorted(k.tolist()) and len(k) == 8
    rows, k = apply_ref(base, None, ins, None, dels)
    off, r = node_rows(rows, [[0, 1, 1]])
    assert k is None and r[:, 4].tolist() == [8, 9, 5, 6, 7, 4]  # base order, then the inserts in argument order
    rows, k = apply_ref(base, keys, np.zeros((0, 6), np.uint32), np.zeros(0, np.uint64), np.zeros((0, 6), np.uint32))
    assert np.array_equal(rows, base) and np.array_equal(k, keys)  # the empty delta
    rows, k = apply_ref(base, keys, ins[:1], ins_keys[:1], base)
    assert np.array_equal(rows, ins[:1]) and k.tolist() == [20]  # everything deleted, one insert
