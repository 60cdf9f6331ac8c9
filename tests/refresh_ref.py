"""Test-only CPU restatement of kg_snapshot_apply's row contract (include/ketogpu.h; the nine merge
kernels of keto_amd/csrc/kg_delta.hip are what it checks).  Plain NumPy, no GPU.

The contract, from the header: the new snapshot holds the base's rows, minus every base row equal
to a tuple of the deletes (every duplicate of it; inserts are never dropped: "deletes apply to base
rows"), plus the inserts.  Within a node (ns, obj, rel) the rows are in order-key order; on equal
keys the kept base rows come first, in their old order, then the inserts in argument order.
Without keys, base rows keep their order and the inserts follow in argument order.

Rows are (n, 6) uint32 tuple ids (ns, obj, rel, sns, sobj, srel), sns == SUBJECT_ID for a subject
id (srel ignored).  A keyed base is in ascending key order, as kg_snapshot_create_ordered requires,
and so is the result: it can be handed to Snapshot(rows, ..., keys=keys) as it is.  The order of a
node's rows is their order in the array."""
import numpy as np

SUBJECT_ID = 0xFFFFFFFF
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)  # inserts without a key into a keyed base go last


def _rows6(a) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(a, np.uint32).reshape(-1, 6)).copy()
    a[a[:, 3] == SUBJECT_ID, 5] = 0  # a subject id has no relation
    return a


def _whole(a: np.ndarray) -> np.ndarray:
    """One comparable scalar per row (its 24 bytes)."""
    return np.ascontiguousarray(a).view(np.dtype((np.void, 24))).ravel()


def apply_ref(rows6, keys, ins6, ins_keys, del6):
    """(rows6, keys) of the refreshed snapshot; keys is None for a base without keys."""
    base, ins, dels = _rows6(rows6), _rows6(ins6), _rows6(del6)
    keep = ~np.isin(_whole(base), _whole(dels))
    rows = np.concatenate([base[keep], ins])  # kept base rows in their old order, then the inserts in argument order
    if keys is None:
        assert ins_keys is None, "a base without keys takes inserts without keys"
        return rows, None
    keys = np.asarray(keys, np.uint64).ravel()
    assert len(keys) == len(base) and (keys[1:] >= keys[:-1]).all(), "a keyed base is in ascending key order"
    ik = np.full(len(ins), NO_KEY, np.uint64) if ins_keys is None else np.asarray(ins_keys, np.uint64).ravel()
    assert len(ik) == len(ins)
    k = np.concatenate([keys[keep], ik])
    order = np.argsort(k, kind="stable")  # ties: the order above
    return rows[order], k[order]


def node_rows(rows6, nodes3):
    """Snapshot.rows(nodes3) as the rows say: (offsets [n + 1], rows (m, 6)), node i's rows in array
    order at rows[offsets[i]:offsets[i + 1]]."""
    rows, nodes = _rows6(rows6), np.asarray(nodes3, np.uint32).reshape(-1, 3)

    def packed(a):  # (ns, rel, obj) in one u64; row ids are below 2^16 / 2^16 / 2^31
        a = a.astype(np.uint64)
        assert (a[:, 0] < 1 << 16).all() and (a[:, 2] < 1 << 16).all()
        return (a[:, 0] << np.uint64(48)) | (a[:, 2] << np.uint64(32)) | a[:, 1]

    rk, qk = packed(rows[:, :3]), packed(nodes)
    order = np.argsort(rk, kind="stable")  # grouped by node, array order kept inside a node
    sk = rk[order]
    lo, hi = np.searchsorted(sk, qk, "left"), np.searchsorted(sk, qk, "right")
    off = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.int64)
    idx = np.repeat(lo - off[:-1], hi - lo) + np.arange(off[-1])
    return off, rows[order[idx]]


def multiset(rows6) -> np.ndarray:
    """The rows sorted lexicographically: equal for equal multisets."""
    rows = _rows6(rows6)
    return rows[np.lexsort(rows.T[::-1])]


def nodes_of(*rows6) -> np.ndarray:
    """The distinct (ns, obj, rel) of the objects and the subject sets of the given row arrays."""
    out = [np.zeros((0, 3), np.uint32)]
    for a in rows6:
        a = _rows6(a)
        out += [a[:, :3], a[a[:, 3] != SUBJECT_ID, 3:]]
    return np.unique(np.concatenate(out), axis=0)
