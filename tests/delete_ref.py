"""Test-only CPU restatement of kg_snapshot_delete_matching's row contract (include/ketogpu.h; the kernels
of keto_amd/csrc/kg_delete.hip are what it checks).  Plain NumPy, no GPU.

The contract, from the header: the new snapshot holds the base's rows minus every row that matches any of
the queries.  A query is (mask, tuple ids): a row matches when the fields named in mask (KG_Q_NS, KG_Q_OBJ,
KG_Q_REL) are equal and -- with KG_Q_SUBJECT -- its subject is the query's, subject kinds distinguished: a
query with sns == SUBJECT_ID matches subject-id rows only, any other only subject-set rows with exactly that
set.  mask == 0 matches every row.  The kept rows keep their order and their keys.

Rows are (n, 6) uint32 tuple ids as in refresh_ref.  The order key of a row is keys[i], or -- keys is None --
its position + 1, so a base without keys is passed in kg_snapshot_export's order (Snapshot.export())."""
import numpy as np

from refresh_ref import SUBJECT_ID, _rows6

Q_NS, Q_OBJ, Q_REL, Q_SUBJECT = 1, 2, 4, 8


def as_queries(queries):
    """[(mask, (6,) ids)] from such pairs or from kg_row_query records (fields "mask" and "t")."""
    if isinstance(queries, np.ndarray) and queries.dtype.names:
        return [(int(m), np.asarray(t, np.uint32)) for m, t in zip(queries["mask"], queries["t"])]
    return [(int(m), np.asarray(t, np.uint32).reshape(6)) for m, t in queries]


def match_one(rows: np.ndarray, mask: int, t: np.ndarray) -> np.ndarray:
    """bool [n]: the rows of _rows6 form that the query matches."""
    hit = np.ones(len(rows), bool)
    for bit, col in ((Q_NS, 0), (Q_OBJ, 1), (Q_REL, 2)):
        if mask & bit:
            hit &= rows[:, col] == t[col]
    if mask & Q_SUBJECT:
        if t[3] == SUBJECT_ID:
            hit &= (rows[:, 3] == SUBJECT_ID) & (rows[:, 4] == t[4])
        else:
            hit &= (rows[:, 3] != SUBJECT_ID) & (rows[:, 3] == t[3]) & (rows[:, 4] == t[4]) & (rows[:, 5] == t[5])
    return hit


def delete_ref(rows6, keys, queries):
    """(rows6, keys, deleted_keys, matched) after the delete: keys is None for a base without keys (the
    deleted keys are then positions + 1); deleted_keys ascending with duplicates kept; matched [n_queries]
    counts a row for every query that matches it."""
    rows = _rows6(rows6)
    qs = as_queries(queries)
    gone = np.zeros(len(rows), bool)
    matched = np.zeros(len(qs), np.uint64)
    for i, (mask, t) in enumerate(qs):
        hit = match_one(rows, mask, t)
        matched[i] = hit.sum()
        gone |= hit
    if keys is None:
        k = np.arange(1, len(rows) + 1, dtype=np.uint64)
        return rows[~gone], None, k[gone], matched
    k = np.asarray(keys, np.uint64).ravel()
    assert len(k) == len(rows)
    return rows[~gone], k[~gone], np.sort(k[gone], kind="stable"), matched
