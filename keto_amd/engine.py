"""Host-side mirror of the reference's check / expand engine surface, running on the MI355X
library through the C ABI.

Reference interfaces mirrored (paths relative to the reference checkout):
  check.NewEngine / Engine.CheckIsMember / CheckRelationTuple   internal/check/engine.go:42-80
  Engine.BatchCheck (new)                         == a loop of CheckIsMember
  expand.Engine.BuildTree                                       internal/expand/engine.go:35-104
  config.Provider.MaxReadDepth (default 5, 1..65535)            internal/driver/config/provider.go:160-162
  checkgroup.Result{Membership, Tree, Err}                      internal/check/checkgroup/definitions.go:46-69
    (the tree of a member result: keto_amd/explain.py)
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .ketoapi import CheckTree, RelationTuple, SubjectSet, Tree, TREE_LEAF, TREE_UNION
from .mapper import Interner, Mapper, SUBJECT_ID
from .namespace import Namespace, Program, compile_program

MEMBERSHIP_UNKNOWN, IS_MEMBER, NOT_MEMBER = 0, 1, 2  # checkgroup.Membership

ERR_TEXT = {
    _lib.KG_ERR_RELATION_NOT_FOUND: "relation not found",       # engine.go:228
    _lib.KG_ERR_NOT_IMPLEMENTED: "not implemented",             # rewrites.go:15-17
    _lib.KG_ERR_REWRITE_CYCLE: "computed subject-set rewrite cycle",
    _lib.KG_ERR_RESOURCE: "engine capacity exceeded",
}


class CheckError(RuntimeError):
    def __init__(self, code: int):
        super().__init__(ERR_TEXT.get(code, f"error {code}"))
        self.code = code


@dataclass
class Result:
    membership: int
    err: Optional[CheckError] = None
    tree: Optional[CheckTree] = None


@dataclass
class Config:
    max_read_depth: int = 5
    namespaces: List[Namespace] = field(default_factory=list)

    def __post_init__(self):
        if not 1 <= self.max_read_depth <= 65535:  # embedx/config.schema.json:308-315
            raise ValueError("max_read_depth must be in [1, 65535]")


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class Snapshot:
    """An HBM-resident, immutable snapshot of the relation tuples (rows in shard order)."""

    def __init__(self, tuples: np.ndarray, interner: Interner, program: Optional[Program] = None, device: int = 0,
                 _handle=None, shard: Optional[Tuple[int, int]] = None, devices: Optional[Sequence[int]] = None,
                 keys: Optional[np.ndarray] = None):
        """devices: one replica per entry (entries may repeat); the library splits host-buffer batches
        over them (kg_snapshot_create_on).  Default: one replica on `device`.
        shard = (rank, nranks): keep only the rows of the nodes this rank owns (hash-sharded mode,
        keto_amd.sharded); every rank passes the same full tuple list.
        keys: ascending u64 order key per row (shard ids): kept so `apply` places inserted rows in order
        (kg_snapshot_create_ordered)."""
        L = _lib.load()
        self.interner = interner
        self.device = device
        self.program = program
        self.shard = shard
        self._keep = []
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
            return
        t = np.ascontiguousarray(tuples, dtype=np.uint32).reshape(-1, 6)
        d = _lib.kg_dict(interner.n_namespaces, interner.n_relations, interner.wildcard_rel)
        prog_c = self._prog(program)
        pc = C.byref(prog_c) if prog_c is not None else None
        self.devices = list(devices) if devices else [device]
        if shard is None and keys is not None:
            dv = np.asarray(self.devices, np.int32)
            k = np.ascontiguousarray(keys, dtype=np.uint64)
            rc = L.kg_snapshot_create_ordered(_ptr(t), _ptr(k), t.shape[0], C.byref(d), pc, _ptr(dv), len(dv),
                                              C.byref(self._h))
        elif shard is None:
            dv = np.asarray(self.devices, np.int32)
            rc = L.kg_snapshot_create_on(_ptr(t), t.shape[0], C.byref(d), pc, _ptr(dv), len(dv), C.byref(self._h))
        else:
            rc = L.kg_snapshot_create_shard(_ptr(t), t.shape[0], C.byref(d), pc, device, shard[0], shard[1],
                                            C.byref(self._h))
        _lib.check(rc, "kg_snapshot_create")

    def _prog(self, program: Optional[Program]):
        self._keep = []
        if program is None or program.empty:
            return None
        arrs = [np.ascontiguousarray(program.ns_has_rel, np.uint8), np.ascontiguousarray(program.rel_ns, np.uint32),
                np.ascontiguousarray(program.rel_rel, np.uint32), np.ascontiguousarray(program.rel_root, np.int32),
                np.ascontiguousarray(program.rw, np.int32).reshape(-1, 5), np.ascontiguousarray(program.child, np.int32)]
        self._keep = arrs
        return _lib.kg_rewrite_prog(len(arrs[0]), _ptr(arrs[0]), len(arrs[1]), _ptr(arrs[1]), _ptr(arrs[2]),
                                    _ptr(arrs[3]), arrs[4].shape[0], _ptr(arrs[4]), len(arrs[5]), _ptr(arrs[5]))

    def apply(self, ins: np.ndarray, dels: np.ndarray, ins_keys: Optional[np.ndarray] = None) -> "Snapshot":
        """kg_snapshot_apply: a new snapshot holding this one's rows minus every row equal to a tuple of
        `dels`, plus `ins` (uint32 (n, 6) tuple ids; ins_keys: their order keys).  This snapshot stays
        valid for readers; the next delta goes to the returned one."""
        L = _lib.load()
        it = self.interner
        a = np.ascontiguousarray(ins, dtype=np.uint32).reshape(-1, 6)
        dl = np.ascontiguousarray(dels, dtype=np.uint32).reshape(-1, 6)
        k = None if ins_keys is None else np.ascontiguousarray(ins_keys, dtype=np.uint64)
        d = _lib.kg_dict(it.n_namespaces, it.n_relations, it.wildcard_rel)
        new = Snapshot(None, it, self.program, self.device, _handle=C.c_void_p())
        prog_c = new._prog(self.program)
        pc = C.byref(prog_c) if prog_c is not None else None
        h = C.c_void_p()
        _lib.check(L.kg_snapshot_apply(self._h, _ptr(a) if len(a) else None, _ptr(k) if k is not None and len(a) else None,
                                       a.shape[0], _ptr(dl) if len(dl) else None, dl.shape[0], C.byref(d), pc,
                                       C.byref(h)), "kg_snapshot_apply")
        new._h = h
        new.devices = getattr(self, "devices", [self.device])
        return new

    def delete_matching(self, reqs: np.ndarray, want_keys: bool = False, with_stats: bool = False):
        """kg_snapshot_delete_matching (DeleteAllRelationTuples on the device): a new snapshot holding this
        one's rows minus every row that matches any of `reqs` (kg_row_query records, row_queries() builds
        them; `after` and `limit` are ignored; at most KG_DELETE_MAX_QUERIES).  Returns (snapshot or None
        when no row matched, matched u64 [n] per query, the deleted rows' order keys u64 [m] ascending or
        None without want_keys) and, with_stats, a dict of n_deleted / rows_scanned / kernel_ms.  This
        snapshot stays valid for readers; the next refresh goes to the returned one."""
        L = _lib.load()
        it = self.interner
        reqs = np.ascontiguousarray(reqs, dtype=_lib.ROW_QUERY_DTYPE).reshape(-1)
        n = reqs.shape[0]
        d = _lib.kg_dict(it.n_namespaces, it.n_relations, it.wildcard_rel)
        new = Snapshot(None, it, self.program, self.device, _handle=C.c_void_p())
        prog_c = new._prog(self.program)
        pc = C.byref(prog_c) if prog_c is not None else None
        h = C.c_void_p()
        buf = _lib.kg_delete_buf()
        _lib.check(L.kg_snapshot_delete_matching(self._h, _ptr(reqs) if n else None, n,
                                                 _lib.KG_DELETE_KEYS if want_keys else 0, C.byref(d), pc, C.byref(h),
                                                 C.byref(buf)), "kg_snapshot_delete_matching")
        try:
            m = int(buf.n_deleted)
            matched = np.ctypeslib.as_array(buf.matched, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
            keys = None
            if want_keys:
                keys = np.ctypeslib.as_array(buf.keys, shape=(m,)).copy() if m else np.zeros(0, np.uint64)
            stats = {"n_deleted": m, "rows_scanned": int(buf.rows_scanned), "kernel_ms": float(buf.kernel_ms)}
        finally:
            L.kg_delete_free(C.byref(buf))
        if h.value:
            new._h = h
            new.devices = getattr(self, "devices", [self.device])
        else:
            new = None
        return (new, matched, keys, stats) if with_stats else (new, matched, keys)

    @classmethod
    def synthetic(cls, n_tuples: int, seed: int = 20250131, device: int = 0, n_layers: int = 8,
                  max_degree: int = 100000, set_fraction: float = 0.25, doc_set_fraction: float = 0.5,
                  preset: int = 0, shard: Optional[Tuple[int, int]] = None,
                  devices: Optional[Sequence[int]] = None, doc_alpha: float = 0.0,
                  group_alpha: float = 0.0) -> "Snapshot":
        """Device-generated Drive-like graph (keto_amd/csrc/kg_synth.h); preset 0 = C2/C4, 1 = C3.
        shard = (rank, nranks): only this rank's rows (hash-sharded mode)."""
        from . import synth
        L = _lib.load()
        it = synth.interner()
        prog = synth.program(preset, it)
        snap = cls(None, it, device=device, _handle=C.c_void_p())
        p = _lib.kg_synth_params(n_tuples, seed, n_layers, max_degree, set_fraction, doc_set_fraction, preset, doc_alpha,
                                 group_alpha)
        prog_c = snap._prog(prog)
        h = C.c_void_p()
        pc = C.byref(prog_c) if prog_c is not None else None
        if shard is None:
            dv = np.asarray(list(devices) if devices else [device], np.int32)
            _lib.check(L.kg_snapshot_synthetic_on(C.byref(p), pc, _ptr(dv), len(dv), C.byref(h)),
                       "kg_snapshot_synthetic_on")
        else:
            _lib.check(L.kg_snapshot_synthetic_shard(C.byref(p), pc, device, shard[0], shard[1], C.byref(h)),
                       "kg_snapshot_synthetic_shard")
        snap._h = h
        snap.shard = shard
        snap.program = prog
        return snap

    @property
    def handle(self):
        return self._h

    def replicas(self) -> List[int]:
        """Devices of the snapshot's replicas (replica 0 first)."""
        L = _lib.load()
        n = L.kg_snapshot_replicas(self._h, None, 0)
        if n < 0:
            raise _lib.KetoGPUError(_lib.last_error())
        a = np.zeros(max(n, 1), np.int32)
        L.kg_snapshot_replicas(self._h, _ptr(a), n)
        return [int(x) for x in a[:n]]

    def info(self) -> dict:
        a = np.zeros(4, np.uint64)
        _lib.check(_lib.load().kg_snapshot_info(self._h, _ptr(a)), "kg_snapshot_info")
        return {"nodes": int(a[0]), "rows": int(a[1]), "set_edges": int(a[2]), "device_bytes": int(a[3])}

    def materialized(self) -> dict:
        """Rewrite materialisation counts (kg_snapshot_materialized): union nodes, of them new ids,
        check-row entries."""
        a = np.zeros(3, np.uint64)
        _lib.check(_lib.load().kg_snapshot_materialized(self._h, _ptr(a)), "kg_snapshot_materialized")
        return {"union_nodes": int(a[0]), "new_nodes": int(a[1]), "check_rows": int(a[2])}

    def holder_sig(self) -> int:
        """Bits per subject id of the holder signature table k_resolve prunes checks with (8 or 16), 0 when the
        snapshot has none: a namespace program, a hash shard, or KG_HSIG_BITS=0 at build."""
        rc = _lib.load().kg_snapshot_holder_sig(self._h)
        if rc < 0:
            raise _lib.KetoGPUError(_lib.last_error())
        return rc

    def tune(self, key: str, value: int) -> None:
        """Engine knobs (kg_snapshot_tune): include/ketogpu.h describes every key, its default and its range, from
        the table in keto_amd/csrc/kg_knobs.h.  Answers never depend on them; an unknown key or a value outside the
        range raises.  Build-time, from the environment: KG_ADJX_ORDER=0 lays adjx out in node order instead of
        hot-first; KG_HSIG_BITS (0, 8 or 16) is the width of the holder signatures (0: none)."""
        _lib.check(_lib.load().kg_snapshot_tune(self._h, key.encode(), int(value)), "kg_snapshot_tune")
        self.__dict__.setdefault("tuned", {})[key] = int(value)  # what the Python drivers need to know

    def synth_ids(self) -> dict:
        a = np.zeros(6, np.uint32)
        _lib.check(_lib.load().kg_synth_ids(self._h, _ptr(a)), "kg_synth_ids")
        return dict(zip(["n_docs", "n_groups", "n_users", "n_folders", "user_obj0", "folder_obj0"], map(int, a)))

    def export(self) -> np.ndarray:
        L = _lib.load()
        n = L.kg_snapshot_export(self._h, None, 0)
        if n < 0:
            raise _lib.KetoGPUError(_lib.last_error())
        out = np.zeros((n, 6), np.uint32)
        got = L.kg_snapshot_export(self._h, _ptr(out), n)
        if got != n:
            raise _lib.KetoGPUError(_lib.last_error())
        return out

    def rows(self, keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """GetRelationTuples(ns, obj, rel) for a (n,3) array of keys on the device snapshot
        (kg_snapshot_rows): returns (offsets[n+1], tuples (m,6) uint32), key i's rows in shard order at
        tuples[offsets[i]:offsets[i+1]]."""
        L = _lib.load()
        keys = np.asarray(keys, np.uint32).reshape(-1, 3)
        ks = np.zeros((keys.shape[0], 4), np.uint32)
        ks[:, :3] = keys[:, [0, 1, 2]]
        off = np.zeros(keys.shape[0] + 1, np.uint64)
        n = L.kg_snapshot_rows(self._h, _ptr(ks), keys.shape[0], _ptr(off), None, 0)
        if n < 0:
            raise _lib.KetoGPUError(_lib.last_error())
        out = np.zeros((max(n, 1), 6), np.uint32)
        if n:
            got = L.kg_snapshot_rows(self._h, _ptr(ks), keys.shape[0], _ptr(off), _ptr(out), n)
            if got != n:
                raise _lib.KetoGPUError(_lib.last_error())
        return off.astype(np.int64), out[:n]

    def query(self, reqs: np.ndarray, with_stats: bool = False):
        """GetRelationTuples on the device snapshot (kg_snapshot_query).  reqs: kg_row_query records
        (_lib.ROW_QUERY_DTYPE; row_queries() builds them).  Returns (rows (m,6) uint32, keys u64 [m],
        req_off u64 [n+1], next u64 [n], matched u64 [n]) and, with_stats, a dict of the call's
        rows_scanned / passes / kernel_ms: request i's page is rows[req_off[i]:req_off[i+1]], ascending
        order key; next[i] is the next call's `after`, 0 on the last page."""
        L = _lib.load()
        reqs = np.ascontiguousarray(reqs, dtype=_lib.ROW_QUERY_DTYPE).reshape(-1)
        n = reqs.shape[0]
        buf = _lib.kg_query_buf()
        _lib.check(L.kg_snapshot_query(self._h, _ptr(reqs) if n else None, n, C.byref(buf)), "kg_snapshot_query")
        try:
            m = int(buf.n_rows)
            off = np.ctypeslib.as_array(buf.req_off, shape=(n + 1,)).copy()
            if m:
                rows = np.ctypeslib.as_array(C.cast(buf.rows, C.POINTER(C.c_uint32)), shape=(m, 6)).copy()
                keys = np.ctypeslib.as_array(buf.keys, shape=(m,)).copy()
            else:
                rows, keys = np.zeros((0, 6), np.uint32), np.zeros(0, np.uint64)
            nxt = np.ctypeslib.as_array(buf.next, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
            matched = np.ctypeslib.as_array(buf.matched, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
            stats = {"rows_scanned": int(buf.rows_scanned), "passes": int(buf.passes), "kernel_ms": float(buf.kernel_ms)}
        finally:
            L.kg_query_free(C.byref(buf))
        return (rows, keys, off, nxt, matched, stats) if with_stats else (rows, keys, off, nxt, matched)

    def close(self) -> None:
        if self._h:
            _lib.load().kg_snapshot_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def queries_array(q6: np.ndarray, max_depths) -> np.ndarray:
    """(n,6) tuple ids + per-query max depth -> (n,7) uint32 kg_query rows."""
    q6 = np.asarray(q6, np.uint32).reshape(-1, 6)
    out = np.zeros((q6.shape[0], 7), np.uint32)
    out[:, :6] = q6
    out[:, 6] = np.broadcast_to(np.asarray(max_depths, np.int64), (q6.shape[0],)).astype(np.int32).view(np.uint32)
    return out


def row_queries(masks, tuples6, after=0, limit=100) -> np.ndarray:
    """kg_row_query records from per-request masks (KG_Q_* bits), (n,6) tuple ids, `after` keys and limits."""
    t = np.asarray(tuples6, np.uint32).reshape(-1, 6)
    out = np.zeros(t.shape[0], _lib.ROW_QUERY_DTYPE)
    out["mask"] = masks
    out["t"] = t
    out["after"] = after
    out["limit"] = limit
    return out


class Engine:
    """check.Engine: permission checks against a snapshot."""

    def __init__(self, snapshot: Snapshot, config: Optional[Config] = None):
        self.snapshot = snapshot
        self.config = config or Config()
        self.last_stats: Optional[dict] = None

    # ---- batched (the hot path)
    def batch_check_ids(self, q: np.ndarray, with_stats: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """q: (n,7) uint32 kg_query rows.  Returns (result u8 [0 not member, 1 member, 2 error], err u32)."""
        q = np.ascontiguousarray(q, np.uint32).reshape(-1, 7)
        n = q.shape[0]
        out = np.zeros(n, np.uint8)
        err = np.zeros(n, np.uint32)
        st = _lib.kg_stats()
        rc = _lib.load().kg_check_batch(self.snapshot.handle, _ptr(q), n, self.config.max_read_depth, _ptr(out),
                                        _ptr(err), C.byref(st) if with_stats else None)
        _lib.check(rc, "kg_check_batch")
        self.last_stats = st.as_dict() if with_stats else None
        return out, err

    def batch_check_packed(self, q: np.ndarray, err_cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, int]:
        """The narrow boundary (kg_check_batch_packed): q (n,7) uint32 kg_query rows are packed to 16 B
        (pack_queries = the header's kg_pack_query), answers come back as bytes and the error codes as
        (index, code) pairs of the KG_ERROR answers only.  Returns (result u8, pairs (k, 2) u32, n_err)."""
        pk = _lib.pack_queries(q)
        n = pk.shape[0]
        cap = n if err_cap is None else int(err_cap)
        out = np.zeros(n, np.uint8)
        idx = np.zeros(max(cap, 1), np.uint32)
        code = np.zeros(max(cap, 1), np.uint32)
        n_err = C.c_size_t(0)
        rc = _lib.load().kg_check_batch_packed(self.snapshot.handle, _ptr(pk), n, self.config.max_read_depth, _ptr(out),
                                               _ptr(idx) if cap else None, _ptr(code) if cap else None, cap,
                                               C.byref(n_err), None)
        _lib.check(rc, "kg_check_batch_packed")
        k = min(cap, int(n_err.value))
        return out, np.stack([idx[:k], code[:k]], axis=1), int(n_err.value)

    def batch_check(self, tuples: Sequence[RelationTuple], max_depths) -> Tuple[List[bool], List[Optional[CheckError]]]:
        """BatchCheck(ctx, []*RelationTuple, maxDepth []int) ([]bool, []error) -- SURVEY.md 8b."""
        it = self.snapshot.interner
        q = queries_array(np.asarray([it.tuple_ids(t) for t in tuples], np.uint32).reshape(-1, 6), max_depths)
        out, err = self.batch_check_ids(q)
        allowed = [bool(o == _lib.KG_IS_MEMBER) for o in out]
        errs = [CheckError(int(e)) if o == _lib.KG_ERROR else None for o, e in zip(out, err)]
        return allowed, errs

    # ---- single-query API of the reference
    def check_relation_tuple(self, t: RelationTuple, rest_depth: int, with_tree: bool = True) -> Result:
        """CheckRelationTuple (engine.go:65-80): membership, error, and for a member the tree of the
        branch that answered it (keto_amd/explain.py)."""
        allowed, errs = self.batch_check([t], [rest_depth])
        if errs[0] is not None:
            return Result(MEMBERSHIP_UNKNOWN, errs[0])
        if not allowed[0]:
            return Result(NOT_MEMBER)
        tree = None
        if with_tree:
            tree = self.check_tree(t, rest_depth)
        return Result(IS_MEMBER, None, tree)

    def check_tree(self, t: RelationTuple, rest_depth: int):
        """The tree of a member check, built inside the library (kg_check_tree: the walk over GPU
        sub-check answers and row reads; keto_amd/explain.py is its CPU-tested restatement)."""
        import ctypes as C
        from .ketoapi import CheckTree, TREE_INTERSECTION
        from .namespace import HIDDEN_TTU_PREFIX
        it = self.snapshot.interner
        L = _lib.load()
        ids = [int(x) for x in it.tuple_ids(t)]
        q = (C.c_uint32 * 7)(*ids, rest_depth & 0xFFFFFFFF)
        hidden = [r for r in range(it.n_relations) if it.rel_name(r).startswith(HIDDEN_TTU_PREFIX)]
        hid = (C.c_uint32 * max(1, len(hidden)))(*hidden)
        n = C.c_size_t(0)
        res, err = C.c_uint8(0), C.c_uint32(0)
        cap = 64
        while True:
            buf = (_lib.kg_check_node * cap)()
            rc = L.kg_check_tree(self.snapshot.handle, q, self.config.max_read_depth, hid, len(hidden), buf, cap,
                                 C.byref(n), C.byref(res), C.byref(err))
            if rc == -3 and n.value > cap:
                cap = n.value
                continue
            _lib.check(rc, "kg_check_tree")
            break
        if res.value != _lib.KG_IS_MEMBER:
            return None
        pos = 0

        def build():
            nonlocal pos
            r = buf[pos]
            pos += 1
            kids = [build() for _ in range(r.n_children)]
            tup = it.relation_tuple((r.t.ns, r.t.obj, r.t.rel, r.t.sns, r.t.sobj, r.t.srel)) if r.has_tuple else None
            typ = _lib.KG_CTREE[r.type]
            return CheckTree(TREE_INTERSECTION if typ == "intersection" else typ, tup, kids)

        return build()

    def check_is_member(self, t: RelationTuple, rest_depth: int) -> bool:
        """CheckIsMember (engine.go:54-60): membership only (no tree)."""
        allowed, errs = self.batch_check([t], [rest_depth])
        if errs[0] is not None:
            raise errs[0]
        return allowed[0]

    # ---- reverse lookup (no reference counterpart: OpenFGA ListObjects / SpiceDB LookupResources)
    def lookup_objects_ids(self, reqs: np.ndarray,
                           with_stats: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """reqs: (n,6) uint32 kg_lookup rows (ns, rel, sns, sobj, srel, max_depth).  Returns (req_off u64
        [n+1], objs u32 ascending per request, err_code u32 [n], n_errors u64 [n]): request i's objects are
        objs[req_off[i]:req_off[i+1]] -- the objects of its namespace whose check is IsMember.  with_stats:
        last_stats holds the call's counters; a request on a boolean rewrite (formula mode) counts its
        checks in candidates and nothing in exact."""
        return self._lookup("kg_lookup_objects", np.ascontiguousarray(reqs, np.uint32).reshape(-1, 6), with_stats)

    def _lookup(self, call: str, reqs: np.ndarray, with_stats: bool):
        """One kg_lookup_objects / kg_lookup_subjects call: the four output arrays copied out of the
        kg_lookup_buf, its counters in last_stats."""
        n = reqs.shape[0]
        buf = _lib.kg_lookup_buf()
        L = _lib.load()
        _lib.check(getattr(L, call)(self.snapshot.handle, _ptr(reqs) if n else None, n, self.config.max_read_depth,
                                    C.byref(buf)), call)
        try:
            m = int(buf.n_objs)
            off = np.ctypeslib.as_array(buf.req_off, shape=(n + 1,)).copy()
            objs = np.ctypeslib.as_array(buf.objs, shape=(m,)).copy() if m else np.zeros(0, np.uint32)
            err = np.ctypeslib.as_array(buf.err_code, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
            nerr = np.ctypeslib.as_array(buf.n_errors, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
            self.last_stats = {k: getattr(buf, k) for k in ("n_objs", "exact", "candidates", "confirmed",
                                                            "reverse_edges", "levels", "kernel_ms")} if with_stats else None
        finally:
            L.kg_lookup_free(C.byref(buf))
        return off, objs, err, nerr

    def lookup_objects(self, namespace: str, relation: str, subject, rest_depth: int) -> List[str]:
        """The objects of `namespace` on which `subject` (a SubjectSet or a subject-id string) has
        `relation`, sorted by name.  Raises CheckError when the check of any object ends in an error."""
        it = self.snapshot.interner
        if isinstance(subject, SubjectSet):
            sub = list(it.subject_set_ids(subject))
        else:
            sub = [SUBJECT_ID, it.obj_id(subject), 0]
        row = np.asarray([it.ns_id(namespace), it.rel_id(relation), *sub, np.int32(rest_depth).view(np.uint32)],
                         np.uint32)
        _, objs, err, nerr = self.lookup_objects_ids(row)
        if int(nerr[0]):
            raise CheckError(int(err[0]))
        return sorted(it.obj_name(int(o)) for o in objs)

    # ---- subject lookup (OpenFGA ListUsers / SpiceDB LookupSubjects)
    def lookup_subjects_ids(self, reqs: np.ndarray,
                            with_stats: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """reqs: (n,4) uint32 kg_lookup_subj rows (ns, obj, rel, max_depth).  Returns (req_off u64 [n+1],
        subject ids u32 ascending per request, err_code u32 [n], n_errors u64 [n]): request i's subject ids
        are ids[req_off[i]:req_off[i+1]] -- the subject ids of the snapshot's tuples whose check on the
        request's object is IsMember.  last_stats as lookup_objects_ids."""
        return self._lookup("kg_lookup_subjects", np.ascontiguousarray(reqs, np.uint32).reshape(-1, 4), with_stats)

    def lookup_subjects(self, namespace: str, object: str, relation: str, rest_depth: int) -> List[str]:
        """The subject ids that have `relation` on `namespace:object`, sorted by name.  Raises CheckError
        when the check of any subject id ends in an error."""
        it = self.snapshot.interner
        row = np.asarray([it.ns_id(namespace), it.obj_id(object), it.rel_id(relation),
                          np.int32(rest_depth).view(np.uint32)], np.uint32)
        _, ids, err, nerr = self.lookup_subjects_ids(row)
        if int(nerr[0]):
            raise CheckError(int(err[0]))
        return sorted(it.obj_name(int(i)) for i in ids)

    # ---- subject-set lookup: the subject sets of one (namespace, relation) that hold a relation on an object
    def lookup_subject_sets_ids(self, reqs: np.ndarray,
                                with_stats: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """reqs: (n,6) uint32 kg_lookup_subj_set rows (ns, obj, rel, sns, srel, max_depth).  Returns (req_off u64
        [n+1], ids u32 ascending per request, err_code u32 [n], n_errors u64 [n]): request i's ids are the
        object ids o of the subject sets sns:o#srel that occur as a tuple's subject and whose check on the
        request's object is IsMember -- with sns == KG_SUBJECT_ID, lookup_subjects_ids' subject ids.
        last_stats as lookup_objects_ids."""
        return self._lookup("kg_lookup_subject_sets", np.ascontiguousarray(reqs, np.uint32).reshape(-1, 6), with_stats)

    def lookup_subject_sets_page_ids(self, reqs: np.ndarray, pages: np.ndarray, with_stats: bool = False):
        """reqs as lookup_subject_sets_ids; pages and the result as lookup_objects_page_ids."""
        return self._lookup_page("kg_lookup_subject_sets_page", np.ascontiguousarray(reqs, np.uint32).reshape(-1, 6),
                                 pages, with_stats)

    def _subject_set_row(self, namespace: str, object: str, relation: str, subject_namespace: str,
                         subject_relation: str, rest_depth: int) -> Optional[np.ndarray]:
        """The request row, or None where the filter names a namespace or relation the snapshot has never seen
        (nothing is interned for it: no tuple's subject can match)."""
        it = self.snapshot.interner
        try:
            sns, srel = it.ns_id(subject_namespace, create=False), it.rel_id(subject_relation, create=False)
        except KeyError:
            return None
        return np.asarray([it.ns_id(namespace), it.obj_id(object), it.rel_id(relation), sns, srel,
                           np.int32(rest_depth).view(np.uint32)], np.uint32)

    def lookup_subject_sets(self, namespace: str, object: str, relation: str, subject_namespace: str,
                            subject_relation: str, rest_depth: int) -> List[SubjectSet]:
        """The subject sets subject_namespace:*#subject_relation that have `relation` on `namespace:object`,
        directly or through nesting, sorted by object name.  Raises CheckError as lookup_subjects."""
        row = self._subject_set_row(namespace, object, relation, subject_namespace, subject_relation, rest_depth)
        if row is None:
            return []
        _, ids, err, nerr = self.lookup_subject_sets_ids(row)
        if int(nerr[0]):
            raise CheckError(int(err[0]))
        it = self.snapshot.interner
        return [SubjectSet(subject_namespace, o, subject_relation) for o in sorted(it.obj_name(int(i)) for i in ids)]

    def lookup_subject_sets_page(self, namespace: str, object: str, relation: str, subject_namespace: str,
                                 subject_relation: str, rest_depth: int, frm: int = 0,
                                 limit: int = 100) -> Tuple[List[SubjectSet], Optional[int]]:
        """One page of lookup_subject_sets in id order, as lookup_objects_page."""
        row = self._subject_set_row(namespace, object, relation, subject_namespace, subject_relation, rest_depth)
        if row is None:
            return [], None
        _, ids, err, nerr, nxt = self.lookup_subject_sets_page_ids(row, np.asarray([[frm, limit]], np.uint32))
        names, nx = self._page_names(ids, err, nerr, nxt)
        return [SubjectSet(subject_namespace, o, subject_relation) for o in names], nx

    # ---- paged lookups: the next `limit` ids from a cursor (kg_lookup_objects_page / kg_lookup_subjects_page)
    def lookup_objects_page_ids(self, reqs: np.ndarray, pages: np.ndarray, with_stats: bool = False):
        """reqs as lookup_objects_ids; pages: (n,2) uint32 (from, limit >= 1).  Returns (req_off, objs, err_code,
        n_errors, next): request i's page is the first `limit` ids >= `from` of its unpaged answer; next[i] is
        the next call's `from` or KG_LOOKUP_END; err_code / n_errors are about the ids in [from, next).
        last_stats additionally carries `rounds`."""
        return self._lookup_page("kg_lookup_objects_page", np.ascontiguousarray(reqs, np.uint32).reshape(-1, 6), pages,
                                 with_stats)

    def lookup_subjects_page_ids(self, reqs: np.ndarray, pages: np.ndarray, with_stats: bool = False):
        """reqs as lookup_subjects_ids; pages and the result as lookup_objects_page_ids."""
        return self._lookup_page("kg_lookup_subjects_page", np.ascontiguousarray(reqs, np.uint32).reshape(-1, 4), pages,
                                 with_stats)

    def _lookup_page(self, call: str, reqs: np.ndarray, pages: np.ndarray, with_stats: bool):
        n = reqs.shape[0]
        pages = np.ascontiguousarray(pages, np.uint32).reshape(-1, 2)
        if pages.shape[0] != n:
            raise ValueError("one page per request")
        out = _lib.kg_lookup_pages()
        L = _lib.load()
        _lib.check(getattr(L, call)(self.snapshot.handle, _ptr(reqs) if n else None, _ptr(pages) if n else None, n,
                                    self.config.max_read_depth, C.byref(out)), call)
        try:
            buf = out.list
            m = int(buf.n_objs)
            off = np.ctypeslib.as_array(buf.req_off, shape=(n + 1,)).copy()
            objs = np.ctypeslib.as_array(buf.objs, shape=(m,)).copy() if m else np.zeros(0, np.uint32)
            err = np.ctypeslib.as_array(buf.err_code, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
            nerr = np.ctypeslib.as_array(buf.n_errors, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
            nxt = np.ctypeslib.as_array(out.next, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
            if with_stats:
                self.last_stats = {k: getattr(buf, k) for k in ("n_objs", "exact", "candidates", "confirmed",
                                                                "reverse_edges", "levels", "kernel_ms")}
                self.last_stats["rounds"] = int(out.rounds)
            else:
                self.last_stats = None
        finally:
            L.kg_lookup_pages_free(C.byref(out))
        return off, objs, err, nerr, nxt

    def _page_names(self, objs, err, nerr, nxt) -> Tuple[List[str], Optional[int]]:
        if int(nerr[0]):
            raise CheckError(int(err[0]))
        it = self.snapshot.interner
        return [it.obj_name(int(o)) for o in objs], None if int(nxt[0]) == _lib.KG_LOOKUP_END else int(nxt[0])

    def lookup_objects_page(self, namespace: str, relation: str, subject, rest_depth: int, frm: int = 0,
                            limit: int = 100) -> Tuple[List[str], Optional[int]]:
        """One page of lookup_objects in id order: (the names of the first `limit` objects with id >= frm, the
        next page's frm or None at the end).  Raises CheckError only when an object of the page's id range
        [frm, next) ends in an error."""
        it = self.snapshot.interner
        if isinstance(subject, SubjectSet):
            sub = list(it.subject_set_ids(subject))
        else:
            sub = [SUBJECT_ID, it.obj_id(subject), 0]
        row = np.asarray([it.ns_id(namespace), it.rel_id(relation), *sub, np.int32(rest_depth).view(np.uint32)],
                         np.uint32)
        _, objs, err, nerr, nxt = self.lookup_objects_page_ids(row, np.asarray([[frm, limit]], np.uint32))
        return self._page_names(objs, err, nerr, nxt)

    def lookup_subjects_page(self, namespace: str, object: str, relation: str, rest_depth: int, frm: int = 0,
                             limit: int = 100) -> Tuple[List[str], Optional[int]]:
        """One page of lookup_subjects in id order, as lookup_objects_page."""
        it = self.snapshot.interner
        row = np.asarray([it.ns_id(namespace), it.obj_id(object), it.rel_id(relation),
                          np.int32(rest_depth).view(np.uint32)], np.uint32)
        _, ids, err, nerr, nxt = self.lookup_subjects_page_ids(row, np.asarray([[frm, limit]], np.uint32))
        return self._page_names(ids, err, nerr, nxt)


    # ---- access masks: a lookup's answer as bitmap rows in HBM, and the ranked select through them
    def _mask_device(self):
        import torch
        return torch.device("cuda", getattr(self.snapshot, "devices", [self.snapshot.device])[0])

    def _mask_call(self, call: str, reqs: np.ndarray, base: int, n_bits: Optional[int], out, with_stats: bool):
        import torch
        dev = self._mask_device()
        n = reqs.shape[0]
        if n_bits is None:
            n_bits = self.snapshot.interner.n_objects
        if out is None:
            out = torch.empty((n, (int(n_bits) + 31) // 32), dtype=torch.int32, device=dev)
        elif out.dtype != torch.int32 or out.device != dev or out.dim() != 2 or out.shape[0] != n \
                or not out.is_contiguous():
            raise ValueError(f"out: a contiguous int32 tensor of {n} rows on {dev}")
        buf = _lib.kg_lookup_mask_buf()
        L = _lib.load()
        _lib.check(getattr(L, call)(self.snapshot.handle, _ptr(reqs) if n else None, n, self.config.max_read_depth,
                                    int(base), int(n_bits), C.c_void_p(out.data_ptr()), out.shape[1], C.byref(buf),
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), call)
        try:
            n_set = np.ctypeslib.as_array(buf.n_set, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
            err = np.ctypeslib.as_array(buf.err_code, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
            nerr = np.ctypeslib.as_array(buf.n_errors, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
            self.last_stats = {k: getattr(buf, k) for k in ("exact", "candidates", "confirmed", "reverse_edges",
                                                            "levels", "kernel_ms")} if with_stats else None
        finally:
            L.kg_lookup_mask_free(C.byref(buf))
        return out, n_set, err, nerr

    def lookup_objects_mask_ids(self, reqs: np.ndarray, base: int = 0, n_bits: Optional[int] = None, out=None,
                                with_stats: bool = False):
        """kg_lookup_objects_mask_device: reqs as lookup_objects_ids.  Returns (mask, n_set u64 [n], err_code u32
        [n], n_errors u64 [n]): mask is a torch.int32 tensor [n, row_words] on the snapshot's device whose row i
        has bit (o - base) & 31 of word (o - base) >> 5 set exactly for the objects o of request i's answer with
        base <= o < base + n_bits (None: the interner's object-id count); n_set[i] is the row's popcount;
        err_code, n_errors and last_stats are lookup_objects_ids' (the range limits what is written, not what
        is checked).  out: a caller tensor [n, row_words >= ceil(n_bits / 32)] to write instead of a new one;
        work the current torch stream has enqueued on it is waited for.  The mask is complete on return."""
        return self._mask_call("kg_lookup_objects_mask_device", np.ascontiguousarray(reqs, np.uint32).reshape(-1, 6),
                               base, n_bits, out, with_stats)

    def lookup_subject_sets_mask_ids(self, reqs: np.ndarray, base: int = 0, n_bits: Optional[int] = None, out=None,
                                     with_stats: bool = False):
        """kg_lookup_subject_sets_mask_device: reqs as lookup_subject_sets_ids (sns == KG_SUBJECT_ID: the row is
        over subject ids); the result as lookup_objects_mask_ids."""
        return self._mask_call("kg_lookup_subject_sets_mask_device",
                               np.ascontiguousarray(reqs, np.uint32).reshape(-1, 6), base, n_bits, out, with_stats)

    def object_mask(self, namespace: str, relation: str, subject, rest_depth: int):
        """lookup_objects as a 1-D torch.int32 bitmap over the interner's object ids, on the snapshot's device:
        bit o & 31 of word o >> 5 is set when `subject` has `relation` on the object with id o.  Raises
        CheckError when the check of any object ends in an error."""
        it = self.snapshot.interner
        if isinstance(subject, SubjectSet):
            sub = list(it.subject_set_ids(subject))
        else:
            sub = [SUBJECT_ID, it.obj_id(subject), 0]
        row = np.asarray([it.ns_id(namespace), it.rel_id(relation), *sub, np.int32(rest_depth).view(np.uint32)],
                         np.uint32)
        mask, _, err, nerr = self.lookup_objects_mask_ids(row)
        if int(nerr[0]):
            raise CheckError(int(err[0]))
        return mask[0]

    def mask_select(self, mask, cand, limit: int, base: int = 0, n_bits: Optional[int] = None):
        """kg_mask_select_device: cand is a torch.int32 tensor [n, k_in] of ranked ids (-1 = KG_LOOKUP_END pads a
        row), mask [n, row_words] one bitmap row per row of cand (a 1-D mask and a 1-D cand are one row).
        Returns (out int32 [n, limit], count int32 [n]): out[i] holds the first `limit` ids of cand[i] whose bit
        is set, in their order, then -1; count[i] is the number of such ids in the whole row.  n_bits None: the
        interner's object-id count, or the bits the rows hold if that is fewer.  Enqueued on the current torch
        stream; nothing is copied to the host."""
        import torch
        dev = self._mask_device()
        mask = mask.unsqueeze(0) if mask.dim() == 1 else mask
        cand = cand.unsqueeze(0) if cand.dim() == 1 else cand
        for name, t in (("mask", mask), ("cand", cand)):
            if t.dtype != torch.int32 or t.device != dev or t.dim() != 2 or not t.is_contiguous():
                raise ValueError(f"{name}: a contiguous 2-D int32 tensor on {dev}")
        n, k_in = cand.shape
        if mask.shape[0] != n:
            raise ValueError("one mask row per row of candidates")
        if n_bits is None:  # the ids handed out since the mask was written have no bit in it: they are not allowed
            n_bits = min(self.snapshot.interner.n_objects, 32 * mask.shape[1])
        out = torch.empty((n, max(int(limit), 0)), dtype=torch.int32, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        cur = torch.cuda.current_stream(dev)
        # the library takes a NULL stream for its own: on torch's default stream the select runs on a side
        # stream of this engine that is ordered behind and ahead of the current one
        side = None
        if cur.cuda_stream == 0:
            side = getattr(self, "_mask_side", None)
            if side is None:
                side = self._mask_side = torch.cuda.Stream(dev)
            side.wait_stream(cur)
        run = side if side is not None else cur
        _lib.check(_lib.load().kg_mask_select_device(
            self.snapshot.handle, C.c_void_p(mask.data_ptr()), mask.shape[1], int(base), int(n_bits),
            C.c_void_p(cand.data_ptr()), n, k_in, int(limit), C.c_void_p(out.data_ptr()), C.c_void_p(count.data_ptr()),
            C.c_void_p(run.cuda_stream)), "kg_mask_select_device")
        if side is not None:
            cur.wait_stream(side)
            for t in (mask, cand, out, count):
                t.record_stream(side)
        return out, count


class ExpandEngine:
    """expand.Engine: subject-set trees."""

    def __init__(self, snapshot: Snapshot, config: Optional[Config] = None):
        self.snapshot = snapshot
        self.config = config or Config()

    def build_trees_ids(self, roots: np.ndarray, device: bool = False) -> List[Optional[np.ndarray]]:
        """roots: (n,4) uint32 kg_set rows (sns, sobj, srel, max_depth).  Returns per root the pre-order
        records (m, 6) = (type, is_set, ns, obj, rel, n_children), or None for a nil tree.  device: through
        kg_expand_batch_device (roots and trees in HBM; the trees are copied back here to be returned)."""
        roots = np.ascontiguousarray(roots, np.uint32).reshape(-1, 4)
        buf = _lib.kg_tree_buf()
        L = _lib.load()
        if device:
            import torch
            dev = torch.device("cuda", self.snapshot.device)
            droots = torch.from_numpy(roots.view(np.int32)).to(dev)
            rc = L.kg_expand_batch_device(self.snapshot.handle, C.c_void_p(droots.data_ptr()), roots.shape[0],
                                          self.config.max_read_depth, C.byref(buf),
                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            _lib.check(rc, "kg_expand_batch_device")
        else:
            rc = L.kg_expand_batch(self.snapshot.handle, _ptr(roots), roots.shape[0], self.config.max_read_depth,
                                   C.byref(buf))
            _lib.check(rc, "kg_expand_batch")
        try:
            n = int(buf.n_nodes)
            if device:
                recs = np.zeros((n, 5), np.uint32)
                offs = np.zeros(roots.shape[0] + 1, np.uint64)
                _lib.device_to_host(recs, buf.nodes, n * 20)
                _lib.device_to_host(offs, buf.root_off, offs.nbytes)
            else:
                recs = np.ctypeslib.as_array(C.cast(buf.nodes, C.POINTER(C.c_uint32)), shape=(n * 5,)).reshape(n, 5) \
                    if n else np.zeros((0, 5), np.uint32)
                offs = np.ctypeslib.as_array(buf.root_off, shape=(roots.shape[0] + 1,)).copy()
            out: List[Optional[np.ndarray]] = []
            for r in range(roots.shape[0]):
                a, b = int(offs[r]), int(offs[r + 1])
                if a == b:
                    out.append(None)
                    continue
                seg = recs[a:b]
                rec = np.zeros((b - a, 6), np.int64)
                rec[:, 0] = seg[:, 0] & 0xFF
                rec[:, 1] = (seg[:, 0] >> 8) & 0xFF
                rec[:, 2:5] = seg[:, 1:4]
                rec[:, 5] = seg[:, 4]
                out.append(rec)
            return out
        finally:
            L.kg_tree_free(C.byref(buf))

    def build_tree(self, subject, rest_depth: int) -> Optional[Tree]:
        """BuildTree(ctx, subject, restDepth): subject is a SubjectSet or a subject-id string."""
        it = self.snapshot.interner
        if isinstance(subject, SubjectSet):
            row = [*it.subject_set_ids(subject), rest_depth]
        else:
            row = [SUBJECT_ID, it.obj_id(subject), 0, rest_depth]
        row[3] = np.int32(row[3]).view(np.uint32)
        rec = self.build_trees_ids(np.asarray([row], np.uint32))[0]
        return records_to_tree(rec, it)


def records_to_tree(rec: Optional[np.ndarray], it: Interner) -> Optional[Tree]:
    if rec is None or len(rec) == 0:
        return None
    pos = 0

    def walk() -> Tree:
        nonlocal pos
        r = rec[pos]
        pos += 1
        t = Tree(TREE_UNION if int(r[0]) == 1 else TREE_LEAF, it.subject_from_ids(bool(r[1]), int(r[2]), int(r[3]),
                                                                                  int(r[4])))
        for _ in range(int(r[5])):
            t.children.append(walk())
        return t

    return walk()


class Registry:
    """Test/embedding convenience mirroring driver.Registry's engine wiring
    (internal/driver/registry_default.go:180-192): tuples + namespaces -> snapshot + engines."""

    def __init__(self, tuples: Sequence[RelationTuple], namespaces: Sequence[Namespace] = (), max_read_depth: int = 5,
                 device: int = 0, interner: Optional[Interner] = None, devices: Optional[Sequence[int]] = None):
        self.interner = interner or Interner()
        self.config = Config(max_read_depth, list(namespaces))
        self.program = compile_program(list(namespaces), self.interner)
        arr = self.interner.tuples_array(tuples)
        self.snapshot = Snapshot(arr, self.interner, self.program, device, devices=devices)
        self.mapper = Mapper(self.interner, list(namespaces) if namespaces else None)

    def permission_engine(self) -> Engine:
        return Engine(self.snapshot, self.config)

    def expand_engine(self) -> ExpandEngine:
        return ExpandEngine(self.snapshot, self.config)
