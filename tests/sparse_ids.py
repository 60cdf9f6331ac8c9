"""Any dense test case on chosen ids: per id space (namespace, relation, object / subject id) a strictly
increasing map dense id -> chosen id, applied to tuples, query rows, lookup rows, expand roots, listing
requests and the namespace program.  Monotone maps keep id-ordered answers in order, so the dense answers
mapped through `IdMaps.obj` must equal the answers on the chosen ids.

`order_objects` first renumbers the dense object ids (still dense) so that a chosen id comes first and
another last: the strictly increasing pool then puts 0 and 0x7FFFFFFE on ids that matter.

An example with 4 objects, object 2 wanted at 0 and object 1 at the top:
    perm     = order_objects(4, first=2, last=1)   -> [1, 3, 0, 2]     dense id -> renumbered dense id
    obj_pool = [0, 31, 0xFFFF, 0x7FFFFFFE]                             renumbered dense id -> chosen id, increasing
    obj      = obj_pool[perm]                      -> [31, 0x7FFFFFFE, 0, 0xFFFF]   dense id -> chosen id
The "dense" layout has the same perm and obj_pool = [0, 1, 2, 3]: its answers are in renumbered dense ids, and
lift() of the sparse maps (obj = obj_pool, rel = rel_pool) carries them to the chosen ids in the same order.

Also here, because both GPU modules use them: the three knob sets of the check tiers and the packed device call."""
import copy
from types import SimpleNamespace

import numpy as np

SUBJECT_ID = 0xFFFFFFFF
NONE = 0xFFFFFFFF  # kg_dict.wildcard_rel: no wildcard relation
TOP = 0x7FFFFFFE   # the largest object / subject id
OBJ_FIXED = [0, 1, 31, 32, 63, 64, 0xFFFF, 0x10000, 0xFFFFFF, 0x1000000, 0x7FFFFFFD, TOP]
EDGE = [0, 255, 256, 4094, 4095, 65534]
PACK = [0, 255, 256, 4094]
NIBBLE = [0, 15, 16, 4094]

# layout -> (namespace pool, relation pool): `fixed` ids every map holds, the rest random below `top`
LAYOUTS = {
    "dense": None,
    "top-subject": (dict(fixed=EDGE, top=65534), dict(fixed=EDGE, top=65534)),   # no program: no table
    "top-object": (dict(fixed=EDGE, top=65534), dict(fixed=EDGE, top=65534)),
    "packed": (dict(fixed=PACK, top=4094), dict(fixed=PACK, top=4094)),          # no program
    "wide-ns": (dict(fixed=EDGE, top=65534), dict(fixed=[0, 63], top=63)),
    "wide-rel": (dict(fixed=[0, 63], top=63), dict(fixed=EDGE, top=65534)),
    "packed-ns": (dict(fixed=PACK, top=4094), dict(fixed=[0, 255, 256, 1023], top=1023)),
    "packed-rel": (dict(fixed=[0, 255, 256, 1023], top=1023), dict(fixed=NIBBLE + [255, 256], top=4094)),
}
PROGRAM_LAYOUTS = ["wide-ns", "wide-rel", "packed-ns", "packed-rel"]
WILDCARDS = ["zero", "top", "none"]


def pool(rng, n, fixed, top):
    """n ascending ids: as many of `fixed` as fit (the lowest and the highest first), random ones below top."""
    fixed = sorted(fixed)
    keep = ([fixed[0], fixed[-1]] + fixed[1:-1])[:n]
    ids = set(keep)
    while len(ids) < n:
        ids.add(int(rng.integers(1, top)))
    return np.asarray(sorted(ids), np.uint32)


def order_objects(n_obj, first, last):
    """dense id -> dense id with `first` at 0 and `last` at n_obj - 1, the others in their order."""
    rest = [i for i in range(n_obj) if i not in (first, last)]
    perm = np.zeros(n_obj, np.uint32)
    perm[[first] + rest + [last]] = np.arange(n_obj, dtype=np.uint32)
    return perm


class IdMaps:
    """ns / rel / obj: dense id -> chosen id.  Dense relation 0 is the wildcard "..." (Interner reserves it):
    wildcard "zero" leaves it in the increasing map, "top" gives it the layout's highest relation id, "none"
    takes it out (kg_dict.wildcard_rel = 0xFFFFFFFF; the graph must hold no "..." tuple) so that relation
    id 0 is an ordinary relation."""

    def __init__(self, layout, n_ns, n_rel, n_obj, seed=0, wildcard="zero", perm=None):
        rng = np.random.default_rng(seed)
        self.layout, self.perm = layout, np.arange(n_obj, dtype=np.uint32) if perm is None else perm
        if LAYOUTS[layout] is None:
            self.ns, rel, self.obj_pool = np.arange(n_ns, dtype=np.uint32), np.arange(n_rel), np.arange(n_obj)
        else:
            pn, pr = LAYOUTS[layout]
            self.ns, rel = pool(rng, n_ns, **pn), pool(rng, n_rel, **pr)
            self.obj_pool = pool(rng, n_obj, OBJ_FIXED, TOP)
        self.rel_pool = np.asarray(rel, np.uint32)  # strictly increasing
        self.rel = self.rel_pool.copy()
        self.wildcard = int(self.rel[0])
        if wildcard == "top":
            self.rel = np.concatenate([self.rel_pool[-1:], self.rel_pool[:-1]])
            self.wildcard = int(self.rel[0])
        elif wildcard == "none":  # dense relation 1 -> id 0; "..." -> the second id, which no row may use
            self.rel[0], self.rel[1], self.wildcard = self.rel_pool[1], self.rel_pool[0], NONE
        self.obj_pool = np.asarray(self.obj_pool, np.uint32)
        self.obj = self.obj_pool[self.perm]

    def lift(self):
        """The strictly increasing maps alone, (renumbered) dense id -> chosen id: what dense answers go through."""
        up = copy.copy(self)
        up.rel, up.obj = self.rel_pool, self.obj_pool
        return up

    def _cols(self, a, ns=(), rel=(), obj=(), sns=None, srel=None):
        a = np.asarray(a, np.uint32)
        out = a.copy().reshape(-1, a.shape[-1])
        for c in ns:
            out[:, c] = self.ns[out[:, c]]
        for c in rel:
            out[:, c] = self.rel[out[:, c]]
        for c in obj:
            out[:, c] = self.obj[out[:, c]]
        if sns is not None:  # a subject: a set (sns, srel mapped) or a subject id (marker and 0 kept)
            is_set = a.reshape(out.shape)[:, sns] != SUBJECT_ID
            out[is_set, sns] = self.ns[out[is_set, sns]]
            if srel is not None:
                out[is_set, srel] = self.rel[out[is_set, srel]]
        return out.reshape(a.shape)

    def tuples(self, a):      # (n, 6 or 7): ns obj rel sns sobj srel [depth]
        return self._cols(a, ns=[0], rel=[2], obj=[1, 4], sns=3, srel=5)

    def lookup_objects(self, a):       # (n,6) kg_lookup: ns rel sns sobj srel depth
        return self._cols(a, ns=[0], rel=[1], obj=[3], sns=2, srel=4)

    def lookup_subjects(self, a):      # (n,4) kg_lookup_subj: ns obj rel depth
        return self._cols(a, ns=[0], rel=[2], obj=[1])

    def lookup_subject_sets(self, a):  # (n,6) kg_lookup_subj_set: ns obj rel sns srel depth
        return self._cols(a, ns=[0], rel=[2], obj=[1], sns=3, srel=4)

    def roots(self, a):                # (n,4) kg_set: sns sobj srel depth
        return self._cols(a, obj=[1], sns=0, srel=2)

    def row_queries(self, reqs):       # kg_row_query records: the tuple fields
        out = reqs.copy()
        out["t"] = self.tuples(reqs["t"])
        return out

    def records(self, rec):            # expand records (type, is_set, ns, obj, rel, n_children)
        if rec is None:
            return None
        out = np.asarray(rec, np.int64).copy()
        s = out[:, 1] != 0
        out[s, 2], out[s, 4] = self.ns[out[s, 2]], self.rel[out[s, 4]]
        out[:, 3] = self.obj[out[:, 3]]
        return out

    def program(self, p):
        if p is None:
            return None
        has = np.zeros(int(self.ns.max()) + 1, np.uint8)
        k = min(len(p.ns_has_rel), len(self.ns))
        has[self.ns[:k]] = p.ns_has_rel[:k]
        rw = np.asarray(p.rw, np.int32).reshape(-1, 5).copy()
        for c in (1, 2):
            m = rw[:, c] >= 0
            rw[m, c] = self.rel[rw[m, c]].astype(np.int32)
        return type(p)(has, self.ns[p.rel_ns], self.rel[p.rel_rel], p.rel_root.copy(), rw, p.child.copy())

    def interner(self):
        """What engine.Snapshot reads from an interner: id counts (max id + 1) and the wildcard id."""
        return SimpleNamespace(n_namespaces=int(self.ns.max()) + 1, n_relations=int(self.rel.max()) + 1,
                               wildcard_rel=self.wildcard)


# ---- shared by the GPU modules: the check tiers' knob sets, and a batch through the packed device calls
KNOBS = {"default": dict(stream_ecap=512, back_edges=0, grid_ms=1),
         "tail-ms": dict(stream_ecap=1, back_edges=1, grid_ms=1),     # every walk handed on, the tail as MS-BFS
         "tail-grid": dict(stream_ecap=1, back_edges=1, grid_ms=0)}   # ... as per-query grid rounds


def tune(snap, knobs):
    for k, v in knobs.items():
        snap.tune(k, v)


def device_packed(snap, q7, gmax):
    """kg_pack_queries_device, then kg_check_batch_packed_device: (rc of the packer, answers, error codes); the packed
    rows must be keto_amd._lib.pack_queries' (the header's kg_pack_query)."""
    import torch
    from keto_amd import _lib
    L, n = _lib.load(), len(q7)
    dq = torch.from_numpy(np.ascontiguousarray(q7).view(np.int32)).cuda()
    dp = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    rc = L.kg_pack_queries_device(snap.handle, dq.data_ptr(), n, dp.data_ptr(), None)
    if rc:
        return rc, None, None
    assert np.array_equal(dp.cpu().numpy().view(np.uint32), _lib.pack_queries(q7))
    o = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    e = torch.full((n,), 99, dtype=torch.int32, device="cuda")
    _lib.check(L.kg_check_batch_packed_device(snap.handle, dp.data_ptr(), n, gmax, o.data_ptr(), e.data_ptr(), None, None),
               "kg_check_batch_packed_device")
    torch.cuda.synchronize()
    return 0, o.cpu().numpy(), e.cpu().numpy().view(np.uint32)
