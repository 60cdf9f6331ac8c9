"""Request handling of the check and expand APIs above the engines (the transport itself -- HTTP
routing, gRPC servers -- is out of scope): request decoding, the unknown-namespace
rule, status mirroring and the response shapes, as the reference's handlers do them.

  REST  GET/POST /relation-tuples/check            200 {"allowed": true} | 403 {"allowed": false}
        GET/POST /relation-tuples/check/openapi    200 {"allowed": ...} always
                                                    internal/check/handler.go:101-232
        GET /relation-tuples/expand                 internal/expand/handler.go:81-107
        GET /relation-tuples                        internal/relationtuple/read_server.go:122-175
        DELETE /admin/relation-tuples               internal/relationtuple/transact_server.go:152-181
        GET /relation-tuples/list-objects           no reference counterpart (ListObjectsHandler)
        GET /relation-tuples/list-subjects          no reference counterpart (ListSubjectsHandler)
  gRPC  CheckService.Check                          internal/check/handler.go:234-275
        ExpandService.Expand                        internal/expand/handler.go:109-146
        ReadService.ListRelationTuples              internal/relationtuple/read_server.go:65-102
        WriteService.DeleteRelationTuples           internal/relationtuple/transact_server.go:64-85

An unknown namespace is "not allowed" over REST (handler.go:156-160, 221-225) but an error over gRPC
(:261-264, the mapper's herodot.ErrNotFound).  Request errors are herodot's 400s
(ketoapi/public_api_definitions.go:15-19, x/max_depth.go:10-21); engine errors are 500s.
"""
from __future__ import annotations

import json
import re
from typing import Mapping, Optional, Tuple, Union
from urllib.parse import parse_qs

from .engine import CheckError, Engine, ExpandEngine
from .ketoapi import RelationTuple, SubjectSet, TREE_LEAF
from .mapper import Mapper, NamespaceNotFound

SUBJECT_ID_KEY = "subject_id"
SUBJECT_SET_NS_KEY, SUBJECT_SET_OBJ_KEY, SUBJECT_SET_REL_KEY = ("subject_set.namespace", "subject_set.object",
                                                                "subject_set.relation")


class HandlerError(Exception):
    """A herodot error: HTTP status + message (gRPC code alongside)."""

    GRPC = {400: 3, 404: 5, 500: 13}  # InvalidArgument, NotFound, Internal

    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status
        self.message = message

    @property
    def grpc_code(self) -> int:
        return self.GRPC.get(self.status, 2)

    def body(self) -> dict:
        return {"error": {"code": self.status, "message": self.message}}


def _bad(msg: str) -> HandlerError:
    return HandlerError(400, msg)


ERR_DROPPED_SUBJECT_KEY = 'provide "subject_id" or "subject_set.*"; support for "subject" was dropped'
ERR_DUPLICATE_SUBJECT = "exactly one of subject_set or subject_id has to be provided"
ERR_INCOMPLETE_SUBJECT = 'incomplete subject, provide "subject_id" or a complete "subject_set.*"'
ERR_NIL_SUBJECT = "subject is not allowed to be nil"
ERR_INCOMPLETE_TUPLE = 'incomplete tuple, provide "namespace", "object", "relation", and a subject'

Query = Mapping[str, Union[str, list]]


def parse_query(q: Union[str, Query]) -> dict:
    """url.Values: a raw query string or a mapping; values keep every occurrence (Get = the first)."""
    if isinstance(q, str):
        return parse_qs(q.lstrip("?"), keep_blank_values=True)
    return {k: (v if isinstance(v, list) else [v]) for k, v in q.items()}


def _get(q: dict, k: str) -> str:
    v = q.get(k)
    return v[0] if v else ""


_GO_INT = re.compile(r"^[+-]?(0[xX][0-9a-fA-F_]+|0[bB][01_]+|0[oO][0-7_]+|0[0-7_]*|[1-9][0-9_]*)$")


def parse_go_int(s: str) -> int:
    """strconv.ParseInt(s, 0, 0): sign, base prefix 0x / 0b / 0o or a leading 0 (octal), underscores
    only between digits after a prefix; 64-bit range."""
    if not _GO_INT.match(s) or "__" in s or s.endswith("_"):
        raise ValueError(s)
    neg = s.startswith("-")
    body = s.lstrip("+-")
    if "_" in body and not (len(body) > 1 and body[0] == "0"):
        raise ValueError(s)  # underscores need a base prefix
    body = body.replace("_", "")
    if len(body) > 1 and body[0] == "0" and body[1] not in "xXbBoO":
        v = int(body[1:], 8)
    else:
        v = int(body, 0)
    v = -v if neg else v
    if not -(1 << 63) <= v < (1 << 63):
        raise ValueError(s)
    return v


def max_depth_from_query(q: dict) -> int:
    """x.GetMaxDepthFromQuery (internal/x/max_depth.go:10-21): absent -> 0 (the global default)."""
    if "max-depth" not in q:
        return 0
    s = _get(q, "max-depth")
    try:
        return parse_go_int(s)
    except ValueError:
        raise _bad(f"unable to parse 'max-depth' query parameter to int: {s!r}")


def subject_from_url_query(q: dict) -> Tuple[Optional[str], Optional[SubjectSet]]:
    """The subject part of RelationTuple.FromURLQuery (ketoapi/enc_url_query.go:12-97): (subject id,
    subject set), one of them set."""
    if "subject" in q:
        raise _bad(ERR_DROPPED_SUBJECT_KEY)
    has_id = SUBJECT_ID_KEY in q
    has_set = [k in q for k in (SUBJECT_SET_NS_KEY, SUBJECT_SET_OBJ_KEY, SUBJECT_SET_REL_KEY)]
    sid: Optional[str] = None
    sset: Optional[SubjectSet] = None
    if not has_id and not any(has_set):
        pass
    elif has_id and any(has_set):
        raise _bad(ERR_DUPLICATE_SUBJECT)
    elif has_id:
        sid = _get(q, SUBJECT_ID_KEY)
    elif all(has_set):
        sset = SubjectSet(_get(q, SUBJECT_SET_NS_KEY), _get(q, SUBJECT_SET_OBJ_KEY), _get(q, SUBJECT_SET_REL_KEY))
    else:
        raise _bad(ERR_INCOMPLETE_SUBJECT)
    if sid is None and sset is None:
        raise _bad(ERR_NIL_SUBJECT)
    return sid, sset


def tuple_from_url_query(q: dict) -> RelationTuple:
    """RelationTuple.FromURLQuery (ketoapi/enc_url_query.go:12-97)."""
    sid, sset = subject_from_url_query(q)
    if "namespace" not in q or "object" not in q or "relation" not in q:
        raise _bad(ERR_INCOMPLETE_TUPLE)
    return RelationTuple(_get(q, "namespace"), _get(q, "object"), _get(q, "relation"), sid, sset)


def tuple_from_json(body: Union[bytes, str, dict]) -> RelationTuple:
    """json.Decode into ketoapi.RelationTuple (handler.go:215-218); absent fields stay empty."""
    try:
        d = json.loads(body) if isinstance(body, (bytes, str)) else body
        if not isinstance(d, dict):
            raise ValueError("expected a JSON object")
        return RelationTuple.from_json(d)
    except (ValueError, AttributeError, TypeError) as e:
        raise _bad(f"could not unmarshal json: {e}")


class CheckHandler:
    """internal/check/handler.go: REST (mirrored / openapi) and gRPC Check over one engine."""

    def __init__(self, engine: Engine, mapper: Mapper):
        self.engine, self.mapper = engine, mapper

    def _check(self, t: RelationTuple, max_depth: int, unknown_ns_false: bool) -> bool:
        if t.subject_id is None and t.subject_set is None:
            raise _bad(ERR_NIL_SUBJECT)
        try:
            self.mapper.from_tuple(t)
        except NamespaceNotFound as e:
            if unknown_ns_false:  # handler.go:156-160 / 221-225: "not allowed", not "not found"
                return False
            raise HandlerError(404, f"Unable to locate the resource: namespace {e.args[0]!r}")
        try:
            return self.engine.check_is_member(t, max_depth)
        except CheckError as e:
            raise HandlerError(500, str(e))

    def _rest(self, produce, mirror_status: bool) -> Tuple[int, dict]:
        try:
            allowed = produce()
        except HandlerError as e:
            return e.status, e.body()
        if allowed or not mirror_status:
            return 200, {"allowed": allowed}
        return 403, {"allowed": False}  # handler.go:138-141

    def get_check(self, query: Union[str, Query], mirror_status: bool = True) -> Tuple[int, dict]:
        """GET /relation-tuples/check (mirror_status) or /relation-tuples/check/openapi."""
        def produce():
            q = parse_query(query)
            d = max_depth_from_query(q)
            return self._check(tuple_from_url_query(q), d, True)
        return self._rest(produce, mirror_status)

    def post_check(self, body: Union[bytes, str, dict], query: Union[str, Query] = "",
                   mirror_status: bool = True) -> Tuple[int, dict]:
        """POST /relation-tuples/check (mirror_status) or /relation-tuples/check/openapi."""
        def produce():
            d = max_depth_from_query(parse_query(query))
            return self._check(tuple_from_json(body), d, True)
        return self._rest(produce, mirror_status)

    def grpc_check(self, req: dict) -> dict:
        """CheckService.Check (handler.go:234-275): req = {"tuple": {...}} or the deprecated flat
        fields, plus "max_depth".  Raises HandlerError (grpc_code) on failure."""
        src = req.get("tuple") if req.get("tuple") is not None else req
        sub = src.get("subject")
        if not sub:
            raise _bad(ERR_NIL_SUBJECT)
        if "id" in sub:
            t = RelationTuple(src.get("namespace", ""), src.get("object", ""), src.get("relation", ""),
                              subject_id=sub["id"])
        else:
            s = sub.get("set") or {}
            t = RelationTuple(src.get("namespace", ""), src.get("object", ""), src.get("relation", ""),
                              subject_set=SubjectSet(s.get("namespace", ""), s.get("object", ""), s.get("relation", "")))
        allowed = self._check(t, int(req.get("max_depth", 0)), False)
        return {"allowed": allowed, "snaptoken": "not yet implemented"}


class ExpandHandler:
    """internal/expand/handler.go: REST GET and gRPC Expand over one expand engine."""

    def __init__(self, engine: ExpandEngine, mapper: Mapper):
        self.engine, self.mapper = engine, mapper

    def _tree(self, s: SubjectSet, max_depth: int):
        try:
            self.mapper.from_subject_set(s)
        except NamespaceNotFound as e:
            raise HandlerError(404, f"Unable to locate the resource: namespace {e.args[0]!r}")
        return self.engine.build_tree(s, max_depth)

    def get_expand(self, query: Union[str, Query]) -> Tuple[int, Optional[dict]]:
        """GET /relation-tuples/expand?namespace=&object=&relation=&max-depth= (handler.go:81-107).
        The reference has no nil guard before Mapper.ToTree (uuid_mapping.go:314 dereferences the
        nil tree of an empty or unknown set): that request fails with a server error here too."""
        try:
            q = parse_query(query)
            d = max_depth_from_query(q)
            s = SubjectSet(_get(q, "namespace"), _get(q, "object"), _get(q, "relation"))
            tree = self._tree(s, d)
        except HandlerError as e:
            return e.status, e.body()
        if tree is None:
            return 500, HandlerError(500, "expand: empty tree (no nil guard in the reference)").body()
        return 200, tree.to_json()

    def grpc_expand(self, req: dict) -> dict:
        """ExpandService.Expand (handler.go:109-146): a subject id is a leaf of itself; a nil tree is
        an empty response (:136-138)."""
        sub = req.get("subject") or {}
        if "id" in sub:
            return {"tree": {"node_type": TREE_LEAF, "subject": {"id": sub["id"]}}}
        s = sub.get("set") or {}
        tree = self._tree(SubjectSet(s.get("namespace", ""), s.get("object", ""), s.get("relation", "")),
                          int(req.get("max_depth", 0)))
        if tree is None:
            return {}
        return {"tree": tree.to_json()}


def parse_id_page(order: str, page_token: str, page_size: int) -> Optional[Tuple[int, int]]:
    """The page of a list request with order=id: (from, limit) for the paged lookup -- the token is the
    decimal id to start from (empty: 0).  None: no order given, the name-ordered paging.  A malformed
    token, size or order is the 400 of the name-ordered paging."""
    if not order:
        return None
    try:
        if order != "id":
            raise ValueError
        if page_token and not (page_token.isascii() and page_token.isdigit()):
            raise ValueError
        frm = int(page_token) if page_token else 0
        if frm > 0xFFFFFFFF or not 1 <= page_size <= 0xFFFFFFFF:
            raise ValueError
    except ValueError:
        raise _bad("malformed page_token or page_size")
    return frm, page_size


class ListObjectsHandler:
    """Reverse lookup over one engine (no reference counterpart; OpenFGA ListObjects' shape): the objects of
    a namespace on which a subject has a relation, in name order, paged -- or, with order=id, in id order
    through the paged lookup: the page token is the id to go on from, and only the page is computed."""

    DEFAULT_PAGE_SIZE = 100

    def __init__(self, engine: Engine, mapper: Mapper):
        self.engine, self.mapper = engine, mapper

    def _list(self, namespace: str, relation: str, sid: Optional[str], sset: Optional[SubjectSet], max_depth: int,
              page_size: int, page_token: str, order: str = "") -> dict:
        if sid is None and sset is None:
            raise _bad(ERR_NIL_SUBJECT)
        try:  # the namespaces of the request as the check's mapper sees them
            self.mapper.check_namespace(namespace)
            if sset is not None:
                self.mapper.check_namespace(sset.namespace)
        except NamespaceNotFound as e:
            raise HandlerError(404, f"Unable to locate the resource: namespace {e.args[0]!r}")
        by_id = parse_id_page(order, page_token, page_size)
        if by_id is not None:
            try:
                names, nxt = self.engine.lookup_objects_page(namespace, relation, sset if sset is not None else sid,
                                                             max_depth, by_id[0], by_id[1])
            except CheckError as e:
                raise HandlerError(500, str(e))
            return {"objects": names, "next_page_token": "" if nxt is None else str(nxt)}
        try:
            at = int(page_token) if page_token else 0
            if at < 0 or page_size < 1:
                raise ValueError
        except ValueError:
            raise _bad("malformed page_token or page_size")
        try:
            names = self.engine.lookup_objects(namespace, relation, sset if sset is not None else sid, max_depth)
        except CheckError as e:
            raise HandlerError(500, str(e))
        page = names[at:at + page_size]
        return {"objects": page, "next_page_token": str(at + page_size) if at + page_size < len(names) else ""}

    def get_list_objects(self, query: Union[str, Query]) -> Tuple[int, dict]:
        """GET ?namespace=&relation=&subject_id= | subject_set.*=&max-depth=&page_size=&page_token=&order=."""
        try:
            q = parse_query(query)
            d = max_depth_from_query(q)
            sid, sset = subject_from_url_query(q)
            if "namespace" not in q or "relation" not in q:
                raise _bad('incomplete request, provide "namespace", "relation", and a subject')
            try:
                size = parse_go_int(_get(q, "page_size")) if "page_size" in q else self.DEFAULT_PAGE_SIZE
            except ValueError:
                raise _bad("malformed page_token or page_size")
            return 200, self._list(_get(q, "namespace"), _get(q, "relation"), sid, sset, d, size, _get(q, "page_token"),
                                   _get(q, "order"))
        except HandlerError as e:
            return e.status, e.body()

    def grpc_list_objects(self, req: dict) -> dict:
        """req = {"namespace", "relation", "subject": {"id"} | {"set": {...}}, "max_depth", "page_size",
        "page_token", "order"}.  Raises HandlerError (grpc_code) on failure."""
        sub = req.get("subject")
        if not sub:
            raise _bad(ERR_NIL_SUBJECT)
        sid, sset = None, None
        if "id" in sub:
            sid = sub["id"]
        else:
            s = sub.get("set") or {}
            sset = SubjectSet(s.get("namespace", ""), s.get("object", ""), s.get("relation", ""))
        return self._list(req.get("namespace", ""), req.get("relation", ""), sid, sset, int(req.get("max_depth", 0)),
                          int(req.get("page_size", 0)) or self.DEFAULT_PAGE_SIZE, str(req.get("page_token", "")),
                          str(req.get("order", "")))


class ListSubjectsHandler:
    """Subject lookup over one engine (no reference counterpart; OpenFGA ListUsers' shape): the subject ids
    that have a relation on an object, in name order -- or id order with order=id -- paged like
    ListObjectsHandler.  With a filter subject_set.namespace + subject_set.relation (OpenFGA's user filter
    {type, relation}) the subject sets of that namespace and relation instead, paged the same way."""

    DEFAULT_PAGE_SIZE = ListObjectsHandler.DEFAULT_PAGE_SIZE
    ERR_FILTER = 'a subject-set filter takes "subject_set.namespace" and "subject_set.relation", and no object'

    def __init__(self, engine: Engine, mapper: Mapper):
        self.engine, self.mapper = engine, mapper

    def _list(self, namespace: str, object: str, relation: str, max_depth: int, page_size: int,
              page_token: str, order: str = "", sfilter: Optional[Tuple[str, str]] = None) -> dict:
        try:
            self.mapper.check_namespace(namespace)
        except NamespaceNotFound as e:
            raise HandlerError(404, f"Unable to locate the resource: namespace {e.args[0]!r}")
        if sfilter is None:
            key, one = "subject_ids", (lambda name: name)
            unpaged = lambda: self.engine.lookup_subjects(namespace, object, relation, max_depth)
            paged = lambda frm, limit: self.engine.lookup_subjects_page(namespace, object, relation, max_depth, frm, limit)
        else:
            key = "subject_sets"
            one = lambda s: {"namespace": s.namespace, "object": s.object, "relation": s.relation}
            unpaged = lambda: self.engine.lookup_subject_sets(namespace, object, relation, sfilter[0], sfilter[1], max_depth)
            paged = lambda frm, limit: self.engine.lookup_subject_sets_page(namespace, object, relation, sfilter[0],
                                                                            sfilter[1], max_depth, frm, limit)
        by_id = parse_id_page(order, page_token, page_size)
        if by_id is not None:
            try:
                names, nxt = paged(by_id[0], by_id[1])
            except CheckError as e:
                raise HandlerError(500, str(e))
            return {key: [one(x) for x in names], "next_page_token": "" if nxt is None else str(nxt)}
        try:
            at = int(page_token) if page_token else 0
            if at < 0 or page_size < 1:
                raise ValueError
        except ValueError:
            raise _bad("malformed page_token or page_size")
        try:
            names = unpaged()
        except CheckError as e:
            raise HandlerError(500, str(e))
        page = names[at:at + page_size]
        return {key: [one(x) for x in page], "next_page_token": str(at + page_size) if at + page_size < len(names) else ""}

    def _filter(self, ns, obj, rel) -> Optional[Tuple[str, str]]:
        """The subject-set filter of a request (each part None where it is not given), or None without one."""
        if ns is None and obj is None and rel is None:
            return None
        if obj is not None or not ns or not rel:
            raise _bad(self.ERR_FILTER)
        return str(ns), str(rel)

    def get_list_subjects(self, query: Union[str, Query]) -> Tuple[int, dict]:
        """GET ?namespace=&object=&relation=&max-depth=&page_size=&page_token=&order=
        [&subject_set.namespace=&subject_set.relation=]."""
        try:
            q = parse_query(query)
            d = max_depth_from_query(q)
            if "namespace" not in q or "object" not in q or "relation" not in q:
                raise _bad('incomplete request, provide "namespace", "object" and "relation"')
            sfilter = self._filter(*(_get(q, k) if k in q else None
                                     for k in (SUBJECT_SET_NS_KEY, SUBJECT_SET_OBJ_KEY, SUBJECT_SET_REL_KEY)))
            try:
                size = parse_go_int(_get(q, "page_size")) if "page_size" in q else self.DEFAULT_PAGE_SIZE
            except ValueError:
                raise _bad("malformed page_token or page_size")
            return 200, self._list(_get(q, "namespace"), _get(q, "object"), _get(q, "relation"), d, size,
                                   _get(q, "page_token"), _get(q, "order"), sfilter)
        except HandlerError as e:
            return e.status, e.body()

    def grpc_list_subjects(self, req: dict) -> dict:
        """req = {"namespace", "object", "relation", "max_depth", "page_size", "page_token", "order"} and, to list
        subject sets, "subject_set": {"namespace", "relation"}.  Raises HandlerError (grpc_code) on failure."""
        for k in ("namespace", "object", "relation"):
            if not req.get(k):
                raise _bad('incomplete request, provide "namespace", "object" and "relation"')
        f = req.get("subject_set")
        sfilter = None if f is None else self._filter(f.get("namespace") or "", f.get("object"), f.get("relation") or "")
        return self._list(req["namespace"], req["object"], req["relation"], int(req.get("max_depth", 0)),
                          int(req.get("page_size", 0)) or self.DEFAULT_PAGE_SIZE, str(req.get("page_token", "")),
                          str(req.get("order", "")), sfilter)


def relation_query_from_url_query(q: dict):
    """RelationQuery.FromURLQuery (ketoapi/enc_url_query.go:12-53): every field optional; a subject, where
    one is given, as subject_from_url_query reads it."""
    from .persister import RelationQuery
    sid: Optional[str] = None
    sset: Optional[SubjectSet] = None
    if any(k in q for k in ("subject", SUBJECT_ID_KEY, SUBJECT_SET_NS_KEY, SUBJECT_SET_OBJ_KEY, SUBJECT_SET_REL_KEY)):
        sid, sset = subject_from_url_query(q)
    return RelationQuery(_get(q, "namespace") if "namespace" in q else None, _get(q, "object") if "object" in q else None,
                         _get(q, "relation") if "relation" in q else None, sid, sset)


def _subject_proto(t: RelationTuple) -> dict:
    if t.subject_set is not None:
        s = t.subject_set
        return {"set": {"namespace": s.namespace, "object": s.object, "relation": s.relation}}
    return {"id": t.subject_id}


class RelationTuplesHandler:
    """internal/relationtuple/read_server.go: REST GET /relation-tuples and gRPC ListRelationTuples over one
    relationtuple.Manager (a SnapshotPersister, host or device reads); of transact_server.go, the
    delete-by-query pair: REST DELETE /admin/relation-tuples and gRPC DeleteRelationTuples."""

    def __init__(self, manager, mapper: Mapper):
        self.manager, self.mapper = manager, mapper

    def _map_query(self, query) -> None:
        try:  # Mapper.FromQuery (uuid_mapping.go:60-120): the namespaces that are named must exist
            if query.namespace is not None:
                self.mapper.check_namespace(query.namespace)
            if query.subject_set is not None:
                self.mapper.check_namespace(query.subject_set.namespace)
        except NamespaceNotFound as e:
            raise HandlerError(404, f"Unable to locate the resource: namespace {e.args[0]!r}")

    def _list(self, query, page_token: str, page_size: int):
        from .persister import MalformedPageToken
        self._map_query(query)
        try:
            return self.manager.get_relation_tuples(query, page_token, page_size)
        except MalformedPageToken:
            raise HandlerError(500, "malformed page token")  # a plain error: herodot's default status

    def get_relations(self, query: Union[str, Query]) -> Tuple[int, dict]:
        """GET /relation-tuples?namespace=&object=&relation=&subject_id= | subject_set.*=&page_token=&page_size=
        (read_server.go:122-175)."""
        try:
            q = parse_query(query)
            rq = relation_query_from_url_query(q)
            size = 0
            ps = _get(q, "page_size")
            if ps != "":
                try:
                    size = parse_go_int(ps)
                except ValueError:
                    raise _bad(f"strconv.ParseInt: parsing {json.dumps(ps)}: invalid syntax")
            tuples, token = self._list(rq, _get(q, "page_token"), size)
        except HandlerError as e:
            return e.status, e.body()
        return 200, {"relation_tuples": [t.to_json() for t in tuples], "next_page_token": token}

    def grpc_list_relation_tuples(self, req: dict) -> dict:
        """ReadService.ListRelationTuples (read_server.go:65-102): req = {"relation_query": {...}} or the
        deprecated {"query": {...}} whose empty strings mean unset, each with an optional "subject"
        ({"id"} | {"set": {...}}), plus "page_size" and "page_token".  Raises HandlerError on failure."""
        rq = self._query_from_proto(req)
        if rq is None:
            raise _bad("you must provide a query")
        tuples, token = self._list(rq, str(req.get("page_token", "")), int(req.get("page_size", 0)))
        return {"relation_tuples": [{"namespace": t.namespace, "object": t.object, "relation": t.relation,
                                     "subject": _subject_proto(t)} for t in tuples],
                "next_page_token": token}

    @staticmethod
    def _query_from_proto(req: dict):
        """RelationQuery.FromDataProvider over req["relation_query"], or over the deprecated req["query"]
        (whose empty strings mean unset); None with neither."""
        from .persister import RelationQuery
        if req.get("relation_query") is not None:
            src = req["relation_query"]
            ns, obj, rel = src.get("namespace"), src.get("object"), src.get("relation")
        elif req.get("query") is not None:
            src = req["query"]
            ns, obj, rel = (src.get(k) or None for k in ("namespace", "object", "relation"))
        else:
            return None
        sub = src.get("subject") or {}
        sid, sset = None, None
        if "id" in sub:
            sid = sub["id"]
        elif "set" in sub:
            s = sub.get("set") or {}
            sset = SubjectSet(s.get("namespace", ""), s.get("object", ""), s.get("relation", ""))
        return RelationQuery(ns, obj, rel, sid, sset)

    # ---- DELETE /admin/relation-tuples, WriteService.DeleteRelationTuples
    def delete_relations(self, query: Union[str, Query]) -> Tuple[int, Optional[dict]]:
        """DELETE /admin/relation-tuples?namespace=&object=&relation=&subject_id= | subject_set.*=
        (transact_server.go:152-181): every tuple the query matches goes; 204 without a body."""
        try:
            rq = relation_query_from_url_query(parse_query(query))
            self._map_query(rq)
            self.manager.delete_all_relation_tuples(rq)
        except HandlerError as e:
            return e.status, e.body()
        return 204, None

    def grpc_delete_relation_tuples(self, req: dict) -> dict:
        """WriteService.DeleteRelationTuples (transact_server.go:64-85): req = {"relation_query": {...}} or
        the deprecated {"query": {...}}, as grpc_list_relation_tuples reads them.  Raises HandlerError."""
        rq = self._query_from_proto(req)
        if rq is None:
            raise _bad("invalid request")
        self._map_query(rq)
        self.manager.delete_all_relation_tuples(rq)
        return {}
