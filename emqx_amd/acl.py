"""Encoders of the ACL check's C structs (include/emqx_tm.h, tm_acl_*): compiled
emqx_access_rule rules, clients and requests -> ctypes arrays.  Every encoder
returns the struct(s) and a list that keeps the memory they point into alive.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from . import emqx_access_rule as R
from . import emqx_topic as T
from .gen import Strings

ACCESS = {"publish": N.TM_ACL_PUBLISH, "subscribe": N.TM_ACL_SUBSCRIBE, "pubsub": N.TM_ACL_PUBSUB}
VERDICTS = {N.TM_ACL_DENY: "deny", N.TM_ACL_ALLOW: "allow", N.TM_ACL_NOMATCH: "nomatch"}


def _addr16(t) -> bytes:
    """An inet tuple in network order, IPv4 in the first 4 of 16 bytes."""
    if len(t) == 4:
        return bytes(t) + bytes(12)
    return b"".join(int(x).to_bytes(2, "big") for x in t)


def _buf(b: bytes, keep):
    a = C.create_string_buffer(b, max(len(b), 1))
    keep.append(a)
    return C.cast(a, C.c_void_p)


def who_nodes(who, keep, out=None):
    """A compiled who term as the pre-order node list of tm_acl_who."""
    out = [] if out is None else out
    n = N.AclWho()
    out.append(n)
    if R._is_all(who):
        n.kind = N.TM_WHO_ALL
        return out
    k, v = who
    if k in ("client", "user"):
        if R._is_all(v):
            n.kind = N.TM_WHO_CLIENT_ALL if k == "client" else N.TM_WHO_USER_ALL
        else:
            n.kind = N.TM_WHO_CLIENT if k == "client" else N.TM_WHO_USER
            n.val, n.val_len = _buf(v, keep), len(v)
    elif k == "ipaddr":
        start, end, _len = v
        n.kind = N.TM_WHO_IPADDR
        n.family = 4 if len(start) == 4 else 6
        n.lo = (C.c_uint8 * 16)(*_addr16(start))
        n.hi = (C.c_uint8 * 16)(*_addr16(end))
    elif k in ("and", "or"):
        n.kind = N.TM_WHO_AND if k == "and" else N.TM_WHO_OR
        n.n_children = len(v)
        for c in v:
            who_nodes(c, keep, out)
    else:
        raise R.RuleError(("function_clause", who))
    return out


def encode_rules(compiled):
    """Compiled rules (emqx_access_rule.compile/1 output) -> (AclRule array, keep)."""
    keep = []
    arr = (N.AclRule * max(len(compiled), 1))()
    for j, rule in enumerate(compiled):
        r = arr[j]
        r.allow = N.TM_ACL_ALLOW if rule[0] == "allow" else N.TM_ACL_DENY
        if len(rule) == 2:
            r.access = 0
            continue
        _a, who, access, topics = rule
        r.access = ACCESS[access]
        nodes = who_nodes(who, keep)
        wa = (N.AclWho * len(nodes))(*nodes)
        ta = (N.AclTopic * max(len(topics), 1))()
        for i, t in enumerate(topics):
            eq = isinstance(t, tuple) and t[0] == "eq"
            ws = t[1] if isinstance(t, tuple) else t
            b = T.join(ws)
            ta[i].filter, ta[i].len, ta[i].eq = _buf(b, keep), len(b), int(eq)
        keep += [wa, ta]
        r.who, r.n_who, r.topics, r.n_topics = wa, len(nodes), ta, len(topics)
    return arr, keep


def encode_clients(clients):
    """[{clientid, username, peerhost}] -> (AclClients, keep)."""
    m = len(clients)
    ids = [bytes(c.get("clientid") or b"") for c in clients]
    names = [bytes(c.get("username") or b"") for c in clients]
    flags = np.zeros(max(m, 1), np.uint8)
    fam = np.zeros(max(m, 1), np.uint8)
    peer = np.zeros((max(m, 1), 16), np.uint8)
    for i, c in enumerate(clients):
        flags[i] = (1 if c.get("clientid") is not None else 0) | (2 if c.get("username") is not None else 0)
        ip = R.peer_tuple(c.get("peerhost"))
        if ip is not None:
            fam[i] = 4 if len(ip) == 4 else 6
            peer[i] = np.frombuffer(_addr16(ip), np.uint8)
    si, su = Strings.from_list(ids), Strings.from_list(names)
    ib = np.ascontiguousarray(si.buf if si.buf.size else np.zeros(1, np.uint8))
    ub = np.ascontiguousarray(su.buf if su.buf.size else np.zeros(1, np.uint8))
    io = np.ascontiguousarray(si.offs, dtype=np.uint64)
    uo = np.ascontiguousarray(su.offs, dtype=np.uint64)
    cs = N.AclClients(m, ib.ctypes.data, io.ctypes.data, ub.ctypes.data, uo.ctypes.data, flags.ctypes.data,
                      fam.ctypes.data, peer.ctypes.data)
    return cs, [ib, io, ub, uo, flags, fam, peer]


def encode_requests(requests):
    """[(client index, "publish" | "subscribe", topic)] -> (bytes, offsets, client_of, access) arrays."""
    s = Strings.from_list([bytes(t) for _c, _a, t in requests])
    buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
    offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
    cof = np.asarray([c for c, _a, _t in requests], dtype=np.uint32)
    acc = np.asarray([ACCESS[a] for _c, a, _t in requests], dtype=np.uint8)
    return buf, offs, cof, acc
