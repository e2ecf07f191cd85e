"""emqx_access_rule mirror (src/emqx_access_rule.erl) -- ACL rules on the host.

The CPU restatement of compile/1 and match/3 that the device path
(Engine.acl_check, kernel tm_acl_check) is compared against, clause by clause.

Terms: Erlang tuples are Python tuples, binaries are bytes, Erlang strings are
str (bin/1 encodes them), the atoms allow / deny / publish / subscribe /
pubsub / client / user / ipaddr / and / or / eq / pattern are plain str in
their positions, and the atom `all` is ALL (a bare "all" is accepted where no
binary can stand: `{A, all}` and a top-level who).  A client is a dict with
`clientid`, `username` (bytes) and `peerhost` (an address string, an
ipaddress object or an inet tuple), each None for `undefined`.
"""

from __future__ import annotations

import ipaddress

from . import emqx_topic as T

ALL = T.Atom("all")
ALLOW_DENY = ("allow", "deny")          # ?ALLOW_DENY, :40
PUBSUB = ("subscribe", "publish", "pubsub")   # ?PUBSUB, :41


class RuleError(ValueError):
    """function_clause / badarg of the reference: a term compile/1 has no clause for."""


def _is_all(x) -> bool:
    return x is ALL or (isinstance(x, T.Atom) and str.__eq__(x, "all"))


def bin_(x) -> bytes:
    """src/emqx_access_rule.erl:83-86"""
    if isinstance(x, str) and not isinstance(x, T.Atom):
        return x.encode()
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    raise RuleError(("function_clause", x))


def parse_cidr(cidr):
    """esockd_cidr:parse(CIDR, true): {Start, End, Len}, the start masked
    (test/emqx_access_rule_SUITE.erl:38-39, :78-79)."""
    if isinstance(cidr, (bytes, bytearray)):
        cidr = bytes(cidr).decode()
    net = ipaddress.ip_network(cidr, strict=False)
    return (_inet_tuple(net.network_address), _inet_tuple(net.broadcast_address), net.prefixlen)


def _inet_tuple(a):
    p = a.packed
    if len(p) == 4:
        return tuple(p)
    return tuple(int.from_bytes(p[i:i + 2], "big") for i in range(0, 16, 2))


def peer_tuple(host):
    """A client's peerhost as an inet tuple (4 or 8 elements), None = undefined."""
    if host is None:
        return None
    if isinstance(host, tuple):
        if len(host) not in (4, 8):
            raise RuleError(("badarg", host))
        return tuple(int(x) for x in host)
    if isinstance(host, (bytes, bytearray)):
        host = bytes(host).decode()
    return _inet_tuple(ipaddress.ip_address(host))


def compile(rule):   # noqa: A001 (the reference's name)
    """src/emqx_access_rule.erl:43-51"""
    if not isinstance(rule, tuple) or not rule or rule[0] not in ALLOW_DENY:
        raise RuleError(("function_clause", rule))
    if len(rule) == 2 and (_is_all(rule[1]) or rule[1] == "all"):
        return (rule[0], ALL)                                            # :44-45
    if len(rule) != 4 or rule[2] not in PUBSUB:
        raise RuleError(("function_clause", rule))
    a, who, access, topics = rule
    if isinstance(topics, (bytes, bytearray)):                           # :47-48, is_binary(Topic)
        return (a, compile_who(who), access, [compile_topic(bytes(topics))])
    if not isinstance(topics, (list, tuple)) or (isinstance(topics, tuple) and topics[:1] == ("eq",)):
        raise RuleError(("function_clause", rule))
    return (a, compile_who(who), access, [compile_topic(t) for t in topics])   # :50-51


def compile_who(who):
    """src/emqx_access_rule.erl:53-68"""
    if _is_all(who) or (isinstance(who, str) and who == "all"):          # :53-54
        return ALL
    if isinstance(who, tuple) and len(who) == 2:
        k, v = who
        if k == "ipaddr":                                                # :55-56
            return ("ipaddr", v if isinstance(v, tuple) else parse_cidr(v))
        if k in ("client", "user"):                                      # :57-64
            return (k, ALL if _is_all(v) else bin_(v))
        if k in ("and", "or") and isinstance(v, (list, tuple)):          # :65-68
            return (k, [compile_who(c) for c in v])
    raise RuleError(("function_clause", who))   # a bare binary is in the type, not in compile/2


def compile_topic(topic):
    """src/emqx_access_rule.erl:70-81"""
    if isinstance(topic, tuple) and len(topic) == 2 and topic[0] == "eq":
        return ("eq", T.words(bin_(topic[1])))                           # :70-71
    ws = T.words(bin_(topic))                                            # :72-77
    if any((not isinstance(w, T.Atom)) and w in (b"%u", b"%c") for w in ws):   # 'pattern?', :79-81
        return ("pattern", ws)
    return ws


def match(clientinfo, topic, rule):
    """src/emqx_access_rule.erl:88-99 -> ("matched", A) | "nomatch" (rule compiled)."""
    if len(rule) == 2 and _is_all(rule[1]) and rule[0] in ALLOW_DENY:    # :91-92
        return ("matched", rule[0])
    a, who, _pubsub, filters = rule
    if match_who(clientinfo, who) and match_topics(clientinfo, topic, filters):
        return ("matched", a)
    return "nomatch"


def match_who(ci, who) -> bool:
    """src/emqx_access_rule.erl:101-124"""
    if _is_all(who):                                                     # :101-102
        return True
    if isinstance(who, tuple) and len(who) == 2:
        k, v = who
        if k in ("user", "client") and _is_all(v):                       # :103-106
            return True
        if k == "client":                                                # :107-108 (a binary never equals undefined)
            return ci.get("clientid") is not None and bytes(ci["clientid"]) == v
        if k == "user":                                                  # :109-110
            return ci.get("username") is not None and bytes(ci["username"]) == v
        if k == "ipaddr":                                                # :111-114
            ip = peer_tuple(ci.get("peerhost"))
            if ip is None:
                return False
            start, end, _len = v
            # esockd_cidr:match/2: Start =< IP =< End, tuples of one family only
            return len(ip) == len(start) and start <= ip <= end
        if k == "and":                                                   # :115-118
            ok = True
            for c in v:
                ok = match_who(ci, c) and ok
            return ok
        if k == "or":                                                    # :119-122
            ok = False
            for c in v:
                ok = match_who(ci, c) or ok
            return ok
    return False                                                         # :123-124


def match_topics(ci, topic, filters) -> bool:
    """src/emqx_access_rule.erl:126-134"""
    for f in filters:
        if isinstance(f, tuple) and f[0] == "pattern":                   # :128-131
            f = feed_var(ci, f[1])
        if match_topic(T.words(bytes(topic)), f):
            return True
    return False                                                         # :126-127


def match_topic(topic_words, f) -> bool:
    """src/emqx_access_rule.erl:136-139; word lists, so emqx_topic:match/2
    runs its list clauses only (src/emqx_topic.erl:74-87, no '$' rule)."""
    if isinstance(f, tuple) and f[0] == "eq":
        return _words_eq(topic_words, f[1])
    return T.match(topic_words, f)


def _words_eq(a, b) -> bool:
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if isinstance(x, T.Atom) or isinstance(y, T.Atom):
            if x is not y:
                return False
        elif x != y:
            return False
    return True


def feed_var(ci, pattern):
    """src/emqx_access_rule.erl:141-154: the value goes in as ONE word (a
    binary, never one of the atoms '' / '+' / '#', never re-tokenised)."""
    out = []
    for w in pattern:
        if not isinstance(w, T.Atom) and w == b"%c" and ci.get("clientid") is not None:   # :145-148
            out.append(bytes(ci["clientid"]))
        elif not isinstance(w, T.Atom) and w == b"%u" and ci.get("username") is not None:  # :149-152
            out.append(bytes(ci["username"]))
        else:
            out.append(w)                                                # :146, :150, :153-154
    return out
