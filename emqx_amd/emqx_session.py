"""What a session does with one drained mailbox before anything is sent: a
pure-host restatement of the reference's two per-delivery lookups of
maps:find(To, Subscriptions), written from the Erlang and used by the tests as
the reference of tm_batch_deliver.

  ignore_local/3    src/emqx_channel.erl:682-693
  enrich_subopts/3  src/emqx_session.erl:485-529

A delivery is (To, Msg); Msg is a dict with `from` (the publisher, None when
there is none), `qos`, `retain` (#message.flags.retain) and `retained`
(headers.retained =:= true).  Subscriptions map To -> {qos, nl, rap[, subid]}.
"""

from __future__ import annotations

TM_MSG_RETAIN = 4
TM_MSG_RETAINED = 8
TM_MSG_NL = 8


def _own(to, msg, subscriber, subs) -> bool:
    o = subs.get(to)                                   # maps:find(Topic, Subs)
    return (o is not None and o.get("nl", 0) == 1      # {ok, #{nl := 1}}
            and msg.get("from") is not None and msg["from"] == subscriber)   # when Subscriber =:= Publisher


def ignore_local(delivers, subscriber, subs, nl_all: bool = False):
    """ignore_local/3: lists:dropwhile -- the LEADING run of own deliveries on
    No-Local subscriptions is dropped, and nothing after the first delivery
    that is not own (:684-693).  nl_all drops every own delivery instead
    (MQTT-3.8.3-3; not the reference).  -> (deliveries left, dropped count)."""
    delivers = list(delivers)
    if nl_all:
        left = [d for d in delivers if not _own(d[0], d[1], subscriber, subs)]
        return left, len(delivers) - len(left)
    k = 0
    while k < len(delivers) and _own(delivers[k][0], delivers[k][1], subscriber, subs):
        k += 1
    return delivers[k:], k


def enrich_one(opts, msg, upgrade_qos: bool = False):
    """enrich_subopts/3 over get_subopts/2's list (:500-529); opts None is
    maps:find's `error`: the message goes out as it came (:506, :509)."""
    out = {"from": msg.get("from"), "qos": msg.get("qos", 0), "retain": bool(msg.get("retain", False)),
           "retained": bool(msg.get("retained", False)), "nl": bool(msg.get("nl", False)),
           "subid": msg.get("subid")}
    if opts is None:
        return out
    if opts.get("nl", 0) == 1:                         # :510-511
        out["nl"] = True
    sq = opts.get("qos", 0)                            # :514-519
    out["qos"] = max(sq, out["qos"]) if upgrade_qos else min(sq, out["qos"])
    if opts.get("rap", 0) == 0 and not out["retained"]:   # :520-525
        out["retain"] = False
    if opts.get("subid"):                              # :502-503, 526-529 (0 / None: no subid key)
        out["subid"] = opts["subid"]
    return out


def enrich(delivers, subs, upgrade_qos: bool = False):
    """enrich_fun/1 mapped over the deliveries (:485-488) -> [(To, Msg)]."""
    return [(to, enrich_one(subs.get(to), msg, upgrade_qos)) for to, msg in delivers]


def msg_of(byte: int, from_=None) -> dict:
    """The message of a publish byte of tm_deliver_opts.msg."""
    return {"from": from_, "qos": byte & 3, "retain": bool(byte & TM_MSG_RETAIN),
            "retained": bool(byte & TM_MSG_RETAINED)}


def byte_of(msg: dict) -> int:
    """The delivery byte of tm_session_inboxes.msg."""
    return msg["qos"] | (TM_MSG_RETAIN if msg["retain"] else 0) | (TM_MSG_NL if msg.get("nl") else 0)


def session_inboxes(mailboxes, subopts, from_=None, msg=None, upgrade_qos: bool = False, nl_all: bool = False):
    """Every mailbox of a batch through ignore_local and enrich.

    mailboxes  {pid: [(publish index, To)]} in mailbox order (emqx_broker.mailboxes)
    subopts    {pid: {To: opts}}
    from_      per publish: the publisher pid, or None (None: nobody)
    msg        per publish: the byte of tm_deliver_opts.msg (None: all 0)
    -> ({pid: [(publish index, To, delivery byte, subid or 0)]} without the
        pids that lost every delivery, dropped count)"""
    out, dropped = {}, 0
    for pid, box in mailboxes.items():
        subs = subopts.get(pid, {})
        delivers = [(to, dict(msg_of(msg[i] if msg is not None else 0, from_[i] if from_ is not None else None), i=i))
                    for i, to in box]
        left, k = ignore_local(delivers, pid, subs, nl_all)
        dropped += k
        if not left:
            continue
        res = []
        for (to, m), (_, e) in zip(left, enrich(left, subs, upgrade_qos)):
            res.append((m["i"], to, byte_of(e), e["subid"] or 0))
        out[pid] = res
    return out, dropped
