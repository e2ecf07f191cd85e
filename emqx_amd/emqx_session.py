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


# ---------------------------------------------------------------------------
# The session's send window: deliver/2 and enqueue/2 as the literal folds of
# the reference, the tests' reference of tm_batch_window.  No closed form here:
# the kernels hold that, and the tests compare the two.
#
#   deliver/2, deliver/3, deliver_msg/2  src/emqx_session.erl:421-457
#   enqueue/2                            src/emqx_session.erl:459-472
#   await/3                              src/emqx_session.erl:535-537
#   next_pkt_id/1                        src/emqx_session.erl:665-668
#   emqx_inflight:is_full/1              src/emqx_inflight.erl:83-87
#   emqx_mqueue:in/2                     src/emqx_mqueue.erl:148-168
#   handle_deliver/2                     src/emqx_channel.erl:657-680
#
# A session is a dict: next_pkt_id; inflight_max (0 = never full) and
# inflight (the window's keys: a list of packet ids); mqueue, a dict
# {store_qos0, max_len (0 = ?MAX_LEN_INFINITY), len, dropped, q: deque}.  A
# message is any object with m["qos"]; the queue holds the objects themselves.
# Here get_priority/3 is always the default priority, one queue: priority
# tables are restated in emqx_mqueue.py (window_one_prio) over emqx_pqueue.py.
# Not restated: maybe_ack / maybe_nack (shared deliveries), expiry.

from collections import deque  # noqa: E402

(TM_DISP_SEND0, TM_DISP_SEND, TM_DISP_QUEUED, TM_DISP_DROP_QOS0, TM_DISP_DROP_FULL, TM_DISP_HOST) = range(6)
TM_SESS_DISCONNECTED, TM_SESS_STORE_QOS0, TM_SESS_HOST = 1, 2, 4
TM_SESS_UNBOUNDED = 0xFFFFFFFF


def new_mqueue(max_len: int = 0, store_qos0: bool = False, items=()):
    """emqx_mqueue:init/1 plus `items` already in the queue (oldest first)."""
    q = deque(items)
    return {"store_qos0": bool(store_qos0), "max_len": int(max_len), "len": len(q), "dropped": 0, "q": q}


def new_session(next_pkt_id: int = 1, inflight_max: int = 0, inflight=(), mqueue=None):
    return {"next_pkt_id": int(next_pkt_id), "inflight_max": int(inflight_max), "inflight": list(inflight),
            "mqueue": mqueue if mqueue is not None else new_mqueue()}


def inflight_is_full(session) -> bool:
    """emqx_inflight:is_full/1 (src/emqx_inflight.erl:83-87)."""
    if session["inflight_max"] == 0:                                   # :84-85
        return False
    return session["inflight_max"] <= len(session["inflight"])        # :86-87


def mqueue_in(msg, mq):
    """emqx_mqueue:in/2 (src/emqx_mqueue.erl:148-168) -> the dropped message
    or None; mq changes in place."""
    if msg["qos"] == 0 and not mq["store_qos0"]:                       # :149-150
        return msg
    plen = len(mq["q"])                                                # :159, one priority: plen = len of the queue
    if mq["max_len"] != 0 and plen == mq["max_len"]:                   # :160
        dropped = mq["q"].popleft()                                    # :163 the oldest
        mq["q"].append(msg)                                            # :164
        mq["dropped"] += 1                                             # :165
        return dropped
    mq["len"] += 1                                                     # :167
    mq["q"].append(msg)
    return None


def next_pkt_id(session):
    """next_pkt_id/1 (:665-668)."""
    if session["next_pkt_id"] == 0xFFFF:                               # :665-666
        session["next_pkt_id"] = 1
    else:
        session["next_pkt_id"] += 1                                    # :668-669


def enqueue(msgs, session):
    """enqueue/2 (:459-472) -> [(dropped message, the message that entered)] in
    order (what log_dropped/2 sees)."""
    out = []
    for msg in msgs:                                                   # lists:foldl(fun enqueue/2, ...) :467
        dropped = mqueue_in(msg, session["mqueue"])                    # :470
        if dropped is not None:                                        # :471
            out.append((dropped, msg))
    return out


def deliver_msg(msg, session):
    """deliver_msg/2 (:440-457) -> ([(PacketId | None, Msg)], enqueue/2's dropped pairs)."""
    if msg["qos"] == 0:                                                # :440-441
        return [(None, msg)], []
    if inflight_is_full(session):                                      # :446-452 (maybe_nack: not shared -> false)
        return [], enqueue([msg], session)
    pid = session["next_pkt_id"]                                       # :454
    session["inflight"].append(pid)                                    # :455 await/3 (:535-537)
    next_pkt_id(session)                                               # :456
    return [(pid, msg)], []


def deliver(msgs, session):
    """deliver/2,3 (:421-438) -> (Publishes, enqueue/2's dropped pairs)."""
    publishes, dropped = [], []
    for msg in msgs:                                                   # :432-438
        p, d = deliver_msg(msg, session)
        publishes += p
        dropped += d
    return publishes, dropped


def session_of_state(st):
    """A mirror session of a tm_session_state dict.  The window's max size is
    inflight_free beyond what it holds now (the ids held do not matter to
    is_full/1, only their number: none are held); the queue holds mqueue_len
    messages of an earlier batch."""
    free = st.get("inflight_free", TM_SESS_UNBOUNDED)
    flags = st.get("flags", 0)
    old = [{"qos": 1, "old": k} for k in range(st.get("mqueue_len", 0))]
    return new_session(st.get("next_pkt_id", 1), 0 if free == TM_SESS_UNBOUNDED else free + 1,
                       [] if free == TM_SESS_UNBOUNDED else [0],
                       new_mqueue(st.get("mqueue_max", 0), bool(flags & TM_SESS_STORE_QOS0), old))


def window_one(qos_list, st):
    """handle_deliver/2 (src/emqx_channel.erl:657-680) for one inbox: the
    deliveries' enriched QoS in mailbox order and a tm_session_state dict ->
    ([(disp, packet id or 0)], (next_pkt_id, n_inflight, n_queued, n_dropped_old)).
    A dropped message that is the entering one itself never entered the queue
    (in/2's first clause); any other is the oldest, pushed out."""
    flags = st.get("flags", 0)
    if flags & TM_SESS_HOST:
        return [(TM_DISP_HOST, 0)] * len(qos_list), (st.get("next_pkt_id", 1), 0, 0, 0)
    s = session_of_state(st)
    msgs = [{"qos": q, "k": k} for k, q in enumerate(qos_list)]
    res = [None] * len(msgs)
    n0 = len(s["inflight"])
    if flags & TM_SESS_DISCONNECTED:                                   # :659-663
        dropped = enqueue(msgs, s)
    else:                                                              # :672-680
        publishes, dropped = deliver(msgs, s)
        for pid, m in publishes:
            res[m["k"]] = (TM_DISP_SEND0, 0) if pid is None else (TM_DISP_SEND, pid)
    n_old = 0
    for m, entering in dropped:
        if "old" in m:
            n_old += 1
        elif m is entering:
            res[m["k"]] = (TM_DISP_DROP_QOS0, 0)                       # 'delivery.dropped.qos0_msg'
        else:
            res[m["k"]] = (TM_DISP_DROP_FULL, 0)                       # 'delivery.dropped.queue_full'
    n_queued = 0
    for m in s["mqueue"]["q"]:
        if "old" not in m:
            res[m["k"]] = (TM_DISP_QUEUED, 0)
            n_queued += 1
    assert all(r is not None for r in res)
    return res, (s["next_pkt_id"], len(s["inflight"]) - n0, n_queued, n_old)


def session_window(inboxes, states, defaults=None):
    """Every inbox of session_inboxes' output through window_one.

    inboxes   {pid: [(publish index, To, delivery byte, subid)]}
    states    {pid: tm_session_state dict}; defaults for a pid not in it
    -> {pid: ([(disp, packet id or 0)], (next_pkt_id, n_inflight, n_queued, n_dropped_old))}"""
    defaults = defaults or {}
    return {pid: window_one([d[2] & 3 for d in box], states.get(pid, defaults)) for pid, box in inboxes.items()}


# ---------------------------------------------------------------------------
# The dequeue after acks: what puback/2 and pubcomp/2 run once an inflight slot
# is free, the tests' reference of tm_sessions_drain (with emqx_mqueue.drain_one
# around it).
#
#   dequeue/1, dequeue/3  src/emqx_session.erl:389-409
#   acc_cnt/2             src/emqx_session.erl:411-413
#   batch_n/1             src/emqx_session.erl:680-684
#   ?DEFAULT_BATCH_N      src/emqx_session.erl:153
#
# Here a session's mqueue is an emqx_mqueue value (a dict whose q is an
# emqx_pqueue), and `now` stands for erlang:system_time(millisecond).

DEFAULT_BATCH_N = 1000
TM_DRAIN_BATCH_N = DEFAULT_BATCH_N
(TM_DRAIN_SEND0, TM_DRAIN_SEND, TM_DRAIN_KEPT, TM_DRAIN_EXPIRED) = range(4)
TM_DRAIN_NO_ORDER = 0xFFFFFFFF
TM_QMSG_EXPIRY = 4


def batch_n(session) -> int:
    """batch_n/1 (:680-684)."""
    if session["inflight_max"] == 0:                                   # :682
        return DEFAULT_BATCH_N
    return session["inflight_max"] - len(session["inflight"])         # :683


def acc_cnt(msg, cnt: int) -> int:
    """acc_cnt/2 (:411-413)."""
    if msg["qos"] == 0:                                                # :412
        return cnt
    return cnt - 1                                                     # :413


def dequeue_n(cnt: int, mq, now: int):
    """dequeue/3 (:397-409) -> (Msgs in out order, the new queue, the expired
    messages it threw away, in out order: inc_expired_cnt(delivery) once each)."""
    from . import emqx_message as M
    from . import emqx_mqueue as MQ
    msgs, expired = [], []
    while cnt != 0:                                                    # :397-398
        r, mq1 = MQ.out(mq)                                            # :401
        if r == "empty":                                               # :402
            break
        mq = mq1
        msg = r[1]                                                     # :403
        if M.is_expired(msg, now):                                     # :404-406
            expired.append(msg)
        else:                                                          # :407
            cnt = acc_cnt(msg, cnt)
            msgs.append(msg)
    return msgs, mq, expired


def dequeue(session, now: int):
    """dequeue/1 (:389-395) -> (Publishes, the expired messages); the session
    changes in place as deliver/2's does."""
    from . import emqx_mqueue as MQ
    if MQ.is_empty(session["mqueue"]):                                 # :390-391
        return [], []
    msgs, session["mqueue"], expired = dequeue_n(batch_n(session), session["mqueue"], now)   # :393
    publishes, dropped = MQ.deliver(msgs, session)                     # :394
    assert not dropped                                                 # the window had batch_n free slots
    return publishes, expired
