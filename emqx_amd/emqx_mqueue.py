"""emqx_mqueue restated clause by clause (src/emqx_mqueue.erl) over
emqx_pqueue, and the session's send window over a queue that has a priority
table: the tests' reference of tm_ptable_create and tm_batch_window_prio.  Pure
host code, written from the Erlang.

  init/1          src/emqx_mqueue.erl:106-116
  is_empty/1      :132        len/1      :134       dropped/1  :139-140
  in/2            :148-168    out/1      :170-176
  get_priority/3  :195-196    get_priority_opt/1  :184-189

A queue is a dict {store_qos0, max_len (0 = ?MAX_LEN_INFINITY), len, dropped,
p_table (None = ?NO_PRIORITY_TABLE, else {topic bytes: priority}), default_p,
q (an emqx_pqueue value)}; in_ / out return the new queue, nothing changes in
place.  A message is a dict with `qos` and `topic`.  A priority is an integer
or emqx_pqueue.INFINITY.
"""

from __future__ import annotations

from . import emqx_pqueue as PQ
from . import emqx_session as S

INFINITY = PQ.INFINITY
NO_PRIORITY_TABLE = None
LOWEST_PRIORITY = 0
HIGHEST_PRIORITY = INFINITY
MAX_LEN_INFINITY = 0

TM_PRIO_INFINITY = 0xFFFF
TM_PRIO_MAX_CLASSES = 8
TM_PRIO_NOCLASS = 0xFF


def get_priority_opt(opts):
    """get_priority_opt/1 (:184-189)."""
    dp = opts.get("default_priority")
    if dp is None:                                                      # get_opt/3: undefined -> the default (:178-182)
        dp = LOWEST_PRIORITY
    if dp == "lowest":                                                  # :186
        return LOWEST_PRIORITY
    if dp == "highest":                                                 # :187
        return HIGHEST_PRIORITY
    assert isinstance(dp, int) or dp == INFINITY                        # :188 (infinity: what `highest` becomes)
    return dp


def init(opts):
    """init/1 (:106-116): opts has max_len and store_qos0, and may have
    priorities and default_priority."""
    max_len0 = opts["max_len"]
    max_len = max_len0 if isinstance(max_len0, int) and max_len0 > MAX_LEN_INFINITY else MAX_LEN_INFINITY   # :108-111
    ptab = opts.get("priorities")                                       # :114 get_opt/3
    return {"store_qos0": bool(opts["store_qos0"]), "max_len": max_len, "len": 0, "dropped": 0,
            "p_table": NO_PRIORITY_TABLE if ptab is None else dict(ptab),
            "default_p": get_priority_opt(opts), "q": PQ.new()}


def is_empty(mq) -> bool:
    return mq["len"] == 0                                               # :132


def len_(mq) -> int:
    return mq["len"]                                                    # :134


def dropped(mq) -> int:
    return mq["dropped"]                                                # :140


def get_priority(topic, ptab, dp):
    """get_priority/3 (:195-196)."""
    if ptab is NO_PRIORITY_TABLE:                                       # :195: the default is disregarded
        return LOWEST_PRIORITY
    return ptab.get(topic, dp)                                          # :196 maps:get/3


def in_(msg, mq):
    """in/2 (:148-168) -> (the dropped message or None, the new queue)."""
    if msg["qos"] == 0 and not mq["store_qos0"]:                        # :149-150
        return msg, mq
    priority = get_priority(msg["topic"], mq["p_table"], mq["default_p"])   # :158
    plen = PQ.plen(priority, mq["q"])                                   # :159
    if mq["max_len"] != MAX_LEN_INFINITY and plen == mq["max_len"]:     # :160
        (_, dropped_msg), q1 = PQ.out(priority, mq["q"])                # :163 the oldest of that priority
        q2 = PQ.in_(msg, priority, q1)                                  # :164
        return dropped_msg, dict(mq, q=q2, dropped=mq["dropped"] + 1)   # :165
    return None, dict(mq, len=mq["len"] + 1, q=PQ.in_(msg, priority, mq["q"]))   # :167


def out(mq):
    """out/1 (:170-176) -> ("empty" | ("value", Msg), the new queue)."""
    if mq["len"] == 0:                                                  # :171-173
        assert PQ.len_(mq["q"]) == 0
        return "empty", mq
    r, q1 = PQ.out(mq["q"])                                             # :175
    return r, dict(mq, q=q1, len=mq["len"] - 1)                         # :176


# ---------------------------------------------------------------------------
# A priority table as the device sees it (tm_ptable_create): its classes are
# the distinct priorities it holds together with its default, descending,
# infinity first; class 0 is the highest.

def _key(p):
    return (1, 0) if p == INFINITY else (0, p)


def table_default(table):
    """The default priority of a table dict {"priorities", "default_priority"}."""
    return get_priority_opt({"default_priority": table.get("default_priority", "lowest")})


def classes_of(table):
    """The classes of a table, highest first; [0] without a table
    (get_priority/3 :195: one queue of priority 0)."""
    if table is None:
        return [LOWEST_PRIORITY]
    return sorted(set(table["priorities"].values()) | {table_default(table)}, key=_key, reverse=True)


def enqueue(msgs, session):
    """emqx_session:enqueue/2 (src/emqx_session.erl:459-472) over this
    module's in/2 -> [(dropped message, the message that entered)]."""
    out_ = []
    for msg in msgs:                                                    # lists:foldl(fun enqueue/2, ...) :467
        dropped_msg, session["mqueue"] = in_(msg, session["mqueue"])    # :470
        if dropped_msg is not None:                                     # :471
            out_.append((dropped_msg, msg))
    return out_


def deliver(msgs, session):
    """emqx_session:deliver/2,3 and deliver_msg/2 (src/emqx_session.erl:421-457)
    -> (Publishes, enqueue/2's dropped pairs)."""
    publishes, dropped_ = [], []
    for msg in msgs:                                                    # :432-438
        if msg["qos"] == 0:                                             # :440-441
            publishes.append((None, msg))
        elif S.inflight_is_full(session):                               # :446-452
            dropped_ += enqueue([msg], session)
        else:
            pid = session["next_pkt_id"]                                # :454
            session["inflight"].append(pid)                             # :455 await/3
            S.next_pkt_id(session)                                      # :456
            publishes.append((pid, msg))
    return publishes, dropped_


def window_one_prio(deliveries, st, table, plens):
    """handle_deliver/2 (src/emqx_channel.erl:657-680) for one inbox whose
    session's mqueue has a priority table: emqx_session.window_one's fold over
    emqx_mqueue:in/2 with get_priority/3.

    deliveries  [(qos, topic bytes)] in mailbox order
    st          a tm_session_state dict
    table       None (?NO_PRIORITY_TABLE) or {"priorities": {topic: priority},
                "default_priority": "lowest" | "highest" | int}
    plens       {priority: messages of that priority already in the queue};
                their sum is st's mqueue_len
    -> ([(disp, packet id or 0, class or TM_PRIO_NOCLASS)],
        (next_pkt_id, n_inflight, n_queued, n_dropped_old),
        {priority: (n_queued, n_dropped_old)} over classes_of(table))"""
    flags = st.get("flags", 0)
    classes = classes_of(table)
    if flags & S.TM_SESS_HOST:
        return ([(S.TM_DISP_HOST, 0, TM_PRIO_NOCLASS)] * len(deliveries), (st.get("next_pkt_id", 1), 0, 0, 0),
                {p: (0, 0) for p in classes})
    assert sum(plens.values()) == st.get("mqueue_len", 0) and all(p in classes for p, k in plens.items() if k)
    ptab = None if table is None else table["priorities"]
    dp = LOWEST_PRIORITY if table is None else table_default(table)
    mq = init({"max_len": st.get("mqueue_max", 0), "store_qos0": bool(flags & S.TM_SESS_STORE_QOS0),
               "priorities": ptab, "default_priority": dp})
    for p, k in plens.items():                                          # the queue of an earlier batch
        for j in range(k):
            mq = dict(mq, len=mq["len"] + 1, q=PQ.in_({"qos": 1, "old": j, "p": p}, p, mq["q"]))
    free = st.get("inflight_free", S.TM_SESS_UNBOUNDED)
    unb = free == S.TM_SESS_UNBOUNDED
    s = S.new_session(st.get("next_pkt_id", 1), 0 if unb else free + 1, [] if unb else [0], mq)
    msgs = [{"qos": q, "topic": t, "k": k} for k, (q, t) in enumerate(deliveries)]
    cls = [TM_PRIO_NOCLASS if table is None else classes.index(get_priority(t, ptab, dp)) for _, t in deliveries]
    res = [None] * len(msgs)
    n0 = len(s["inflight"])
    if flags & S.TM_SESS_DISCONNECTED:                                  # src/emqx_channel.erl:659-663
        dropped_ = enqueue(msgs, s)
    else:                                                               # :672-680
        publishes, dropped_ = deliver(msgs, s)
        for pid, m in publishes:
            res[m["k"]] = (S.TM_DISP_SEND0, 0) if pid is None else (S.TM_DISP_SEND, pid)
    per = {p: [0, 0] for p in classes}
    for m, entering in dropped_:
        if "old" in m:
            per[m["p"]][1] += 1
        elif m is entering:
            res[m["k"]] = (S.TM_DISP_DROP_QOS0, 0)
        else:
            res[m["k"]] = (S.TM_DISP_DROP_FULL, 0)
    mq = s["mqueue"]
    while True:                                                         # what the queue holds at the end
        r, mq = out(mq)
        if r == "empty":
            break
        m = r[1]
        if "old" not in m:
            res[m["k"]] = (S.TM_DISP_QUEUED, 0)
            per[get_priority(m["topic"], ptab, dp)][0] += 1
    assert all(r is not None for r in res)
    rec = (s["next_pkt_id"], len(s["inflight"]) - n0, sum(v[0] for v in per.values()), sum(v[1] for v in per.values()))
    return [(d, p, c) for (d, p), c in zip(res, cls)], rec, {p: tuple(v) for p, v in per.items()}


# ---------------------------------------------------------------------------
# The session drain (tm_sessions_drain): emqx_session:dequeue/1 over a queue
# rebuilt from its messages in arrival order, and the same without the pqueue
# for inputs too large for it.

def qmsg_of(qos: int, cls: int = 0, flagged: bool = False) -> int:
    """The qmsg byte of a queued message (include/emqx_tm.h)."""
    return qos | (S.TM_QMSG_EXPIRY if flagged else 0) | cls << 4


def drain_one(msgs, state, classes, now):
    """emqx_session:dequeue/1 (src/emqx_session.erl:389-395) for one session.

    msgs     [(qmsg byte, created_ms, expiry_s)] in arrival order, the order
             in/2 saw them; the two numbers matter only with TM_QMSG_EXPIRY
    state    {"next_pkt_id", "inflight_free"}
    classes  the priorities of the queue's table, highest first (classes_of);
             a message of class c has priority classes[c]
    -> ([(disp, packet id or 0, order, expiry_out)] per message,
        (next_pkt_id, n_send, n_send0, n_expired), popped per class (8 long))"""
    from . import emqx_message as M
    ptab = {c: p for c, p in enumerate(classes)}
    mq = init({"max_len": 0, "store_qos0": True, "priorities": ptab})
    for k, (b, created, expiry) in enumerate(msgs):
        m = {"qos": b & 3, "topic": (b >> 4) & 7, "k": k, "timestamp": created, "headers": {}}
        if b & S.TM_QMSG_EXPIRY:
            m["headers"] = {"properties": {M.EXPIRY: expiry}}
        d, mq = in_(m, mq)
        assert d is None
    free = state.get("inflight_free", S.TM_SESS_UNBOUNDED)
    unb = free == S.TM_SESS_UNBOUNDED
    s = S.new_session(state.get("next_pkt_id", 1), 0 if unb else free + 1, [] if unb else [0], mq)
    n0 = len(s["inflight"])
    publishes, expired = S.dequeue(s, now)
    res = [(S.TM_DRAIN_KEPT, 0, S.TM_DRAIN_NO_ORDER, e) for _, _, e in msgs]
    popped = [0] * TM_PRIO_MAX_CLASSES
    for m in expired:                                                   # 'delivery.dropped.expired'
        res[m["k"]] = (S.TM_DRAIN_EXPIRED, 0, S.TM_DRAIN_NO_ORDER, msgs[m["k"]][2])
        popped[m["topic"]] += 1
    n_send0 = 0
    for place, (pid, m) in enumerate(publishes):
        m1 = M.update_expiry(m, now)                                    # src/emqx_channel.erl:814
        e = m1["headers"]["properties"][M.EXPIRY] if msgs[m["k"]][0] & S.TM_QMSG_EXPIRY else msgs[m["k"]][2]
        res[m["k"]] = (S.TM_DRAIN_SEND0, 0, place, e) if pid is None else (S.TM_DRAIN_SEND, pid, place, e)
        n_send0 += pid is None
        popped[m["topic"]] += 1
    return res, (s["next_pkt_id"], len(s["inflight"]) - n0, n_send0, len(expired)), popped


def drain_flat(msgs, state, now):
    """drain_one without the pqueue, for queues too long for its fold: one
    deque per class, popped highest class first, the same clauses after the
    pop.  Same arguments (no classes: a class is its own index) and result."""
    from collections import deque
    qs = [deque() for _ in range(TM_PRIO_MAX_CLASSES)]
    for k, (b, _, _) in enumerate(msgs):                                # in/2: max_len 0, store_qos0
        qs[(b >> 4) & 7].append(k)
    free = state.get("inflight_free", S.TM_SESS_UNBOUNDED)
    cnt = S.DEFAULT_BATCH_N if free == S.TM_SESS_UNBOUNDED else free    # batch_n/1
    pid = state.get("next_pkt_id", 1)
    res = [(S.TM_DRAIN_KEPT, 0, S.TM_DRAIN_NO_ORDER, e) for _, _, e in msgs]
    popped = [0] * TM_PRIO_MAX_CLASSES
    n_send = n_send0 = n_expired = place = 0
    c = 0
    while cnt != 0:                                                     # dequeue/3
        while c < TM_PRIO_MAX_CLASSES and not qs[c]:
            c += 1
        if c == TM_PRIO_MAX_CLASSES:                                    # {empty, _Q}
            break
        k = qs[c].popleft()
        popped[c] += 1
        b, created, expiry = msgs[k]
        flagged = bool(b & S.TM_QMSG_EXPIRY)
        el = max(0, now - created) if flagged else 0                    # elapsed/1
        if flagged and el > 1000 * expiry:                              # is_expired/1
            res[k] = (S.TM_DRAIN_EXPIRED, 0, S.TM_DRAIN_NO_ORDER, expiry)
            n_expired += 1
            continue
        e = max(1, expiry - el // 1000) if flagged and el > 0 else expiry   # update_expiry/1
        if b & 3 == 0:                                                  # deliver_msg/2, QoS 0
            res[k] = (S.TM_DRAIN_SEND0, 0, place, e)
            n_send0 += 1
        else:
            res[k] = (S.TM_DRAIN_SEND, pid, place, e)
            pid = 1 if pid == 0xFFFF else pid + 1                       # next_pkt_id/1
            n_send += 1
            cnt -= 1                                                    # acc_cnt/2
        place += 1
    return res, (pid, n_send, n_send0, n_expired), popped
