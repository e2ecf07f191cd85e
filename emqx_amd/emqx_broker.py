"""emqx_broker mirror (src/emqx_broker.erl): the local subscriber bag and
publish -> dispatch, resolved on the device.

subscribe/unsubscribe/subscriber_down keep the ?SUBSCRIBER / ?SUBSCRIPTION
bags inside the engine (tm_subscribe / tm_unsubscribe / tm_subscriber_down);
the first subscriber of a topic adds its node() route and the last one removes
it, as the broker pool does through emqx_router (:438-469).  publish_batch runs
the whole publish path of a batch on the device: match (emqx_router:
match_routes/1) then fan-out (dispatch/2 for every local route,
tm_batch_dispatch).  The other local clause of do_route/2, {To, Group}
(:245-248), is emqx_shared_sub.dispatch_batch (tm_batch_dispatch_shared);
shared and non-shared subscribers share the pid -> u32 id map below, and
deliver_batch(shared=...) returns both kinds in one mailbox per pid
(tm_batch_shared_mode; mailboxes_shared is its host restatement).

Subscriber pids are arbitrary hashable terms here, mapped to u32 ids.
"""

from __future__ import annotations

from . import emqx_router as R

_ids = {}      # subscriber term -> u32 id
_terms = []    # id -> term


def _sid(pid) -> int:
    i = _ids.get(pid)
    if i is None:
        i = _ids[pid] = len(_terms)
        _terms.append(pid)
    return i


def _node_dest() -> int:
    return R._agg_id(R.NODE)


def clear_tables():
    global _ids, _terms, _topics_of, _nsubs
    R.clear_tables()
    _ids, _terms = {}, []
    _topics_of, _nsubs = {}, {}
    _order.clear()
    from . import emqx_shared_sub
    emqx_shared_sub.clear()        # its members lived in the engine that was just replaced


_topics_of = {}   # subscriber id -> [topic]: which node() routes subscriptions hold
_nsubs = {}       # topic -> local subscriber count
_order = {}       # topic -> [subscriber term], subscription order


def subscribe(topic: bytes, pid="self", subopts=None):
    """subscribe/1,2,3 -> do_subscribe/4, non-shared clause (:117-158).
    subopts: {qos, nl, rap, rh, subid}, merged over ?DEFAULT_SUBOPTS (:127-136);
    on an existing subscription only the options change (set_subopts/2)."""
    if not isinstance(topic, (bytes, bytearray)):
        raise TypeError("function_clause")
    topic, sid = bytes(topic), _sid(pid)
    if subopts is None:
        R.engine().subscribe(topic, sid, _node_dest())
    else:
        R.engine().subscribe_opts(topic, sid, dict(subopts), _node_dest())
    ts = _topics_of.setdefault(sid, [])
    if topic not in ts:
        ts.append(topic)
        _nsubs[topic] = _nsubs.get(topic, 0) + 1
        _order.setdefault(topic, []).append(pid)
        dests = R._routes.setdefault(topic, [])
        if R.NODE not in dests:
            dests.append(R.NODE)
    return "ok"


def _dropped(topic: bytes, sid: int):
    _topics_of[sid].remove(topic)
    _nsubs[topic] -= 1
    _order[topic].remove(_terms[sid])
    if not _nsubs[topic]:
        del _nsubs[topic]
        del _order[topic]
        dests = R._routes.get(topic, [])
        if R.NODE in dests:
            dests.remove(R.NODE)
        if not dests:
            R._routes.pop(topic, None)


def unsubscribe(topic: bytes, pid="self"):
    """unsubscribe/1 -> do_unsubscribe/4 (:168-191); `ok` whether subscribed or not."""
    topic, sid = bytes(topic), _sid(pid)
    if R.engine().unsubscribe(topic, sid, _node_dest()):
        _dropped(topic, sid)
    return "ok"


def subscriber_down(pid) -> int:
    """subscriber_down/1 (:332-347): drops every subscription of pid."""
    sid = _sid(pid)
    n = R.engine().subscriber_down(sid, _node_dest())
    for t in list(_topics_of.get(sid, [])):
        _dropped(t, sid)
    return n


def get_subopts(pid, topic: bytes):
    """get_subopts/2 (:373-386): the options map, or None for `undefined`."""
    return R.engine().get_subopts(bytes(topic), _sid(pid))


def set_subopts(topic: bytes, newopts: dict, pid="self") -> bool:
    """set_subopts/2 (:388-393): maps:merge(Old, New); False when not subscribed."""
    return R.engine().set_subopts(bytes(topic), _sid(pid), dict(newopts))


def subscriptions(pid):
    """subscriptions/1 (:349-356): [(Topic, SubOpts)] of pid, in subscription order."""
    sid = _sid(pid)
    return [(t, R.engine().get_subopts(t, sid)) for t in _topics_of.get(sid, [])]


def subscribers(topic: bytes):
    """subscribers/1 (:320-325): the topic's local subscribers in subscription
    order (host view of the bag the engine holds)."""
    return list(_order.get(bytes(topic), []))


def topics():
    """topics/0 (:402-404) = emqx_router:topics/0."""
    return R.topics()


def publish_batch(topic_list):
    """publish/1 -> route/2 -> dispatch/2 for a batch: per publish the list of
    deliveries (To, SubPid); To in Erlang binary order, each To's subscribers
    in subscription order.  [] is {error, no_subscribers}."""
    eng = R.engine()
    b = eng.prepare(topic_list)
    b.launch()
    b.wait()
    roff, ids = b.result()
    offs, moff, subs = b.dispatch(match_offsets=True)
    b.free()
    cache = {}
    out = []
    for i in range(len(topic_list)):
        row = []
        for j in range(int(roff[i]), int(roff[i + 1])):
            if moff[j] == moff[j + 1]:
                continue
            fid = int(ids[j])
            f = cache.get(fid)
            if f is None:
                f = cache[fid] = eng.filter_bytes(fid)
            row.extend((f, _terms[int(s)]) for s in subs[moff[j]:moff[j + 1]])
        assert len(row) == offs[i + 1] - offs[i]
        out.append(row)
    return out


def mailboxes(rows):
    """The `SubPid ! {deliver, To, Msg}` loop of dispatch/2 (:298-302) over the
    publishes of a batch in order, as mailboxes: rows[i] = publish i's
    deliveries [(To, pid)] -> {pid: [(i, To)]}, each list in arrival order --
    what emqx_misc:drain_deliver/1 (src/emqx_misc.erl:128-142) hands the
    session.  Pure host code."""
    boxes = {}
    for i, row in enumerate(rows):
        for to, pid in row:
            boxes.setdefault(pid, []).append((i, to))
    return boxes


def mailboxes_shared(rows, shared_rows):
    """mailboxes() with the shared deliveries in them: route/2 folds over
    aggre(match_routes(Topic)) (:209, 238-248), and within one filter To the
    {To, node()} route precedes every {To, Group} route (lists:usort orders an
    atom before a tuple, :255-261).  rows[i] = publish i's ordinary deliveries
    [(To, pid)] (publish_batch), shared_rows[i] = its picked shared deliveries
    [(To, Group, pid)] (emqx_shared_sub.dispatch_batch / _mirror), both with To
    in Erlang binary order; merged filter by filter -> {pid: [(i, To, Group |
    None)]} in arrival order.  With no shared row anywhere this is mailboxes()
    with None appended to every entry.  Pure host code."""
    boxes = {}
    for i, (row, srow) in enumerate(zip(rows, shared_rows)):
        for to in sorted({to for to, _ in row} | {to for to, _, _ in srow}):
            for t, pid in row:
                if t == to:
                    boxes.setdefault(pid, []).append((i, to, None))
            for t, group, pid in srow:
                if t == to:
                    boxes.setdefault(pid, []).append((i, to, group))
    return boxes


def deliver_batch(topic_list, shared=None):
    """publish_batch regrouped by subscriber on the device (tm_batch_inboxes):
    {pid: [(publish index, To)]}, every pid's list in mailbox order; equals
    mailboxes(publish_batch(topic_list)).
    shared = {"strategy": ..., "keys": ..., "seed": ...} arms the batch
    (tm_batch_shared_mode): the result is {pid: [(publish index, To, Group |
    None)]} and equals mailboxes_shared(publish_batch(topic_list),
    emqx_shared_sub.dispatch_batch_mirror(topic_list, strategy, keys, seed))
    for the hash and random strategies."""
    eng = R.engine()
    b = eng.prepare(topic_list)
    b.launch()
    b.wait()
    if shared is not None:
        b.shared_mode(shared["strategy"], keys=shared.get("keys"), seed=shared.get("seed", 0))
    subs, offs, pubs, fids = b.inboxes()
    groups = b.inbox_groups() if shared is not None else None
    b.free()
    cache = {}
    out = {}
    for r, s in enumerate(subs):
        box = []
        for q in range(int(offs[r]), int(offs[r + 1])):
            fid = int(fids[q])
            f = cache.get(fid)
            if f is None:
                f = cache[fid] = eng.filter_bytes(fid)
            if groups is None:
                box.append((int(pubs[q]), f))
            else:
                g = int(groups[q])
                box.append((int(pubs[q]), f, None if g == 0xFFFFFFFF else R._agg_of[g][1]))
        out[_terms[int(s)]] = box
    return out
