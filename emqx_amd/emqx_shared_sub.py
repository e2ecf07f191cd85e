"""emqx_shared_sub mirror (src/emqx_shared_sub.erl): membership, routes and the
dispatch of shared subscriptions, resolved on the device.

A shared subscription `$share/Group/Topic` is routed as `#route{topic = Topic,
dest = {Group, node()}}`: the group's first member on a node adds that route and
its last member (unsubscribe or process down) deletes it (:297-315, 358-367).
On the device the route aggregates to the Group (emqx_broker:aggre/1,
src/emqx_broker.erl:250-261), so `emqx_router.aggre_batch` returns `(To, Group)`
pairs for it.

subscribe / unsubscribe / member_down keep the ?SHARED_SUBS bag inside the
engine too (tm_shared_subscribe / _unsubscribe / _member_down; the engine adds
and deletes the group's route itself, this module only books it in the host
route table), and `dispatch_batch` runs do_route({To, Group}, _)
(src/emqx_broker.erl:245-248) for a batch on the device: one member per
(publish, matched filter, group), picked by the random / round_robin / hash
strategy (tm_batch_dispatch_shared).  subscribe(..., subopts=...) stores the
member's subscription options too (tm_shared_subscribe_opts), and
emqx_broker.deliver_batch(shared=...) puts the picked deliveries into the
members' mailboxes (tm_batch_shared_mode).

pick/5, do_pick/5, pick_subscriber/5 and do_pick_subscriber/5 below restate
:229-275 clause by clause on the CPU; `dispatch_batch_mirror` is the batch
built from them, which the tests hold the device against.  Two deviations, both
the device's (include/emqx_tm.h):
  - round_robin keeps its counter per (Group, Topic) instead of per publishing
    process (a batch has no publisher identity);
  - random is a hash of (seed, publish index, filter id, group id)
    (`random_nth`) instead of rand:uniform/1.
The sticky strategy (per-publisher state) and the ack / nack redispatch with
FailedSubs (:113-125, 160-184) stay on the host.
"""

from __future__ import annotations

from . import emqx_broker as B
from . import emqx_router as R
from . import emqx_topic as T

_members = {}   # (group, topic) -> [subpid] (?SHARED_SUBS bag, insertion order)
_of_pid = {}    # subpid -> [(group, topic)] (the mnesia ?TAB records of the pid)
_groups_of = {}  # topic -> [group] in first-added order (the order of the topic's group routes)
_rr = {}        # (group, topic) -> N, the {shared_sub_round_robin, Group, Topic} counter

_M64 = (1 << 64) - 1
_G = 0x9E3779B97F4A7C15


def clear():
    _members.clear()
    _of_pid.clear()
    _groups_of.clear()
    _rr.clear()


def subscribe(group, topic: bytes, subpid, node=R.NODE, subopts=None):
    """handle_call({subscribe, Group, Topic, SubPid}) (:297-305).
    subopts ({qos, nl, rap, rh, subid}): emqx_broker:subscribe/3 with share =>
    Group (src/emqx_broker.erl:127-136) in front of it -- the options are
    stored under {SubPid, Topic} (tm_shared_subscribe_opts); when that key has
    options already, shared or not, only they merge (the `Existed` branch,
    :129-135) and the membership does not change."""
    topic = bytes(topic)
    key = (group, topic)
    dest = (group, node)
    gid, sid = R._agg_id(dest), B._sid(subpid)
    ms = _members.get(key)
    eng = R.engine()
    if subopts is not None and eng.get_subopts(topic, sid) is not None:
        eng.shared_subscribe_opts(topic, gid, sid, dict(subopts))   # Existed: merges, nothing else
        return "ok"

    def join():
        if subopts is None:
            eng.shared_subscribe(topic, gid, sid)
        else:
            eng.shared_subscribe_opts(topic, gid, sid, dict(subopts))

    if ms is None:                                    # not ets:member(?SHARED_SUBS, {Group, Topic})
        dests = R._routes.setdefault(topic, [])
        had = dest in dests                           # lists:member(Route, lookup_routes(Topic))
        join()                                        # adds the route (topic, Group) with the first member
        if had:
            eng.route_delete(topic, gid)              # the table already held this route: one reference, not two
        else:
            dests.append(dest)
        ms = _members[key] = []
        _groups_of.setdefault(topic, []).append(group)
    else:
        join()
    if subpid not in ms:                              # a bag stores an identical object once
        ms.append(subpid)
        _of_pid.setdefault(subpid, []).append(key)
    return "ok"


def unsubscribe(group, topic: bytes, subpid, node=R.NODE):
    """handle_call({unsubscribe, Group, Topic, SubPid}) (:307-315)."""
    key = (group, bytes(topic))
    ms = _members.get(key)
    if ms and subpid in ms:
        ms.remove(subpid)
        ks = _of_pid[subpid]
        ks.remove(key)
        if not ks:
            del _of_pid[subpid]
        R.engine().shared_unsubscribe(key[1], R._agg_id((group, node)), B._sid(subpid))   # the last member's
        #                                                                                  deletes the route
    if key in _members and not _members[key]:
        del _members[key]
        _rr.pop(key, None)
        gs = _groups_of[key[1]]
        gs.remove(group)
        if not gs:
            del _groups_of[key[1]]
        dests = R._routes.get(key[1], [])
        if (group, node) in dests:
            dests.remove((group, node))
        if not dests:
            R._routes.pop(key[1], None)
    return "ok"


def member_down(subpid, node=R.NODE) -> int:
    """cleanup_down/1 (:358-367) on the subscriber's 'DOWN'."""
    keys = list(_of_pid.get(subpid, []))
    for g, t in keys:
        unsubscribe(g, t, subpid, node)
    return len(keys)


def subscribers(group, topic: bytes):
    """subscribers/2: the group's members for the topic."""
    return list(_members.get((group, bytes(topic)), []))


# ---- pick: :229-275 ---------------------------------------------------------

def _mix(z: int) -> int:
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def random_nth(seed: int, publish: int, filter_id: int, group_id: int, count: int) -> int:
    """The device's stand-in for rand:uniform(Count) (include/emqx_tm.h,
    TM_SHARED_RANDOM): 1 + (r >> 32) rem Count."""
    z = _mix((seed + _G * (publish + 1)) & _M64)
    r = _mix(((z ^ ((filter_id << 32) | group_id)) + _G) & _M64)
    return 1 + (r >> 32) % count


def do_pick_subscriber(group, topic, strategy, client_id, count, rnd=None):
    """do_pick_subscriber/5 (:265-275) -> Nth, 1-based.  client_id is the
    publisher's erlang:phash2(ClientId); rnd = (seed, publish index, filter
    id, group id) of the delivery."""
    if strategy == "random":
        return random_nth(*rnd, count)
    if strategy == "hash":
        return 1 + client_id % count
    if strategy == "round_robin":
        n = _rr.get((group, topic))
        rem = 0 if n is None else (n + 1) % count
        _rr[(group, topic)] = rem
        return rem + 1
    raise ValueError("function_clause")


def pick_subscriber(group, topic, strategy, client_id, subs, rnd=None):
    """pick_subscriber/5 (:260-263)."""
    if len(subs) == 1:
        return subs[0]
    nth = do_pick_subscriber(group, topic, strategy, client_id, len(subs), rnd)
    return subs[nth - 1]                               # lists:nth(Nth, Subs)


def do_pick(strategy, client_id, group, topic, failed_subs, rnd=None):
    """do_pick/5 (:246-258) -> False | ('retry' | 'fresh', Sub)."""
    all_ = subscribers(group, topic)
    subs = [s for s in all_ if s not in failed_subs]   # All -- FailedSubs (members are distinct)
    if not subs and not failed_subs:
        return False
    if not subs:
        return ("retry", pick_subscriber(group, topic, strategy, client_id, all_, rnd))
    return ("fresh", pick_subscriber(group, topic, strategy, client_id, subs, rnd))


def pick(strategy, client_id, group, topic, failed_subs=(), rnd=None):
    """pick/5 (:229-244); sticky keeps per-publisher state and is not restated."""
    if strategy == "sticky":
        raise NotImplementedError("sticky depends on the publishing process")
    return do_pick(strategy, client_id, group, topic, list(failed_subs), rnd)


def dispatch_batch_mirror(topic_list, strategy, keys=None, seed=0, matched=None):
    """dispatch_batch on the CPU, publish by publish in order: the matched
    filters in Erlang binary order (emqx_topic:match/2 over the shared
    filters, or matched(name) -> the filters matching it, for big tables), a
    filter's groups in first-added order, pick/5 for each."""
    flts = sorted(_groups_of)
    fids = {}
    out = []
    for i, name in enumerate(topic_list):
        name = bytes(name)
        row = []
        if matched is None:
            tos = [to for to in flts if T.match(name, to)]
        else:
            tos = sorted(to for to in set(matched(name)) if to in _groups_of)
        for to in tos:
            for group in _groups_of[to]:
                rnd = None
                if strategy == "random":
                    if to not in fids:
                        fids[to] = R.engine().filter_id(to)
                    rnd = (seed, i, fids[to], R._agg_id((group, R.NODE)))
                p = pick(strategy, None if keys is None else int(keys[i]), group, to, (), rnd)
                if p:
                    row.append((to, group, p[1]))
        out.append(row)
    return out


def dispatch_batch(topic_list, strategy, keys=None, seed=0):
    """emqx_shared_sub:dispatch/3 for every {To, Group} route of every publish of
    a batch, on the device: per publish [(To, Group, SubPid)], To in Erlang
    binary order, a To's groups in first-added order."""
    eng = R.engine()
    b = eng.prepare(topic_list)
    b.launch()
    b.wait()
    offs, fids, groups, subs = b.dispatch_shared(strategy, keys=keys, seed=seed)
    b.free()
    cache = {}
    out = []
    for i in range(len(topic_list)):
        row = []
        for k in range(int(offs[i]), int(offs[i + 1])):
            fid = int(fids[k])
            f = cache.get(fid)
            if f is None:
                f = cache[fid] = eng.filter_bytes(fid)
            row.append((f, R._agg_of[int(groups[k])][1], B._terms[int(subs[k])]))
        out.append(row)
    return out
