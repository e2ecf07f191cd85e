"""One batch carried through the sizes at which its mirrored result arrays are
created, grown and used at length zero.

Every array a batch result call hands out is a device block with a pinned
mirror, both allocated on first use with at least 1,024 elements and grown by a
quarter past what is asked.  One engine, one batch handle, prepared four times:
results of a few hundred elements (everything fits the first blocks), results
past 1,280 elements in every array (every block is reallocated), topics that
match nothing (every total 0, every copy of length 0, the pointers still
there), and the second set again (blocks that shrank in use are reused).
After each prepare every result call runs in its host and device forms and is
compared with the Python models the per-feature suites use.  All comparisons
are exact."""

import ctypes as C
import random

import numpy as np
import pytest
from test_gpu_inbox import assert_inboxes, reference
from test_gpu_session_window import _device_arrays as window_arrays
from test_gpu_session_window import check as check_window
from test_gpu_session_window import state, table
from test_gpu_shared_inbox import mirror  # noqa: F401  (the fixture)
from test_gpu_shared_inbox import armed, assert_merged, device_session, merged_session, reference_merged
from test_gpu_subopts import _device_arrays as deliver_arrays
from test_gpu_subopts import check as check_deliver
from test_gpu_subopts import own_mailboxes

from emqx_amd import _native as N
from emqx_amd import emqx_broker as B
from emqx_amd import emqx_router as R
from emqx_amd import emqx_shared_sub as S
from emqx_amd.engine import _d2h
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NONE = N.TM_NONE
NF, PER = 400, 4              # filters m/<i>, subscribers of each
NL_PID, HASH_PID, PLUS_PID = 1, 2, 3
MEMBERS = (4, 5, 10)          # of group g on m/+; 10 is m/0's first subscriber too
FIRST = 10                    # m/<i>'s subscribers: FIRST + PER * i ...
MIN_BLOCK, GROWN = 1024, 1280


def build():
    """-> (oracle broker, {pid: {topic: opts}}); pids are registered in order,
    so a pid is its subscriber id."""
    npids = FIRST + NF * PER
    assert [B._sid(p) for p in range(npids)] == list(range(npids))
    orc = O.Broker()
    model = {}
    rng = random.Random(77)

    def sub(f, pid, o):
        B.subscribe(f, pid, o)
        orc.subscribe(f, pid)
        model.setdefault(pid, {})[f] = o

    sub(b"#", NL_PID, {"qos": 1, "nl": 1})                 # the No-Local subscription: pid 1 also publishes
    sub(b"#", HASH_PID, {"qos": 2})
    sub(b"m/+", PLUS_PID, {"qos": 1, "rap": 1, "subid": 7})
    for i in range(NF):
        for k in range(PER):
            pid = FIRST + PER * i + k
            sub(b"m/%d" % i, pid, {"qos": rng.randrange(3), "rap": rng.randrange(2), "subid": rng.choice([0, pid])})
    for pid in MEMBERS:
        S.subscribe("g", b"m/+", pid)
    return orc, model


class Ref:
    """The models' answers for one list of topics, computed once."""

    def __init__(self, orc, T, seed):
        rng = random.Random(seed)
        self.T = T
        self.keys = [rng.getrandbits(32) for _ in T]
        self.msg = [rng.randrange(3) | rng.choice([0, 4]) | rng.choice([0, 8]) for _ in T]
        self.fr = [NL_PID if i % 3 != 2 else None for i in range(len(T))]    # publish 0 and 1: pid 1's leading run
        self.rows = [orc.publish(t) for t in T]
        self.srows = S.dispatch_batch_mirror(T, "hash", keys=self.keys)
        rt = O.RouteTable()
        for to, dests in R._routes.items():
            for d in dests:
                rt.write(to, d)
        self.routes = [[(to, R.aggregate(d)[1]) for to in sorted({to for to, _ in O.match_routes(rt.trie, rt.routes, t)})
                        for d in rt.routes[to]] for t in T]
        self.boxes = B.mailboxes(self.rows)
        self.boxes_shared = B.mailboxes_shared(self.rows, self.srows)
        self.n_routes = sum(map(len, self.routes))
        self.n_ord = sum(map(len, self.rows))
        self.n_shared = sum(map(len, self.srows))


def d2h(ptr, k, ty=np.uint32):
    assert ptr
    a = np.zeros(k, ty)
    _d2h(a, ptr)
    return a


def offsets(rows, ty):
    return np.cumsum([0] + [len(r) for r in rows]).astype(ty)


def check_routes(eng, b, ref):
    offs, fids, dests = b.routes()
    name = {f: eng.filter_bytes(f) for f in set(fids.tolist())}
    got = [(name[f], R._agg_of[d][1]) for f, d in zip(fids.tolist(), dests.tolist())]
    assert np.array_equal(offs, offsets(ref.routes, np.uint32))
    assert got == [x for row in ref.routes for x in row]


def check_dispatch(eng, b, ref):
    n = len(ref.T)
    roff, ids = b.result()
    want_offs = offsets(ref.rows, np.uint64)
    want_subs = np.asarray([pid for row in ref.rows for _, pid in row], np.uint32)
    name = {f: eng.filter_bytes(f) for f in set(ids.tolist())}
    want_moff = np.cumsum([0] + [len(B.subscribers(name[f])) for f in ids.tolist()]).astype(np.uint64)
    offs, moff, subs = b.dispatch(match_offsets=True)
    assert np.array_equal(offs, want_offs) and np.array_equal(moff, want_moff) and np.array_equal(subs, want_subs)
    offs, moff, subs = b.dispatch()
    assert np.array_equal(offs, want_offs) and moff is None and np.array_equal(subs, want_subs)
    offs, moff, subs = b.dispatch(counts_only=True)
    assert np.array_equal(offs, want_offs) and moff is None and subs is None
    total, _, d_row, d_moff, d_subs = b.dispatch_device(match_offsets=True)
    assert total == ref.n_ord
    assert np.array_equal(d2h(d_row, n + 1, np.uint64), want_offs)
    assert np.array_equal(d2h(d_moff, len(ids) + 1, np.uint64), want_moff)
    assert np.array_equal(d2h(d_subs, total), want_subs)


def check_shared(eng, b, ref):
    n = len(ref.T)
    want_offs = offsets(ref.srows, np.uint32)
    offs, fids, grps, subs = b.dispatch_shared("hash", keys=ref.keys)
    name = {f: eng.filter_bytes(f) for f in set(fids.tolist())}
    got = [(name[f], R._agg_of[g][1], s) for f, g, s in zip(fids.tolist(), grps.tolist(), subs.tolist())]
    assert np.array_equal(offs, want_offs) and got == [x for row in ref.srows for x in row]
    c_offs, none = b.dispatch_shared("hash", keys=ref.keys, counts_only=True)[:2]
    assert np.array_equal(c_offs, want_offs) and none is None
    total, _, d_row, d_fid, d_grp, d_sub = b.dispatch_shared_device("hash", keys=ref.keys)
    assert total == ref.n_shared and np.array_equal(d2h(d_row, n + 1), want_offs)
    for ptr, want in ((d_fid, fids), (d_grp, grps), (d_sub, subs)):
        assert np.array_equal(d2h(ptr, total), want)


def check_inboxes(eng, b, ref):
    got = b.inboxes()
    assert_inboxes(got, reference(b))
    assert own_mailboxes(eng, b) == ref.boxes
    r, d, _, _, d_sub, d_off, d_pub, d_fid = b.inboxes_device()
    assert (r, d) == (len(ref.boxes), ref.n_ord)
    assert_inboxes([d2h(d_sub, r), d2h(d_off, r + 1), d2h(d_pub, d), d2h(d_fid, d)], got)


def check_armed(b, ref, model):
    """The merged inboxes and their groups, then deliver with drops over them:
    the groups are compacted with the deliveries."""
    b.shared_mode("hash", keys=ref.keys)
    got = armed(b)
    assert_merged(got, reference_merged(b, "hash", ref.keys))
    assert len(got[2]) == ref.n_ord + ref.n_shared
    assert np.array_equal(d2h(b.inbox_groups_device(), len(got[4])), got[4])
    want, dropped = merged_session(ref.boxes_shared, model, ref.fr, ref.msg)
    fr = [NONE if f is None else f for f in ref.fr]
    dlv = b.deliver(fr, ref.msg, subids=True)
    grp = b.inbox_groups()
    assert len(grp) == len(dlv[2]) == ref.n_ord + ref.n_shared - dropped
    assert b.deliver_info["n_dropped_no_local"] == dropped and (dropped > 0) == (ref.n_ord > 0)
    assert device_session(dlv, grp) == want
    d = b.deliver_device(fr, ref.msg, subids=True)
    assert np.array_equal(d2h(b.inbox_groups_device(), d[1]), grp)
    b.shared_mode(None)


def check_deliver_forms(eng, b, ref, model):
    fr_drop = [NONE if f is None else f for f in ref.fr]
    fr_keep = [HASH_PID] * len(ref.T)            # a publisher without a No-Local subscription: the drop path, nothing dropped
    res = check_deliver(eng, b, model, None, ref.msg, modes=[(False, False)])
    assert res[(False, False)][1] == 0
    res = check_deliver(eng, b, model, fr_keep, ref.msg, modes=[(False, False)])
    assert res[(False, False)][1] == 0
    res = check_deliver(eng, b, model, fr_drop, ref.msg, modes=[(False, False), (True, False)])
    if ref.n_ord:
        assert 0 < res[(False, False)][1] < res[(True, False)][1]
    for fr in (None, fr_keep, fr_drop):
        host = b.deliver(fr, ref.msg, subids=True)
        d = b.deliver_device(fr, ref.msg, subids=True)
        assert d[2] == b.deliver_info["n_dropped_no_local"]
        for g, w in zip(deliver_arrays(d, True), host):
            assert np.array_equal(g, w)


def check_window_forms(b, ref):
    fr_drop = [NONE if f is None else f for f in ref.fr]
    states = {NL_PID: state(65530, 3, 0, 2), PLUS_PID: state(9, 0, 1, 4, N.TM_SESS_DISCONNECTED), FIRST + 1: state(1, 1)}
    dflt = state(100, 2, 0, 3)
    for fr in (None, fr_drop):
        check_window(b, states, dflt, fr, ref.msg, subids=True)
        host = b.window(table(states), dflt, fr, ref.msg, subids=True)
        totals = list(b.window_info["totals"])
        d = b.window_device(table(states), dflt, fr, ref.msg, subids=True)
        assert b.window_info["totals"] == totals and sum(totals) == d[1]
        dev = window_arrays(d)
        for g, w in zip(dev[:5], host[0][:5]):
            assert np.array_equal(g, w)
        assert np.array_equal(d2h(d[7], d[1]), host[0][5])
        assert np.array_equal(dev[5], host[1]) and np.array_equal(dev[6], host[2])
        assert np.array_equal(dev[7].reshape(-1, 4), host[3])


def check_zero(eng, b, ref):
    """Every count 0, the offsets {0}, and every pointer that is handed out
    still a pointer, in the host and the device forms."""
    n = len(ref.T)
    fr = [NL_PID] * n
    r = N.Routes()
    N.check(eng.L.tm_batch_routes(eng.h, b.h, C.byref(r)), "tm_batch_routes")
    assert r.n_routes == 0 and r.row_offsets and r.filter_ids and r.dests
    assert np.ctypeslib.as_array(r.row_offsets, shape=(n + 1,)).tolist() == [0] * (n + 1)
    for flags in (N.TM_DISPATCH_MATCH_OFFSETS, N.TM_DISPATCH_MATCH_OFFSETS | N.TM_DISPATCH_DEVICE):
        d = b._dispatch(flags)
        assert d.n_matches == 0 and d.n_deliveries == 0 and d.row_offsets and d.match_offsets and d.subscribers
    assert np.ctypeslib.as_array(b._dispatch(N.TM_DISPATCH_MATCH_OFFSETS).match_offsets, shape=(1,)).tolist() == [0]
    for flags in (0, N.TM_SHARED_DEVICE):
        s = b._dispatch_shared("hash", ref.keys, 0, flags)
        assert s.n_deliveries == 0 and s.row_offsets and s.filter_ids and s.groups and s.subscribers
    for flags in (0, N.TM_INBOX_DEVICE):
        i = b._inboxes(flags)
        assert i.n_subscribers == 0 and i.n_deliveries == 0 and i.passes == 0
        assert i.subscribers and i.inbox_offsets and i.publishes and i.filter_ids
    assert np.ctypeslib.as_array(b._inboxes(0).inbox_offsets, shape=(1,)).tolist() == [0]
    assert d2h(b.inboxes_device()[5], 1).tolist() == [0]
    for dev in (0, N.TM_DELIVER_DEVICE):
        for who in (None, fr):
            s, _keep = b._deliver(who, ref.msg, N.TM_DELIVER_SUBIDS | dev)
            assert s.n_subscribers == 0 and s.n_deliveries == 0 and s.n_dropped_no_local == 0
            assert s.subscribers and s.inbox_offsets and s.publishes and s.filter_ids and s.msg and s.subids
            off = C.cast(s.inbox_offsets, C.c_void_p).value
            assert (d2h(off, 1) if dev else np.ctypeslib.as_array(s.inbox_offsets, shape=(1,))).tolist() == [0]
    for dev in (0, N.TM_WINDOW_DEVICE):
        w, _keep = b._window([], None, fr, ref.msg, N.TM_DELIVER_SUBIDS, dev)
        assert w.inboxes.n_deliveries == 0 and list(w.totals) == [0] * N.TM_DISP_COUNT
        assert w.inboxes.inbox_offsets and w.inboxes.msg and w.disp and w.packet_ids and w.records
    b.shared_mode("hash", keys=ref.keys)
    got = armed(b)
    assert [len(a) for a in got] == [0, 1, 0, 0, 0] and got[1].tolist() == [0]
    assert b.inbox_groups_device()
    b.shared_mode(None)


def test_one_batch_through_small_grown_zero_and_grown_again(mirror):  # noqa: F811
    eng = mirror
    orc, model = build()
    small = Ref(orc, [b"m/%d" % i for i in range(60)], 1)
    big = Ref(orc, [b"m/%d" % (i * 7 % NF) for i in range(1400)], 2)
    zero = Ref(orc, [b"$none/%d" % i for i in range(40)], 3)
    # the sizes the stages stand for, on the models alone: every result array of
    # `small` fits a first block, every one of `big` needs a block past the first growth
    for ref, fits in ((small, True), (big, False)):
        sizes = [len(ref.T), ref.n_routes, ref.n_ord, ref.n_shared, len(ref.boxes), len(ref.boxes_shared)]
        assert all(0 < x + 1 < MIN_BLOCK for x in sizes) if fits else all(x > GROWN for x in sizes), sizes
    assert zero.n_routes == zero.n_ord == zero.n_shared == 0 and len(zero.T) > 0
    b = None
    for ref in (small, big, zero, big):
        b = eng.prepare(ref.T) if b is None else b.reprepare(ref.T)
        b.launch()
        b.wait()
        check_routes(eng, b, ref)
        check_dispatch(eng, b, ref)
        check_shared(eng, b, ref)
        check_inboxes(eng, b, ref)
        check_armed(b, ref, model)
        check_deliver_forms(eng, b, ref, model)
        check_window_forms(b, ref)
        if ref is zero:
            check_zero(eng, b, ref)
    b.free()
