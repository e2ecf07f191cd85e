"""The session's send window on the device (tm_batch_window): packet ids,
inflight, mqueue per delivery.  The reference of every case is
emqx_session.window_one -- the literal folds of deliver/2, enqueue/2 and
emqx_mqueue:in/2 -- over the batch's own deliver() result.  The conditions a
case relies on (every disposition occurs, a wrap, an edge inside a tile ...)
are asserted on the mirror alone before the device result is looked at.  All
comparisons are exact."""

import random

import numpy as np
import pytest
from conftest import load_golden

from emqx_amd import _native as N
from emqx_amd import emqx_broker as B
from emqx_amd import emqx_router as R
from emqx_amd import emqx_session as S
from emqx_amd.engine import Engine, _d2h

pytestmark = pytest.mark.gpu

NONE = N.TM_NONE
UNB = N.TM_SESS_UNBOUNDED
DISC, STORE, HOST = N.TM_SESS_DISCONNECTED, N.TM_SESS_STORE_QOS0, N.TM_SESS_HOST
DEFAULTS = {"next_pkt_id": 1, "flags": 0, "inflight_free": UNB, "mqueue_len": 0, "mqueue_max": 0}


def state(P=1, F=UNB, L=0, M=0, flags=0):
    return {"next_pkt_id": P, "flags": flags, "inflight_free": F, "mqueue_len": L, "mqueue_max": M}


def run(eng, topics, **kw):
    b = eng.prepare(topics, **kw)
    b.launch()
    b.wait()
    return b


def table(states):
    return [dict(states[s], subscriber=s) for s in sorted(states)]


def mirror(dlv, states, defaults):
    """deliver()'s arrays through the mirror -> (disp, packet ids, records, totals, {sub: (list, record)})."""
    subs, offs, _, _, msg, _ = dlv
    offs, qos = offs.tolist(), (msg & 3).tolist()
    disp, pids, recs, per = [], [], [], {}
    for r, s in enumerate(subs.tolist()):
        got, rec = S.window_one(qos[offs[r]:offs[r + 1]], states.get(s, defaults))
        disp += [d for d, _ in got]
        pids += [p for _, p in got]
        recs.append(rec)
        per[s] = (got, rec)
    totals = [disp.count(k) for k in range(N.TM_DISP_COUNT)]
    return disp, pids, recs, totals, per


def compare(b, got, want, dlv):
    inb, disp, pids, recs = got
    assert disp.dtype == np.uint8 and pids.dtype == np.uint16 and recs.dtype == np.uint32
    for g, w in zip(inb, dlv):   # the tm_session_inboxes part IS deliver()'s result
        assert (g is None and w is None) or np.array_equal(g, w)
    assert len(disp) == len(pids) == len(dlv[4]) and recs.shape == (len(dlv[0]), 4)
    assert disp.tolist() == want[0]
    assert pids.tolist() == want[1]
    assert [tuple(r) for r in recs.tolist()] == want[2]
    assert b.window_info["totals"] == want[3] and sum(want[3]) == len(disp)


def check(b, states, defaults=DEFAULTS, from_=None, msg=None, **kw):
    """window() against the mirror over deliver() of the same options."""
    dlv = b.deliver(from_, msg, **kw)
    want = mirror(dlv, states, defaults)
    got = b.window(table(states), defaults, from_, msg, **kw)
    compare(b, got, want, dlv)
    return want


# ------------------------------------------------------- 1. the known answers

def test_kats_on_the_device():
    eng = Engine(device=0)
    PID = 7
    eng.subscribe_opts(b"k", PID, {"qos": 2})
    ran = 0
    for c in load_golden("kat_session_window.json")["cases"]:
        k = c.get("repeat", 1)
        qos, disp = c["qos"] * k, c["disp"] * k
        pids = c["packet_ids"] * k if c["packet_ids"] is not None else [c["first_packet_id"] + i for i in range(len(qos))]
        b = run(eng, [b"k"] * len(qos))
        for sessions, defaults in (([dict(c["state"], subscriber=PID)], DEFAULTS), ([], c["state"]),
                                   ([dict(DEFAULTS, subscriber=6)], c["state"])):
            inb, gd, gp, gr = b.window(sessions, defaults, None, qos)
            assert inb[0].tolist() == [PID] and inb[1].tolist() == [0, len(qos)] and inb[4].tolist() == qos, c["name"]
            assert gd.tolist() == disp and gp.tolist() == pids and gr.tolist() == [c["record"]], c["name"]
            assert b.window_info["totals"] == [disp.count(x) for x in range(N.TM_DISP_COUNT)]
        b.free()
        ran += 1
    assert ran >= 13
    eng.close()


# ------------------------------------------------------------ 2. random churn

def random_states(rng, sids):
    states = {}
    for s in sids:
        if rng.random() < 1 / 3:
            continue   # uses the defaults
        M = rng.choice([0, 1, 3, 10, 40])
        L = rng.randrange(M + 1) if M else rng.randrange(5)
        flags = rng.choice([0, 0, 0, DISC, DISC | STORE, STORE]) | (HOST if rng.random() < 0.05 else 0)
        states[s] = state(rng.choice([rng.randrange(65500, 65536), rng.randrange(1, 65536)]),
                          rng.choice([0, 1, 3, 12, UNB]), L, M, flags)
    return states


def test_random_churn():
    from test_gpu_subopts import churn_case
    T, rows, model, from_, msg = churn_case()
    boxes = B.mailboxes(rows)
    inboxes, _ = S.session_inboxes(boxes, model, from_, msg)
    rng = random.Random(23)
    pstates = random_states(rng, sorted(inboxes))
    defaults = state(65530, 2, 1, 2, 0)
    want = S.session_window(inboxes, pstates, defaults)
    # the conditions, on the mirror alone
    seen = {d for got, _ in want.values() for d, _ in got}
    assert seen == set(range(N.TM_DISP_COUNT))
    assert any(rec[3] > 0 and any(d == N.TM_DISP_DROP_FULL for d, _ in got) for got, rec in want.values())
    assert any(rec[0] < pstates.get(p, defaults)["next_pkt_id"] and rec[1] > 0 for p, (_, rec) in want.items())   # a wrap
    assert any(p not in pstates for p in want) and any(p in pstates for p in want)
    eng = R.engine()
    sid_from = [NONE if f is None else B._sid(f) for f in from_]
    b = run(eng, T)
    states = {B._sid(p): s for p, s in pstates.items()}
    inb, disp, pids, recs = b.window(table(states), defaults, sid_from, msg)
    offs = inb[1].tolist()
    have = {}
    for r, s in enumerate(inb[0].tolist()):
        have[B._terms[s]] = (list(zip(disp[offs[r]:offs[r + 1]].tolist(), pids[offs[r]:offs[r + 1]].tolist())),
                             tuple(recs[r].tolist()))
    assert have.keys() == want.keys()
    for p in want:
        assert have[p] == want[p], p
    check(b, states, defaults, sid_from, msg, nl_all=True, upgrade_qos=True, subids=True)
    b.free()
    B.clear_tables()


# ------------------------------------------------------ 3. tile and wave edges

def test_tile_and_wave_edges():
    eng = Engine(device=0)
    tile = eng.L.tm_inbox_tile()
    FIRST, H, LAST = 0, 5, 0xFFFFFFF0
    eng.subscribe_opts(b"z/y", FIRST, {"qos": 2})
    eng.subscribe_opts(b"h/x", H, {"qos": 2})
    eng.subscribe_opts(b"l/x", LAST, {"qos": 1})
    n1 = 2 * tile + 12                        # QoS-1 deliveries of H's inbox
    pattern = ([1] * 5 + [0]) * (n1 // 5 + 1)
    hq = pattern[:n1 + n1 // 5]               # a QoS-0 delivery after every 5th: rank != position
    assert hq.count(1) == n1 and hq[5] == 0 and hq[4] == hq[6] == 1
    for lead in (0, 3):
        T = [b"z/y"] * lead + [b"h/x"] * len(hq) + [b"l/x"] * 2
        msg = [2] * lead + hq + [1, 1]
        b = run(eng, T)
        subs, offs, _, _, dm, _ = b.deliver(None, msg)
        assert subs.tolist() == ([FIRST] if lead else []) + [H, LAST] and int(offs[-3]) == lead
        assert dm[lead:lead + len(hq)].tolist() == hq
        for k in (64, 1024, tile, 2 * tile):
            for e in (k - 1, k, k + 1):
                # connected: the window edge F at e
                st = {H: state(65000, e, 2, 0), LAST: state(65535, 1, 0, 1), FIRST: state(9, 0, 1, 1, DISC)}
                want = check(b, st, DEFAULTS, None, msg)
                got, rec = want[4][H]
                assert rec[1] == e and rec[2] == n1 - e
                ranks = [i for i, q in enumerate(hq) if q]
                assert got[ranks[e - 1]][0] == N.TM_DISP_SEND and got[ranks[e]][0] == N.TM_DISP_QUEUED
                # disconnected: the drop edge drops - n_dropped_old at e
                st[H] = state(17, 3, 7, n1 - e, DISC)
                want = check(b, st, DEFAULTS, None, msg)
                got, rec = want[4][H]
                assert rec == (17, 0, n1 - e, 7)
                assert got[ranks[e - 1]][0] == N.TM_DISP_DROP_FULL and got[ranks[e]][0] == N.TM_DISP_QUEUED
                assert got[5][0] == N.TM_DISP_DROP_QOS0
        b.free()
    eng.close()


# -------------------------------------------------------------- 4. hot inbox

def test_hot_inbox():
    eng = Engine(device=0)
    tile = eng.L.tm_inbox_tile()
    HOT = 70000
    eng.subscribe_opts(b"#", HOT, {"qos": 2})
    for i in range(4000):
        eng.subscribe_opts(b"f/%d" % i, (100 + i) if i < 2000 else (80000 + i), {"qos": 1})
    n = 2 * tile + 900
    T = [b"f/%d" % (i // 2) if (i % 2 == 0 and i < 8000) else b"g/%d" % (i % 7) for i in range(n)]
    msg = [i % 3 for i in range(n)]
    b = run(eng, T)
    subs, offs, _, _, dm, _ = b.deliver(None, msg)
    r = subs.tolist().index(HOT)
    assert len(subs) == 4001 and 1000 < r < 3000
    assert int(offs[r + 1]) - int(offs[r]) == n and int(offs[r + 1]) // tile - int(offs[r]) // tile >= 2   # 3 tiles
    assert np.all(np.diff(offs)[np.arange(4001) != r] == 1)                                                 # one-delivery inboxes
    A = sum(1 for q in msg if q)
    rng = random.Random(4)
    others = {int(s): state(rng.randrange(65530, 65536), rng.choice([0, 1, UNB]), 0, rng.choice([0, 1]),
                            rng.choice([0, DISC, DISC | STORE])) for s in subs.tolist() if s != HOT and rng.random() < 0.5}
    # one wrap inside the hot inbox
    st = dict(others)
    st[HOT] = state(65000, UNB)
    want = check(b, st, state(3, 1, 1, 1), None, msg)
    got, rec = want[4][HOT]
    ids = [p for d, p in got if d == N.TM_DISP_SEND]
    assert len(ids) == A > 65535 - 65000 and ids[535] == 65535 and ids[536] == 1 and rec == (ids[-1] + 1, A, 0, 0)
    # the window edge inside the second tile, a full queue behind it
    st[HOT] = state(65000, tile + 1, 40, 100)
    want = check(b, st, state(3, 1, 1, 1), None, msg)
    got, rec = want[4][HOT]
    ds = [d for d, _ in got]
    E = A - (tile + 1)
    assert ds.count(N.TM_DISP_SEND) == tile + 1 and ds.count(N.TM_DISP_QUEUED) == 100
    assert ds.count(N.TM_DISP_DROP_FULL) == E - 100 > 0 and rec == ((65000 - 1 + tile + 1) % 65535 + 1, tile + 1, 100, 40)
    b.free()
    eng.close()


def test_hot_inbox_wraps_twice():
    eng = Engine(device=0)
    eng.subscribe_opts(b"w", 11, {"qos": 1})
    n = 2 * 65535 + 10
    b = run(eng, [b"w"] * n)
    inb, disp, pids, recs = b.window([dict(state(3, UNB), subscriber=11)], DEFAULTS, None, [1] * n)
    want, rec = S.window_one([1] * n, state(3, UNB))
    assert [p for _, p in want[:3]] == [3, 4, 5] and want[65532] == (1, 65535) and want[65533] == (1, 1)
    assert want[65535 + 65533] == (1, 1) and rec == (13, n, 0, 0)
    assert disp.tolist() == [d for d, _ in want] and pids.tolist() == [p for _, p in want]
    assert recs.tolist() == [list(rec)] and b.window_info["totals"] == [0, n, 0, 0, 0, 0]
    b.free()
    eng.close()


# -------------------------------------------------------------- 5. degenerate

def test_degenerate():
    eng = Engine(device=0)
    H = 5
    eng.subscribe_opts(b"h/x", H, {"nl": 1, "qos": 1})
    sessions = [dict(state(9, 1, 0, 1), subscriber=H)]
    # D' = 0 with D > 0; an empty batch; a batch without a delivery
    for T, fr in (([b"h/x"] * 300 + [b"nobody"], [H] * 301), ([], []), ([b"nobody/home"], [NONE])):
        b = run(eng, T)
        inb, disp, pids, recs = b.window(sessions, DEFAULTS, fr, [1] * len(T))
        assert [len(a) for a in inb[:5]] == [0, 1, 0, 0, 0] and inb[1].tolist() == [0]
        assert len(disp) == len(pids) == 0 and recs.shape == (0, 4) and b.window_info["totals"] == [0] * 6
        assert b.window_info["n_dropped_no_local"] == (300 if len(T) == 301 else 0)
        assert b.window_device(sessions, DEFAULTS, fr, [1] * len(T))[:2] == (0, 0)
        b.free()
    # n_sessions = 0: everything uses the defaults; a TM_SESS_HOST session between two ordinary ones
    for pid in (20, 21, 22):
        eng.subscribe_opts(b"m/+", pid, {"qos": 2})
    T = [b"m/%d" % i for i in range(9)]
    msg = [i % 3 for i in range(9)]
    b = run(eng, T)
    want = check(b, {}, state(65534, 3, 1, 2), None, msg)
    assert all(rec == (2, 3, 2, 1) for rec in want[2]) and want[3][N.TM_DISP_DROP_FULL] == 3
    st = {20: state(1, 1), 21: state(50, 0, 1, 1, HOST | DISC), 22: state(65535, 2)}
    want = check(b, st, DEFAULTS, None, msg)
    assert want[4][21] == ([(N.TM_DISP_HOST, 0)] * 9, (50, 0, 0, 0)) and want[3][N.TM_DISP_HOST] == 9
    assert want[4][20][1] == (2, 1, 5, 0) and want[4][22][1] == (2, 2, 4, 0)
    b.free()
    eng.close()


# ------------------------------------------------------ 6. modes and lifetime

def _device_arrays(d):
    nsub, nd = d[0], d[1]
    out = []
    for ptr, k, ty in ((d[2], nsub, np.uint32), (d[3], nsub + 1, np.uint32), (d[4], nd, np.uint32),
                       (d[5], nd, np.uint32), (d[6], nd, np.uint8), (d[8], nd, np.uint8), (d[9], nd, np.uint16),
                       (d[10], nsub * 4, np.uint32)):
        a = np.zeros(k, ty)
        _d2h(a, ptr)
        out.append(a)
    return out


def test_modes_and_lifetime():
    eng = Engine(device=0)
    rng = random.Random(31)
    for pid in range(30):
        for f in rng.sample([b"m/%d" % i for i in range(20)] + [b"m/+"], 5):
            eng.subscribe_opts(f, pid, {"qos": rng.randrange(3), "nl": rng.randrange(2)})
    T = [b"m/%d" % rng.randrange(22) for _ in range(1500)]
    fr = [rng.randrange(30) for _ in T]
    msg = [rng.randrange(3) for _ in T]
    sessions = table(random_states(rng, range(30)))
    # not waited, TM_BATCH_DEDUP, unsorted sessions, packet id 0: refused, and the batch stays usable
    b = eng.prepare(T)
    with pytest.raises(N.TmError) as ei:
        b.window(sessions, DEFAULTS, fr, msg)
    assert ei.value.rc == N.TM_EINVAL and b"waited" in eng.L.tm_last_error()
    b.launch()
    b.wait()
    bd = run(eng, T, dedup=True)
    with pytest.raises(N.TmError) as ei:
        bd.window(sessions, DEFAULTS, fr, msg)
    assert ei.value.rc == N.TM_EINVAL and b"DEDUP" in eng.L.tm_last_error()
    bd.free()
    with pytest.raises(N.TmError) as ei:
        b.window(sessions[::-1], DEFAULTS, fr, msg)
    assert ei.value.rc == N.TM_EINVAL and b"not above" in eng.L.tm_last_error()
    with pytest.raises(N.TmError) as ei:
        b.window([dict(state(0), subscriber=1)], DEFAULTS, fr, msg)
    assert ei.value.rc == N.TM_EINVAL and b"next_pkt_id" in eng.L.tm_last_error()
    # both drop paths of deliver underneath; device pointers read back equal the host result
    for kw in ({}, {"nl_all": True}):
        for f in (fr, None):
            states = {s["subscriber"]: {k: v for k, v in s.items() if k != "subscriber"} for s in sessions}
            check(b, states, state(7, 2, 0, 3), f, msg, **kw)
            host = b.window(sessions, state(7, 2, 0, 3), f, msg, **kw)
            info = dict(b.window_info)
            d = b.window_device(sessions, state(7, 2, 0, 3), f, msg, **kw)
            assert b.window_info["totals"] == info["totals"] and b.window_info["kernel_ms"] > 0
            dev = _device_arrays(d)
            for g, w in zip(dev[:5], host[0][:5]):
                assert np.array_equal(g, w)
            assert np.array_equal(dev[5], host[1]) and np.array_equal(dev[6], host[2])
            assert np.array_equal(dev[7].reshape(-1, 4), host[3])
    # a second call with other sessions on the same waited batch sees them
    other = {s: state(65535, 1, 0, 1, DISC | STORE) for s in range(0, 30, 2)}
    a = check(b, other, DEFAULTS, fr, msg)
    c = check(b, {}, DEFAULTS, fr, msg)
    assert a[0] != c[0] and c[3][N.TM_DISP_DROP_FULL] == 0 < a[3][N.TM_DISP_DROP_FULL]
    # inboxes and deliver after window are unchanged
    dlv = b.deliver(fr, msg)
    b.window(sessions, DEFAULTS, fr, msg)
    for g, w in zip(b.deliver(fr, msg), dlv):
        assert (g is None and w is None) or np.array_equal(g, w)
    b.free()
    eng.close()


# ------------------------------------------------------- 7. NIF on the device

def test_nif_session_window_batch_on_the_device():
    """session_window_batch/4 against the mirror over session_deliver_batch/3
    of the same publishes, with the engine's window() beside it."""
    from nif_harness import Nif
    nif = Nif()
    e = nif.new(0)
    eng = Engine(device=0)
    rng = random.Random(29)
    pids = list(range(1, 25)) + [0xFFFFFFF0]
    for pid in pids:
        for f in rng.sample([b"n/%d" % i for i in range(12)] + [b"n/+", b"#"], 4):
            o = {"qos": rng.randrange(3), "nl": rng.randrange(2), "rap": rng.randrange(2), "rh": 0, "subid": pid & 0xFFFF}
            eng.subscribe_opts(f, pid, o)
            assert nif.call("subscribe", e, f, pid, 0, (o["qos"], o["nl"], o["rap"], o["rh"], o["subid"])) == "ok"
    T = [b"n/%d" % rng.randrange(14) for _ in range(700)]
    fr = [rng.choice([NONE, 1, rng.randrange(1, 25), 0xFFFFFFF0]) for _ in T]
    msg = [rng.randrange(3) | rng.choice([0, 4]) for _ in T]
    pubs = [("none" if f == NONE else f, m & 3, bool(m & 4), bool(m & 8), t) for f, m, t in zip(fr, msg, T)]
    states = random_states(rng, pids)
    states[0xFFFFFFF0] = state(65535, 2, 1, 2)
    states[3] = state(5, 0, 0, 0, HOST)
    dflt = state(65530, 1, 1, 3)
    atoms = ["send0", "send", "queued", "dropped_qos0", "dropped_queue_full", "host"]

    def term(s, sub=0):
        fl = [a for a, bit in (("disconnected", DISC), ("store_qos0", STORE), ("host", HOST)) if s["flags"] & bit]
        return (sub, s["next_pkt_id"], fl, "unbounded" if s["inflight_free"] == UNB else s["inflight_free"],
                s["mqueue_len"], s["mqueue_max"])

    sessions = (term(dflt), [term(states[s], s) for s in sorted(states)])
    b = run(eng, T)
    seen = set()
    for flags, kw in (([], {}), (["nl_all", "upgrade_qos"], {"nl_all": True, "upgrade_qos": True})):
        plain = nif.call("session_deliver_batch", e, pubs, flags)
        want = []
        for sub, box in plain:
            got, rec = S.window_one([d[1] for d in box], states.get(sub, dflt))
            seen |= {d for d, _ in got}
            want.append((sub, (rec[0], rec[3], rec[2]),
                         [(atoms[d], p if d == N.TM_DISP_SEND else "undefined", dl) for (d, p), dl in zip(got, box)]))
        assert nif.call("session_window_batch", e, pubs, sessions, flags) == want, flags
        inb, disp, pids_, recs = b.window(table(states), dflt, fr, msg, subids=True, **kw)
        assert disp.tolist() == [atoms.index(x[0]) for _, _, box in want for x in box]
        assert recs[:, [0, 3, 2]].tolist() == [list(w[1]) for w in want]
    assert seen == set(range(N.TM_DISP_COUNT))
    assert nif.call("session_window_batch", e, [], sessions, []) == []
    # the C call's own checks come back as {error, einval}
    d6 = term(dflt)
    for bad in [(d6, [(4, 1, [], 0, 0, 0), (3, 1, [], 0, 0, 0)]), (d6, [(3, 0, [], 0, 0, 0)]),
                ((0, 65536, [], 0, 0, 0), []), (d6, [(3, 1, [], 0, 3, 2)])]:
        assert nif.call("session_window_batch", e, pubs[:5], bad, []) == ("error", "einval"), bad
    b.free()
    eng.close()
    nif.drop(e)
