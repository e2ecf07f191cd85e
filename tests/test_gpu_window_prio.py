"""The send window over mqueues with priority tables on the device
(tm_ptable_create, tm_batch_window_prio).  The reference of every case is
emqx_mqueue.window_one_prio -- the literal folds of deliver/2, enqueue/2 and
emqx_mqueue:in/2 over emqx_pqueue -- over the batch's own deliver() result and
the publishes' topic bytes.  The conditions a case relies on are asserted on
the mirror alone before the device result is looked at.  All comparisons are
exact."""

import random

import numpy as np
import pytest
from conftest import load_golden

from emqx_amd import _native as N
from emqx_amd import emqx_broker as B
from emqx_amd import emqx_mqueue as MQ
from emqx_amd import emqx_router as R
from emqx_amd import emqx_session as S
from emqx_amd.engine import Engine, _d2h

pytestmark = pytest.mark.gpu

NONE = N.TM_NONE
UNB = N.TM_SESS_UNBOUNDED
NOCLASS = N.TM_PRIO_NOCLASS
DISC, STORE, HOST = N.TM_SESS_DISCONNECTED, N.TM_SESS_STORE_QOS0, N.TM_SESS_HOST
DEFAULTS = {"next_pkt_id": 1, "flags": 0, "inflight_free": UNB, "mqueue_len": 0, "mqueue_max": 0}
(SEND0, SEND, QUEUED, DROP_QOS0, DROP_FULL, DISP_HOST) = range(6)


def state(P=1, F=UNB, L=0, M=0, flags=0):
    return {"next_pkt_id": P, "flags": flags, "inflight_free": F, "mqueue_len": L, "mqueue_max": M}


def run(eng, topics, **kw):
    b = eng.prepare(topics, **kw)
    b.launch()
    b.wait()
    return b


def table(states):
    return [dict(states[s], subscriber=s) for s in sorted(states)]


class Tab:
    """A table as the mirror takes it, and its device handle."""

    def __init__(self, eng, entries, default="lowest"):
        self.dict = {"priorities": dict(entries), "default_priority": default}
        self.h = eng.ptable(entries, default)
        self.classes = MQ.classes_of(self.dict)
        assert self.h.classes == self.classes


def prio_list(prio):
    """{subscriber: (table index or None, plen list)} -> window_prio's prio."""
    return [{"subscriber": s, "table": prio[s][0], "plen": prio[s][1]} for s in sorted(prio)]


def mirror(dlv, T, states, defaults, tabs, prio, default_table):
    """deliver()'s arrays and the publishes' topics through the mirror ->
    (disp, packet ids, records, totals, pclass, precords, {sub: (list, record, class records)})."""
    subs, offs, pubs, _, msg, _ = dlv
    offs, qos, pubs = offs.tolist(), (msg & 3).tolist(), pubs.tolist()
    disp, pids, pcls, recs, precs, per = [], [], [], [], [], {}
    for r, s in enumerate(subs.tolist()):
        st = states.get(s, defaults)
        ti, plen = prio.get(s, (default_table, []))
        tab = None if ti is None else tabs[ti]
        classes = [0] if tab is None else tab.classes
        plens = ({0: st["mqueue_len"]} if tab is None else
                 {p: k for p, k in zip(classes, list(plen) + [0] * (len(classes) - len(plen)))})
        dl = [(qos[q], T[pubs[q]]) for q in range(offs[r], offs[r + 1])]
        got, rec, cr = MQ.window_one_prio(dl, st, None if tab is None else tab.dict, plens)
        disp += [d for d, _, _ in got]
        pids += [p for _, p, _ in got]
        pcls += [c for _, _, c in got]
        recs.append(rec)
        pr = [[0, 0] for _ in range(8)]
        if tab is not None:
            for c, p in enumerate(classes):
                pr[c] = list(cr[p])
        precs.append(pr)
        per[s] = (got, rec, cr)
    totals = [disp.count(k) for k in range(N.TM_DISP_COUNT)]
    return disp, pids, recs, totals, pcls, precs, per


def compare(b, got, want, dlv):
    inb, disp, pids, recs, pclass, precs = got
    assert disp.dtype == pclass.dtype == np.uint8 and pids.dtype == np.uint16 and recs.dtype == precs.dtype == np.uint32
    for g, w in zip(inb, dlv):   # the tm_session_inboxes part IS deliver()'s result
        assert (g is None and w is None) or np.array_equal(g, w)
    assert len(disp) == len(pids) == len(pclass) == len(dlv[4])
    assert recs.shape == (len(dlv[0]), 4) and precs.shape == (len(dlv[0]), 8, 2)
    assert pclass.tolist() == want[4]
    assert disp.tolist() == want[0]
    assert pids.tolist() == want[1]
    assert [tuple(r) for r in recs.tolist()] == want[2]
    assert precs.tolist() == want[5]
    assert b.window_info["totals"] == want[3] and sum(want[3]) == len(disp)


def check(b, T, states, defaults, tabs, prio, default_table, from_=None, msg=None, **kw):
    """window_prio() against the mirror over deliver() of the same options."""
    dlv = b.deliver(from_, msg, **kw)
    want = mirror(dlv, T, states, defaults, tabs, prio, default_table)
    got = b.window_prio(table(states), defaults, [t.h for t in tabs], prio_list(prio), default_table, from_, msg, **kw)
    compare(b, got, want, dlv)
    return want


# ------------------------------------------------------- 1. the known answers

def test_kats_on_the_device():
    eng = Engine(device=0)
    PID = 7
    eng.subscribe_opts(b"#", PID, {"qos": 2})
    other = eng.ptable({b"zz": 200}, "highest")
    ran = 0
    for c in load_golden("kat_mqueue_prio.json")["cases"]:
        k = c.get("repeat", 1)
        qos, disp, pids, pcls = c["qos"] * k, c["disp"] * k, c["packet_ids"] * k, c["pclass"] * k
        T = [t.encode() for t in c["topics"]] * k
        tabled = c["table"] is not None
        t = eng.ptable({a.encode(): p for a, p in c["table"].items()}, c["default_priority"]) if tabled else None
        if tabled:
            assert t.classes == c["classes"], c["name"]
        precs = [[list(r) for r in c["class_records"]] + [[0, 0]] * (8 - len(c["classes"]))] if tabled else [[[0, 0]] * 8]
        listed = [dict(c["state"], subscriber=PID)]
        entry = [{"subscriber": PID, "table": 1 if tabled else None, "plen": c["plens"] if tabled else []}]
        # a listed session; the defaults with default_table; a listed session beside a tabled default it does not use
        variants = [(listed, DEFAULTS, [other, t] if tabled else [], entry if tabled else [], None),
                    ([], c["state"], [t] if tabled else [other], [], 0 if tabled else None),
                    (listed, DEFAULTS, [other, t] if tabled else [other], entry, 0)]
        b = run(eng, T)
        for sessions, defaults, tables, prio, dt in variants:
            if tabled and not sessions and c["state"]["mqueue_len"]:
                # older messages of a tabled session need their classes: the defaults cannot carry them
                with pytest.raises(N.TmError) as ei:
                    b.window_prio(sessions, defaults, tables, prio, dt, None, qos)
                assert ei.value.rc == N.TM_EINVAL and b"no prio entry" in eng.L.tm_last_error()
                continue
            inb, gd, gp, gr, gc, gpr = b.window_prio(sessions, defaults, tables, prio, dt, None, qos)
            assert inb[0].tolist() == [PID] and inb[1].tolist() == [0, len(qos)] and inb[4].tolist() == qos, c["name"]
            assert gc.tolist() == pcls, c["name"]
            assert gd.tolist() == disp and gp.tolist() == pids and gr.tolist() == [c["record"]], c["name"]
            assert gpr.tolist() == precs, c["name"]
            assert b.window_info["totals"] == [disp.count(x) for x in range(N.TM_DISP_COUNT)]
        b.free()
        ran += 1
    assert ran >= 11
    eng.close()


# ------------------------------------------------------------ 2. lookup edges

def _key(n, tag):
    """n bytes, unique per (n, tag), levels of at most 50 bytes."""
    out = (b"%s%d/" % (tag, n)) + b"/".join(b"%s%04d" % (tag * 10, i) for i in range(n // 10 + 1))
    out = out[:n]
    return out[:-1] + b"e" if out.endswith(b"/") else out


def test_lookup_edges():
    eng = Engine(device=0)
    A_SUB, B_SUB, PLAIN, SENT = 10, 20, 30, 40
    for s in (A_SUB, B_SUB, PLAIN, SENT):
        eng.subscribe_opts(b"#", s, {"qos": 2})
    lens = [1, 7, 8, 9, 63, 64, 65, 72, 4096]
    keys = [_key(n, b"k") for n in lens]
    assert [len(k) for k in keys] == lens and len(set(keys)) == len(keys)
    p64, q64 = _key(64, b"p"), _key(64, b"q")
    at64 = [p64 + b"A/tail", p64 + b"B/tail"]          # equal in the first 64 bytes, differ at byte 64
    last = [q64 + b"/zzzz1", q64 + b"/zzzz2"]          # differ at the last byte
    assert at64[0][:64] == at64[1][:64] and at64[0][64] != at64[1][64] and last[0][:-1] == last[1][:-1]
    prefix = [b"pre/fix", b"long/key/of/a/topic"]      # a key that is a prefix of a topic; a topic that is one of a key
    many = [b"big/%d/x" % i for i in range(1000)]      # probe runs form: 1,000 keys in 2,048 slots
    entries_a = {k: 1 + i % 6 for i, k in enumerate(keys + at64 + last + prefix + many)}
    entries_a[b"same"] = 6
    entries_a[b"only/a"] = "infinity"
    entries_b = {b"same": 2, b"only/b": 9, keys[4]: 9}
    tabs = [Tab(eng, entries_a, "lowest"), Tab(eng, entries_b, "highest")]
    assert len(tabs[0].classes) == 8 and tabs[0].classes[0] == "infinity" and tabs[1].classes == ["infinity", 9, 2]
    assert entries_a[at64[0]] != entries_a[at64[1]] and entries_a[last[0]] != entries_a[last[1]]

    def around(k):
        out = [k, k[:-1] + b"~", b"~" + k[1:]]
        if len(k) > 1:
            out.append(k[:-1])
        if len(k) < 4096:
            out.append(k + b"x")
        return out

    T = []
    for k in keys + at64 + last + prefix:
        T += around(k)
    T += [b"pre/fix/more", b"pre/fi", b"long/key", b"long/key/of/a/topic/deeper", p64, q64, p64 + b"C/tail",
          b"same", b"only/a", b"only/b", b"none/of/them", b"big", b"big/1000/x"]
    rng = random.Random(7)
    T += [rng.choice(many) for _ in range(300)] + [b"big/%d/y" % i for i in range(50)]
    T = [t for t in T if t and not t.startswith(b"$")]
    rng.shuffle(T)
    assert all(len(t) <= 4096 for t in T) and sum(t in entries_a for t in T) > 300 > sum(t in entries_b for t in T) > 2
    msg = [1 + i % 2 for i in range(len(T))]
    states = {A_SUB: state(1, 0, 0, 0, DISC), B_SUB: state(1, 0, 0, 0, DISC), PLAIN: state(1, 0, 0, 0, DISC),
              SENT: state(9, UNB, 0, 0, 0)}
    prio = {A_SUB: (0, []), SENT: (0, []), PLAIN: (None, [])}         # B_SUB: table 1 by default
    b = run(eng, T)
    dlv = b.deliver(None, msg)
    want = mirror(dlv, T, states, DEFAULTS, tabs, prio, 1)
    # on the mirror: every class of both tables is hit, hits and misses of every key occur, sent deliveries are classed too
    offs = dlv[1].tolist()
    box = {s: want[4][offs[r]:offs[r + 1]] for r, s in enumerate(dlv[0].tolist())}
    pubs = dlv[2].tolist()
    assert set(box[A_SUB]) == set(range(8)) and set(box[B_SUB]) == {0, 1, 2} and set(box[PLAIN]) == {NOCLASS}
    assert box[SENT] == box[A_SUB] and all(d == SEND for d, _, _ in want[6][SENT][0])
    cls_a = dict(zip((T[p] for p in pubs[offs[0]:offs[1]]), box[A_SUB]))
    dflt_a = tabs[0].classes.index(0)
    for k in keys + at64 + last + prefix:
        assert cls_a[k] == tabs[0].classes.index(entries_a[k]) != dflt_a
        assert all(cls_a[t] == dflt_a for t in around(k)[1:] if t and t not in entries_a), k
    assert cls_a[at64[0]] != cls_a[at64[1]] and cls_a[last[0]] != cls_a[last[1]]
    assert cls_a[b"pre/fix/more"] == cls_a[b"long/key"] == cls_a[b"only/b"] == dflt_a
    cls_b = dict(zip((T[p] for p in pubs[offs[1]:offs[2]]), box[B_SUB]))
    assert cls_b[b"same"] == 2 and cls_a[b"same"] == tabs[0].classes.index(6) and cls_b[b"only/a"] == 0 and cls_b[keys[4]] == 1
    got = b.window_prio(table(states), DEFAULTS, [t.h for t in tabs], prio_list(prio), 1, None, msg)
    compare(b, got, want, dlv)
    assert b.window_info["lookup_kernel_ms"] > 0
    b.free()
    # a batch tokenised on the host carries no device bytes of its own: they are uploaded for the call
    eh = Engine(device=0, host_tokenize=True)
    eh.subscribe_opts(b"#", A_SUB, {"qos": 1})
    th = Tab(eh, entries_a, "lowest")
    bh = run(eh, T[:200])
    check(bh, T[:200], {A_SUB: state(1, 0, 0, 0, DISC)}, DEFAULTS, [th], {}, 0, None, msg[:200])
    bh.free()
    eh.close()
    eng.close()


# ------------------------------------------------------ 3. tile and wave edges

@pytest.mark.parametrize("lead", (0, 3))
def test_tile_and_wave_edges(lead):
    """dnew_1 = e needs more than e entering deliveries of class 1, and one
    max_len bounds every class: with 2 * tile + 12 entering deliveries and e up
    to 2 * tile + 1 that leaves class 0 five of them (M = E_1 - e >= 5 holds
    them all) and class 2 one, which meets a full class and pushes an older
    message out.  They sit at fixed ranks across the inbox, the last two behind
    every edge."""
    eng = Engine(device=0)
    tile = eng.L.tm_inbox_tile()
    FIRST, H, LAST = 0, 5, 0xFFFFFFF0
    eng.subscribe_opts(b"z/y", FIRST, {"qos": 2})
    eng.subscribe_opts(b"h/+", H, {"qos": 2})
    eng.subscribe_opts(b"l/x", LAST, {"qos": 1})
    tab = Tab(eng, {b"h/a": 9, b"h/b": 5}, "lowest")                # h/c: class 2
    tb1 = Tab(eng, {b"l/x": 3}, "lowest")
    n1 = 2 * tile + 12                                              # entering deliveries of H's inbox
    at0, at2 = {10, 700, tile + 5, 2 * tile - 3, 2 * tile + 8}, {2 * tile + 10}
    cls_of_rank = [0 if a in at0 else 2 if a in at2 else 1 for a in range(n1)]
    E1 = cls_of_rank.count(1)
    assert E1 == 2 * tile + 6
    topic = [b"h/a", b"h/b", b"h/c"]
    hq, ht = [], []
    for a in range(n1):
        hq.append(1 + a % 2)
        ht.append(topic[cls_of_rank[a]])
        if a % 5 == 4:                                              # a QoS-0 delivery after every fifth, of class 0
            hq.append(0)
            ht.append(b"h/a")
    ranks = [i for i, q in enumerate(hq) if q]
    assert len(ranks) == n1 and hq[5] == 0 and hq[4] and hq[6]
    T = [b"z/y"] * lead + ht + [b"l/x"] * 2
    msg = [2] * lead + hq + [1, 1]
    b = run(eng, T)
    subs, offs, _, _, dm, _ = b.deliver(None, msg)
    assert subs.tolist() == ([FIRST] if lead else []) + [H, LAST] and int(offs[-3]) == lead
    assert dm[lead:lead + len(hq)].tolist() == hq
    for k in (64, 1024, tile, 2 * tile):
        for e in (k - 1, k, k + 1):
            # connected: the window edge F at e; the class ranks start only behind it
            st = {H: state(65000, e, 5, 5), LAST: state(65535, 1, 0, 1), FIRST: state(9, 0, 1, 1, DISC)}
            prio = {H: (0, [0, 0, 5]), LAST: (1, []), FIRST: (None, [])}
            want = check(b, T, st, DEFAULTS, [tab, tb1], prio, None, None, msg)
            got, rec, cr = want[6][H]
            ent1 = [a for a in range(e, n1) if cls_of_rank[a] == 1]
            assert rec[1] == e and got[ranks[e - 1]][0] == SEND and got[ranks[e]][0] != SEND
            assert cr == {9: (sum(a >= e for a in at0), 0), 5: (5, 0), 0: (1, 1)} and len(ent1) > 5
            assert got[ranks[ent1[0]]][0] == got[ranks[ent1[-6]]][0] == DROP_FULL and got[ranks[ent1[-5]]][0] == QUEUED
            assert got[ranks[e - 1]][2] == cls_of_rank[e - 1] and got[5][0] == SEND0 and got[5][2] == 0
            # disconnected: dnew_1 = e, four older messages of class 1 go first; class 0 drops nothing,
            # class 2 is full and drops one older message for its entering delivery
            M = E1 - e
            st[H] = state(17, 3, 4 + M, M, DISC)
            prio[H] = (0, [0, 4, M])
            assert M >= 5
            want = check(b, T, st, DEFAULTS, [tab, tb1], prio, None, None, msg)
            got, rec, cr = want[6][H]
            assert cr == {9: (5, 0), 5: (E1 - e, 4), 0: (1, 1)} and rec == (17, 0, n1 - e, 5)
            r1 = [a for a in range(n1) if cls_of_rank[a] == 1]
            assert got[ranks[r1[e - 1]]][0] == DROP_FULL and got[ranks[r1[e]]][0] == QUEUED
            assert r1[e] != e and ranks[r1[e]] != r1[e]        # class rank, counted rank and position differ
            assert all(got[ranks[a]][0] == QUEUED for a in at0 | at2) and got[5][0] == DROP_QOS0
    b.free()
    eng.close()


def test_balanced_classes_across_waves():
    """Three classes of about equal weight over three tiles: every wave carries
    counts of every class into the scan, the drop edge of each class sits in a
    different wave, and a second tabled inbox starts inside the last tile."""
    eng = Engine(device=0)
    tile = eng.L.tm_inbox_tile()
    H, G = 5, 9
    eng.subscribe_opts(b"h/+", H, {"qos": 2})
    eng.subscribe_opts(b"h/c", G, {"qos": 1})
    tab = Tab(eng, {b"h/a": "infinity", b"h/b": 5}, 2)
    cyc = [0, 1, 1, 2, 0, 1, 2]
    n = 2 * tile + 900
    T = [[b"h/a", b"h/b", b"h/c"][cyc[i % 7]] for i in range(n)]
    msg = [(i * 5 + 1) % 3 for i in range(n)]
    b = run(eng, T)
    for M, F, plen, flags in ((1024, 0, [3, 1024, 0], DISC | STORE), (70, 1025, [70, 0, 9], 0), (0, 64, [1, 2, 3], 0),
                              (1500, tile - 1, [0, 1495, 0], DISC)):
        st = {H: state(65500, F, sum(plen), M, flags), G: state(4, 1, 2, 2, DISC)}
        want = check(b, T, st, DEFAULTS, [tab], {H: (0, plen), G: (0, [0, 0, 2])}, None, None, msg)
        got, rec, cr = want[6][H]
        if M:
            assert all(cr[p][0] == M for p in tab.classes) and {d for d, _, _ in got} >= {QUEUED, DROP_FULL}
            assert [cr[p][1] for p in tab.classes] == plen
        else:
            assert rec[3] == 0 and DROP_FULL not in {d for d, _, _ in got}
        assert want[6][G][1][3] == 2
    b.free()
    eng.close()


# ------------------------------------------------------------ 4. random churn

def test_random_churn():
    from test_gpu_session_window import random_states
    from test_gpu_subopts import churn_case
    T, rows, model, from_, msg = churn_case()
    boxes = B.mailboxes(rows)
    inboxes, _ = S.session_inboxes(boxes, model, from_, msg)
    rng = random.Random(41)
    uniq = sorted(set(T))
    ent = [{t: rng.choice([1, 4, 9, "infinity"]) for t in rng.sample(uniq, len(uniq) // 3)},
           {t: rng.choice([0, 2, 200]) for t in rng.sample(uniq, len(uniq) // 2)}]
    dicts = [{"priorities": ent[0], "default_priority": "lowest"}, {"priorities": ent[1], "default_priority": "highest"}]
    pstates = random_states(rng, sorted(inboxes))
    defaults = state(65530, 2, 0, 2, 0)
    pprio = {}
    for p, st in pstates.items():
        ti = rng.choice([None, 0, 1])
        if ti is None:
            if rng.random() < 0.5:
                pprio[p] = (None, [])                               # listed, no table
            continue                                                # not listed: table 1 by default
        ncls = len(MQ.classes_of(dicts[ti]))
        M = st["mqueue_max"]
        plen = [rng.randrange(M + 1) if M else rng.randrange(3) for _ in range(ncls)]
        if rng.random() < 0.3:
            plen[rng.randrange(ncls)] = M if M else 5               # a class that is full already
        st["mqueue_len"] = sum(plen)
        pprio[p] = (ti, plen)
    for p, st in pstates.items():                                   # tabled by default: no older messages
        if p not in pprio:
            st["mqueue_len"] = 0
    eng = R.engine()
    tabs = [Tab(eng, ent[0], "lowest"), Tab(eng, ent[1], "highest")]
    sid_from = [NONE if f is None else B._sid(f) for f in from_]
    states = {B._sid(p): s for p, s in pstates.items()}
    prio = {B._sid(p): v for p, v in pprio.items()}
    b = run(eng, T)
    dlv = b.deliver(sid_from, msg)
    want = mirror(dlv, T, states, defaults, tabs, prio, 1)
    # the conditions, on the mirror alone
    assert {B._terms[s] for s in dlv[0].tolist()} == set(inboxes)
    assert set(want[0]) == set(range(N.TM_DISP_COUNT))
    assert any(sum(1 for r in pr if r[1] > 0) >= 1 and any(r[1] == 0 and r[0] > 0 for r in pr) for pr in want[5])
    subs = dlv[0].tolist()
    assert any(s in prio and prio[s][0] is not None for s in subs) and any(s not in prio for s in subs)
    assert any(s in prio and prio[s][0] is None for s in subs) and NOCLASS in want[4] and len(set(want[4])) >= 6
    got = b.window_prio(table(states), defaults, [t.h for t in tabs], prio_list(prio), 1, sid_from, msg)
    compare(b, got, want, dlv)
    check(b, T, states, defaults, tabs, prio, 1, sid_from, msg, nl_all=True, upgrade_qos=True, subids=True)
    b.free()
    B.clear_tables()


# ----------------------------------------------- 5. equivalence and degenerate

def test_equivalence_and_degenerate():
    eng = Engine(device=0)
    rng = random.Random(31)
    for pid in range(30):
        for f in rng.sample([b"m/%d" % i for i in range(20)] + [b"m/+"], 5):
            eng.subscribe_opts(f, pid, {"qos": rng.randrange(3), "nl": rng.randrange(2)})
    from test_gpu_session_window import random_states
    T = [b"m/%d" % rng.randrange(22) for _ in range(1500)]
    fr = [rng.randrange(30) for _ in T]
    msg = [rng.randrange(3) for _ in T]
    sessions = table(random_states(rng, range(30)))
    states = {s["subscriber"]: {k: v for k, v in s.items() if k != "subscriber"} for s in sessions}
    dflt = state(7, 2, 0, 3)
    b = run(eng, T)
    # n_tables = 0: arrays, records and totals of tm_batch_window on the same batch
    for f in (fr, None):
        old = b.window(sessions, dflt, f, msg)
        info = dict(b.window_info)
        new = b.window_prio(sessions, dflt, [], [], None, f, msg)
        for g, w in zip(new[0], old[0]):
            assert (g is None and w is None) or np.array_equal(g, w)
        assert all(np.array_equal(g, w) for g, w in zip(new[1:4], old[1:]))
        assert b.window_info["totals"] == info["totals"] and b.window_info["lookup_kernel_ms"] == 0
        assert new[4].tolist() == [NOCLASS] * len(old[1]) and not new[5].any() and new[5].shape == (len(old[0][0]), 8, 2)
    # a table nobody uses, and entries that name no table: the same again through the class kernels
    t8 = Tab(eng, {b"m/%d" % i: i + 1 for i in range(7)}, "lowest")
    assert len(t8.classes) == 8
    new = b.window_prio(sessions, dflt, [t8.h], [{"subscriber": s["subscriber"], "table": None} for s in sessions[::2]],
                        None, fr, msg)
    old = b.window(sessions, dflt, fr, msg)
    assert all(np.array_equal(g, w) for g, w in zip(new[1:4], old[1:])) and set(new[4].tolist()) == {NOCLASS}
    assert not new[5].any()
    # a table of exactly 8 classes used fully, by every session (sessions listed carry older messages in every class)
    prio = {}
    for s in list(states):
        M = states[s]["mqueue_max"]
        plen = [rng.randrange(M + 1) if M else rng.randrange(3) for _ in range(8)]
        states[s] = dict(states[s], mqueue_len=sum(plen))
        prio[s] = (0, plen)
    want = check(b, T, states, dflt, [t8], prio, 0, fr, msg)
    assert set(want[4]) >= set(range(8)) and any(all(r[0] + r[1] > 0 for r in pr) for pr in want[5])
    # every session TM_SESS_HOST: nothing is classed
    hosts = {s: dict(st, flags=st["flags"] | HOST) for s, st in states.items()}
    want = check(b, T, hosts, dict(dflt, flags=HOST), [t8], prio, 0, fr, msg)
    assert set(want[0]) == {DISP_HOST} and set(want[4]) == {NOCLASS} and not np.asarray(want[5]).any()
    # a second call on the same waited batch, with other tables, sees them
    t2 = Tab(eng, {b"m/1": 5, b"m/2": 5}, "highest")
    one = check(b, T, {}, state(1, 0, 0, 1), [t8], {}, 0, fr, msg)
    two = check(b, T, {}, state(1, 0, 0, 1), [t2], {}, 0, fr, msg)
    three = check(b, T, {}, state(1, 0, 0, 1), [t2, t8], {}, 1, fr, msg)
    assert one[4] != two[4] and one[0] != two[0] and three[4] == one[4] and three[0] == one[0]
    b.free()
    # D' = 0 with D > 0; an empty batch; a batch without a delivery
    e2 = Engine(device=0)
    e2.subscribe_opts(b"h/x", 5, {"nl": 1, "qos": 1})
    tt = Tab(e2, {b"h/x": 3})
    for T0, f0 in (([b"h/x"] * 300 + [b"nobody"], [5] * 301), ([], []), ([b"nobody/home"], [NONE])):
        b0 = run(e2, T0)
        inb, disp, pids, recs, pclass, precs = b0.window_prio([], DEFAULTS, [tt.h], [], 0, f0, [1] * len(T0))
        assert [len(a) for a in inb[:5]] == [0, 1, 0, 0, 0] and inb[1].tolist() == [0]
        assert len(disp) == len(pids) == len(pclass) == 0 and recs.shape == (0, 4) and precs.shape == (0, 8, 2)
        assert b0.window_info["totals"] == [0] * 6 and b0.window_info["lookup_kernel_ms"] == 0
        assert b0.window_prio_device([], DEFAULTS, [tt.h], [], 0, f0, [1] * len(T0))[:2] == (0, 0)
        b0.free()
    e2.close()
    eng.close()


def test_einval_on_the_device():
    """The checks that need a batch, and that a refused call leaves the batch usable."""
    eng = Engine(device=0)
    eng.subscribe_opts(b"a", 3, {"qos": 1})
    t = Tab(eng, {b"a": 4})
    T = [b"a"] * 5
    sessions = [dict(state(1, 0, 2, 0), subscriber=3)]
    prio = [{"subscriber": 3, "table": 0, "plen": [2, 0]}]
    b = eng.prepare(T)
    with pytest.raises(N.TmError) as ei:
        b.window_prio(sessions, DEFAULTS, [t.h], prio, None, None, [1] * 5)
    assert ei.value.rc == N.TM_EINVAL and b"waited" in eng.L.tm_last_error()
    b.launch()
    b.wait()
    for bad, word in (([{"subscriber": 3, "table": 0, "plen": [1, 0]}], b"subscriber 3): sum of plen 1 is not mqueue_len 2"),
                      ([{"subscriber": 3, "table": 0, "plen": [0, 0, 2]}], b"subscriber 3): plen[2] = 2 for a class its table lacks"),
                      ([{"subscriber": 3, "table": 1, "plen": [2]}], b"subscriber 3): table = 1 with n_tables = 1"),
                      ([{"subscriber": 4, "table": 0}], b"(subscriber 4) is not in wopts->sessions"),
                      ([], b"(subscriber 3) has a priority table and mqueue_len = 2 but no prio entry")):
        with pytest.raises(N.TmError) as ei:
            b.window_prio(sessions, DEFAULTS, [t.h], bad, 0, None, [1] * 5)
        assert ei.value.rc == N.TM_EINVAL and word in eng.L.tm_last_error(), eng.L.tm_last_error()
    bd = run(eng, T, dedup=True)
    with pytest.raises(N.TmError) as ei:
        bd.window_prio(sessions, DEFAULTS, [t.h], prio, None, None, [1] * 5)
    assert ei.value.rc == N.TM_EINVAL and b"DEDUP" in eng.L.tm_last_error()
    bd.free()
    # a token batch has no topic bytes on the device: refused with a table, fine without one
    bt = eng.prepare_tokens_host(eng.tokenize(T))
    bt.launch()
    bt.wait()
    with pytest.raises(N.TmError) as ei:
        bt.window_prio(sessions, DEFAULTS, [t.h], prio, None, None, [1] * 5)
    assert ei.value.rc == N.TM_EINVAL and b"no device copy of its topic bytes" in eng.L.tm_last_error()
    assert bt.window_prio(sessions, DEFAULTS, [], [], None, None, [1] * 5)[1].tolist() == [QUEUED] * 5
    bt.free()
    inb, disp, pids, recs, pclass, precs = b.window_prio(sessions, DEFAULTS, [t.h], prio, None, None, [1] * 5)
    assert disp.tolist() == [QUEUED] * 5 and pclass.tolist() == [0] * 5 and recs.tolist() == [[1, 0, 5, 0]]
    assert precs[0].tolist() == [[5, 0], [0, 0]] + [[0, 0]] * 6
    b.free()
    eng.close()


# ------------------------------------------------------- 6. an armed shared batch

def test_armed_shared_batch():
    eng = Engine(device=0)
    G1, G2 = 900, 901
    for s in (11, 12, 13):
        eng.subscribe_opts(b"e/+", s, {"qos": 2})
    for s in (12, 21, 22):
        eng.shared_subscribe(b"e/x", G1, s)
    for s in (13, 21):
        eng.shared_subscribe(b"e/+", G2, s)
    tab = Tab(eng, {b"e/x": 7, b"e/y": 3}, "lowest")
    rng = random.Random(3)
    T = [rng.choice([b"e/x", b"e/y", b"e/z", b"q"]) for _ in range(3000)]
    msg = [rng.randrange(3) for _ in T]
    keys = [rng.getrandbits(32) for _ in T]
    b = run(eng, T)
    b.shared_mode("hash", keys=keys)
    states = {11: state(65000, 100, 4, 50), 12: state(5, 0, 0, 20, DISC), 21: state(1, 7, 30, 30, DISC | STORE),
              22: state(9, 3, 0, 0)}
    prio = {11: (0, [1, 3, 0]), 21: (0, [0, 0, 30])}
    dlv = b.deliver(None, msg)
    grp = b.inbox_groups()
    want = mirror(dlv, T, states, DEFAULTS, [tab], prio, 0)
    # on the mirror: sessions that only shared deliveries reach are classed, and both kinds share a class queue
    subs, offs = dlv[0].tolist(), dlv[1].tolist()
    assert set(subs) == {11, 12, 13, 21, 22}
    r21 = subs.index(21)
    assert all(g != NONE for g in grp[offs[r21]:offs[r21 + 1]].tolist()) and len(set(want[4][offs[r21]:offs[r21 + 1]])) == 3
    r12 = subs.index(12)
    g12 = grp[offs[r12]:offs[r12 + 1]].tolist()
    assert NONE in g12 and G1 in g12 and want[6][12][1][2] < offs[r12 + 1] - offs[r12]   # its queue of 20 overflows per class
    assert {QUEUED, DROP_FULL, DROP_QOS0, SEND, SEND0} <= set(want[0])
    got = b.window_prio(table(states), DEFAULTS, [tab.h], prio_list(prio), 0, None, msg)
    assert np.array_equal(b.inbox_groups(), grp)
    compare(b, got, want, dlv)
    b.free()
    eng.close()


# ----------------------------------------------------------- 7. TM_WINDOW_DEVICE

def test_window_device_mode():
    eng = Engine(device=0)
    rng = random.Random(12)
    for pid in range(40):
        for f in rng.sample([b"m/%d" % i for i in range(20)] + [b"m/+"], 5):
            eng.subscribe_opts(f, pid, {"qos": rng.randrange(3), "nl": rng.randrange(2)})
    tabs = [Tab(eng, {b"m/%d" % i: i % 4 for i in range(12)}, "highest"), Tab(eng, {b"m/3": 8}, 1)]
    T = [b"m/%d" % rng.randrange(22) for _ in range(6000)]
    fr = [rng.randrange(40) for _ in T]
    msg = [rng.randrange(3) for _ in T]
    states = {s: state(rng.randrange(1, 65536), rng.choice([0, 5, UNB]), 0, rng.choice([0, 2, 30]),
                       rng.choice([0, DISC, DISC | STORE])) for s in range(0, 40, 2)}
    prio = {s: (rng.choice([0, 1, None]), []) for s in range(0, 40, 4)}
    for f in (fr, None):
        want = check(b := run(eng, T), T, states, state(7, 2, 0, 3), tabs, prio, 1, f, msg)
        host = b.window_prio(table(states), state(7, 2, 0, 3), [t.h for t in tabs], prio_list(prio), 1, f, msg)
        info = dict(b.window_info)
        d = b.window_prio_device(table(states), state(7, 2, 0, 3), [t.h for t in tabs], prio_list(prio), 1, f, msg)
        assert b.window_info["totals"] == info["totals"] == want[3] and b.window_info["kernel_ms"] > 0
        nsub, nd = d[0], d[1]
        dev = []
        for ptr, k, ty in ((d[2], nsub, np.uint32), (d[3], nsub + 1, np.uint32), (d[4], nd, np.uint32),
                           (d[5], nd, np.uint32), (d[6], nd, np.uint8), (d[8], nd, np.uint8), (d[9], nd, np.uint16),
                           (d[10], nsub * 4, np.uint32), (d[11], nd, np.uint8), (d[12], nsub * 16, np.uint32)):
            a = np.zeros(k, ty)
            _d2h(a, ptr)
            dev.append(a)
        for g, w in zip(dev[:5], host[0][:5]):
            assert np.array_equal(g, w)
        assert np.array_equal(dev[5], host[1]) and np.array_equal(dev[6], host[2])
        assert np.array_equal(dev[7].reshape(-1, 4), host[3]) and np.array_equal(dev[8], host[4])
        assert np.array_equal(dev[9].reshape(-1, 8, 2), host[5])
        # deliver after the call is unchanged
        dlv = b.deliver(f, msg)
        for g, w in zip(dlv, host[0]):
            assert (g is None and w is None) or np.array_equal(g, w)
        b.free()
    eng.close()
