"""Shared-subscription deliveries in the inboxes, deliver and the send window
(tm_batch_shared_mode, tm_batch_inbox_groups, tm_shared_subscribe_opts).

An armed batch sorts the merged list L': publishes in order, a publish's match
entries in match order, within an entry first the ordinary subscribers
(emqx_broker:dispatch/3, the {To, node()} route) and then one picked member per
group ({To, Group} routes; lists:usort puts the atom first,
src/emqx_broker.erl:255-261).  Two references, both on the host: the literal
restatement emqx_broker.mailboxes_shared over the oracle Broker's rows and
emqx_shared_sub.dispatch_batch_mirror's rows, and `reference_merged`, NumPy on
the batch's own publish-major dispatch() / dispatch_shared() arrays.  What a
case relies on is asserted on the host side alone before the device result is
looked at.  All comparisons are exact."""

import ctypes as C
import random
from dataclasses import replace

import numpy as np
import pytest
from test_gpu_inbox import assert_inboxes, reference

from emqx_amd import _native as N
from emqx_amd import emqx_broker as B
from emqx_amd import emqx_router as R
from emqx_amd import emqx_session as SS
from emqx_amd import emqx_shared_sub as S
from emqx_amd import gen
from emqx_amd.engine import Engine, _d2h
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NONE = N.TM_NONE
UNB = N.TM_SESS_UNBOUNDED


def run(eng, topics, **kw):
    b = eng.prepare(topics, **kw)
    b.launch()
    b.wait()
    return b


def merged_list(b, strategy, keys=None, seed=0):
    """L' of the batch from its own publish-major arrays, before the sort:
    (subscriber, match entry, group) of every delivery in L' order, plus
    (pub_of, ids) to name an entry's publish and filter."""
    roff, ids = b.result()
    _, moff, subs = b.dispatch(match_offsets=True)
    soff, sfid, sgrp, ssub = b.dispatch_shared(strategy, keys=keys, seed=seed)
    m, d, s = len(ids), len(subs), len(ssub)
    entry = np.repeat(np.arange(m, dtype=np.int64), np.diff(moff).astype(np.int64))
    pub_of = np.searchsorted(roff, np.arange(m), side="right") - 1
    ent_of = {(int(pub_of[j]), int(ids[j])): j for j in range(m)}
    spub = np.repeat(np.arange(len(soff) - 1), np.diff(soff).astype(np.int64))
    sent = np.asarray([ent_of[int(p), int(f)] for p, f in zip(spub, sfid)], np.int64)
    ent = np.r_[entry, sent]
    kind = np.r_[np.zeros(d, np.int64), np.ones(s, np.int64)]
    idx = np.r_[np.arange(d), np.arange(s)]
    order = np.lexsort((idx, kind, ent))            # by entry, ordinary first, each kind in its own order
    lsub = np.r_[subs, ssub].astype(np.uint32)[order]
    lgrp = np.r_[np.full(d, NONE, np.uint32), sgrp.astype(np.uint32)][order]
    return lsub, ent[order], lgrp, pub_of, ids


def reference_merged(b, strategy, keys=None, seed=0):
    """(subscribers, offsets, publishes, filter_ids, groups) of the armed batch."""
    lsub, lent, lgrp, pub_of, ids = merged_list(b, strategy, keys, seed)
    d = len(lsub)
    order = np.argsort(lsub, kind="stable")
    key = lsub[order]
    heads = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if d else np.zeros(0, np.int64)
    e = lent[order]
    return (key[heads].astype(np.uint32), np.r_[heads, d].astype(np.uint32), pub_of[e].astype(np.uint32),
            ids[e].astype(np.uint32), lgrp[order].astype(np.uint32))


def armed(b):
    got = b.inboxes()
    grp = b.inbox_groups()
    assert grp.dtype == np.uint32 and len(grp) == len(got[2])
    return got + (grp,)


def assert_merged(got, want):
    assert_inboxes(got[:4], want[:4])
    assert np.array_equal(got[4], want[4]), "groups"


@pytest.fixture
def mirror():
    """The broker / shared-sub mirrors on a fresh device engine."""
    if R._engine is not None and R._engine.device != 0:   # a host-only engine left by a CPU test
        R._engine.close()
        R._engine = None
    B.clear_tables()
    yield R.engine()
    B.clear_tables()


def between(box):
    """a shared delivery with an ordinary one before it and one behind it"""
    kinds = [g is not None for _, _, g in box]
    return any(k and (False in kinds[:q]) and (False in kinds[q + 1:]) for q, k in enumerate(kinds))


# ------------------------------------------------------ 1. the hand-worked answer

def test_hand_worked_known_answer(mirror):
    """route/2 folds over aggre(match_routes(Topic)) (src/emqx_broker.erl:209,
    238-248): for `a/x` the routes {a/#, node}, {a/#, h}, {a/+, node}, {a/+, g}
    in that order ('#' sorts before '+', node() before a group).  Hash: Nth = 1
    + key rem Count (src/emqx_shared_sub.erl:267-268): g = [3, 1] gives 3 for
    key 0 and 1 for key 1; h = [2] always 2 (:260)."""
    eng = mirror
    B.subscribe(b"a/+", 1)
    B.subscribe(b"a/#", 2)
    S.subscribe("g", b"a/+", 3)
    S.subscribe("g", b"a/+", 1)
    S.subscribe("h", b"a/#", 2)
    T, keys = [b"a/x", b"a/x", b"b"], [0, 1, 0]
    want = {1: [(0, b"a/+", None), (1, b"a/+", None), (1, b"a/+", "g")],
            2: [(0, b"a/#", None), (0, b"a/#", "h"), (1, b"a/#", None), (1, b"a/#", "h")],
            3: [(0, b"a/+", "g")]}
    # the restatement agrees with the hand-worked lists, and a shared delivery sits between two ordinary ones
    rows = [[(b"a/#", 2), (b"a/+", 1)], [(b"a/#", 2), (b"a/+", 1)], []]
    srows = S.dispatch_batch_mirror(T, "hash", keys=keys)
    assert srows == [[(b"a/#", "h", 2), (b"a/+", "g", 3)], [(b"a/#", "h", 2), (b"a/+", "g", 1)], []]
    assert B.mailboxes_shared(rows, srows) == want and between(want[2])
    b = run(eng, T)
    roff, ids = b.result()
    assert [eng.filter_bytes(int(f)) for f in ids[roff[0]:roff[1]]] == [b"a/#", b"a/+"]   # the engine's match order
    # unarmed: today's inboxes
    plain = b.inboxes()
    assert_inboxes(plain, reference(b))
    assert len(plain[2]) == 4
    with pytest.raises(N.TmError) as ei:
        b.inbox_groups()
    assert ei.value.rc == N.TM_EINVAL
    b.free()
    assert B.deliver_batch(T) == {1: [(0, b"a/+"), (1, b"a/+")], 2: [(0, b"a/#"), (1, b"a/#")]}
    assert B.deliver_batch(T, shared={"strategy": "hash", "keys": keys}) == want


# --------------------------------------------------------------- 2. random churn

def test_random_churn_vs_oracle_and_mirror(mirror):
    rng = random.Random(33)
    p = replace(gen.C1, n_filters=2500)
    F = gen.gen_filters(p).tolist()
    T = gen.gen_topics(p, gen.Strings.from_list(F), 17, 5000).tolist()
    groups = [f"g{i}" for i in range(40)]
    orc = O.Broker()
    for rnd in range(3):
        for _ in range(7000):
            f, g, pid = rng.choice(F), rng.choice(groups), rng.randrange(300)
            r = rng.random()
            if r < 0.15:
                B.unsubscribe(f, pid)
                orc.unsubscribe(f, pid)
            elif r < 0.155:
                assert B.subscriber_down(pid) == orc.subscriber_down(pid)
            elif r < 0.55:
                B.subscribe(f, pid)
                orc.subscribe(f, pid)
            elif r < 0.70:
                S.unsubscribe(g, f, pid)
            elif r < 0.705:
                S.member_down(pid)
            else:
                S.subscribe(g, f, pid)
        trie = O.Trie()
        for f in S._groups_of:
            if O.wildcard(f):
                trie.insert(f)
        matched = lambda t: ([] if trie.empty() else trie.match(t)) + [t]   # noqa: E731
        rows = [orc.publish(t) for t in T]
        for strategy, kw in (("hash", {"keys": [rng.getrandbits(32) for _ in T]}), ("random", {"seed": 1000 + rnd})):
            if strategy == "random" and rnd != 1:
                continue
            srows = S.dispatch_batch_mirror(T, strategy, matched=matched, **kw)
            want = B.mailboxes_shared(rows, srows)
            n_ord, n_sh = sum(map(len, rows)), sum(map(len, srows))
            assert n_ord > 1000 and n_sh > 1000
            assert any(between(box) for box in want.values())
            assert any(all(g is not None for _, _, g in box) for box in want.values())      # a pid that is only a member
            assert any(all(g is None for _, _, g in box) for box in want.values())
            got = B.deliver_batch(T, shared=dict(kw, strategy=strategy))
            assert got.keys() == want.keys(), (rnd, strategy)
            for pid in want:
                assert got[pid] == want[pid], (rnd, strategy, pid)
            assert sum(map(len, got.values())) == n_ord + n_sh


# ------------------------------------------------------- 3. tile and scan edges

VARIED = [0x01020304, 3, 0x00FF00FF, 0x0A000001, 0x0000FE00]
G1, G2, G3 = 900, 901, 902


def edge_engine():
    """one/x: one ordinary subscriber.  v/+: five ordinary subscribers that
    differ in every digit.  s/x: no ordinary subscriber, one group of two.
    e/x: three ordinary subscribers and two groups (5 deliveries an entry)."""
    eng = Engine(device=0)
    eng.subscribe(b"one/x", 7)
    for s in VARIED:
        eng.subscribe(b"v/+", s)
    for s in (0x0B000000, 7):
        eng.shared_subscribe(b"s/x", G1, s)
    for s in (11, 0x00C0FFEE, 7):
        eng.subscribe(b"e/x", s)
    for s in (7, 0x7F000001, 12):
        eng.shared_subscribe(b"e/x", G2, s)
    eng.shared_subscribe(b"e/x", G3, 0x00C0FFEE)
    return eng


def sweep(tile):
    return [0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile + 1, 3 * tile + 17]


def check_edge(eng, T, d, n_shared, seed):
    b = run(eng, T)
    rng = random.Random(seed)
    keys = [rng.getrandbits(32) for _ in T]
    want = reference_merged(b, "hash", keys)
    assert len(want[2]) == d and int(np.count_nonzero(want[4] != NONE)) == n_shared, d
    b.shared_mode("hash", keys=keys)
    got = armed(b)
    assert b.inbox_info["passes"] == (4 if d else 0), d
    assert_merged(got, want)
    if d == 0:
        assert len(got[0]) == 0 and got[1].tolist() == [0]
    b.free()


def test_tile_edges_all_shared():
    """D = 0: every delivery is a pick; tile + 1 = 4,097 entries with one group
    each also crosses the entry scan's tile of 4,096."""
    eng = edge_engine()
    tile = eng.L.tm_inbox_tile()
    assert tile == 4096
    for d in sweep(tile):
        check_edge(eng, [b"s/x"] * d + [b"nobody/home"], d, d, d)
    eng.close()


def test_tile_edges_none_shared_on_an_armed_batch():
    eng = edge_engine()
    tile = eng.L.tm_inbox_tile()
    for d in sweep(tile):
        nv = min(d // len(VARIED), 1200)
        T = [b"one/x"] * (d - nv * len(VARIED)) + [b"v/%d" % i for i in range(nv)] + [b"nobody/home"]
        random.Random(d).shuffle(T)
        check_edge(eng, T, d, 0, d)
    eng.close()


def test_tile_edges_mixed():
    eng = edge_engine()
    tile = eng.L.tm_inbox_tile()
    for d in sweep(tile):
        ne = min(d // 5, 700)                       # e/x: 3 ordinary + 2 picks
        ns = min((d - 5 * ne) // 2, 900)            # s/x: 1 pick
        nv = min((d - 5 * ne - ns) // 5, 600)       # v/+: 5 ordinary
        n1 = d - 5 * ne - ns - 5 * nv               # one/x: 1 ordinary
        T = [b"e/x"] * ne + [b"s/x"] * ns + [b"v/%d" % i for i in range(nv)] + [b"one/x"] * n1 + [b"nobody/home"]
        random.Random(d).shuffle(T)
        check_edge(eng, T, d, 2 * ne + ns, d)
    eng.close()


def test_tile_boundary_between_an_entrys_ordinary_run_and_its_picks():
    eng = edge_engine()
    tile = eng.L.tm_inbox_tile()
    for k in (1, 2):
        lead = k * tile - 3 - 5 * 40                # one/x deliveries, then 40 whole e/x entries, then the one cut
        T = [b"one/x"] * lead + [b"e/x"] * 60
        b = run(eng, T)
        keys = list(range(len(T)))
        lsub, lent, lgrp, _, _ = merged_list(b, "hash", keys)
        cut = k * tile
        assert lent[cut - 1] == lent[cut] and lgrp[cut - 1] == NONE and lgrp[cut] == G2 and lgrp[cut + 1] == G3
        b.shared_mode("hash", keys=keys)
        assert_merged(armed(b), reference_merged(b, "hash", keys))
        b.free()
    eng.close()


def test_pick_count_crosses_a_scan_tile():
    """4,096 entries with one group each, plus one, between entries without a
    group: the picks-before-an-entry offset takes its block sum."""
    eng = edge_engine()
    T = [b"one/x"] * 50 + [b"s/x"] * 4097 + [b"one/x"] * 50 + [b"e/x"] * 3
    b = run(eng, T)
    keys = [i * 2654435761 & 0xFFFFFFFF for i in range(len(T))]
    want = reference_merged(b, "hash", keys)
    assert len(b.result()[1]) == len(T) > 4096 and int(np.count_nonzero(want[4] != NONE)) == 4097 + 6
    b.shared_mode("hash", keys=keys)
    assert_merged(armed(b), want)
    b.free()
    eng.close()


# ----------------------------------------------------------------------- 4. passes

def test_passes_cover_a_shared_members_id():
    """The only subscriber id above 2^24 is a shared member's."""
    eng = Engine(device=0)
    big = (1 << 24) + 3
    eng.subscribe(b"p/x", 5)
    eng.subscribe(b"p/+", 200)
    eng.shared_subscribe(b"p/x", G1, big)
    eng.shared_subscribe(b"p/x", G1, 6)
    T = [b"p/x"] * 300 + [b"p/y"] * 10
    keys = [i % 2 for i in range(len(T))]
    b = run(eng, T)
    want = reference_merged(b, "hash", keys)
    assert want[0].tolist() == [5, 6, 200, big] and len(want[2]) == 300 * 3 + 10
    b.shared_mode("hash", keys=keys)
    got = armed(b)
    assert b.inbox_info["passes"] == 4
    assert_merged(got, want)
    b.free()
    eng.close()


# ------------------------------------------------------------------ 5. round robin

def test_round_robin_takes_the_next_cursor_values():
    eng = Engine(device=0)
    A, Bm = 10, 11
    eng.subscribe(b"rr/x", A)
    eng.subscribe(b"rr/#", A)
    eng.subscribe(b"rr/#", Bm)
    eng.shared_subscribe(b"rr/x", G1, A)
    eng.shared_subscribe(b"rr/x", G1, Bm)
    K = 1001
    b = run(eng, [b"rr/x"] * K)
    roff, ids = b.result()
    rank = {int(f): r for r, f in enumerate(ids[roff[0]:roff[1]])}
    assert [eng.filter_bytes(int(f)) for f in ids[roff[0]:roff[1]]] == [b"rr/#", b"rr/x"]
    b.shared_mode("round_robin")
    lo = 0
    for call in range(2):                            # the second call moves the cursor on
        subs, offs, pubs, fids, grp = armed(b)
        assert subs.tolist() == [A, Bm] and len(pubs) == 4 * K
        picks = {}
        for r, s in enumerate(subs.tolist()):
            box = [(int(pubs[q]), rank[int(fids[q])], int(grp[q] != NONE)) for q in range(int(offs[r]), int(offs[r + 1]))]
            assert box == sorted(box), (call, s)     # (publish, match rank, ordinary before shared)
            picks[s] = [p for p, _, sh in box if sh]
            assert all(int(grp[q]) in (NONE, G1) for q in range(int(offs[r]), int(offs[r + 1])))
        # the multiset of picks is the next K cursor values: member 1 + c rem 2
        want_a = sum(1 for c in range(lo, lo + K) if c % 2 == 0)
        assert (len(picks[A]), len(picks[Bm])) == (want_a, K - want_a), call
        assert sorted(picks[A] + picks[Bm]) == list(range(K))         # one pick per publish
        lo += K
    # tm_batch_dispatch_shared on the same engine continues from there
    _, _, _, ssub = b.dispatch_shared("round_robin")
    assert int(np.count_nonzero(ssub == A)) == sum(1 for c in range(lo, lo + K) if c % 2 == 0)
    b.free()
    eng.close()


# --------------------------------------- 6. deliver and window over merged inboxes

def merged_session(boxes, model, from_, msg, upgrade_qos=False, nl_all=False):
    """emqx_session.py's restatements over the host-merged lists ->
    {pid: [(publish, To, byte, subid, group)]}, dropped count."""
    out, dropped = {}, 0
    for pid, box in boxes.items():
        subs = model.get(pid, {})
        delivers = [(to, dict(SS.msg_of(msg[i], from_[i]), i=i, g=g)) for i, to, g in box]
        left, k = SS.ignore_local(delivers, pid, subs, nl_all)
        dropped += k
        if left:
            out[pid] = [(m["i"], to, SS.byte_of(e), e["subid"] or 0, m["g"])
                        for (to, m), (_, e) in zip(left, SS.enrich(left, subs, upgrade_qos))]
    return out, dropped


def session_case():
    """Pids 1..4.  1: ordinary on t/+ (qos 1); member of g2 on t/1 with options
    (qos 2, rap, subid 9).  2: ordinary on t/# (qos 2, nl); member of g1 on t/+
    with options (qos 1, nl).  3: member of g1 on t/+ WITHOUT options.  4:
    member of g3 on t/# without options, ordinary on t/2 (qos 2)."""
    model = {1: {b"t/+": {"qos": 1}, b"t/1": {"qos": 2, "rap": 1, "subid": 9}},
             2: {b"t/#": {"qos": 2, "nl": 1}, b"t/+": {"qos": 1, "nl": 1}},
             4: {b"t/2": {"qos": 2}}}
    orc = O.Broker()
    for pid, f in ((1, b"t/+"), (2, b"t/#"), (4, b"t/2")):
        B.subscribe(f, pid, model[pid][f])
        orc.subscribe(f, pid)
    S.subscribe("g2", b"t/1", 1, subopts=model[1][b"t/1"])
    S.subscribe("g1", b"t/+", 2, subopts=model[2][b"t/+"])
    S.subscribe("g1", b"t/+", 3)
    S.subscribe("g3", b"t/#", 4)
    rng = random.Random(61)
    T = [b"t/%d" % rng.randrange(4) for _ in range(900)]
    from_ = [rng.choice([None, 1, 2, 2, 3]) for _ in T]
    msg = [rng.randrange(3) | rng.choice([0, 4]) | rng.choice([0, 0, 8]) for _ in T]
    keys = [rng.getrandbits(32) for _ in T]
    T[0], from_[0], keys[0] = b"t/0", 2, 0            # pid 2's inbox starts with two own deliveries, the second a shared one
    boxes = B.mailboxes_shared([orc.publish(t) for t in T], S.dispatch_batch_mirror(T, "hash", keys=keys))
    return model, T, from_, msg, keys, boxes


def device_session(dlv, grp):
    subs, offs, pubs, fids, dm, sid = dlv
    eng = R.engine()
    name = {}
    out = {}
    for r, s in enumerate(subs.tolist()):
        box = []
        for q in range(int(offs[r]), int(offs[r + 1])):
            f = int(fids[q])
            if f not in name:
                name[f] = eng.filter_bytes(f)
            g = int(grp[q])
            box.append((int(pubs[q]), name[f], int(dm[q]), int(sid[q]), None if g == NONE else R._agg_of[g][1]))
        out[B._terms[s]] = box
    return out


def test_deliver_and_window_over_merged_inboxes(mirror):
    eng = mirror
    model, T, from_, msg, keys, boxes = session_case()
    default, d0 = merged_session(boxes, model, from_, msg)
    every, d1 = merged_session(boxes, model, from_, msg, nl_all=True)
    n_all = sum(map(len, boxes.values()))
    # the conditions, on the mirror alone
    assert 0 < d0 < d1 and all(between(box) for pid, box in boxes.items() if pid in (1, 2, 4))
    assert 3 in default and all(g == "g1" and sid == 0 and byte == (msg[i] & 7)     # no options: unenriched
                                for i, _, byte, sid, g in default[3])
    assert any(msg[i] & 4 and msg[i] & 3 for i, _, _, _, _ in default[3])
    own_shared = [(i, to, g) for i, to, g in boxes[2] if g == "g1" and from_[i] == 2]
    kept = [(i, to, g) for i, to, _, _, g in default[2]]
    gone = [(i, to, g) for i, to, _, _, g in every[2]]
    assert boxes[2][:2] == [(0, b"t/#", None), (0, b"t/+", "g1")] and own_shared[0] == (0, b"t/+", "g1")
    assert own_shared[0] not in kept                  # the leading run goes, shared delivery included
    assert any(x in kept for x in own_shared) and not any(x in gone for x in own_shared)
    assert any(g == "g2" and sid == 9 for _, _, _, sid, g in default[1])
    sid_from = [NONE if f is None else B._sid(f) for f in from_]
    b = run(eng, T)
    b.shared_mode("hash", keys=keys)
    for kw, want, dropped in (({}, default, d0), ({"nl_all": True}, every, d1),
                              ({"upgrade_qos": True}, merged_session(boxes, model, from_, msg, upgrade_qos=True)[0], d0)):
        dlv = b.deliver(sid_from, msg, subids=True, **kw)
        grp = b.inbox_groups()                        # parallel after the compaction
        assert len(grp) == len(dlv[2]) == n_all - dropped and b.deliver_info["n_dropped_no_local"] == dropped
        got = device_session(dlv, grp)
        assert got.keys() == want.keys()
        for pid in want:
            assert got[pid] == want[pid], (kw, pid)
        dptr = b.deliver_device(sid_from, msg, subids=True, **kw)
        dg = np.zeros(dptr[1], np.uint32)
        _d2h(dg, b.inbox_groups_device())
        assert np.array_equal(dg, grp)
    # the window: one packet-id sequence per session over both kinds; session 1's window fills on a shared delivery
    counted = [(q, g) for q, (_, _, byte, _, g) in enumerate(default[1]) if byte & 3]
    a = next(k for k, (_, g) in enumerate(counted) if g == "g2" and k > 3)
    states = {1: {"next_pkt_id": 65530, "flags": 0, "inflight_free": a + 1, "mqueue_len": 0, "mqueue_max": 0},
              2: {"next_pkt_id": 7, "flags": 0, "inflight_free": UNB, "mqueue_len": 0, "mqueue_max": 0},
              3: {"next_pkt_id": 1, "flags": N.TM_SESS_DISCONNECTED, "inflight_free": 0, "mqueue_len": 1, "mqueue_max": 4}}
    dflt = {"next_pkt_id": 100, "flags": 0, "inflight_free": 3, "mqueue_len": 0, "mqueue_max": 0}
    want_w = {pid: SS.window_one([byte & 3 for _, _, byte, _, _ in box], states.get(pid, dflt)) for pid, box in default.items()}
    w1 = want_w[1][0]
    assert w1[counted[a][0]][0] == N.TM_DISP_SEND and w1[counted[a + 1][0]][0] == N.TM_DISP_QUEUED
    w2 = [(pid_, g) for (d, pid_), (_, _, _, _, g) in zip(want_w[2][0], default[2]) if d == N.TM_DISP_SEND]
    assert [p for p, _ in w2[:50]] == list(range(7, 57)) and {g for _, g in w2[:50]} >= {None, "g1"}
    sessions = [dict(states[s], subscriber=B._sid(s)) for s in sorted(states, key=B._sid)]
    assert [s["subscriber"] for s in sessions] == sorted(s["subscriber"] for s in sessions)
    inb, disp, pids, recs = b.window(sessions, dflt, sid_from, msg, subids=True)
    grp = b.inbox_groups()
    assert device_session(inb, grp) == default
    offs = inb[1].tolist()
    for r, s in enumerate(inb[0].tolist()):
        got_w, rec = want_w[B._terms[s]]
        assert list(zip(disp[offs[r]:offs[r + 1]].tolist(), pids[offs[r]:offs[r + 1]].tolist())) == got_w, s
        assert tuple(recs[r].tolist()) == rec, s
    assert sum(b.window_info["totals"]) == len(disp) == n_all - d0
    b.free()


# ------------------------------------------------------- 8. modes, errors, lifetime

def test_modes_errors_and_lifetime():
    eng = edge_engine()
    rng = random.Random(8)
    T = [rng.choice([b"e/x", b"s/x", b"one/x", b"v/1", b"v/2", b"q"]) for _ in range(6000)]
    k1 = [rng.getrandbits(32) for _ in T]
    k2 = [k ^ 1 for k in k1]
    b = eng.prepare(T)
    b.shared_mode("hash", keys=k1)                   # a prepared batch can be armed; the calls still need the wait
    with pytest.raises(N.TmError) as ei:
        b.inboxes()
    assert ei.value.rc == N.TM_EINVAL and b"waited" in eng.L.tm_last_error()
    b.launch()
    b.wait()
    with pytest.raises(N.TmError) as ei:              # armed, but no inboxes / deliver / window call yet
        b.inbox_groups()
    assert ei.value.rc == N.TM_EINVAL
    w1, w2 = reference_merged(b, "hash", k1), reference_merged(b, "hash", k2)
    plain = reference(b)
    assert any(not np.array_equal(x, y) for x, y in zip(w1, w2))
    assert len(w1[2]) > len(plain[2]) > 2 * eng.L.tm_inbox_tile()
    assert_merged(armed(b), w1)
    b.shared_mode(None)                              # disarmed: bit for bit as before
    assert_inboxes(b.inboxes(), plain)
    with pytest.raises(N.TmError) as ei:
        b.inbox_groups()
    assert ei.value.rc == N.TM_EINVAL and b"not armed" in eng.L.tm_last_error()
    b.shared_mode("hash", keys=k2)                   # re-armed with other keys
    assert_merged(armed(b), w2)
    b.shared_mode("random", seed=5)
    assert_merged(armed(b), reference_merged(b, "random", seed=5))
    # device-pointer forms
    r, d, ms, passes, d_sub, d_off, d_pub, d_fid = b.inboxes_device()
    want = reference_merged(b, "random", seed=5)
    dev = [np.zeros(k, np.uint32) for k in (r, r + 1, d, d, d)]
    for dst, src in zip(dev, (d_sub, d_off, d_pub, d_fid, b.inbox_groups_device())):
        _d2h(dst, src)
    assert ms > 0 and passes == 4
    assert_merged(dev, want)
    # the host pointer stays valid until the next dispatch-class call
    b.inboxes()
    p = C.POINTER(C.c_uint32)()
    N.check(eng.L.tm_batch_inbox_groups(eng.h, b.h, 0, C.byref(p)), "tm_batch_inbox_groups")
    p2 = C.POINTER(C.c_uint32)()
    N.check(eng.L.tm_batch_inbox_groups(eng.h, b.h, 0, C.byref(p2)), "tm_batch_inbox_groups")
    assert C.cast(p, C.c_void_p).value == C.cast(p2, C.c_void_p).value
    b.result()
    b.stats()
    eng.subscribe(b"later/x", 1)
    assert np.array_equal(np.ctypeslib.as_array(p, shape=(d,)), want[4])
    # TM_EINVAL of tm_batch_shared_mode: strategy, flags, hash without keys, a TM_BATCH_DEDUP batch
    for strategy, keys, flags, word in ((7, None, 0, b"strategy"), ("hash", None, 0, b"keys"),
                                        ("random", None, N.TM_SHARED_COUNT_ONLY, b"COUNT_ONLY"),
                                        ("random", None, N.TM_SHARED_DEVICE, b"TM_SHARED_DEVICE"),
                                        ("random", None, 64, b"unknown flag")):
        o, _keep = b._shared_opts(strategy, keys, 0, flags)
        assert eng.L.tm_batch_shared_mode(eng.h, b.h, C.byref(o)) == N.TM_EINVAL, word
        assert word in eng.L.tm_last_error()
    assert_merged(armed(b), want)                    # a refused call leaves the mode as it was
    assert eng.L.tm_batch_inbox_groups(eng.h, b.h, 2, C.byref(p)) == N.TM_EINVAL and b"flag" in eng.L.tm_last_error()
    assert eng.L.tm_batch_inbox_groups(eng.h, b.h, 0, None) == N.TM_EINVAL
    bd = run(eng, T[:500], dedup=True)
    with pytest.raises(N.TmError) as ei:
        bd.shared_mode("random")
    assert ei.value.rc == N.TM_EINVAL and b"DEDUP" in eng.L.tm_last_error()
    bd.free()
    b.free()
    eng.close()


# ------------------------------------------------------------------------ 9. NIF

def test_nif_session_window_batch_with_a_strategy_flag():
    """session_window_batch/4, session_deliver_batch/3 and deliver_batch/3 with
    {shared_hash, Keys} through the runtime stand-in against the engine's own
    window() / inbox_groups() of the same state."""
    from nif_harness import Nif
    nif = Nif()
    e = nif.new(0)
    eng = Engine(device=0)
    rng = random.Random(47)
    filters = [b"n/%d" % i for i in range(8)] + [b"n/+", b"n/#"]
    for pid in range(1, 13):
        for f in rng.sample(filters, 3):
            o = {"qos": rng.randrange(3), "nl": rng.randrange(2), "rap": rng.randrange(2), "rh": 0, "subid": pid}
            eng.subscribe_opts(f, pid, o)
            assert nif.call("subscribe", e, f, pid, 0, (o["qos"], o["nl"], o["rap"], o["rh"], o["subid"])) == "ok"
    for g in (G1, G2):
        for f in rng.sample(filters, 4):
            for pid in rng.sample(range(20, 28), 3):
                if rng.random() < 0.5:                               # a member without options
                    eng.shared_subscribe(f, g, pid)
                    assert nif.call("shared_subscribe", e, f, g, pid) == "ok"
                else:
                    o = (rng.randrange(3), rng.randrange(2), rng.randrange(2), 0, 100 + pid)
                    eng.shared_subscribe_opts(f, g, pid, dict(zip(("qos", "nl", "rap", "rh", "subid"), o)))
                    assert nif.call("shared_subscribe", e, f, g, pid, o) == "ok"
    T = [b"n/%d" % rng.randrange(10) for _ in range(500)]
    fr = [rng.choice([NONE, 3, 21, 24]) for _ in T]
    msg = [rng.randrange(3) | rng.choice([0, 4]) for _ in T]
    keys = [rng.getrandbits(32) for _ in T]
    pubs = [("none" if f == NONE else f, m & 3, bool(m & 4), False, t) for f, m, t in zip(fr, msg, T)]
    dflt = {"next_pkt_id": 65500, "flags": 0, "inflight_free": 4, "mqueue_len": 0, "mqueue_max": 0}
    atoms = ["send0", "send", "queued", "dropped_qos0", "dropped_queue_full", "host"]
    b = run(eng, T)
    b.shared_mode("hash", keys=keys)
    (subs, offs, ps, fids, dm, sid), disp, pids, recs = b.window([], dflt, fr, msg, subids=True)
    grp = b.inbox_groups()
    assert int(np.count_nonzero(grp != NONE)) > 100 and int(np.count_nonzero(grp == NONE)) > 100

    def tf(x):
        return "true" if x else "false"                             # the stand-in prints atoms

    def pair(q):
        f = eng.filter_bytes(int(fids[q]))
        return (int(ps[q]), f if grp[q] == NONE else (f, int(grp[q])))

    want = [(int(s), (int(recs[r][0]), int(recs[r][3]), int(recs[r][2])),
             [(atoms[disp[q]], int(pids[q]) if disp[q] == N.TM_DISP_SEND else "undefined",
               (pair(q), int(dm[q] & 3), tf(dm[q] & 4), tf(dm[q] & 8), int(sid[q])))
              for q in range(int(offs[r]), int(offs[r + 1]))]) for r, s in enumerate(subs.tolist())]
    sessions = ((0, 65500, [], 4, 0, 0), [])
    assert nif.call("session_window_batch", e, pubs, sessions, [("shared_hash", keys)]) == want
    assert nif.call("session_deliver_batch", e, pubs, [("shared_hash", keys)]) == [(s, [d for _, _, d in box]) for s, _, box in want]
    isubs, ioffs, ips, ifids = b.inboxes()
    igrp = b.inbox_groups()
    boxes = [(int(s), [(int(ips[q]), eng.filter_bytes(int(ifids[q])) if igrp[q] == NONE
                        else (eng.filter_bytes(int(ifids[q])), int(igrp[q])))
                       for q in range(int(ioffs[r]), int(ioffs[r + 1]))]) for r, s in enumerate(isubs.tolist())]
    assert nif.call("deliver_batch", e, T, [("shared_hash", keys)]) == boxes
    b.shared_mode("random", seed=5)
    rsubs, roffs, rps, rfids = b.inboxes()
    rgrp = b.inbox_groups()
    rboxes = [(int(s), [(int(rps[q]), eng.filter_bytes(int(rfids[q])) if rgrp[q] == NONE
                         else (eng.filter_bytes(int(rfids[q])), int(rgrp[q])))
                        for q in range(int(roffs[r]), int(roffs[r + 1]))]) for r, s in enumerate(rsubs.tolist())]
    assert nif.call("deliver_batch", e, T, [("shared_random", 5)]) == rboxes
    # unarmed forms are unchanged; malformed flags are badarg
    b.shared_mode(None)
    assert nif.call("deliver_batch", e, T, []) == nif.call("deliver_batch", e, T)
    assert len(nif.call("deliver_batch", e, T, ["shared_round_robin"])) >= len(nif.call("deliver_batch", e, T))
    for bad in ([("shared_hash", keys[:-1])], [("shared_hash", keys), "shared_round_robin"], ["shared_sticky"]):
        assert nif.call("deliver_batch", e, T, bad) == ("#badarg",), bad
    b.free()
    eng.close()
    nif.drop(e)
