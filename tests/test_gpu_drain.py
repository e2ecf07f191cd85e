"""The session drain on the device (tm_sessions_drain).  The reference of every
case is emqx_mqueue.drain_one -- emqx_session:dequeue/1 as the literal fold
over emqx_mqueue:out/1 and emqx_message:is_expired/1 -- or, where the input is
too large for the pqueue fold, emqx_mqueue.drain_flat, which tests/test_drain.py
holds equal to it.  The conditions a case relies on are asserted on the mirror
alone before the device result is looked at.  All comparisons are exact."""

import numpy as np
import pytest

import drain_cases as K
from emqx_amd import emqx_mqueue as MQ
from emqx_amd.engine import Engine

pytestmark = pytest.mark.gpu

UNB, NOW = K.UNB, K.NOW
SEND0, SEND, KEPT, EXPIRED = K.SEND0, K.SEND, K.KEPT, K.EXPIRED
KATS = K.load_kats()["cases"]
EMPTY = ([], {"next_pkt_id": 77, "inflight_free": 3})
EMPTY_WANT = ([], (77, 0, 0, 0), [0] * 8)


@pytest.fixture(scope="module")
def eng():
    e = Engine(device=0)
    yield e
    e.close()


def q1(cls=0):
    return (MQ.qmsg_of(1, cls), 0, 0)


def q0(cls=0):
    return (MQ.qmsg_of(0, cls), 0, 0)


def gone(cls=0, qos=1):
    """a message whose interval of 1 s ran out 1 ms ago"""
    return (MQ.qmsg_of(qos, cls, True), NOW - 1001, 1)


def fresh(cls=0, qos=1):
    """a message with an interval that has an hour left"""
    return (MQ.qmsg_of(qos, cls, True), NOW - 5, 3600)


def st(P=1, F=UNB):
    return {"next_pkt_id": P, "inflight_free": F}


def drain(eng, sessions, now=NOW, **kw):
    s, q = K.pack(sessions)
    return eng.drain(s, q, now, **kw)


def check(eng, sessions, wants, now=NOW, what=""):
    want = K.want_arrays(wants)
    got = drain(eng, sessions, now)
    K.assert_same(got, want, what)
    assert eng.drain_info["totals"] == K.totals_of(want), what
    assert (got["popped"].sum(1) == got["records"][:, 1:].sum(1)).all(), what
    return got


# ---- 1. the known answers -------------------------------------------------------------

@pytest.mark.parametrize("case", KATS, ids=lambda c: c["name"])
def test_kats_on_the_device(eng, case):
    msgs, state, classes, now, want = K.kat_session(case)
    assert MQ.drain_one(msgs, state, classes, now) == want
    check(eng, [(msgs, state)], [want], now, "alone")
    check(eng, [EMPTY, (msgs, state), EMPTY], [EMPTY_WANT, want, EMPTY_WANT], now, "between two empty sessions")
    # 64 copies back to back: with one message each, the 64 heads of one wave round
    n = len(msgs)
    _, q = K.pack([(msgs, state)] * 64)
    assert (np.diff(q["q_off"].astype(np.int64)) == n).all() and int(q["q_off"][-1]) == 64 * n
    check(eng, [(msgs, state)] * 64, [want] * 64, now, "64 copies")


# ---- 2. expiry edges ------------------------------------------------------------------

def test_expiry_edges_in_one_session(eng):
    F = MQ.qmsg_of(1, 0, True)
    msgs = [(F, NOW - 7000, 7),                       # elapsed = interval * 1000: not expired, 1 left
            (F, NOW - 7001, 7),                       # one millisecond more: expired
            (F, NOW + 500, 0),                        # made in the future, interval 0: elapsed 0, not expired, unchanged
            (F, NOW - 1, 0),                          # interval 0, elapsed 1: expired
            (F, NOW - 4294967296, 0xFFFFFFFF),        # 0xFFFFFFFF * 1000 does not fit 32 bits: not expired
            (MQ.qmsg_of(1, 0), -(2 ** 62), 0xDEADBEEF),   # no flag: whatever the two arrays hold
            (MQ.qmsg_of(0, 0, True), NOW - 7000, 7),  # QoS 0 is updated as well when it is sent
            (F, NOW - 4294967295001, 0xFFFFFFFF)]     # and one past that product: expired
    want = MQ.drain_one(msgs, st(10), [0], NOW)
    per = want[0]
    assert [p[0] for p in per] == [SEND, EXPIRED, SEND, EXPIRED, SEND, SEND, SEND0, EXPIRED]
    assert [p[3] for p in per] == [1, 7, 0, 0, 0xFFFFFFFF - 4294967, 0xDEADBEEF, 1, 0xFFFFFFFF]
    assert [p[1] for p in per] == [10, 0, 11, 0, 12, 13, 0, 0] and want[1] == (14, 4, 1, 3)
    got = check(eng, [(msgs, st(10))], [want])
    # expiry_out not wanted: everything else is the same
    s, q = K.pack([(msgs, st(10))])
    bare = eng.drain(s, q, NOW, expiry_out=False)
    assert bare["expiry_out"] is None
    K.assert_same(bare, {k: v for k, v in got.items() if k != "expiry_out"})
    # both arrays NULL: legal when no message has the flag
    plain = [q1(), q0(), q1(1), q0(1)]
    wantp = MQ.drain_one(plain, st(5, 1), [1, 0], NOW)
    s, q = K.pack([(plain, st(5, 1))], with_expiry=False)
    gotp = eng.drain(s, q, NOW)
    K.assert_same(gotp, K.want_arrays([wantp]))
    assert not gotp["expiry_out"].any()


def test_every_message_expired(eng):
    msgs = [gone(k % 3, k % 3) for k in range(200)]
    want = MQ.drain_one(msgs, st(40000, 2), [2, 1, 0], NOW)
    assert all(p[0] == EXPIRED for p in want[0]) and want[1] == (40000, 0, 0, 200)
    check(eng, [(msgs, st(40000, 2))], [want])
    # an hour earlier none of them is, and two go out
    early = MQ.drain_one(msgs, st(40000, 2), [2, 1, 0], NOW - 3_600_000)
    assert early[1][:2] == (40002, 2) and early[1][3] == 0
    check(eng, [(msgs, st(40000, 2))], [early], NOW - 3_600_000)


# ---- 3. the cut ---------------------------------------------------------------------

def test_the_cut(eng):
    two = [1, 0]
    cases = []   # (msgs, state, classes, the dispositions the case is about)
    cases.append(([q1(), q0(), gone(), fresh()], st(9, 0), [0], [KEPT] * 4))                   # inflight_free 0
    # the cut on the first counted message: what is in front of it does not use Cnt up, what is behind it stays
    cases.append(([q0(), gone(), q1(), q0(), gone(), q1()], st(9, 1), [0], [SEND0, EXPIRED, SEND, KEPT, KEPT, KEPT]))
    # the cut on the last message of the queue
    cases.append(([q1(), q0(), q1(), q1()], st(9, 3), [0], [SEND, SEND0, SEND, SEND]))
    # the cut on the last counted message of a class: the next class is untouched though it starts with QoS 0
    cases.append(([q0(1), q1(0), q1(1), q1(0)], st(9, 2), two, [KEPT, SEND, KEPT, SEND]))
    # the same with the class's own QoS 0 and expired tail behind the cut
    cases.append(([q1(0), q0(1), q0(0), gone(0), q1(1)], st(9, 1), two, [SEND, KEPT, KEPT, KEPT, KEPT]))
    # expired and QoS 0 in front of the cut, in the class above it
    cases.append(([q1(1), gone(0), q0(0), q1(1), q1(1)], st(9, 2), two, [SEND, EXPIRED, SEND0, SEND, KEPT]))
    # more counted messages than Cnt by one, fewer by one, exactly Cnt
    cases.append(([q1()] * 4, st(9, 3), [0], [SEND] * 3 + [KEPT]))
    cases.append(([q1()] * 4 + [q0()], st(9, 5), [0], [SEND] * 4 + [SEND0]))
    cases.append(([q1()] * 4 + [q0()], st(9, 4), [0], [SEND] * 4 + [KEPT]))
    wants = []
    for msgs, state, classes, disp in cases:
        w = MQ.drain_one(msgs, state, classes, NOW)
        assert [p[0] for p in w[0]] == disp, (msgs, state)
        wants.append(w)
    assert wants[3][2][:2] == [2, 0] and wants[4][2][:2] == [1, 0] and wants[5][2][:2] == [2, 2]
    check(eng, [(m, s) for m, s, _, _ in cases], wants)
    for k, (m, s, _, _) in enumerate(cases):   # and each alone
        check(eng, [(m, s)], [wants[k]], what=f"case {k}")


def test_unbounded_takes_a_thousand_and_ids_wrap(eng):
    msgs = []
    for k in range(1003):   # 1,003 counted messages, QoS 0 and expired ones between them
        msgs.append(q1(k % 2))
        if k % 5 == 0:
            msgs.append(q0(k % 2))
        if k % 7 == 0:
            msgs.append(gone(k % 2))
    want = MQ.drain_one(msgs, st(65000), ["infinity", 0], NOW)
    per = want[0]
    ids = sorted((p[2], p[1]) for p in per if p[0] == SEND)   # in publish order
    assert len(ids) == 1000 == want[1][1] and want[1][0] == (65000 - 1 + 1000) % 65535 + 1 == 465
    seq = [i for _, i in ids]
    assert seq[:2] == [65000, 65001] and seq[535:538] == [65535, 1, 2] and seq[-1] == 464
    assert sum(1 for b, _, _ in msgs if b & 3 and not b & 4) == 1003
    kept = [p[0] for p in per].count(KEPT)
    assert kept >= 3 and want[2][0] == sum(1 for b, _, _ in msgs if not (b >> 4) & 7)   # class 0 whole, the cut in class 1
    check(eng, [(msgs, st(65000))], [want])


# ---- 4. wave and tile edges ---------------------------------------------------------

def _big_session():
    """2 tiles + 12 messages over 3 classes, the members interleaved so that
    every class has messages in every wave; Cnt puts the cut on the first
    counted message the middle class has in the last wave."""
    n = 2 * K.TILE + 12
    msgs = []
    for k in range(n):
        c = k % 3
        if k >= 2 * K.TILE:
            msgs.append(q1(c))
        elif k % 11 == 0:
            msgs.append(q0(c))
        elif k % 13 == 0:
            msgs.append(gone(c))
        elif k % 17 == 0:
            msgs.append(fresh(c, 2))
        else:
            msgs.append(q1(c))
    counted = lambda b: (b & 3) > 0 and not (b & 4 and b & 3 == 1)   # noqa: E731  (gone() is QoS 1 with the flag)
    k0 = sum(1 for b, _, _ in msgs if (b >> 4) == 0 and counted(b))
    k1a = sum(1 for b, _, _ in msgs[:2 * K.TILE] if (b >> 4) == 1 and counted(b))
    return msgs, st(60000, k0 + k1a + 1)


@pytest.mark.parametrize("before", [0, K.WAVE - 1, K.WAVE], ids=["alone", "after_wave_less_one", "after_a_whole_wave"])
def test_wave_and_tile_edges(eng, before):
    msgs, state = _big_session()
    want = MQ.drain_one(msgs, state, [2, 1, 0], NOW)
    per = want[0]
    nw = (len(msgs) + K.WAVE - 1) // K.WAVE
    assert nw == 9 and all({(b >> 4) & 7 for b, _, _ in msgs[w * K.WAVE:(w + 1) * K.WAVE]} == {0, 1, 2} for w in range(nw))
    sent = [k for k, p in enumerate(per) if p[0] == SEND]
    last = max(sent, key=lambda k: per[k][2])            # the Cnt-th counted message
    assert len(sent) == state["inflight_free"] and last >= 2 * K.TILE and (msgs[last][0] >> 4) == 1
    assert want[2][0] == sum(1 for b, _, _ in msgs if (b >> 4) == 0) and 0 < want[2][1] and want[2][2] == 0
    assert per[last + 3][0] == KEPT and per[last + 1][0] == KEPT      # the middle class's next member, the lowest class
    sessions, wants = [(msgs, state)], [want]
    if before:
        pre = [q1(k % 2) if k % 3 else q0(k % 2) for k in range(before)]
        ps = st(3, 100)
        sessions.insert(0, (pre, ps))
        wants.insert(0, MQ.drain_one(pre, ps, [1, 0], NOW))
        assert len(pre) % K.WAVE == (before % K.WAVE)
    check(eng, sessions, wants)


# ---- 5. the second scan level ---------------------------------------------------------

def test_second_scan_level(eng):
    Q = K.SCAN_BLOCK + 1030
    rng = np.random.default_rng(5)
    lens = []
    while sum(lens) < Q:
        lens.append(int(rng.integers(1, 5001)))
    lens[-1] -= sum(lens) - Q
    assert lens[-1] >= 1 and sum(lens) == Q and (Q + K.WAVE - 1) // K.WAVE > K.SCAN_BLOCK // K.WAVE
    n = len(lens)
    qos = rng.choice(np.array([0, 1, 1, 2], np.uint8), Q)
    cls = (rng.random(Q) < 0.5).astype(np.uint8)
    flag = rng.random(Q) < 0.2
    expiry = rng.integers(1, 100, Q).astype(np.uint32)
    created = NOW - rng.integers(0, 200_000, Q)
    qmsg = (qos | flag.astype(np.uint8) << 2 | cls << 4).astype(np.uint8)
    free = rng.choice(np.array([0, 5, 32, 700, UNB], np.uint32), n)
    P = rng.integers(1, 65536, n).astype(np.uint32)
    off = np.cumsum([0] + lens)
    flat = list(zip(qmsg.tolist(), created.tolist(), expiry.tolist()))
    wants = [MQ.drain_flat(flat[off[r]:off[r + 1]], st(int(P[r]), int(free[r])), NOW) for r in range(n)]
    want = K.want_arrays(wants)
    assert all(K.totals_of(want).values())
    got = eng.drain(np.stack([P, free], 1), {"q_off": off.astype(np.uint64), "qmsg": qmsg, "created_ms": created,
                                              "expiry_s": expiry}, NOW)
    K.assert_same(got, want)
    assert eng.drain_info["totals"] == K.totals_of(want)
    assert (got["popped"].sum(1) == got["records"][:, 1:].sum(1)).all()
    assert eng.drain_info["kernel_ms"] > 0


# ---- 6. random property ---------------------------------------------------------------

@pytest.mark.parametrize("seed", range(5))
def test_random_sessions_equal_drain_one(eng, seed):
    rng = np.random.default_rng(seed)
    sessions, wants = [], []
    for _ in range(3000):
        classes = K.CLASS_SETS[int(rng.integers(0, len(K.CLASS_SETS)))]
        msgs, state = K.random_session(rng, int(rng.integers(0, 301)), len(classes))
        sessions.append((msgs, state))
        wants.append(MQ.drain_one(msgs, state, classes, NOW))
    assert any(not m for m, _ in sessions) and any(s["inflight_free"] == UNB for _, s in sessions)
    check(eng, sessions, wants)


# ---- 7. no session; no state between calls -------------------------------------------------

def test_no_session_and_no_state_between_calls(eng):
    got = eng.drain([], {"q_off": np.zeros(1, np.uint64), "qmsg": np.zeros(0, np.uint8)}, NOW)
    assert got["records"].shape == (0, 4) and got["popped"].shape == (0, 8) and len(got["disp"]) == 0
    assert eng.drain_info["totals"] == {"send0": 0, "send": 0, "kept": 0, "expired": 0}
    # only empty sessions: the records keep next_pkt_id
    got = drain(eng, [EMPTY, EMPTY])
    K.assert_same(got, K.want_arrays([EMPTY_WANT, EMPTY_WANT]))
    msgs = [fresh(k % 2, k % 3) for k in range(3000)]
    sessions = [(msgs, st(7, 50)), EMPTY, (msgs[:10], st(8))]
    late = NOW + 3_600_000
    w1 = [MQ.drain_one(m, s, [1, 0], NOW) for m, s in sessions]
    w2 = [MQ.drain_one(m, s, [1, 0], late) for m, s in sessions]
    assert w1[0][1][3] == 0 and w2[0][1][3] == 3000 and w1[0][1][1] == 50 and w2[0][1][1] == 0
    check(eng, sessions, w1, NOW)
    check(eng, sessions, w2, late)
    check(eng, sessions, w1, NOW)
