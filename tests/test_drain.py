"""The session drain on the CPU: the mirrors of emqx_session:dequeue/1 and
emqx_message's expiry clauses against the reference's known answers, the flat
fold and the closed form of include/emqx_tm.h against the pqueue fold on
seeded random sessions, and every argument check of tm_sessions_drain on a
host-only engine."""

import ctypes as C
import os

import numpy as np
import pytest

import drain_cases as K
from emqx_amd import _native as N
from emqx_amd import emqx_message as M
from emqx_amd import emqx_mqueue as MQ
from emqx_amd import emqx_session as S
from emqx_amd.engine import Engine

KATS = K.load_kats()


@pytest.mark.parametrize("case", KATS["cases"], ids=lambda c: c["name"])
def test_kat_through_drain_one(case):
    msgs, state, classes, now, want = K.kat_session(case)
    assert MQ.drain_one(msgs, state, classes, now) == want
    assert MQ.drain_flat(msgs, state, now) == want
    assert K.closed_form(msgs, state, now) == want
    assert sum(want[2]) == sum(want[1][1:])


def test_kat_message_expiry():
    for c in KATS["message"]["is_expired"]:
        m = {"qos": 0, "timestamp": 10_000, "headers": {} if c["interval"] is None else {"properties": {M.EXPIRY: c["interval"]}}}
        assert M.is_expired(m, 10_000 + c["elapsed_ms"]) is c["want"], c
    for c in KATS["message"]["update_expiry"]:
        m = {"qos": 0, "timestamp": 10_000, "headers": {} if c["interval"] is None else {"properties": {M.EXPIRY: c["interval"]}}}
        m1 = M.update_expiry(m, 10_000 + c["elapsed_ms"])
        if c["want"] is None:
            assert m1 is m
        else:
            assert m1["headers"]["properties"][M.EXPIRY] == c["want"] and m["headers"]["properties"][M.EXPIRY] == c["interval"]
    # the clauses' edges: elapsed/1 never negative, `>` not `>=`, the interval never below 1, unchanged at elapsed 0
    assert M.elapsed(5, 3) == 0 and M.elapsed(3, 5) == 2
    m = {"timestamp": 0, "headers": {"properties": {M.EXPIRY: 2}}}
    assert not M.is_expired(m, 2000) and M.is_expired(m, 2001) and not M.is_expired(m, -5)
    assert M.update_expiry(m, 0) is m and M.update_expiry(m, -7) is m
    assert M.update_expiry(m, 1)["headers"]["properties"][M.EXPIRY] == 2
    assert M.update_expiry(m, 1999)["headers"]["properties"][M.EXPIRY] == 1
    assert M.update_expiry(m, 2000)["headers"]["properties"][M.EXPIRY] == 1
    # t_next_pakt_id (test/emqx_session_SUITE.erl:358-363) on the session mirror itself
    s = S.new_session(0xFFFF)
    S.next_pkt_id(s)
    assert s["next_pkt_id"] == 1
    S.next_pkt_id(s)
    assert s["next_pkt_id"] == 2
    assert S.batch_n(S.new_session(1, 0)) == S.DEFAULT_BATCH_N == N.TM_DRAIN_BATCH_N == 1000
    assert S.batch_n(S.new_session(1, 5, [1, 2])) == 3


def test_flat_fold_and_closed_form_equal_the_pqueue_fold():
    """About 2,000 seeded sessions: 1 to 8 classes (infinity and priority 0
    together among them), QoS 0 mixed in, expiry edges, inflight_free 0, small
    and unbounded, queues up to 1,200 messages."""
    rng = np.random.default_rng(20240611)
    longest, seen_classes, n_msgs = 0, set(), 0
    disp_seen = np.zeros(4, np.int64)
    for i in range(2000):
        classes = K.CLASS_SETS[int(rng.integers(0, len(K.CLASS_SETS)))]
        n = int(rng.integers(1001, 1201)) if i % 50 == 0 else int(rng.integers(0, 40))
        msgs, state = K.random_session(rng, n, len(classes))
        if i % 50 == 0 and i % 100:
            state["inflight_free"] = K.UNB   # Cnt = 1000 inside a queue longer than that
        want = MQ.drain_one(msgs, state, classes, K.NOW)
        assert MQ.drain_flat(msgs, state, K.NOW) == want, (i, state)
        assert K.closed_form(msgs, state, K.NOW) == want, (i, state)
        assert sum(want[2]) == sum(want[1][1:])
        longest, n_msgs = max(longest, n), n_msgs + n
        seen_classes.add(len(classes))
        disp_seen += np.bincount([r[0] for r in want[0]], minlength=4)
    assert longest > 1000 and seen_classes == set(range(1, 9)) and disp_seen.all(), (longest, seen_classes, disp_seen)


def test_the_bench_tools_numpy_route_equals_the_fold():
    """tools/drain_bench.py checks the device against a NumPy route before it
    keeps a time; that route against drain_one, over empty sessions too."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("drain_bench", os.path.join(K.HERE, "..", "tools", "drain_bench.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(3)
    sessions, wants = [], []
    for i in range(300):
        classes = K.CLASS_SETS[int(rng.integers(0, len(K.CLASS_SETS)))]
        msgs, state = K.random_session(rng, int(rng.integers(0, 60)) if i % 40 else 1100, len(classes))
        sessions.append((msgs, state))
        wants.append(MQ.drain_one(msgs, state, classes, K.NOW))
    st, q = K.pack(sessions)
    got = tool.numpy_route(st, q["q_off"], q["qmsg"], q["created_ms"], q["expiry_s"], K.NOW)
    want = K.want_arrays(wants)
    K.assert_same(dict(zip(("disp", "packet_ids", "order", "expiry_out", "records", "popped"), got[:6])), want)
    assert dict(zip(("send0", "send", "kept", "expired"), got[6].tolist())) == K.totals_of(want)


# ---- tm_sessions_drain on a host-only engine -------------------------------------------

def _last_error(L) -> str:
    return (L.tm_last_error() or b"").decode()


class _Call:
    """One well-formed call (two sessions, three messages) whose parts a case breaks."""

    def __init__(self):
        self.sess = np.array([[1, 5], [65535, K.UNB]], np.uint32)
        self.q_off = np.array([0, 2, 3], np.uint64)
        self.qmsg = np.array([1, MQ.qmsg_of(2, 3, True), 0], np.uint8)
        self.created = np.zeros(3, np.int64)
        self.expiry = np.ones(3, np.uint32)
        self.disp, self.pid = np.zeros(3, np.uint8), np.zeros(3, np.uint16)
        self.order, self.eout = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
        self.rec, self.popped = np.zeros((2, 4), np.uint32), np.zeros((2, 8), np.uint32)
        self.di, self.do = N.DrainIn(), N.DrainOut()
        d, o = self.di, self.do
        d.sessions = C.cast(self.sess.ctypes.data, C.POINTER(N.DrainSession))
        d.q_off, d.qmsg, d.created_ms, d.expiry_s = (x.ctypes.data for x in (self.q_off, self.qmsg, self.created, self.expiry))
        d.now_ms, d.n_sessions = 5, 2
        o.disp, o.packet_ids, o.order, o.expiry_out = (x.ctypes.data for x in (self.disp, self.pid, self.order, self.eout))
        o.records = C.cast(self.rec.ctypes.data, C.POINTER(N.DrainRecord))
        o.popped = self.popped.ctypes.data


def test_sessions_drain_validation_host_only():
    """Every TM_EINVAL of tm_sessions_drain, each message naming the offender,
    found before the device is asked for; then TM_ENODEV."""
    eng = Engine(device=-1)
    L = eng.L

    def run(c):
        return L.tm_sessions_drain(eng.h, C.byref(c.di), C.byref(c.do))

    ok = _Call()
    assert run(ok) == N.TM_ENODEV
    assert L.tm_sessions_drain(None, C.byref(ok.di), C.byref(ok.do)) == N.TM_EINVAL
    assert L.tm_sessions_drain(eng.h, None, C.byref(ok.do)) == N.TM_EINVAL and "in is NULL" in _last_error(L)
    assert L.tm_sessions_drain(eng.h, C.byref(ok.di), None) == N.TM_EINVAL and "out is NULL" in _last_error(L)

    def broken(word, f):
        c = _Call()
        f(c)
        assert run(c) == N.TM_EINVAL and word in _last_error(L), (word, _last_error(L))
        assert "tm_sessions_drain" in _last_error(L)

    for name in ("sessions", "q_off", "qmsg"):
        broken(name + " is NULL", lambda c, name=name: setattr(c.di, name, None))
    for name in ("disp", "packet_ids", "order", "records", "popped"):
        broken(name + " is NULL", lambda c, name=name: setattr(c.do, name, None))
    broken("session 0: next_pkt_id 0 outside", lambda c: c.sess.__setitem__((0, 0), 0))
    broken("session 1: next_pkt_id 65536 outside", lambda c: c.sess.__setitem__((1, 0), 65536))
    broken("session 1: offsets not monotone (1 after 2)", lambda c: c.q_off.__setitem__(2, 1))
    broken("q_off[0] = 1", lambda c: c.q_off.__setitem__(0, 1))
    broken("4294967296 messages, not below 2^32", lambda c: c.q_off.__setitem__(2, 1 << 32))
    broken("message 2: QoS 3", lambda c: c.qmsg.__setitem__(2, 3))
    broken("message 0: reserved bits set (qmsg = 0x09)", lambda c: c.qmsg.__setitem__(0, 9))
    broken("message 2: reserved bits set (qmsg = 0x80)", lambda c: c.qmsg.__setitem__(2, 0x80))
    broken("message 1 has TM_QMSG_EXPIRY but created_ms is NULL", lambda c: setattr(c.di, "created_ms", None))
    broken("message 1 has TM_QMSG_EXPIRY but expiry_s is NULL", lambda c: setattr(c.di, "expiry_s", None))
    broken("pad0 = 7", lambda c: setattr(c.di, "pad0", 7))
    # legal: both arrays NULL when no message carries the flag; expiry_out NULL; every class; no session at all
    c = _Call()
    c.qmsg[1] = MQ.qmsg_of(2, 7)
    c.di.created_ms = c.di.expiry_s = None
    c.do.expiry_out = None
    assert run(c) == N.TM_ENODEV
    c = _Call()
    c.di.n_sessions = 0
    c.di.sessions = c.di.q_off = c.di.qmsg = None
    assert run(c) == N.TM_ENODEV
    # through the wrapper
    st, q = K.pack([([(1, 0, 0)], {"next_pkt_id": 1, "inflight_free": 1})])
    with pytest.raises(N.TmError) as ei:
        eng.drain(st, q, 0)
    assert ei.value.rc == N.TM_ENODEV
    q["qmsg"][0] = 3
    with pytest.raises(N.TmError) as ei:
        eng.drain(st, q, 0)
    assert ei.value.rc == N.TM_EINVAL and "QoS 3" in str(ei.value)
    with pytest.raises(ValueError):
        eng.drain(st, dict(q, q_off=np.array([0, 2], np.uint64)), 0)
    eng.close()
