"""Shared by the session-drain tests (not a test module): the known answers of
tests/golden/kat_session_drain.json, the closed form of include/emqx_tm.h
written out per session, seeded random sessions, and the packing of sessions
into tm_sessions_drain's arrays.

A message is (qmsg byte, created_ms, expiry_s); a session is (msgs, state) with
state = {"next_pkt_id", "inflight_free"}.
"""

import json
import os

import numpy as np

from emqx_amd import emqx_mqueue as MQ
from emqx_amd import emqx_session as S

HERE = os.path.dirname(os.path.abspath(__file__))
UNB = S.TM_SESS_UNBOUNDED
NO_ORDER = S.TM_DRAIN_NO_ORDER
SEND0, SEND, KEPT, EXPIRED = S.TM_DRAIN_SEND0, S.TM_DRAIN_SEND, S.TM_DRAIN_KEPT, S.TM_DRAIN_EXPIRED
# the builder's constants (emqx_amd/csrc/tm_kernels.hip: INBOX_WAVE_PAIRS, INBOX_TILE; tm_internal.hpp: PRIO_SCAN_TILE)
WAVE = 1024                  # messages per wave
TILE = 4096                  # messages per workgroup
SCAN_BLOCK = 1024 * WAVE     # messages one first-level scan block covers


def load_kats():
    with open(os.path.join(HERE, "golden", "kat_session_drain.json")) as f:
        return json.load(f)


def kat_session(case):
    """A case of the golden file -> (msgs, state, classes, now, want) with want
    = (per-message [(disp, id, order, expiry_out)], record, popped)."""
    rep = case.get("repeat", 1)
    msgs, per = [], []
    for i in range(rep):
        for j, (qos, cls, flag, created, expiry) in enumerate(case["msgs"]):
            msgs.append((MQ.qmsg_of(qos, cls, bool(flag)), created, expiry))
            d, pid, order = case["disp"][j], case["packet_ids"][j], case["order"][j]
            per.append((d, pid + i if d == SEND else pid, order + i if order != NO_ORDER else order,
                        case["expiry_out"][j]))
    return msgs, dict(case["state"]), case["classes"], case["now_ms"], (per, tuple(case["record"]), case["popped"])


def closed_form(msgs, state, now):
    """The closed form of include/emqx_tm.h for one session: the out order is
    the stable sort by class, C(m) and U(m) the counted / not-expired messages
    before m in it, m is popped iff C(m) < Cnt.  Same result as MQ.drain_one."""
    free = state.get("inflight_free", UNB)
    cnt = S.TM_DRAIN_BATCH_N if free == UNB else free
    P = state.get("next_pkt_id", 1)
    res = [None] * len(msgs)
    popped = [0] * MQ.TM_PRIO_MAX_CLASSES
    C = U = n_send = n_send0 = n_expired = 0
    for k in sorted(range(len(msgs)), key=lambda k: (msgs[k][0] >> 4) & 7):   # (sorted is stable)
        b, created, expiry = msgs[k]
        flagged = bool(b & S.TM_QMSG_EXPIRY)
        el = max(0, now - created)
        expired = flagged and el > expiry * 1000
        counted = not expired and (b & 3) > 0
        if C >= cnt:
            res[k] = (KEPT, 0, NO_ORDER, expiry)
        else:
            popped[(b >> 4) & 7] += 1
            if expired:
                res[k] = (EXPIRED, 0, NO_ORDER, expiry)
                n_expired += 1
            else:
                e = max(1, expiry - el // 1000) if flagged and el > 0 else expiry
                if counted:
                    res[k] = (SEND, ((P - 1 + C % 65535) % 65535) + 1, U, e)
                    n_send += 1
                else:
                    res[k] = (SEND0, 0, U, e)
                    n_send0 += 1
        C += counted
        U += not expired
    return res, (((P - 1 + n_send % 65535) % 65535) + 1, n_send, n_send0, n_expired), popped


NOW = 1_700_000_000_000


def random_session(rng, n, ncls, flag_p=0.3, now=NOW):
    """n messages over ncls classes: QoS 0 mixed in, flag_p of them with an
    interval, created around the edge of it (elapsed = interval * 1000 - 1, + 0,
    + 1 among them), some in the future; a bounded or an unbounded window."""
    qos = rng.choice([0, 1, 1, 2], n)
    cls = rng.integers(0, ncls, n)
    flag = rng.random(n) < flag_p
    expiry = rng.choice(np.array([0, 1, 2, 30, 3600, 0xFFFFFFFF], np.int64), n)
    el = expiry * 1000 + rng.choice([-1500, -1, 0, 1, 999, 1000, 2500], n)
    el = np.where(rng.random(n) < 0.1, -rng.integers(0, 5000, n), el)          # made after `now`
    created = now - np.where(expiry == 0xFFFFFFFF, rng.choice([0, 1, 4294967296, 4294967295001], n), el)
    # an unflagged message: whatever is in the two arrays
    created = np.where(flag, created, rng.integers(-2**62, 2**62, n))
    expiry = np.where(flag, expiry, rng.integers(0, 2**32, n))
    msgs = [(MQ.qmsg_of(int(q), int(c), bool(f)), int(t), int(e)) for q, c, f, t, e in zip(qos, cls, flag, created, expiry)]
    free = int(rng.choice([0, 1, 2, 3, 7, 32, 200, 999, 1000, 1001, UNB, UNB]))
    return msgs, {"next_pkt_id": int(rng.choice([1, 2, 65000, 65534, 65535, int(rng.integers(1, 65536))])),
                  "inflight_free": free}


CLASS_SETS = [[0], [5, 0], ["infinity", 0], ["infinity", 7, 0], [3, 2, 1, 0], ["infinity", 9, 4, 2, 0],
              [200, 100, 50, 25, 12, 6], [7, 6, 5, 4, 3, 2, 1], ["infinity", 255, 7, 6, 5, 4, 1, 0]]


def pack(sessions, with_expiry=True):
    """[(msgs, state)] -> (sessions u32[n, 2], queues dict) for Engine.drain."""
    st = np.array([[s["next_pkt_id"], s["inflight_free"]] for _, s in sessions], np.uint32).reshape(-1, 2)
    lens = [len(m) for m, _ in sessions]
    flat = [x for m, _ in sessions for x in m]
    q = {"q_off": np.cumsum([0] + lens).astype(np.uint64),
         "qmsg": np.array([x[0] for x in flat], np.uint8),
         "created_ms": np.array([x[1] for x in flat], np.int64) if with_expiry else None,
         "expiry_s": np.array([x[2] for x in flat], np.uint32) if with_expiry else None}
    return st, q


def want_arrays(results):
    """[(per-message list, record, popped)] -> the arrays Engine.drain returns."""
    per = np.array([x for r, _, _ in results for x in r], np.int64).reshape(-1, 4)
    col = lambda i, dt: per[:, i].astype(dt)  # noqa: E731
    return {"disp": col(0, np.uint8), "packet_ids": col(1, np.uint16), "order": col(2, np.uint32),
            "expiry_out": col(3, np.uint32),
            "records": np.array([r for _, r, _ in results], np.uint32).reshape(-1, 4),
            "popped": np.array([p for _, _, p in results], np.uint32).reshape(-1, MQ.TM_PRIO_MAX_CLASSES)}


def assert_same(got, want, what=""):
    for k, w in want.items():
        if got.get(k) is None:
            continue
        assert got[k].shape == w.shape, (what, k, got[k].shape, w.shape)
        bad = np.flatnonzero((got[k] != w).reshape(len(w), -1).any(1)) if len(w) else []
        assert len(bad) == 0, (what, k, int(bad[0]), got[k][bad[0]], w[bad[0]])


def totals_of(want):
    c = np.bincount(want["disp"], minlength=4)
    return {"send0": int(c[SEND0]), "send": int(c[SEND]), "kept": int(c[KEPT]), "expired": int(c[EXPIRED])}
