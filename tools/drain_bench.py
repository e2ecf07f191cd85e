"""Timing of tm_sessions_drain (the dequeue after acks with message expiry) on
one batch of acks over many sessions.  Dev/measurement tool, no pass/fail on
time.

    python tools/drain_bench.py [sessions] [reps] [warmup] [out.json]

The workload (seed 1): `sessions` sessions (1,000,000), queue lengths uniform in
0..120 (about 60 M messages), three classes, QoS 0 / 1 / 2 mixed, 10 % of the
messages with a Message-Expiry-Interval and 5 % of those expired, inflight_free
32 with 1 % of the sessions unbounded, next_pkt_id anywhere in 1..65535.
Before any time is kept the result must equal a NumPy route array for array:
a stable argsort on (session, class) gives the out order, cumulative sums less
the session's base give C(m) and U(m), then the closed form of
include/emqx_tm.h.  Kept: kernel_ms (HIP events around the drain kernels),
host-to-host ms of the call, the NumPy route's ms, and kernel_ms over the byte
floor at bench.py's HBM peak:
    13 Q + 16 n + 8 n    read: qmsg, created_ms, expiry_s; q_off; sessions
  + 11 Q + 48 n          written: disp, packet_ids, order, expiry_out; records, popped
The JSON file keeps one entry per session count.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emqx_amd import _native as N  # noqa: E402
from emqx_amd.engine import Engine  # noqa: E402

HBM_PEAK_GBS = 8000.0            # bench.py's roofline peak
UNB = N.TM_SESS_UNBOUNDED
SEND0, SEND, KEPT, EXPIRED = N.TM_DRAIN_SEND0, N.TM_DRAIN_SEND, N.TM_DRAIN_KEPT, N.TM_DRAIN_EXPIRED


def numpy_route(sess, q_off, qmsg, created, expiry, now):
    """-> (disp, packet_ids, order, expiry_out, records, popped, totals)"""
    n, Q = len(sess), len(qmsg)
    off = q_off.astype(np.int64)
    lens = np.diff(off)
    ri = np.repeat(np.arange(n, dtype=np.int64), lens)
    cls = ((qmsg >> 4) & 7).astype(np.int64)
    flagged = (qmsg & N.TM_QMSG_EXPIRY) != 0
    el = np.maximum(0, now - created)
    iv = expiry.astype(np.int64)
    expired = flagged & (el > iv * 1000)
    counted = ~expired & ((qmsg & 3) > 0)
    srt = np.argsort(ri * 8 + cls, kind="stable")   # the out order of every session, sessions in place
    rs = ri[srt]
    start = off[rs]                                 # a session's span is the same in both orders

    def rank(flags):
        f = flags[srt].astype(np.int64)
        cs = np.cumsum(f) - f
        return cs - cs[start]

    Cm, Um = rank(counted), rank(~expired)
    P, F = sess[:, 0].astype(np.int64), sess[:, 1].astype(np.int64)
    cnt = np.where(F == UNB, N.TM_DRAIN_BATCH_N, F)
    pop = Cm < cnt[rs]
    ex_s, co_s = expired[srt], counted[srt]
    d_s = np.where(~pop, KEPT, np.where(ex_s, EXPIRED, np.where(co_s, SEND, SEND0)))
    sent = d_s < KEPT
    pid_s = np.where(d_s == SEND, (P[rs] - 1 + Cm % 65535) % 65535 + 1, 0)
    ord_s = np.where(sent, Um, N.TM_DRAIN_NO_ORDER)
    el_s, iv_s = el[srt], iv[srt]
    eo_s = np.where(sent & flagged[srt] & (el_s > 0), np.maximum(1, iv_s - el_s // 1000), iv_s)
    disp, pid = np.empty(Q, np.uint8), np.empty(Q, np.uint16)
    order, eout = np.empty(Q, np.uint32), np.empty(Q, np.uint32)
    disp[srt], pid[srt], order[srt], eout[srt] = d_s, pid_s, ord_s, eo_s
    per = np.stack([np.bincount(rs[d_s == k], minlength=n) for k in (SEND, SEND0, EXPIRED)], 1)
    rec = np.concatenate([((P - 1 + per[:, 0] % 65535) % 65535 + 1)[:, None], per], 1).astype(np.uint32)
    popped = np.bincount((rs * 8 + cls[srt])[pop], minlength=n * 8).reshape(n, 8).astype(np.uint32)
    return disp, pid, order, eout, rec, popped, np.bincount(disp, minlength=N.TM_DRAIN_COUNT).astype(np.uint64)


def main():
    args = sys.argv[1:]
    n = int(args[0]) if len(args) > 0 else 1_000_000
    reps = int(args[1]) if len(args) > 1 else 10
    warm = int(args[2]) if len(args) > 2 else 3
    out_path = args[3] if len(args) > 3 else os.path.join(ROOT, "profiles", "drain", "drain_bench.json")

    rng = np.random.default_rng(1)
    lens = rng.integers(0, 121, n)
    q_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    Q = int(q_off[-1])
    now = 1_700_000_000_000
    flagged = rng.random(Q) < 0.10
    gone = flagged & (rng.random(Q) < 0.05)
    qmsg = (rng.integers(0, 3, Q) | flagged.astype(np.int64) << 2 | rng.integers(0, 3, Q) << 4).astype(np.uint8)
    expiry = rng.integers(60, 3600, Q).astype(np.uint32)
    age = np.where(gone, expiry.astype(np.int64) * 1000 + rng.integers(1, 600_000, Q),
                   (rng.random(Q) * expiry * 1000).astype(np.int64))
    created = (now - age).astype(np.int64)
    sess = np.empty((n, 2), np.uint32)
    sess[:, 0] = rng.integers(1, 65536, n)
    sess[:, 1] = np.where(rng.random(n) < 0.01, UNB, 32)

    eng = Engine(device=0)
    out = [np.zeros(Q, np.uint8), np.zeros(Q, np.uint16), np.zeros(Q, np.uint32), np.zeros(Q, np.uint32),
           np.zeros((n, 4), np.uint32), np.zeros((n, 8), np.uint32)]
    di, do = N.DrainIn(), N.DrainOut()
    di.sessions = C.cast(sess.ctypes.data, C.POINTER(N.DrainSession))
    di.q_off, di.qmsg, di.created_ms, di.expiry_s = q_off.ctypes.data, qmsg.ctypes.data, created.ctypes.data, expiry.ctypes.data
    di.now_ms, di.n_sessions = now, n
    do.disp, do.packet_ids, do.order, do.expiry_out = (a.ctypes.data for a in out[:4])
    do.records = C.cast(out[4].ctypes.data, C.POINTER(N.DrainRecord))
    do.popped = out[5].ctypes.data

    def run():
        t = time.perf_counter()
        N.check(eng.L.tm_sessions_drain(eng.h, C.byref(di), C.byref(do)), "tm_sessions_drain")
        return 1e3 * (time.perf_counter() - t), float(do.kernel_ms)

    run()
    t = time.perf_counter()
    want = numpy_route(sess, q_off, qmsg, created, expiry, now)
    numpy_ms = 1e3 * (time.perf_counter() - t)
    got = out + [np.array(list(do.totals), np.uint64)]
    same = all(np.array_equal(g, w) for g, w in zip(got, want))
    if not same:
        print(json.dumps({"sessions": n, "equal_results": False,
                          "first_difference": [k for k, (g, w) in enumerate(zip(got, want)) if not np.array_equal(g, w)]}))
        sys.exit(1)
    hs, ks = [], []
    for it in range(warm + reps):
        h, k = run()
        if it >= warm:
            hs.append(h)
            ks.append(k)
    stats = lambda x: {"min": round(float(np.min(x)), 3), "median": round(float(np.median(x)), 3),  # noqa: E731
                       "max": round(float(np.max(x)), 3)}
    floor = 13 * Q + 16 * n + 8 * n + 11 * Q + 48 * n
    floor_ms = floor / (HBM_PEAK_GBS * 1e9) * 1e3
    entry = {"sessions": n, "messages": Q, "classes": 3, "reps": reps, "warmup": warm, "equal_results": True,
             "totals": dict(zip(["send0", "send", "kept", "expired"], [int(x) for x in want[6]])),
             "kernel_ms": stats(ks), "host_to_host_ms": stats(hs), "numpy_route_ms": round(numpy_ms, 1),
             "byte_floor": {"bytes": floor, "formula": "13 Q + 16 n + 8 n read, 11 Q + 48 n written",
                            "peak_gbs": HBM_PEAK_GBS, "floor_ms": round(floor_ms, 4),
                            "kernel_ms_over_floor": round(float(np.median(ks)) / floor_ms, 2)}}
    doc = {}
    if os.path.exists(out_path):
        try:
            with open(out_path) as fh:
                doc = json.load(fh)
        except (OSError, ValueError):
            doc = {}
    doc[str(n)] = entry
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({str(n): entry}))
    eng.close()


if __name__ == "__main__":
    main()
