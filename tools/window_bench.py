"""Timing of tm_batch_window (the session's send window on the device: packet
ids, inflight, mqueue per delivery) against what a caller had to do before it
for the same result: tm_batch_deliver to the host, then the window in NumPy
with segmented cumulative sums.  Dev/measurement tool, no pass/fail on time.

    python tools/window_bench.py SHAPE [publishes] [reps] [warmup] [out.json]

SHAPE dispatch: the filters and subscriber rule of `bench.py --workload
dispatch` (C2 trie, every filter with local subscribers: 75% one, 24% 2-8, 64
hot filters with 4096, ids from a pool of 1M), 1,000,000 publishes -- the
size tools/deliver_bench.py measured.  SHAPE c1: the C1 filters with the same
subscriber rule, 100,000 publishes.
Options, seeded: random subscription QoS, nl = 1 on about 10 %; random QoS per
publish, `from` drawn from the subscriber pool for about half of them.
Sessions, seeded: two thirds of the subscriber pool are in the table (sorted by
id), the rest use the defaults; next_pkt_id near the wrap for half; an
inflight window of 0, 1, 8, 64 free slots or unbounded; a queue of max 0
(infinity), 4, 100 or 1000 with a random length; a fifth disconnected, half of
those with store_qos0; 1 % left to the host.
Both routes start from the same waited batch (the match is not timed) and run
alternating after the warm-up rounds; their results (the six deliver arrays,
disp, packet ids, records, totals) must be equal before any time is kept.
  host route  tm_batch_deliver to the host, then NumPy: the session of every
              inbox by np.searchsorted, ranks by one cumulative sum less the
              inbox's base, totals by np.add.reduceat, the closed form; wall time
  new route   tm_batch_window host-to-host, wall time, its kernel_ms, and the
              deliver kernels' kernel_ms of the same call
kernel_ms is also given over its byte floor at the bandwidth bench.py's
roofline uses.  The floor counts what the problem must move, once:
    1 D'            the delivery bytes read
  + 3 D'            disp and packet id written
  + 24 R'           per inbox: subscriber and offset read, the record written
  + 24 NS           the uploaded session table
for D' deliveries in R' inboxes and NS sessions (the implementation's head
bits, per-wave counts and its second read of the bytes are not the floor's).
The JSON file keeps one entry per shape.
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
from emqx_amd import gen  # noqa: E402
from emqx_amd.engine import Engine  # noqa: E402

HBM_PEAK_GBS = 8000.0            # bench.py's roofline peak

shape = sys.argv[1] if len(sys.argv) > 1 else "c1"
n_pub = int(sys.argv[2]) if len(sys.argv) > 2 else (1_000_000 if shape == "dispatch" else 100_000)
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
WARM = int(sys.argv[4]) if len(sys.argv) > 4 else 3
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "window", "window_bench.json")

p = gen.C2 if shape == "dispatch" else gen.C1
filters = gen.gen_filters(p)
topics = gen.gen_topics(p, filters, 1000, n_pub)
eng = Engine(device=0)
L = eng.L
fl = filters.tolist()
eng.insert_many(fl)
rng = np.random.default_rng(77)
u = rng.random(len(fl))
nsub = np.where(u < 0.75, 1, rng.integers(2, 9, len(fl)))
nsub[rng.choice(len(fl), 64, replace=False)] = 4096
total = int(nsub.sum())
pool = rng.integers(0, 1_000_000, total, dtype=np.uint32)
o_qos = rng.integers(0, 3, total).astype(np.uint8)
o_nl = (rng.random(total) < 0.10).astype(np.uint8)
so = N.SubOpts()
k = 0
for f, c in zip(fl, nsub.tolist()):
    for j in range(k, k + c):
        so.qos, so.nl = int(o_qos[j]), int(o_nl[j])
        N.check(L.tm_subscribe_opts(eng.h, f, len(f), int(pool[j]), 0, C.byref(so)), "tm_subscribe_opts")
    k += c
eng.sync()
b = eng.prepare(topics).launch().wait()
n = len(topics)
from_ = np.where(rng.random(n) < 0.5, pool[rng.integers(0, total, n)], N.TM_NONE).astype(np.uint32)
msg = rng.integers(0, 3, n).astype(np.uint8)

# the session table: u32[NS, 6] = subscriber, next_pkt_id, flags, inflight_free, mqueue_len, mqueue_max
ids = np.unique(pool)
ids = ids[rng.random(len(ids)) < 2 / 3]
NS = len(ids)
tab = np.zeros((NS, 6), np.uint32)
tab[:, 0] = ids
tab[:, 1] = np.where(rng.random(NS) < 0.5, rng.integers(65000, 65536, NS), rng.integers(1, 65536, NS))
disc = rng.random(NS) < 0.2
tab[:, 2] = (disc * N.TM_SESS_DISCONNECTED | (disc & (rng.random(NS) < 0.5)) * N.TM_SESS_STORE_QOS0
             | (rng.random(NS) < 0.01) * N.TM_SESS_HOST)
tab[:, 3] = rng.choice(np.array([0, 1, 8, 64, N.TM_SESS_UNBOUNDED], np.uint32), NS)
tab[:, 5] = rng.choice(np.array([0, 4, 100, 1000], np.uint32), NS)
tab[:, 4] = (rng.random(NS) * (np.where(tab[:, 5] > 0, tab[:, 5], 50) + 1)).astype(np.uint32)
tab[:, 4] = np.where(tab[:, 5] > 0, np.minimum(tab[:, 4], tab[:, 5]), tab[:, 4])
dflt = np.array([0, 65530, 0, 2, 1, 3], np.uint32)

do = N.DeliverOpts()
do.from_, do.msg, do.flags = from_.ctypes.data, msg.ctypes.data, 0
wo = N.WindowOpts()
wo.sessions = C.cast(tab.ctypes.data, C.POINTER(N.SessionState))
wo.n_sessions = NS
wo.defaults = N.SessionState(*[int(x) for x in dflt])
wo.flags = 0
sw = N.SessionWindow()
si = N.SessionInboxes()


def view(ptr, cnt):
    return np.ctypeslib.as_array(ptr, shape=(max(cnt, 1),))[:cnt]


def inbox_views(s):
    r, d = int(s.n_subscribers), int(s.n_deliveries)
    return (view(s.subscribers, r), view(s.inbox_offsets, r + 1), view(s.publishes, d), view(s.filter_ids, d),
            view(s.msg, d))


def run_new():
    t = time.perf_counter()
    N.check(L.tm_batch_window(eng.h, b.h, C.byref(do), C.byref(wo), C.byref(sw)), "tm_batch_window")
    ms = 1e3 * (time.perf_counter() - t)
    r, d = int(sw.inboxes.n_subscribers), int(sw.inboxes.n_deliveries)
    rec = np.ctypeslib.as_array(C.cast(sw.records, C.POINTER(C.c_uint32)), shape=(max(r, 1), 4))[:r]
    return ms, float(sw.kernel_ms), float(sw.inboxes.kernel_ms), inbox_views(sw.inboxes) + (
        view(sw.disp, d), view(sw.packet_ids, d), rec, np.array(list(sw.totals), np.uint64))


def numpy_window(subs, offs, dm, tab, dflt):
    """The window of deliver's arrays: the session of every inbox by
    np.searchsorted, ranks by one cumulative sum less the inbox's base, totals
    by np.add.reduceat, then the closed form of include/emqx_tm.h."""
    r, d, ns = len(subs), len(dm), len(tab)
    i = np.minimum(np.searchsorted(tab[:, 0], subs), max(ns - 1, 0))
    st = np.where((tab[i, 0] == subs)[:, None], tab[i], dflt[None, :]) if ns else np.repeat(dflt[None, :], r, 0)
    P, flg, F = st[:, 1].astype(np.int64), st[:, 2], st[:, 3].astype(np.int64)
    Lq, M = st[:, 4].astype(np.int64), st[:, 5].astype(np.int64)
    host, dsc = (flg & N.TM_SESS_HOST) != 0, (flg & N.TM_SESS_DISCONNECTED) != 0
    store = dsc & ((flg & N.TM_SESS_STORE_QOS0) != 0)
    o64 = offs.astype(np.int64)
    lens = np.diff(o64)
    ri = np.repeat(np.arange(r), lens)
    counted = ~host[ri] & (((dm & 3) > 0) | store[ri])
    cs = np.cumsum(counted) - counted                       # exclusive
    rank = cs - np.repeat(cs[o64[:-1]], lens) if d else cs
    tot = np.add.reduceat(counted.astype(np.int64), o64[:-1]) if d else np.zeros(0, np.int64)
    nsend = np.where(dsc, 0, np.minimum(F, tot))
    E = tot - nsend
    drops = np.where(M > 0, np.maximum(0, Lq + E - M), 0)
    old = np.minimum(drops, Lq)
    dnew = drops - old
    disp = np.where(rank < np.repeat(nsend, lens), 1, np.where(rank < np.repeat(nsend + dnew, lens), 4, 2))
    disp = np.where(counted, disp, np.where(dsc[ri], 3, 0))
    disp = np.where(host[ri], 5, disp).astype(np.uint8)
    pid = np.where(disp == 1, (np.repeat(P, lens) - 1 + rank) % 65535 + 1, 0).astype(np.uint16)
    rec = np.stack([np.where(host, P, (P - 1 + nsend) % 65535 + 1), np.where(host, 0, nsend),
                    np.where(host, 0, E - dnew), np.where(host, 0, old)], 1).astype(np.uint32)
    return disp, pid, rec, np.bincount(disp, minlength=N.TM_DISP_COUNT).astype(np.uint64)


def run_host():
    """tm_batch_deliver over PCIe, then the window in NumPy."""
    t = time.perf_counter()
    N.check(L.tm_batch_deliver(eng.h, b.h, C.byref(do), C.byref(si)), "tm_batch_deliver")
    subs, offs, pubs, fids, dm = inbox_views(si)
    res = (subs, offs, pubs, fids, dm) + numpy_window(subs, offs, dm, tab, dflt)
    ms = 1e3 * (time.perf_counter() - t)
    return ms, res


def stats(x):
    return {"min": round(float(np.min(x)), 3), "median": round(float(np.median(x)), 3),
            "max": round(float(np.max(x)), 3)}


new_ms, new_k, dlv_k, host_ms = [], [], [], []
same = True
for it in range(WARM + reps):
    a, km, dk, got = run_new()
    got = tuple(x.copy() for x in got)
    h, want = run_host()
    same = same and all(np.array_equal(x, y) for x, y in zip(got, want))
    totals = [int(x) for x in got[8]]
    d_left, r_left = len(got[4]), len(got[0])
    n_defaults = int((~np.isin(got[0], tab[:, 0])).sum())
    del got, want
    if it >= WARM:
        new_ms.append(a); new_k.append(km); dlv_k.append(dk); host_ms.append(h)
if not same:
    print(json.dumps({"shape": shape, "equal_results_both_routes": False}))
    sys.exit(1)
floor_b = 4 * d_left + 24 * r_left + 24 * NS
floor_ms = floor_b / (HBM_PEAK_GBS * 1e9) * 1e3
entry = {"publishes": n_pub, "filters": len(fl), "subscriptions": total, "sessions": NS,
         "deliveries_left": d_left, "inboxes": r_left, "inboxes_on_defaults": n_defaults,
         "totals": dict(zip(["send0", "send", "queued", "drop_qos0", "drop_full", "host"], totals)),
         "reps": reps, "warmup": WARM, "equal_results_both_routes": True,
         "window_host_ms": stats(new_ms), "window_kernel_ms": stats(new_k), "deliver_kernel_ms_same_call": stats(dlv_k),
         "deliver_plus_numpy_host_ms": stats(host_ms),
         "speedup_host_median": round(float(np.median(host_ms) / np.median(new_ms)), 2),
         "byte_floor": {"bytes": floor_b, "formula": "4 D' + 24 R' + 24 NS", "peak_gbs": HBM_PEAK_GBS,
                        "floor_ms": round(floor_ms, 5),
                        "kernel_ms_over_floor": round(float(np.median(new_k)) / floor_ms, 2) if floor_ms else None}}
doc = {}
if os.path.exists(out_path):
    try:
        with open(out_path) as fh:
            doc = json.load(fh)
    except (OSError, ValueError):
        doc = {}
doc[shape] = entry
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(json.dumps(doc, indent=1) + "\n")
print(json.dumps({shape: entry}))
