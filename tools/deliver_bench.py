"""Timing of tm_batch_deliver (what the session sends: ignore_local/3 and
enrich_subopts/3 on the device) against what a caller had to do before it for
the same result: tm_batch_inboxes to the host, then the two per-delivery
lookups in NumPy with searches on sorted keys.  Dev/measurement tool, no
pass/fail on time.

    python tools/deliver_bench.py SHAPE [publishes] [reps] [warmup] [out.json]

SHAPE dispatch: the workload of `bench.py --workload dispatch` (C2 trie, every
filter with local subscribers: 75% one, 24% 2-8, 64 hot filters with 4096,
ids from a pool of 1M; 10,000,000 publishes).  SHAPE c1: the C1 filters with
the same subscriber rule, 100,000 publishes.
Options, seeded: nl = 1 on about 10 % of the subscriptions, random QoS / rap,
a subid on half; `from` drawn from the subscriber pool for about half of the
publishes (TM_NONE otherwise), random QoS / retain / retained per publish.  A
publisher drawn at random hardly ever receives its own publish, so for about
an eighth of the publishes `from` is then set to one of the publish's own
No-Local receivers (picked from the batch's inboxes): those deliveries are
own, and the ones that lead their inbox drop.
Both routes start from the same waited batch (the match is common to both and
not timed) and run alternating after the warm-up rounds; their results
(subscribers, inbox offsets, publishes, filter ids, msg, subids) must be equal
before any time is kept.
  host route  tm_batch_inboxes to the host, then NumPy: the options of every
              delivery by np.searchsorted on the sorted (subscriber << 32 |
              filter id) keys, the leading own run per inbox by
              np.minimum.reduceat, the compaction by a boolean mask; wall time
  new route   tm_batch_deliver host-to-host (TM_DELIVER_SUBIDS), wall time,
              its kernel_ms, and tm_batch_inboxes' kernel_ms of the same run
kernel_ms is also given over its byte floor at the bandwidth bench.py's
roofline uses.  The floor counts what the problem must move, once:
    12 D            the inboxes read (subscriber key, publish, filter id)
  + 13 D'           the result written (publish, filter id, msg, subid)
  + 5 n             from and msg
  + 8 T + 4 NS      the options table (node id, payload; the subscribers)
for D deliveries in, D' left, n publishes, T subscriptions of NS subscribers
(the implementation's re-reads of the keys and its flag bytes are not the
floor's).  The no-drop fast path (from = NULL) is timed the same way; its floor
is 12 D + 5 D + 1 n + 8 T + 4 NS.  The JSON file keeps one entry per shape.
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
n_pub = int(sys.argv[2]) if len(sys.argv) > 2 else (10_000_000 if shape == "dispatch" else 100_000)
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
WARM = int(sys.argv[4]) if len(sys.argv) > 4 else 3
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "deliver", "deliver_bench.json")

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
o_rap = rng.integers(0, 2, total).astype(np.uint8)
o_subid = np.where(rng.random(total) < 0.5, rng.integers(1, N.TM_SUBID_MAX + 1, total), 0).astype(np.uint32)
so = N.SubOpts()
tkey = np.zeros(total, np.uint64)
k = 0
for f, c in zip(fl, nsub.tolist()):
    fid = eng.filter_id(f)
    for j in range(k, k + c):
        so.qos, so.nl, so.rap, so.subid = int(o_qos[j]), int(o_nl[j]), int(o_rap[j]), int(o_subid[j])
        N.check(L.tm_subscribe_opts(eng.h, f, len(f), int(pool[j]), 0, C.byref(so)), "tm_subscribe_opts")
        tkey[j] = (int(pool[j]) << 32) | fid
    k += c
# the host route's table: the LAST options given to a (subscriber, filter) win the
# four flags (a repeated pair merges), the subid only when non-zero -- read back
order = np.argsort(tkey, kind="stable")
tkey = tkey[order]
last = np.r_[tkey[1:] != tkey[:-1], True]
tkey = tkey[last]
got = N.SubOpts()
tval = np.zeros(len(tkey), np.uint32)
fbytes = {}
for i, key in enumerate(tkey.tolist()):
    fid = key & 0xFFFFFFFF
    f = fbytes.get(fid)
    if f is None:
        f = fbytes[fid] = eng.filter_bytes(fid)
    N.check(L.tm_get_subopts(eng.h, f, len(f), key >> 32, C.byref(got)), "tm_get_subopts")
    tval[i] = got.subid << 4 | got.rap << 3 | got.nl << 2 | got.qos
eng.sync()
b = eng.prepare(topics).launch().wait()
n = len(topics)
from_ = np.where(rng.random(n) < 0.5, pool[rng.integers(0, total, n)], N.TM_NONE).astype(np.uint32)
msg = (rng.integers(0, 3, n) | rng.choice([0, 4], n) | rng.choice([0, 8], n)).astype(np.uint8)
ib = N.Inboxes()
si = N.SessionInboxes()
do = N.DeliverOpts()
# own deliveries: n / 8 deliveries on No-Local subscriptions, their publish published by their subscriber
N.check(L.tm_batch_inboxes(eng.h, b.h, 0, C.byref(ib)), "tm_batch_inboxes")
_r, _d = int(ib.n_subscribers), int(ib.n_deliveries)
_subs = np.ctypeslib.as_array(ib.subscribers, shape=(max(_r, 1),))[:_r]
_offs = np.ctypeslib.as_array(ib.inbox_offsets, shape=(_r + 1,)).astype(np.int64)
_pubs = np.ctypeslib.as_array(ib.publishes, shape=(max(_d, 1),))[:_d]
_fids = np.ctypeslib.as_array(ib.filter_ids, shape=(max(_d, 1),))[:_d]
_key = np.repeat(_subs, np.diff(_offs))
_nl = (tval[np.searchsorted(tkey, _key.astype(np.uint64) << np.uint64(32) | _fids)] & 4) != 0
_cand = np.flatnonzero(_nl)
_pick = rng.choice(_cand, min(len(_cand), n // 8), replace=False) if len(_cand) else _cand
from_[_pubs[_pick]] = _key[_pick]
n_own_pub = int(len(np.unique(_pubs[_pick])))
del _subs, _offs, _pubs, _fids, _key, _nl, _cand, _pick


def view(ptr, cnt):
    return np.ctypeslib.as_array(ptr, shape=(max(cnt, 1),))[:cnt]


def run_new(with_from=True):
    do.from_ = from_.ctypes.data if with_from else None
    do.msg = msg.ctypes.data
    do.flags = N.TM_DELIVER_SUBIDS
    t = time.perf_counter()
    N.check(L.tm_batch_deliver(eng.h, b.h, C.byref(do), C.byref(si)), "tm_batch_deliver")
    ms = 1e3 * (time.perf_counter() - t)
    r, d = int(si.n_subscribers), int(si.n_deliveries)
    return ms, float(si.kernel_ms), (view(si.subscribers, r), view(si.inbox_offsets, r + 1), view(si.publishes, d),
                                     view(si.filter_ids, d), view(si.msg, d), view(si.subids, d))


def run_host(with_from=True):
    """The inboxes over PCIe, then ignore_local and enrich_subopts in NumPy."""
    t = time.perf_counter()
    N.check(L.tm_batch_inboxes(eng.h, b.h, 0, C.byref(ib)), "tm_batch_inboxes")
    r, d = int(ib.n_subscribers), int(ib.n_deliveries)
    subs, offs = view(ib.subscribers, r), view(ib.inbox_offsets, r + 1).astype(np.int64)
    pubs, fids = view(ib.publishes, d), view(ib.filter_ids, d)
    key = np.repeat(subs, np.diff(offs))
    v = tval[np.searchsorted(tkey, key.astype(np.uint64) << np.uint64(32) | fids)]
    pm = msg[pubs]
    sq, pq = (v & 3).astype(np.uint8), pm & 3
    retain = ((pm & 4) != 0) & (((v & 8) != 0) | ((pm & 8) != 0))
    nl = (v & 4) != 0
    out = np.minimum(sq, pq) | (retain.astype(np.uint8) << 2) | (nl.astype(np.uint8) << 3)
    if with_from and d:
        fr = from_[pubs]
        own = nl & (fr == key) & (fr != N.TM_NONE)
        q = np.arange(d, dtype=np.int64)
        first = np.minimum.reduceat(np.where(own, d, q), offs[:-1])
        keep = ~own | (q > np.repeat(first, np.diff(offs)))
        left = np.add.reduceat(keep.astype(np.int64), offs[:-1])
        live = left > 0
        res = (subs[live], np.r_[0, np.cumsum(left[live])].astype(np.uint32), pubs[keep], fids[keep], out[keep],
               (v >> 4)[keep])
    else:
        res = (subs, offs.astype(np.uint32), pubs, fids, out, v >> 4)
    ms = 1e3 * (time.perf_counter() - t)
    return ms, float(ib.kernel_ms), res


def stats(x):
    return {"min": round(float(np.min(x)), 3), "median": round(float(np.median(x)), 3),
            "max": round(float(np.max(x)), 3)}


new_ms, new_k, host_ms, inbox_k, fast_k, fast_ms = [], [], [], [], [], []
same = True
for i in range(WARM + reps):
    a, km, got_new = run_new()
    d_left, dropped = int(si.n_deliveries), int(si.n_dropped_no_local)
    got_new = tuple(x.copy() for x in got_new)
    h, ik, want = run_host()
    same = same and d_left + dropped == int(ib.n_deliveries)
    same = same and all(np.array_equal(x, y) for x, y in zip(got_new, want))
    fa, fk, got_fast = run_new(with_from=False)
    got_fast = tuple(x.copy() for x in got_fast)
    _, _, want_fast = run_host(with_from=False)
    same = same and all(np.array_equal(x, y) for x, y in zip(got_fast, want_fast))
    del want, want_fast, got_new, got_fast
    if i >= WARM:
        new_ms.append(a); new_k.append(km); host_ms.append(h); inbox_k.append(ik); fast_k.append(fk); fast_ms.append(fa)
if not same:
    print(json.dumps({"shape": shape, "equal_results_both_routes": False}))
    sys.exit(1)
d = int(ib.n_deliveries)
T, NS = len(tkey), len(np.unique(tkey >> np.uint64(32)))
floor_b = 12 * d + 13 * d_left + 5 * n + 8 * T + 4 * NS
fast_b = 12 * d + 5 * d + n + 8 * T + 4 * NS
floor_ms = floor_b / (HBM_PEAK_GBS * 1e9) * 1e3
fast_floor_ms = fast_b / (HBM_PEAK_GBS * 1e9) * 1e3
entry = {"publishes": n_pub, "filters": len(fl), "subscriptions": T, "subscribers": NS,
         "nl_subscriptions": int(((tval >> 2) & 1).sum()), "publishes_with_from": int((from_ != N.TM_NONE).sum()),
         "publishes_from_an_own_no_local_receiver": n_own_pub,
         "deliveries": d, "deliveries_left": d_left, "dropped_no_local": dropped,
         "reps": reps, "warmup": WARM, "equal_results_both_routes": True,
         "deliver_host_ms": stats(new_ms), "deliver_kernel_ms": stats(new_k), "inboxes_kernel_ms_same_run": stats(inbox_k),
         "inboxes_plus_numpy_host_ms": stats(host_ms),
         "speedup_host_median": round(float(np.median(host_ms) / np.median(new_ms)), 2),
         "byte_floor": {"bytes": floor_b, "formula": "12 D + 13 D' + 5 n + 8 T + 4 NS", "peak_gbs": HBM_PEAK_GBS,
                        "floor_ms": round(floor_ms, 5),
                        "kernel_ms_over_floor": round(float(np.median(new_k)) / floor_ms, 2) if floor_ms else None},
         "no_drop_fast_path": {"host_ms": stats(fast_ms), "kernel_ms": stats(fast_k), "bytes": fast_b,
                               "formula": "12 D + 5 D + n + 8 T + 4 NS", "floor_ms": round(fast_floor_ms, 5),
                               "kernel_ms_over_floor": (round(float(np.median(fast_k)) / fast_floor_ms, 2)
                                                        if fast_floor_ms else None)}}
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
