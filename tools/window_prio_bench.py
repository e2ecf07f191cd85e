"""Timing of tm_batch_window_prio (the send window over mqueues with priority
tables) beside tm_batch_window, on the workloads of tools/window_bench.py.
Dev/measurement tool, no pass/fail on time.

    python tools/window_prio_bench.py SHAPE [publishes] [reps] [warmup] [out.json] [--ab PARENT_LIB]

SHAPE dispatch / c1, the subscriptions, the publishes' options and the session
table are those of tools/window_bench.py (same seeds).  On ONE waited batch,
alternating after the warm-up rounds:
  (a) tm_batch_window
  (b) tm_batch_window_prio with no table (n_tables = 0)
  (c) tm_batch_window_prio with one 3-class table as default_table: 1 % of the
      distinct topics are keys (priority 1 or 2, default lowest), every listed
      session has a prio entry with random plens (their sum is its mqueue_len,
      each at most its mqueue_max); the defaults' queue is empty
For each: wall time, kernel_ms, lookup_kernel_ms.  Before any time is kept, (b)
must equal (a) array for array, and (c) must equal a NumPy route over
tm_batch_deliver's arrays: the class of every publish from a dict, the rank in
(inbox, class) by a stable sort of the entering deliveries, the closed form of
include/emqx_tm.h per class.
(c)'s kernel_ms + lookup_kernel_ms is given over its byte floor, counted as
tools/window_bench.py counts it plus what the classes must move, once:
    4 D' + 24 R' + 24 NS     the window's floor
  + 1 D'                     pclass written
  + 64 R'                    precords written
  + 40 NP                    the uploaded prio entries
  + 1 n + B                  the class of every publish written, its topic bytes read
for n publishes of B bytes and NP prio entries.
--ab PARENT_LIB: tm_batch_window's kernel_ms on the parent commit's library and
on this one, alternating, 7 runs each (a fresh process per run, the median of
`reps` calls); recorded with both spreads (max - min of the 7 medians) and
whether this build's median stays within three of the parent's spreads.
The JSON file keeps one entry per shape.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emqx_amd import _native as N  # noqa: E402

PRIO_SYMS = ("tm_ptable_create", "tm_ptable_free", "tm_ptable_classes", "tm_batch_window_prio")
args = [a for a in sys.argv[1:]]
ab_lib = None
if "--ab" in args:
    i = args.index("--ab")
    ab_lib = os.path.abspath(args[i + 1])
    del args[i:i + 2]
child = "--ab-child" in args
if child:
    args.remove("--ab-child")
    if os.environ.get("EMQX_TM_LIB"):   # the parent's library has no priority tables
        for s in PRIO_SYMS:
            N.SIGNATURES.pop(s, None)
from emqx_amd import gen  # noqa: E402
from emqx_amd.engine import Engine  # noqa: E402

HBM_PEAK_GBS = 8000.0            # bench.py's roofline peak

shape = args[0] if len(args) > 0 else "c1"
n_pub = int(args[1]) if len(args) > 1 else (1_000_000 if shape == "dispatch" else 100_000)
reps = int(args[2]) if len(args) > 2 else 10
WARM = int(args[3]) if len(args) > 3 else 3
out_path = args[4] if len(args) > 4 else os.path.join(ROOT, "profiles", "window", "window_prio_bench.json")

# ---- the workload of tools/window_bench.py
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


def wopts(t, d):
    wo = N.WindowOpts()
    wo.sessions = C.cast(t.ctypes.data, C.POINTER(N.SessionState))
    wo.n_sessions = len(t)
    wo.defaults = N.SessionState(*[int(x) for x in d])
    wo.flags = 0
    return wo


wo_a = wopts(tab, dflt)
sw = N.SessionWindow()
si = N.SessionInboxes()


def view(ptr, cnt):
    return np.ctypeslib.as_array(ptr, shape=(max(cnt, 1),))[:cnt]


def inbox_views(s):
    r, d = int(s.n_subscribers), int(s.n_deliveries)
    return (view(s.subscribers, r), view(s.inbox_offsets, r + 1), view(s.publishes, d), view(s.filter_ids, d),
            view(s.msg, d))


def window_views():
    r, d = int(sw.inboxes.n_subscribers), int(sw.inboxes.n_deliveries)
    rec = np.ctypeslib.as_array(C.cast(sw.records, C.POINTER(C.c_uint32)), shape=(max(r, 1), 4))[:r]
    return inbox_views(sw.inboxes) + (view(sw.disp, d), view(sw.packet_ids, d), rec, np.array(list(sw.totals), np.uint64))


def run_a():
    t = time.perf_counter()
    N.check(L.tm_batch_window(eng.h, b.h, C.byref(do), C.byref(wo_a), C.byref(sw)), "tm_batch_window")
    return 1e3 * (time.perf_counter() - t), float(sw.kernel_ms), 0.0, window_views()


def stats(x):
    return {"min": round(float(np.min(x)), 3), "median": round(float(np.median(x)), 3),
            "max": round(float(np.max(x)), 3)}


if child:   # one run of the A/B: (a) alone
    ks = []
    for it in range(WARM + reps):
        _, km, _, _ = run_a()
        if it >= WARM:
            ks.append(km)
    print(json.dumps({"ab_child_kernel_ms": float(np.median(ks))}))
    sys.exit(0)

# ---- (b) no table, (c) one 3-class table for everybody
pw = N.WindowPrio()
po_b = N.WindowPrioOpts()
po_b.default_table = N.TM_NONE
tl = topics.tolist()
uniq = sorted(set(tl))
keys = [uniq[i] for i in rng.choice(len(uniq), max(len(uniq) // 100, 1), replace=False)]
entries = {t: int(rng.integers(1, 3)) for t in keys}
ptab = eng.ptable(entries, "lowest")
assert ptab.classes == [2, 1, 0]
cls_of = {t: 2 - pr for t, pr in entries.items()}
cls_pub = np.fromiter((cls_of.get(t, 2) for t in tl), np.uint8, n)
tab_c = tab.copy()
Mx = tab[:, 5].astype(np.int64)
cap = np.where(Mx > 0, Mx, 20)
plen = np.zeros((NS, 8), np.uint32)
plen[:, :3] = (rng.random((NS, 3)) * (cap[:, None] + 1)).astype(np.uint32)
tab_c[:, 4] = plen.sum(1)
dflt_c = dflt.copy()
dflt_c[4] = 0
prio = np.zeros((NS, 10), np.uint32)
prio[:, 0], prio[:, 1], prio[:, 2:] = ids, 0, plen
tables = (C.c_void_p * 1)(ptab.h.value)
po_c = N.WindowPrioOpts()
po_c.tables, po_c.n_tables = C.cast(tables, C.POINTER(C.c_void_p)), 1
po_c.prio, po_c.n_prio = C.cast(prio.ctypes.data, C.POINTER(N.SessionPrio)), NS
po_c.default_table = 0
wo_c = wopts(tab_c, dflt_c)


def run_prio(wo, po):
    t = time.perf_counter()
    N.check(L.tm_batch_window_prio(eng.h, b.h, C.byref(do), C.byref(wo), C.byref(po), C.byref(sw), C.byref(pw)),
            "tm_batch_window_prio")
    ms = 1e3 * (time.perf_counter() - t)
    r, d = int(sw.inboxes.n_subscribers), int(sw.inboxes.n_deliveries)
    prec = np.ctypeslib.as_array(C.cast(pw.precords, C.POINTER(C.c_uint32)), shape=(max(r, 1), 8, 2))[:r]
    return ms, float(sw.kernel_ms), float(pw.lookup_kernel_ms), window_views() + (view(pw.pclass, d), prec)


def numpy_window_prio(subs, offs, pubs, dm):
    """(c) from deliver's arrays: np.searchsorted for the session and the prio
    entry of every inbox, the counted rank by one cumulative sum, the rank in
    (inbox, class) by a stable sort of the entering deliveries, then the
    per-class closed form."""
    r, d = len(subs), len(dm)
    i = np.minimum(np.searchsorted(tab_c[:, 0], subs), NS - 1)
    listed = tab_c[i, 0] == subs
    st = np.where(listed[:, None], tab_c[i], dflt_c[None, :])
    Lc = np.where(listed[:, None], plen[i], 0).astype(np.int64)
    P, flg, F, M = st[:, 1].astype(np.int64), st[:, 2], st[:, 3].astype(np.int64), st[:, 5].astype(np.int64)
    host, dsc = (flg & N.TM_SESS_HOST) != 0, (flg & N.TM_SESS_DISCONNECTED) != 0
    store = dsc & ((flg & N.TM_SESS_STORE_QOS0) != 0)
    o64 = offs.astype(np.int64)
    lens = np.diff(o64)
    ri = np.repeat(np.arange(r), lens)
    counted = ~host[ri] & (((dm & 3) > 0) | store[ri])
    cs = np.cumsum(counted) - counted
    rank = cs - np.repeat(cs[o64[:-1]], lens)
    tot = np.add.reduceat(counted.astype(np.int64), o64[:-1])
    nsend = np.where(dsc, 0, np.minimum(F, tot))
    cls = cls_pub[pubs].astype(np.int64)
    ent = counted & (rank >= nsend[ri])
    idx = np.flatnonzero(ent)
    key = ri[idx] * 8 + cls[idx]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    first = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]]) if len(ks) else np.zeros(0, np.int64)
    run = np.arange(len(ks)) - np.repeat(first, np.diff(np.r_[first, len(ks)]))
    crank = np.zeros(d, np.int64)
    crank[idx[order]] = run
    E = np.bincount(key, minlength=r * 8).reshape(r, 8)
    drops = np.where(M[:, None] > 0, np.maximum(0, Lc + E - M[:, None]), 0)
    old = np.minimum(drops, Lc)
    dnew = drops - old
    disp = np.where(rank < nsend[ri], 1, np.where(crank < dnew[ri, cls], 4, 2))
    disp = np.where(counted, disp, np.where(dsc[ri], 3, 0))
    disp = np.where(host[ri], 5, disp).astype(np.uint8)
    pid = np.where(disp == 1, (P[ri] - 1 + rank) % 65535 + 1, 0).astype(np.uint16)
    prec = np.stack([E - dnew, old], 2).astype(np.uint32)
    rec = np.stack([np.where(host, P, (P - 1 + nsend) % 65535 + 1), np.where(host, 0, nsend),
                    (E - dnew).sum(1), old.sum(1)], 1).astype(np.uint32)
    pclass = np.where(host[ri], N.TM_PRIO_NOCLASS, cls).astype(np.uint8)
    return disp, pid, rec, np.bincount(disp, minlength=N.TM_DISP_COUNT).astype(np.uint64), pclass, prec


def run_host():
    N.check(L.tm_batch_deliver(eng.h, b.h, C.byref(do), C.byref(si)), "tm_batch_deliver")
    subs, offs, pubs, fids, dm = inbox_views(si)
    return (subs, offs, pubs, fids, dm) + numpy_window_prio(subs, offs, pubs, dm)


T = {k_: {"ms": [], "kernel": [], "lookup": []} for k_ in "abc"}
same = True
for it in range(WARM + reps):
    res = {}
    for name, fn in (("a", run_a), ("b", lambda: run_prio(wo_a, po_b)), ("c", lambda: run_prio(wo_c, po_c))):
        ms, km, lk, got = fn()
        res[name] = tuple(x.copy() for x in got)
        if it >= WARM:
            T[name]["ms"].append(ms); T[name]["kernel"].append(km); T[name]["lookup"].append(lk)
    if it == 0 or it == WARM + reps - 1:   # the NumPy route is slow: first and last round
        want = run_host()
        same = same and all(np.array_equal(x, y) for x, y in zip(res["c"], want))
    same = same and all(np.array_equal(x, y) for x, y in zip(res["b"][:9], res["a"]))
    same = same and bool((res["b"][9] == N.TM_PRIO_NOCLASS).all()) and not res["b"][10].any()
    d_left, r_left = len(res["c"][4]), len(res["c"][0])
    totals_c = [int(x) for x in res["c"][8]]
    classes_c = np.bincount(res["c"][9], minlength=256)[[0, 1, 2, 255]].tolist()
    del res
if not same:
    print(json.dumps({"shape": shape, "equal_results": False}))
    sys.exit(1)
nbytes = int(topics.offs[-1] - topics.offs[0])
floor_a = 4 * d_left + 24 * r_left + 24 * NS
floor_c = floor_a + d_left + 64 * r_left + 40 * NS + n + nbytes
to_ms = lambda by: by / (HBM_PEAK_GBS * 1e9) * 1e3  # noqa: E731
kc = float(np.median(np.array(T["c"]["kernel"]) + np.array(T["c"]["lookup"])))
ka = float(np.median(T["a"]["kernel"]))
entry = {"publishes": n_pub, "topic_bytes": nbytes, "sessions": NS, "prio_entries": NS, "table_keys": len(entries),
         "deliveries_left": d_left, "inboxes": r_left, "reps": reps, "warmup": WARM, "equal_results": True,
         "totals_c": dict(zip(["send0", "send", "queued", "drop_qos0", "drop_full", "host"], totals_c)),
         "pclass_c": dict(zip(["class0", "class1", "class2", "noclass"], classes_c))}
for name, label in (("a", "a_window"), ("b", "b_prio_no_table"), ("c", "c_prio_one_table")):
    entry[label] = {"host_ms": stats(T[name]["ms"]), "kernel_ms": stats(T[name]["kernel"]),
                    "lookup_kernel_ms": stats(T[name]["lookup"])}
entry["c_over_a_kernel_median"] = round(kc / ka, 2) if ka else None
entry["b_over_a_kernel_median"] = round(float(np.median(T["b"]["kernel"])) / ka, 3) if ka else None
entry["byte_floor_c"] = {"bytes": floor_c, "formula": "4 D' + 24 R' + 24 NS + D' + 64 R' + 40 NP + n + B",
                         "peak_gbs": HBM_PEAK_GBS, "floor_ms": round(to_ms(floor_c), 5),
                         "kernel_plus_lookup_ms_over_floor": round(kc / to_ms(floor_c), 2)}
if ab_lib:
    def one(libpath):
        env = dict(os.environ)
        env.pop("EMQX_TM_LIB", None)
        if libpath:
            env["EMQX_TM_LIB"] = libpath
        out = subprocess.run([sys.executable, os.path.abspath(__file__), shape, str(n_pub), str(reps), str(WARM), "--ab-child"],
                             env=env, check=True, capture_output=True, text=True).stdout
        return json.loads(out.strip().splitlines()[-1])["ab_child_kernel_ms"]
    ptab.free()
    b.free()
    eng.close()
    par, new = [], []
    for k in range(7):
        par.append(one(ab_lib))
        new.append(one(None))
        print(f"A/B run {k + 1}/7: parent {par[-1]:.4f} ms, change {new[-1]:.4f} ms", file=sys.stderr, flush=True)
    sp, sn = max(par) - min(par), max(new) - min(new)
    entry["ab_window_kernel_ms"] = {"runs": 7, "parent": [round(x, 4) for x in par], "change": [round(x, 4) for x in new],
                                    "parent_median": round(float(np.median(par)), 4),
                                    "change_median": round(float(np.median(new)), 4),
                                    "parent_spread": round(sp, 4), "change_spread": round(sn, 4),
                                    "change_within_3_parent_spreads": bool(np.median(new) <= np.median(par) + 3 * sp)}
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
