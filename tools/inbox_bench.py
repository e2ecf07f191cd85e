"""Timing of the per-subscriber inboxes (tm_batch_inboxes) against what a caller
had to do before it for the same result: tm_batch_dispatch to the host, then a
stable sort by subscriber and the gathers in numpy.  Dev/measurement tool, no
pass/fail on time.

    python tools/inbox_bench.py SHAPE [publishes] [reps] [warmup] [out.json] [ref_binary]

SHAPE dispatch: the workload of `bench.py --workload dispatch` (C2 trie, every
filter with local subscribers: 75% one, 24% 2-8, 64 hot filters with 4096,
ids from a pool of 1M; 10,000,000 publishes).  SHAPE c1: the C1 filters with
the same subscriber rule, 100,000 publishes.
Both routes start from the same waited batch (the match is common to both and
not timed) and run alternating after the warm-up rounds; their results
(subscribers, inbox offsets, publishes, filter ids) must be equal before any
time is printed.
  old route  tm_batch_result + tm_batch_dispatch (match offsets) to the host,
             np.argsort(subscribers, kind="stable"), the gathers; wall time
  new route  tm_batch_inboxes host-to-host, wall time, and its kernel_ms (HIP
             events around the inbox kernels, the fan-out before them excluded)
kernel_ms is also given as a fraction of its byte floor at the bandwidth
bench.py's roofline uses: 16 B per pass (the pairs read and written) plus the
finish's 20 B, per delivery (the per-pass histogram's 4-B re-read of the keys
is the implementation's, not the floor's).
ref_binary: tools/inbox_sort_ref.hip built; run as a child process for the
hipcub yardstick (recorded, not a gate).  The JSON file keeps one entry per
shape.
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
from emqx_amd import gen  # noqa: E402
from emqx_amd.engine import Engine  # noqa: E402

HBM_PEAK_GBS = 8000.0            # bench.py's roofline peak

shape = sys.argv[1] if len(sys.argv) > 1 else "c1"
n_pub = int(sys.argv[2]) if len(sys.argv) > 2 else (10_000_000 if shape == "dispatch" else 100_000)
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
WARM = int(sys.argv[4]) if len(sys.argv) > 4 else 3
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "inbox", "inbox_bench.json")
ref_bin = sys.argv[6] if len(sys.argv) > 6 else None

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
pool = rng.integers(0, 1_000_000, int(nsub.sum()), dtype=np.uint32)
k = 0
for f, c in zip(fl, nsub.tolist()):
    for s in pool[k:k + c].tolist():
        eng.subscribe(f, s)
    k += c
eng.sync()
b = eng.prepare(topics).launch().wait()
ib = N.Inboxes()
dl = N.Deliveries()
res = N.Result()


def view(ptr, n):
    return np.ctypeslib.as_array(ptr, shape=(max(n, 1),))[:n]


def run_new():
    t = time.perf_counter()
    N.check(L.tm_batch_inboxes(eng.h, b.h, 0, C.byref(ib)), "tm_batch_inboxes")
    ms = 1e3 * (time.perf_counter() - t)
    r, d = int(ib.n_subscribers), int(ib.n_deliveries)
    return ms, float(ib.kernel_ms), (view(ib.subscribers, r), view(ib.inbox_offsets, r + 1), view(ib.publishes, d),
                                     view(ib.filter_ids, d))


def run_old():
    """The publish-major CSR over PCIe, then the transpose on the host."""
    t = time.perf_counter()
    N.check(L.tm_batch_result(eng.h, b.h, C.byref(res)), "tm_batch_result")
    N.check(L.tm_batch_dispatch(eng.h, b.h, N.TM_DISPATCH_MATCH_OFFSETS, C.byref(dl)), "tm_batch_dispatch")
    n, m, d = dl.n_topics, int(dl.n_matches), int(dl.n_deliveries)
    roff = view(res.row_offsets, n + 1)
    ids = view(res.filter_ids, m)
    moff = view(dl.match_offsets, m + 1)
    subs = view(dl.subscribers, d)
    order = np.argsort(subs, kind="stable")
    key = subs[order]
    entry = np.repeat(np.arange(m, dtype=np.uint32), np.diff(moff).astype(np.int64))[order]
    pub_of = np.repeat(np.arange(n, dtype=np.uint32), np.diff(roff).astype(np.int64))
    heads = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1]))) if d else np.zeros(0, np.int64)
    out = (key[heads], np.concatenate((heads, [d])).astype(np.uint32), pub_of[entry], ids[entry])
    ms = 1e3 * (time.perf_counter() - t)
    return ms, out


def stats(v):
    return {"min": round(float(np.min(v)), 3), "median": round(float(np.median(v)), 3),
            "max": round(float(np.max(v)), 3)}


new_ms, new_k, old_ms = [], [], []
same = True
for i in range(WARM + reps):
    a, km, got = run_new()
    o, want = run_old()
    same = same and all(np.array_equal(x, y) for x, y in zip(got, want))
    del want
    if i >= WARM:
        new_ms.append(a); new_k.append(km); old_ms.append(o)
if not same:
    print(json.dumps({"shape": shape, "equal_results_both_routes": False}))
    sys.exit(1)
d, passes = int(ib.n_deliveries), int(ib.passes)
floor_ms = (passes * 16 + 20) * d / (HBM_PEAK_GBS * 1e9) * 1e3
entry = {"publishes": n_pub, "filters": len(fl), "subscriptions": int(k), "matches": int(b.stats()["matches"]),
         "deliveries": d, "subscribers_with_deliveries": int(ib.n_subscribers), "passes": passes,
         "reps": reps, "warmup": WARM, "equal_results_both_routes": True,
         "inboxes_host_ms": stats(new_ms), "inboxes_kernel_ms": stats(new_k),
         "dispatch_plus_numpy_stable_sort_host_ms": stats(old_ms),
         "speedup_host_median": round(float(np.median(old_ms) / np.median(new_ms)), 2),
         "byte_floor": {"bytes_per_delivery": passes * 16 + 20, "peak_gbs": HBM_PEAK_GBS, "floor_ms": round(floor_ms, 4),
                        "kernel_ms_over_floor": round(float(np.median(new_k)) / floor_ms, 2) if floor_ms else None}}
if ref_bin and d:
    r = subprocess.run([ref_bin, str(d), str(int(pool.max())), "10"], capture_output=True, text=True, timeout=300)
    entry["hipcub_yardstick"] = json.loads(r.stdout) if r.returncode == 0 else {"error": r.stderr[-300:]}
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
