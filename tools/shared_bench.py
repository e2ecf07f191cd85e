"""Timing of the shared-subscription dispatch (tm_batch_dispatch_shared) against
what a caller could do before it for the same deliveries: tm_batch_routes ->
route CSR over PCIe -> a vectorised numpy pick over the group dests on the
host.  Dev/measurement tool, no pass/fail on time.

    python tools/shared_bench.py [publishes] [filters] [share] [reps] [out.json]

Workload: C1-style filters, every one with a node() route; `share` (0.2) of
them also carry 1-4 groups of 2-64 members.  `publishes` (100,000) publishes,
hash strategy with random keys.  Both routes start from the same waited batch
(the match is common to both and not timed) and run alternating after 3
warm-up rounds; their deliveries (row offsets, filter ids, groups,
subscribers) must be equal before any time is printed.
Host-to-host = wall time of the C call (+ the numpy pick for the old route);
kernel = HIP events around the count, scan and pick kernels
(tm_shared_deliveries.kernel_ms).  tm_batch_routes records no events of its
own: its kernel time is not reported here.
"""
import ctypes as C
import json
import os
import random
import sys
import time
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emqx_amd import _native as N  # noqa: E402
from emqx_amd import gen  # noqa: E402
from emqx_amd.engine import Engine  # noqa: E402

n_pub = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
n_filters = int(sys.argv[2]) if len(sys.argv) > 2 else gen.C1.n_filters
share = float(sys.argv[3]) if len(sys.argv) > 3 else 0.2
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 10
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "shared", "shared_bench.json")
WARM = 3
NODE_DEST, GROUP0 = 0, 1          # dest ids: node(), then the groups

rng = random.Random(5)
p = replace(gen.C1, n_filters=n_filters)
F = gen.gen_filters(p)
flist = sorted(set(F.tolist()))
topics = gen.gen_topics(p, F, 9, n_pub)
eng = Engine(device=0)
L = eng.L

n_groups = 64
runs = {}                         # (filter, group dest) -> members, in the engine's order
sub = 0
for f in flist:
    eng.route_add(f, NODE_DEST)
    if rng.random() < share:
        for g in rng.sample(range(n_groups), rng.randint(1, 4)):
            mem = runs[(f, GROUP0 + g)] = []
            for _ in range(rng.randint(2, 64)):
                eng.shared_subscribe(f, GROUP0 + g, sub)
                mem.append(sub)
                sub += 1

# the host's member table for the old route: runs sorted by (filter id << 32 | group dest)
items = sorted(((eng.filter_id(f) << 32) | g, m) for (f, g), m in runs.items())
rkey = np.array([k for k, _ in items], np.uint64)
rlen = np.array([len(m) for _, m in items], np.uint32)
rbase = np.concatenate(([0], np.cumsum(rlen)[:-1])).astype(np.int64)
rmem = np.concatenate([np.array(m, np.uint32) for _, m in items])

keys = np.random.default_rng(7).integers(0, 1 << 32, n_pub, dtype=np.uint64).astype(np.uint32)
b = eng.prepare(topics).launch().wait()
opts = N.SharedOpts(N.TM_SHARED_HASH, 0, keys.ctypes.data, 0)
d = N.SharedDeliveries()
r = N.Routes()


def run_new():
    t = time.perf_counter()
    N.check(L.tm_batch_dispatch_shared(eng.h, b.h, C.byref(opts), C.byref(d)), "tm_batch_dispatch_shared")
    ms = 1e3 * (time.perf_counter() - t)
    n, m = d.n_topics, int(d.n_deliveries)
    view = lambda ptr, k: np.ctypeslib.as_array(ptr, shape=(max(k, 1),))[:k]  # noqa: E731
    return ms, float(d.kernel_ms), (view(d.row_offsets, n + 1), view(d.filter_ids, m), view(d.groups, m),
                                    view(d.subscribers, m))


def run_old():
    """tm_batch_routes + the pick a caller had to do on the host."""
    t = time.perf_counter()
    N.check(L.tm_batch_routes(eng.h, b.h, C.byref(r)), "tm_batch_routes")
    n, m = r.n_topics, int(r.n_routes)
    roff = np.ctypeslib.as_array(r.row_offsets, shape=(n + 1,))
    fid = np.ctypeslib.as_array(r.filter_ids, shape=(max(m, 1),))[:m]
    dest = np.ctypeslib.as_array(r.dests, shape=(max(m, 1),))[:m]
    grp = np.flatnonzero(dest != NODE_DEST)                       # the {To, Group} routes
    k = (fid[grp].astype(np.uint64) << np.uint64(32)) | dest[grp].astype(np.uint64)
    run = np.searchsorted(rkey, k)
    pub = np.searchsorted(roff, grp, side="right") - 1             # the publish of every group route
    cnt = rlen[run]
    nth = np.where(cnt > 1, keys[pub] % np.maximum(cnt, 1), 0)
    subs = rmem[rbase[run] + nth]
    offs = np.searchsorted(grp, roff).astype(np.uint32)            # group routes before each row
    ms = 1e3 * (time.perf_counter() - t)
    return ms, (offs, fid[grp], dest[grp], subs)


def stats(v):
    return {"min": round(float(np.min(v)), 3), "median": round(float(np.median(v)), 3),
            "max": round(float(np.max(v)), 3)}


new_ms, new_k, old_ms = [], [], []
same = True
for i in range(WARM + reps):
    a, k, got = run_new()
    o, want = run_old()
    same = same and all(np.array_equal(x, y) for x, y in zip(got, want))
    if i >= WARM:
        new_ms.append(a); new_k.append(k); old_ms.append(o)
if not same:
    print(json.dumps({"equal_deliveries_both_routes": False}))
    sys.exit(1)
st = b.stats()
out = {"publishes": n_pub, "filters": len(flist), "share_with_groups": share, "group_runs": len(runs),
       "members": int(sub), "matches": int(st["matches"]), "routes": int(r.n_routes),
       "shared_deliveries": int(d.n_deliveries), "strategy": "hash", "reps": reps, "warmup": WARM,
       "equal_deliveries_both_routes": True,
       "dispatch_shared_host_ms": stats(new_ms), "dispatch_shared_kernel_ms": stats(new_k),
       "routes_plus_numpy_pick_host_ms": stats(old_ms),
       "speedup_host_median": round(float(np.median(old_ms) / np.median(new_ms)), 2)}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(json.dumps(out) + "\n")
print(json.dumps(out))
