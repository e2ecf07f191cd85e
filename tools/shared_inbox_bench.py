"""Timing of the inboxes of an armed batch (tm_batch_shared_mode) beside the
unarmed ones of the same batch.  Dev/measurement tool, no pass/fail on time.

    python tools/shared_inbox_bench.py SHAPE [publishes] [reps] [warmup] [out.json]

SHAPE dispatch: the workload of `bench.py --workload dispatch` (C2 trie, every
filter with local subscribers: 75% one, 24% 2-8, 64 hot filters with 4096, ids
from a pool of 1M; 10,000,000 publishes) with one group of three members added
on every tenth filter.  SHAPE c1: the C1 filters with the same rules, 100,000
publishes.  Strategy random (no key upload), results kept in HBM
(TM_INBOX_DEVICE); the calls alternate after the warm-up rounds.
kernel_ms is tm_inboxes.kernel_ms: HIP events around the inbox kernels, on an
armed batch the merge kernel included, the fan-out and the pick before them
excluded.  The merge kernel's own device time is not in the ABI: run the tool
under `rocprofv3 --kernel-trace --stats` and read tm_inbox_merge's row.
The merge's byte floor, per delivery of L': 8 B read (subscriber and match
entry; a pick reads its group as well) and 24 B written (key, payload and the
16-B record the finish reads back) = 32 B at the bandwidth bench.py's roofline
uses; the per-entry values it gathers (offsets, publish, filter id: read by
neighbouring deliveries) are the implementation's, not the floor's.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emqx_amd import _native as N  # noqa: E402
from emqx_amd import gen  # noqa: E402
from emqx_amd.engine import Engine  # noqa: E402

HBM_PEAK_GBS = 8000.0            # bench.py's roofline peak
GROUP = 2_000_000                # the group's dest id (subscriber ids come from a pool of 1M)

shape = sys.argv[1] if len(sys.argv) > 1 else "c1"
n_pub = int(sys.argv[2]) if len(sys.argv) > 2 else (10_000_000 if shape == "dispatch" else 100_000)
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
WARM = int(sys.argv[4]) if len(sys.argv) > 4 else 3
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "shared_inbox", "shared_inbox_bench.json")

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
members = rng.integers(0, 1_000_000, (len(fl) // 10 + 1, 3), dtype=np.uint32)
for i, f in enumerate(fl[::10]):
    for s in members[i].tolist():
        eng.shared_subscribe(f, GROUP, s)
eng.sync()
b = eng.prepare(topics).launch().wait()
ib = N.Inboxes()


def run(armed: bool):
    if armed:
        b.shared_mode("random", seed=7)
    else:
        b.shared_mode(None)
    N.check(L.tm_batch_inboxes(eng.h, b.h, N.TM_INBOX_DEVICE, C.byref(ib)), "tm_batch_inboxes")
    return float(ib.kernel_ms), int(ib.n_deliveries), int(ib.n_subscribers), int(ib.passes)


def stats(v):
    return {"min": round(float(np.min(v)), 3), "median": round(float(np.median(v)), 3),
            "max": round(float(np.max(v)), 3)}


total, shared_ms = b.dispatch_shared_device("random", seed=7)[:2]
plain_k, armed_k = [], []
for i in range(WARM + reps):
    pk, d0, r0, passes = run(False)
    ak, d1, r1, _ = run(True)
    if d1 != d0 + total:
        print(json.dumps({"shape": shape, "error": f"{d1} deliveries armed, {d0} + {total} expected"}))
        sys.exit(1)
    if i >= WARM:
        plain_k.append(pk)
        armed_k.append(ak)
floor_ms = 32 * d1 / (HBM_PEAK_GBS * 1e9) * 1e3
entry = {"publishes": n_pub, "filters": len(fl), "subscriptions": int(k), "filters_with_a_group": len(fl[::10]),
         "matches": int(b.stats()["matches"]), "deliveries": d0, "shared_deliveries": int(total),
         "subscribers_with_deliveries": {"unarmed": r0, "armed": r1}, "passes": passes, "reps": reps, "warmup": WARM,
         "pick_kernel_ms": round(shared_ms, 3),
         "inboxes_kernel_ms": {"unarmed": stats(plain_k), "armed": stats(armed_k)},
         "merge_byte_floor": {"bytes_per_delivery": 32, "peak_gbs": HBM_PEAK_GBS, "floor_ms": round(floor_ms, 4)}}
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
