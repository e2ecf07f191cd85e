"""Timing of the batched ACL check (tm_acl_check) against what the engine offered
before it for the same decision: tm_rules_match(dollar_rule = 0) -> n x r
bitmap over PCIe -> first-set-bit fold on the host (numpy).  Dev/measurement
tool, no pass/fail on time.

    python tools/acl_bench.py [names] [rules] [reps]

Case A: `names` (100,000) x `rules` (64) pattern-free rules, who = all --
        both routes in one run, alternating, after 3 warm-up rounds; their
        deciding rule indices must be equal.  Run twice: on the generated
        list (a bare '#' near its head decides most names after a few rules)
        and with the catch-alls made literal (every rule is walked).
Case B: acl_check alone on the second list with every second filter
        patterned (a %c level).
Host-to-host = wall time of the C call (+ the fold for the old route) on
pre-packed arrays; kernel = HIP events around tm_acl_check's kernel
(tm_acl_kernel_ms).  tm_rules_match records no events of its own: its kernel
time is not reported here (rocprofv3 --kernel-trace, in a run of its own).
"""
import ctypes as C
import json
import os
import sys
import time
from dataclasses import replace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emqx_amd import _native as N  # noqa: E402
from emqx_amd import acl as A  # noqa: E402
from emqx_amd import emqx_access_rule as R  # noqa: E402
from emqx_amd import gen  # noqa: E402
from emqx_amd.engine import Engine  # noqa: E402

n_names = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
n_rules = int(sys.argv[2]) if len(sys.argv) > 2 else 64
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
WARM = 3

names = gen.gen_topics(gen.C2, gen.gen_filters(gen.C2), 9, n_names).tolist()
filters = gen.gen_filters(replace(gen.C2, n_filters=n_rules, seed=3)).tolist()
eng = Engine(device=0)
L = eng.L

n_clients = 1024
clients = [{"clientid": b"dev%d" % i, "username": b"u%d" % (i % 50), "peerhost": "10.0.%d.%d" % (i // 256, i % 256)}
           for i in range(n_clients)]
cs, keep_c = A.encode_clients(clients)
requests = [(i % n_clients, "publish", t) for i, t in enumerate(names)]
buf, offs, cof, acc = A.encode_requests(requests)
verdict = np.zeros(n_names, np.uint8)
rule = np.zeros(n_names, np.uint32)


def run_acl(acl):
    t = time.perf_counter()
    N.check(L.tm_acl_check(eng.h, acl.h, C.byref(cs), buf.ctypes.data, offs.ctypes.data, cof.ctypes.data,
                           acc.ctypes.data, n_names, verdict.ctypes.data, rule.ctypes.data), "tm_acl_check")
    return 1e3 * (time.perf_counter() - t), acl.kernel_ms


wpr = (n_rules + 31) // 32
bits = np.zeros(n_names * wpr, np.uint32)
old_rule = np.zeros(n_names, np.uint32)


def run_old(rb, ro):
    """rules_match + the fold a caller had to do: first set bit per row."""
    t = time.perf_counter()
    N.check(L.tm_rules_match(eng.h, buf.ctypes.data, offs.ctypes.data, n_names, rb.ctypes.data, ro.ctypes.data,
                             n_rules, 0, bits.ctypes.data), "tm_rules_match")
    b = np.unpackbits(bits.view(np.uint8).reshape(n_names, wpr * 4), axis=1, bitorder="little")[:, :n_rules]
    hit = b.any(axis=1)
    old_rule[:] = np.where(hit, b.argmax(axis=1), N.TM_NONE)
    return 1e3 * (time.perf_counter() - t)


def stats(v):
    return {"min": round(float(np.min(v)), 3), "median": round(float(np.median(v)), 3),
            "max": round(float(np.max(v)), 3)}


def compare(flts):
    """Both routes on one pattern-free rule list, alternating; the deciding rule indices must agree
    (the old kernel takes a last '#' before an equal word -- name '#/a' against '#' -- but publish
    names hold no '#')."""
    rs = gen.Strings.from_list(flts)
    rb, ro = np.ascontiguousarray(rs.buf), np.ascontiguousarray(rs.offs, dtype=np.uint64)
    acl = eng.acl_create([("allow" if j % 2 else "deny", R.ALL, "pubsub", [f]) for j, f in enumerate(flts)])
    new_ms, new_k, old_ms = [], [], []
    for i in range(WARM + reps):
        a, k = run_acl(acl)
        o = run_old(rb, ro)
        if i >= WARM:
            new_ms.append(a); new_k.append(k); old_ms.append(o)
    decided = rule != N.TM_NONE
    return {"decided": int(decided.sum()),
            "mean_rules_walked": round(float(np.where(decided, rule.astype(np.int64) + 1, n_rules).mean()), 2),
            "same_rule_index_both_routes": bool(np.array_equal(rule, old_rule)),
            "acl_check_host_ms": stats(new_ms), "acl_check_kernel_ms": stats(new_k),
            "rules_match_plus_fold_host_ms": stats(old_ms),
            "speedup_host_median": round(float(np.median(old_ms) / np.median(new_ms)), 2)}


# case A: pattern-free, who = all, as generated (a bare '#' among the first rules decides most names early),
# and the same list with the bare '#' rules made literal, so that nearly every name walks all the rules
out = {"names": n_names, "rules": n_rules, "reps": reps, "warmup": WARM, "A_pattern_free": compare(filters)}
no_catch_all = [b"none/" + f if f in (b"#", b"+/#") else f for f in filters]
out["A_no_catch_all"] = compare(no_catch_all)
same = out["A_pattern_free"]["same_rule_index_both_routes"] and out["A_no_catch_all"]["same_rule_index_both_routes"]

# case B: half of the filters patterned
pat = []
for j, f in enumerate(no_catch_all):
    ws = f.split(b"/")
    if j % 2 and len(ws) > 1:
        ws[1] = b"%c"
    pat.append(("allow" if j % 2 else "deny", R.ALL, "pubsub", [b"/".join(ws)]))
acl_b = eng.acl_create(pat)
b_ms, b_k = [], []
for i in range(WARM + reps):
    a, k = run_acl(acl_b)
    if i >= WARM:
        b_ms.append(a); b_k.append(k)
out["B_half_patterned"] = {"decided": int((rule != N.TM_NONE).sum()), "acl_check_host_ms": stats(b_ms),
                           "acl_check_kernel_ms": stats(b_k)}
print(json.dumps(out))
sys.exit(0 if same else 1)
