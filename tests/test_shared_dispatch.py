"""Shared-subscription dispatch without a device: the emqx_shared_sub mirror
against tests/golden/kat_shared_sub.json, the membership C ABI on a host-only
engine against the mirror, ABI validation, struct layouts, NIF term shapes and
the random strategy's uniformity (src/emqx_shared_sub.erl:229-315, 358-367)."""

import ctypes as C
import os
import random
import shutil
import subprocess
from collections import Counter

import pytest
import shared_cases as K

from emqx_amd import _native as N
from emqx_amd import emqx_broker as B
from emqx_amd import emqx_router as R
from emqx_amd import emqx_shared_sub as S
from emqx_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the random strategy's share of one member of a group of 4 over 40,000
# publishes: 10,000 +- 520 = 6 sigma of Binomial(40,000, 1/4), sigma = 86.6
UNIFORM_N, UNIFORM_TOL, UNIFORM_SEED = 40000, 520, 20240607


@pytest.fixture
def host_router():
    R.use(Engine(device=-1))
    R._routes.clear()
    S.clear()
    yield R.engine()
    R._routes.clear()
    S.clear()
    R._engine = None


@pytest.mark.parametrize("case", K.kat()["cases"], ids=lambda c: c["name"])
def test_mirror_kat(case, host_router):
    K.run_case(case, [S.dispatch_batch_mirror])


def test_kat_covers_what_the_suite_asserts():
    names = " ".join(c["name"] for c in K.kat()["cases"])
    for part in ("suite_round_robin", "suite_hash", "one_member", "route_appears", "3_to_2", "two_groups",
                 "insertion_order"):
        assert part in names, part


def test_pick_clauses(host_router):
    """do_pick/5's three clauses (:246-258) and the retry pick over All."""
    assert S.pick("hash", 3, "g", b"t") is False                       # genuinely no subscriber
    for p in ("p1", "p2", "p3"):
        S.subscribe("g", b"t", p)
    assert S.pick("hash", 4, "g", b"t") == ("fresh", "p2")
    assert S.pick("hash", 4, "g", b"t", ["p2"]) == ("fresh", "p1")       # All -- FailedSubs = [p1, p3]
    assert S.pick("hash", 4, "g", b"t", ["p1", "p2", "p3"]) == ("retry", "p2")   # all failed: pick one anyway
    assert S.pick("hash", 4, "g", b"t", ["p1", "p3"]) == ("fresh", "p2")  # [Sub] -> Sub
    with pytest.raises(NotImplementedError):
        S.pick("sticky", 0, "g", b"t")
    with pytest.raises(ValueError):
        S.pick("fastest", 0, "g", b"t")


def test_membership_abi_random_ops_vs_mirror(host_router):
    """A second host-only engine driven through the C ABI with the ops the
    mirror gets: members, first / last member routes, idempotence, TM_ENOENT
    and member_down counts agree after every op."""
    rng = random.Random(3)
    eng = Engine(device=-1)
    L = eng.L
    topics = [b"a/+", b"a/b", b"#", b"s/+/t", b"$SYS/#", b"x"]
    groups = ["g0", "g1", "g2"]
    for step in range(4000):
        g, t, pid = rng.choice(groups), rng.choice(topics), rng.randrange(12)
        gid, sid = R._agg_id((g, R.NODE)), B._sid(pid)
        r = rng.random()
        if r < 0.5:
            S.subscribe(g, t, pid)
            assert L.tm_shared_subscribe(eng.h, t, len(t), gid, sid) == 0
        elif r < 0.93:
            was = pid in S.subscribers(g, t)
            S.unsubscribe(g, t, pid)
            rc = L.tm_shared_unsubscribe(eng.h, t, len(t), gid, sid)
            assert rc == (0 if was else N.TM_ENOENT), (step, rc, was)
        else:
            assert eng.shared_member_down(sid) == S.member_down(pid), step
        assert [B._terms[s] for s in eng.shared_members(t, gid)] == S.subscribers(g, t), step
        assert eng.stats()["filters"] == host_router.stats()["filters"] == len(R._routes), step
        if step % 97 == 0:
            for tt in topics:
                for gg in groups:
                    got = [B._terms[s] for s in eng.shared_members(tt, R._agg_id((gg, R.NODE)))]
                    assert got == S.subscribers(gg, tt), (step, tt, gg)
    for pid in range(12):
        assert eng.shared_member_down(B._sid(pid)) == S.member_down(pid)
    assert eng.empty() and host_router.empty() and not R._routes
    eng.close()


def test_shared_route_is_counted_once_next_to_the_feed(host_router):
    """The engine adds the group's route itself; a route the table already held
    (the cluster feed wrote it) is not counted twice."""
    R.do_add_route(b"t/+", ("g", R.NODE))
    S.subscribe("g", b"t/+", "p")
    S.unsubscribe("g", b"t/+", "p")                  # the last member deletes the route
    assert host_router.empty() and not R._routes
    S.subscribe("g", b"t/+", "p")
    R.do_add_route(b"t/+", ("g", "other@h"))         # {g, other} aggregates to the same id: a second reference
    S.member_down("p")
    assert host_router.filter_id(b"t/+") >= 0
    R.do_delete_route(b"t/+", ("g", "other@h"))
    assert host_router.empty()


def test_members_buffer_protocol():
    eng = Engine(device=-1)
    for s in range(100):
        eng.shared_subscribe(b"big", 7, 1000 + s)
    n = C.c_uint32()
    buf = (C.c_uint32 * 4)()
    assert eng.L.tm_shared_members(eng.h, b"big", 3, 7, buf, 4, C.byref(n)) == 0
    assert n.value == 100 and list(buf) == [1000, 1001, 1002, 1003]      # cap ids written, the full count reported
    assert eng.L.tm_shared_members(eng.h, b"big", 3, 7, None, 0, C.byref(n)) == 0 and n.value == 100
    assert eng.shared_members(b"big", 7) == list(range(1000, 1100))
    assert eng.shared_members(b"big", 8) == [] and eng.shared_members(b"none", 7) == []
    eng.close()


def _last_error(L) -> str:
    return (L.tm_last_error() or b"").decode()


def test_abi_validation_host_only():
    """Every TM_EINVAL of tm_batch_dispatch_shared that needs no batch, and
    TM_ENODEV (a host-only engine has no batch to wait for: 'batch not waited'
    and the TM_BATCH_DEDUP refusal are in test_gpu_shared_dispatch.py)."""
    eng = Engine(device=-1)
    L = eng.L
    out = N.SharedDeliveries()
    keys = (C.c_uint32 * 1)(0)

    def call(strategy, flags=0, k=None):
        o = N.SharedOpts(strategy, flags, C.cast(k, C.c_void_p) if k is not None else None, 0)
        return L.tm_batch_dispatch_shared(eng.h, None, C.byref(o), C.byref(out))

    assert call(3) == N.TM_EINVAL and "unknown strategy" in _last_error(L)
    assert call(N.TM_SHARED_RANDOM, 4) == N.TM_EINVAL and "unknown flag" in _last_error(L)
    assert call(N.TM_SHARED_HASH) == N.TM_EINVAL and "without keys" in _last_error(L)
    for strategy in (N.TM_SHARED_RANDOM, N.TM_SHARED_ROUND_ROBIN):
        assert call(strategy) == N.TM_ENODEV
    assert call(N.TM_SHARED_HASH, 0, keys) == N.TM_ENODEV
    assert call(N.TM_SHARED_HASH, N.TM_SHARED_COUNT_ONLY) == N.TM_ENODEV      # counts need no keys
    o = N.SharedOpts(0, 0, None, 0)
    assert L.tm_batch_dispatch_shared(eng.h, None, None, C.byref(out)) == N.TM_EINVAL
    assert L.tm_batch_dispatch_shared(eng.h, None, C.byref(o), None) == N.TM_EINVAL
    assert L.tm_batch_dispatch_shared(None, None, C.byref(o), C.byref(out)) == N.TM_EINVAL
    b = eng.prepare([b"a"])                                                # a host-only engine's batch never runs
    for kw in ({"strategy": "hash", "keys": [1]}, {"strategy": "round_robin"}, {"strategy": "random", "seed": 1},
               {"strategy": "hash", "counts_only": True}):
        with pytest.raises(N.TmError) as ei:
            b.dispatch_shared(**kw)
        assert ei.value.rc == N.TM_ENODEV, kw
    with pytest.raises(N.TmError) as ei:
        b.dispatch_shared("hash")
    assert ei.value.rc == N.TM_EINVAL
    with pytest.raises(ValueError):
        b.dispatch_shared("hash", keys=[1, 2])                             # one key per publish
    b.free()
    # the membership calls
    n = C.c_uint32()
    assert L.tm_shared_subscribe(None, b"a", 1, 0, 0) == N.TM_EINVAL
    assert L.tm_shared_subscribe(eng.h, None, 1, 0, 0) == N.TM_EINVAL
    assert L.tm_shared_unsubscribe(eng.h, None, 1, 0, 0) == N.TM_EINVAL
    assert L.tm_shared_unsubscribe(eng.h, b"a", 1, 0, 0) == N.TM_ENOENT
    assert L.tm_shared_member_down(None, 0, None) == N.TM_EINVAL
    assert L.tm_shared_member_down(eng.h, 0, None) == 0                    # n_removed may be NULL
    assert L.tm_shared_members(eng.h, b"a", 1, 0, None, 0, None) == N.TM_EINVAL
    assert L.tm_shared_members(eng.h, b"a", 1, 0, None, 4, C.byref(n)) == N.TM_EINVAL
    assert eng.empty()
    eng.close()


@pytest.mark.skipif(not shutil.which("gcc"), reason="needs gcc")
def test_ctypes_mirrors_match_the_header(tmp_path):
    pairs = [("tm_shared_opts", N.SharedOpts), ("tm_shared_deliveries", N.SharedDeliveries)]
    consts = {"TM_SHARED_RANDOM": N.TM_SHARED_RANDOM, "TM_SHARED_ROUND_ROBIN": N.TM_SHARED_ROUND_ROBIN,
              "TM_SHARED_HASH": N.TM_SHARED_HASH, "TM_SHARED_COUNT_ONLY": N.TM_SHARED_COUNT_ONLY,
              "TM_SHARED_DEVICE": N.TM_SHARED_DEVICE}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "emqx_tm.h"', "int main(void) {"]
    for cname, py in pairs:
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    for c in consts:
        lines.append(f'printf("const {c} %u\\n", (unsigned){c});')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        k1, k2, v = ln.split()
        got[(k1, k2)] = int(v)
    for cname, py in pairs:
        assert got[(cname, "size")] == C.sizeof(py), cname
        for f in py._fields_:
            assert got[(cname, f[0])] == getattr(py, f[0]).offset, (cname, f[0])
    for c, v in consts.items():
        assert got[("const", c)] == v, c
    assert N.SHARED_STRATEGIES == {"random": 0, "round_robin": 1, "hash": 2}


@pytest.fixture(scope="module")
def nif():
    from nif_harness import Nif
    return Nif()


def test_nif_membership_terms(nif):
    for name, arity in [("shared_subscribe", 4), ("shared_unsubscribe", 4), ("shared_member_down", 2),
                        ("shared_dispatch_batch", 4)]:
        assert nif.flags(name, arity) == 2, name          # ERL_NIF_DIRTY_JOB_IO_BOUND
    e = nif.new(-1)
    assert nif.call("empty", e) == "true"
    assert nif.call("shared_subscribe", e, b"t/+", 5, 1) == "ok"
    assert nif.call("shared_subscribe", e, b"t/+", 5, 1) == "ok"            # a bag stores an object once
    assert nif.call("shared_subscribe", e, b"t/+", 5, 2) == "ok"
    assert nif.call("shared_subscribe", e, b"u", 6, 2) == "ok"
    assert nif.call("empty", e) == "false"                                    # the first member added the route
    assert nif.call("shared_unsubscribe", e, b"t/+", 5, 9) == "ok"          # not a member: ok
    assert nif.call("shared_unsubscribe", e, b"t/+", 5, 1) == "ok"
    assert nif.call("shared_member_down", e, 2) == ("ok", 2)
    assert nif.call("shared_member_down", e, 2) == ("ok", 0)
    assert nif.call("empty", e) == "true"                                     # the last members deleted the routes
    for bad in [("shared_subscribe", e, "t", 5, 1), ("shared_subscribe", e, b"t", -1, 1),
                ("shared_subscribe", e, b"t", 5, b"p"), ("shared_subscribe", b"e", b"t", 5, 1),
                ("shared_unsubscribe", e, b"t", "g", 1), ("shared_member_down", e, "p"),
                ("shared_dispatch_batch", e, [b"t"], "sticky", 0),          # not on the device
                ("shared_dispatch_batch", e, [b"t"], "hash", [1, 2]),       # one key per publish
                ("shared_dispatch_batch", e, [b"t"], "hash", 7),
                ("shared_dispatch_batch", e, [b"t"], "hash", [b"k"]),
                ("shared_dispatch_batch", e, [b"t"], "random", b"seed"),
                ("shared_dispatch_batch", e, ["t"], "round_robin", 0)]:
        assert nif.call(*bad) == ("#badarg",), bad[0:1] + bad[2:]
    # a host-only engine refuses the dispatch itself, after the terms were accepted
    assert nif.call("shared_dispatch_batch", e, [b"t"], "hash", [1]) == ("error", "enodev")
    assert nif.call("shared_dispatch_batch", e, [], "round_robin", 0) == ("error", "enodev")
    assert nif.call("shared_dispatch_batch", e, [b"t"], "random", 12345) == ("error", "enodev")
    nif.drop(e)


def test_random_nth_is_the_headers_function():
    """Hand-evaluated with the constants written in include/emqx_tm.h."""
    m = (1 << 64) - 1

    def mix(z):
        z ^= z >> 30
        z = z * 0xBF58476D1CE4E5B9 & m
        z ^= z >> 27
        z = z * 0x94D049BB133111EB & m
        return z ^ z >> 31

    g = 0x9E3779B97F4A7C15
    for seed, i, f, grp, cnt in [(0, 0, 0, 0, 2), (1, 2, 3, 4, 5), (m, 99999, 0xFFFFFFFF, 0xFFFFFFFF, 64),
                                 (UNIFORM_SEED, 39999, 1, 1, 4)]:
        r = mix(((mix((seed + g * (i + 1)) & m) ^ (f << 32 | grp)) + g) & m)
        assert S.random_nth(seed, i, f, grp, cnt) == 1 + (r >> 32) % cnt
    with open(N.HEADER) as fh:
        text = fh.read()
    for const in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB"):
        assert const in text


def test_random_strategy_is_uniform_on_the_mirror(host_router):
    for p in ("p0", "p1", "p2", "p3"):
        S.subscribe("g", b"u/+", p)
    rows = S.dispatch_batch_mirror([b"u/1"] * UNIFORM_N, "random", seed=UNIFORM_SEED)
    assert rows == S.dispatch_batch_mirror([b"u/1"] * UNIFORM_N, "random", seed=UNIFORM_SEED)   # reproducible
    share = Counter(row[0][2] for row in rows)
    assert all(len(row) == 1 for row in rows) and sum(share.values()) == UNIFORM_N
    for p in ("p0", "p1", "p2", "p3"):
        assert abs(share[p] - UNIFORM_N // 4) <= UNIFORM_TOL, share
    assert S.dispatch_batch_mirror([b"u/1"] * 2000, "random", seed=UNIFORM_SEED + 1) != rows[:2000]   # another seed
