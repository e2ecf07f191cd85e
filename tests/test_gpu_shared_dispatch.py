"""Shared-subscription dispatch on the device (tm_batch_dispatch_shared) against
the emqx_shared_sub mirror (src/emqx_shared_sub.erl:229-315): the known answers,
the three strategies, the round-robin cursor across table uploads and batches,
table and scan-tile edges, randomised churn, two replicas and the NIF."""

import random
from collections import Counter
from dataclasses import replace

import numpy as np
import pytest
import shared_cases as K
from test_shared_dispatch import UNIFORM_N, UNIFORM_SEED, UNIFORM_TOL

from emqx_amd import _native as N
from emqx_amd import emqx_broker as B
from emqx_amd import emqx_router as R
from emqx_amd import emqx_shared_sub as S
from emqx_amd import gen
from emqx_amd.engine import Engine, _d2h
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _fresh(engine):
    old = R._engine
    R.use(engine)
    if old is not None and old is not engine:
        old.close()
    R._routes.clear()
    S.clear()
    return engine


@pytest.fixture
def dev():
    yield _fresh(Engine(device=0))
    _drop()


def _drop():
    if R._engine is not None:
        R._engine.close()
    R._engine = None
    R._routes.clear()
    S.clear()


def _batch(topics):
    return R.engine().prepare(topics).launch().wait()


def _index(rows, members):
    return [members.index(r[0][2]) for r in rows]


@pytest.mark.parametrize("case", K.kat()["cases"], ids=lambda c: c["name"])
def test_kat_on_device(case, dev):
    K.run_case(case, [S.dispatch_batch_mirror, S.dispatch_batch])


def test_round_robin_single_publisher(dev):
    mem = ["a", "b", "c"]
    for p in mem:
        S.subscribe("g", b"rr/+", p)
    one = lambda: S.dispatch_batch([b"rr/1"], "round_robin")           # noqa: E731
    ref = lambda: S.dispatch_batch_mirror([b"rr/1"], "round_robin")    # noqa: E731
    got = [one() for _ in range(5)]
    assert _index([r[0] for r in got], mem) == [0, 1, 2, 0, 1]
    assert got == [ref() for _ in range(5)]
    S.unsubscribe("g", b"rr/+", "c")                                   # Count 3 -> 2: (1 + 1) rem 2
    assert one() == ref() == [[(b"rr/+", "g", "a")]]
    S.subscribe("h", b"other/#", "z")                                  # re-uploads the tables: the cursor stays
    S.subscribe("g", b"rr/+", "z")                                     # and grows the run: (0 + 1) rem 3
    assert one() == ref() == [[(b"rr/+", "g", "b")]]
    assert one() == ref() == [[(b"rr/+", "g", "z")]]
    S.member_down("z")
    S.subscribe("g", b"rr/+", "z")                                     # a re-subscribe: [a, b, z] again, N = 2
    assert one() == ref() == [[(b"rr/+", "g", "a")]]
    # a run that lost its last member starts over when it comes back
    for p in ("a", "b", "z"):
        S.unsubscribe("g", b"rr/+", p)
    for p in mem:
        S.subscribe("g", b"rr/+", p)
    assert one() == ref() == [[(b"rr/+", "g", "a")]]


def test_round_robin_batched(dev):
    mem = ["a", "b", "c"]
    for p in mem:
        S.subscribe("g", b"rr/+", p)
    k = 1000
    for lo in (0, k):                                                  # the second batch continues from the first
        rows = S.dispatch_batch([b"rr/7"] * k, "round_robin")
        assert all(len(r) == 1 for r in rows)
        want = Counter((lo + i) % 3 for i in range(k))                 # the next k cursor values
        assert Counter(_index(rows, mem)) == want
        assert Counter(_index(S.dispatch_batch_mirror([b"rr/7"] * k, "round_robin"), mem)) == want
    assert S.dispatch_batch([b"rr/7"], "round_robin") == [[(b"rr/+", "g", mem[2 * k % 3])]]
    offs, _, _, _ = _batch([b"rr/7"] * 5).dispatch_shared("round_robin", counts_only=True)
    assert offs.tolist() == [0, 1, 2, 3, 4, 5]                         # counting takes no ticket
    assert S.dispatch_batch([b"rr/7"], "round_robin") == [[(b"rr/+", "g", mem[(2 * k + 1) % 3])]]


def _hash_table():
    """a/+ carries two groups, a/b one, # none; member counts 1, 2 and 3;
    non-shared subscribers sit on the same filters."""
    S.subscribe("g1", b"a/+", "p1")
    for p in ("q1", "q2"):
        S.subscribe("g2", b"a/+", p)
    for p in ("r1", "r2", "r3"):
        S.subscribe("g3", b"a/b", p)
    S.subscribe("g2", b"$SYS/#", "q1")
    S.subscribe("g2", b"$SYS/#", "q2")
    for f in (b"a/+", b"a/b", b"#"):
        B.subscribe(f, "plain-" + f.decode())
    topics = [b"a/b", b"a/c", b"$SYS/x", b"zzz", b"a/b", b"a/b", b"a", b"a/b/c", b"$SYS/x", b"a/b"]
    return topics, list(range(10))


def test_hash_rows_forms_and_repeat(dev):
    topics, keys = _hash_table()
    want = S.dispatch_batch_mirror(topics, "hash", keys=keys)
    assert want[0] == [(b"a/+", "g1", "p1"), (b"a/+", "g2", "q1"), (b"a/b", "g3", "r1")]
    assert want[2] == [(b"$SYS/#", "g2", "q1")] and want[3] == [] and want[5][2] == (b"a/b", "g3", "r3")
    assert S.dispatch_batch(topics, "hash", keys=keys) == want
    assert not any(pid.startswith("plain-") for row in want for _, _, pid in row)
    b = _batch(topics)
    offs, fids, grp, subs = b.dispatch_shared("hash", keys=keys)
    assert offs.tolist() == np.cumsum([0] + [len(r) for r in want]).tolist()
    o2, f2, g2, s2 = b.dispatch_shared("hash", keys=keys)               # the same waited batch again
    assert all(np.array_equal(x, y) for x, y in ((offs, o2), (fids, f2), (grp, g2), (subs, s2)))
    oc, fc, gc, sc = b.dispatch_shared("hash", counts_only=True)
    assert np.array_equal(oc, offs) and fc is None and gc is None and sc is None
    total, ms, p_off, p_fid, p_grp, p_sub = b.dispatch_shared_device("hash", keys=keys)
    assert total == len(subs) and ms >= 0.0
    for ptr, host in ((p_off, offs), (p_fid, fids), (p_grp, grp), (p_sub, subs)):
        d = np.zeros_like(host)
        _d2h(d, ptr)
        assert np.array_equal(d, host)
    # the local fan-out of the same batch is untouched by the shared members
    doffs, _, dsubs = b.dispatch()
    assert [B._terms[int(s)] for s in dsubs[doffs[0]:doffs[1]]] == ["plain-#", "plain-a/+", "plain-a/b"]
    b.free()


def test_einval_on_device(dev):
    topics, keys = _hash_table()
    eng = R.engine()
    b = eng.prepare(topics)
    for launch in (False, True):                                       # prepared, then launched: not waited
        if launch:
            b.launch()
        with pytest.raises(N.TmError) as ei:
            b.dispatch_shared("hash", keys=keys)
        assert ei.value.rc == N.TM_EINVAL and "not been waited" in eng.L.tm_last_error().decode(), launch
    b.wait()
    with pytest.raises(N.TmError) as ei:
        b.dispatch_shared("hash")
    assert ei.value.rc == N.TM_EINVAL and "without keys" in eng.L.tm_last_error().decode()
    with pytest.raises(N.TmError) as ei:
        b.dispatch_shared(3, keys=keys)
    assert ei.value.rc == N.TM_EINVAL and "unknown strategy" in eng.L.tm_last_error().decode()
    assert len(b.dispatch_shared("hash", keys=keys)[3]) == 16          # the batch is fine
    b.free()
    d = eng.prepare(topics, dedup=True).launch().wait()
    with pytest.raises(N.TmError) as ei:
        d.dispatch_shared("hash", keys=keys)
    assert ei.value.rc == N.TM_EINVAL and "TM_BATCH_DEDUP" in eng.L.tm_last_error().decode()
    d.free()


def test_table_edges(dev):
    for g in range(300):                                               # past the saturating count byte
        for m in range(1 + g % 3):
            S.subscribe(f"g{g}", b"many/#", f"m{g}.{m}")
    S.subscribe("solo", b"few", "s")
    B.subscribe(b"plain/+", "x")
    topics = [b"many/1", b"plain/1", b"few", b"many"]
    keys = [5, 6, 7, 8]
    want = S.dispatch_batch_mirror(topics, "hash", keys=keys)
    assert [len(r) for r in want] == [300, 0, 1, 300]
    assert [g for _, g, _ in want[0]] == [f"g{g}" for g in range(300)]  # groups in first-added order
    assert S.dispatch_batch(topics, "hash", keys=keys) == want
    rr = [b"many/1", b"few"]                                           # every run once: tickets within a batch are unordered
    assert S.dispatch_batch(rr, "round_robin") == S.dispatch_batch_mirror(rr, "round_robin")
    assert S.dispatch_batch(rr, "round_robin") == S.dispatch_batch_mirror(rr, "round_robin")
    assert S.dispatch_batch([], "hash", keys=[]) == []                  # n = 0
    offs, fids, grp, subs = _batch([]).dispatch_shared("round_robin")
    assert offs.tolist() == [0] and len(fids) == len(grp) == len(subs) == 0
    rows = S.dispatch_batch([b"plain/1", b"plain/2", b"nothing"], "hash", keys=[1, 2, 3])
    assert rows == [[], [], []]                                        # matches, but no shared delivery
    offs, *_ = _batch([b"plain/1"] * 3).dispatch_shared("random", seed=1, counts_only=True)
    assert offs.tolist() == [0, 0, 0, 0]


def test_scan_tile_and_block_boundaries(dev):
    """3,000 publishes x 2 matches = 6,000 match entries: past the 4,096-entry
    scan tile and over 24 blocks of 256; groups only on every 37th filter."""
    rng = random.Random(9)
    eng = R.engine()
    eng.route_add(b"s/+", R._agg_id(R.NODE))
    for i in range(300):
        eng.route_add(b"s/%d" % i, R._agg_id(R.NODE))
        if i % 37 == 0:
            for g in ("ga", "gb"):
                for m in range(rng.randint(1, 3)):
                    S.subscribe(g, b"s/%d" % i, f"{g}{i}.{m}")
    topics = [b"s/%d" % (i % 300) for i in range(3000)]
    keys = [rng.getrandbits(32) for _ in topics]
    b = _batch(topics)
    assert len(b.result()[1]) == 6000
    b.free()
    want = S.dispatch_batch_mirror(topics, "hash", keys=keys)
    assert sum(len(r) for r in want) == 2 * 10 * 9 and len(want[37]) == 2 and want[36] == []
    assert S.dispatch_batch(topics, "hash", keys=keys) == want
    assert S.dispatch_batch(topics, "random", seed=77) == S.dispatch_batch_mirror(topics, "random", seed=77)


def test_random_churn_vs_mirror(dev):
    rng = random.Random(21)
    p = replace(gen.C1, n_filters=2500)
    F = gen.gen_filters(p).tolist()
    T = gen.gen_topics(p, gen.Strings.from_list(F), 17, 5000).tolist()
    groups = [f"g{i}" for i in range(40)]
    for rnd in range(3):
        for _ in range(6000):
            f, g, pid = rng.choice(F), rng.choice(groups), rng.randrange(300)
            r = rng.random()
            if r < 0.3:
                S.unsubscribe(g, f, pid)
            elif r < 0.31:
                S.member_down(pid)
            else:
                S.subscribe(g, f, pid)
        trie = O.Trie()
        for f in S._groups_of:
            if O.wildcard(f):
                trie.insert(f)
        matched = lambda t: ([] if trie.empty() else trie.match(t)) + [t]   # noqa: E731
        keys = [rng.getrandbits(32) for _ in T]
        want = S.dispatch_batch_mirror(T, "hash", keys=keys, matched=matched)
        assert sum(len(r) for r in want) > 1000
        got = S.dispatch_batch(T, "hash", keys=keys)
        for t, a, b in zip(T, got, want):
            assert a == b, (rnd, t)
        if rnd == 1:
            assert S.dispatch_batch(T, "random", seed=rnd) == S.dispatch_batch_mirror(T, "random", seed=rnd,
                                                                                     matched=matched)


def test_random_strategy_on_device(dev):
    mem = ["p0", "p1", "p2", "p3"]
    for p in mem:
        S.subscribe("g", b"u/+", p)
    topics = [b"u/1"] * UNIFORM_N
    rows = S.dispatch_batch(topics, "random", seed=UNIFORM_SEED)
    assert rows == S.dispatch_batch(topics, "random", seed=UNIFORM_SEED)          # same seed, same rows
    assert rows == S.dispatch_batch_mirror(topics, "random", seed=UNIFORM_SEED)
    assert rows[:2000] != S.dispatch_batch(topics[:2000], "random", seed=UNIFORM_SEED + 1)
    share = Counter(r[0][2] for r in rows)
    for p in mem:
        assert abs(share[p] - UNIFORM_N // 4) <= UNIFORM_TOL, share


def test_two_replicas_on_one_device():
    eng = _fresh(Engine(devices=[0, 0]))
    try:
        assert eng.replicas == 2
        for p in ("a", "b", "c"):
            S.subscribe("g", b"r/+", p)
        S.subscribe("h", b"r/1", "d")
        topics, keys = [b"r/1", b"r/2", b"x"], [4, 5, 6]
        want = S.dispatch_batch_mirror(topics, "hash", keys=keys)
        assert want[0] == [(b"r/+", "g", "b"), (b"r/1", "h", "d")]
        for rep in (1, 0, 1):
            b = eng.prepare(topics, replica=rep).launch().wait()
            assert b.replica == rep
            offs, fids, grp, subs = b.dispatch_shared("hash", keys=keys)
            got = [[(eng.filter_bytes(int(fids[k])), R._agg_of[int(grp[k])][1], B._terms[int(subs[k])])
                    for k in range(int(offs[i]), int(offs[i + 1]))] for i in range(len(topics))]
            assert got == want, rep
            b.free()
        S.subscribe("g", b"r/+", "e")                                   # made after both replicas synced once
        for rep in (1, 0):                                             # a cursor per replica: both start at member 1
            picks = []
            for _ in range(2):
                b = eng.prepare([b"r/2"], replica=rep).launch().wait()
                picks.append(B._terms[int(b.dispatch_shared("round_robin")[3][0])])
                b.free()
            assert picks == ["a", "b"], rep
    finally:
        _drop()


def test_nif_shared_dispatch_batch(dev):
    from nif_harness import Nif
    nif = Nif()
    e = nif.new(0)
    topics, keys = _hash_table()
    for (group, topic), pids in S._members.items():
        for pid in pids:
            assert nif.call("shared_subscribe", e, topic, R._agg_id((group, R.NODE)), B._sid(pid)) == "ok"
    for f in (b"a/+", b"a/b", b"#"):
        assert nif.call("subscribe", e, f, B._sid("plain-" + f.decode()), R._agg_id(R.NODE)) == "ok"
    b = _batch(topics)
    offs, fids, grp, subs = b.dispatch_shared("hash", keys=keys)
    eng = R.engine()
    want = [[(eng.filter_bytes(int(fids[k])), int(grp[k]), int(subs[k])) for k in range(int(offs[i]), int(offs[i + 1]))]
            for i in range(len(topics))]
    assert sum(len(r) for r in want) == 16
    assert nif.call("shared_dispatch_batch", e, topics, "hash", keys) == want
    rnd = b.dispatch_shared("random", seed=99)
    want = [[(eng.filter_bytes(int(rnd[1][k])), int(rnd[2][k]), int(rnd[3][k]))
             for k in range(int(rnd[0][i]), int(rnd[0][i + 1]))] for i in range(len(topics))]
    # the two engines number their trie nodes alike (same inserts in the same order), so the hash of
    # (seed, publish, filter id, group id) picks alike
    assert nif.call("shared_dispatch_batch", e, topics, "random", 99) == want
    rr = [nif.call("shared_dispatch_batch", e, [b"a/b"], "round_robin", 0)[0] for _ in range(4)]
    assert [row[-1][2] for row in rr] == [B._sid(p) for p in ("r1", "r2", "r3", "r1")]
    assert nif.call("shared_dispatch_batch", e, [], "round_robin", 0) == []
    assert nif.call("shared_member_down", e, B._sid("q1")) == ("ok", 2)
    b.free()
    nif.drop(e)
