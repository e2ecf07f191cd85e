"""Per-subscriber inboxes on the device (tm_batch_inboxes): the deliveries of
tm_batch_dispatch grouped by subscriber by a stable radix sort.  The reference
for every case is NumPy on the host arrays of the same batch's
dispatch(match_offsets=True) and result() -- the entry of each delivery from
the match offsets, its publish from the row offsets, a stable argsort by
subscriber for the order -- and the oracle's Broker for the end-to-end case.
All comparisons are exact."""

import random
from dataclasses import replace

import numpy as np
import pytest

from emqx_amd import _native as N
from emqx_amd import emqx_broker as B
from emqx_amd import gen
from emqx_amd.engine import Engine, _d2h
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def reference(b):
    """(subscribers, offsets, publishes, filter_ids) from the batch's own
    publish-major dispatch, on the host."""
    roff, ids = b.result()
    _, moff, subs = b.dispatch(match_offsets=True)
    m, d = len(ids), len(subs)
    entry = np.repeat(np.arange(m, dtype=np.int64), np.diff(moff).astype(np.int64))
    pub_of = np.searchsorted(roff, np.arange(m), side="right") - 1
    order = np.argsort(subs, kind="stable")
    key = subs[order]
    heads = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if d else np.zeros(0, np.int64)
    e = entry[order]
    return (key[heads].astype(np.uint32), np.r_[heads, d].astype(np.uint32), pub_of[e].astype(np.uint32),
            ids[e].astype(np.uint32))


def assert_inboxes(got, want):
    for g, w, what in zip(got, want, ("subscribers", "offsets", "publishes", "filter_ids")):
        assert g.dtype == np.uint32 and np.array_equal(g, w), what
    subs, offs = got[0], got[1]
    assert np.all(np.diff(subs.astype(np.int64)) > 0) and np.all(np.diff(offs.astype(np.int64)) > 0)
    assert len(offs) == len(subs) + 1 and int(offs[0]) == 0 and int(offs[-1]) == len(got[2])


def run(eng, topics, **kw):
    b = eng.prepare(topics, **kw)
    b.launch()
    b.wait()
    return b


def test_deliver_batch_random_churn_vs_oracle():
    rng = random.Random(5)
    p = replace(gen.C1, n_filters=2500)
    F = gen.gen_filters(p).tolist()
    T = gen.gen_topics(p, gen.Strings.from_list(F), 17, 5000).tolist()
    B.clear_tables()
    orc = O.Broker()
    for rnd in range(3):
        for _ in range(6000):
            f, pid = rng.choice(F), rng.randrange(300)
            r = rng.random()
            if r < 0.3:
                B.unsubscribe(f, pid)
                orc.unsubscribe(f, pid)
            elif r < 0.31:
                assert B.subscriber_down(pid) == orc.subscriber_down(pid)
            else:
                B.subscribe(f, pid)
                orc.subscribe(f, pid)
        want = B.mailboxes([orc.publish(t) for t in T])
        got = B.deliver_batch(T)
        assert got.keys() == want.keys(), rnd
        for pid in want:
            assert got[pid] == want[pid], (rnd, pid)


def test_tile_edges():
    """D swept around the multiples of the sort tile: one filter with one
    subscriber (a tile of one key) and a second filter whose five subscribers
    differ in every digit."""
    eng = Engine(device=0)
    tile = eng.L.tm_inbox_tile()
    eng.subscribe(b"one/x", 7)
    varied = [0x01020304, 3, 0x00FF00FF, 0x0A000001, 0x0000FE00]
    for s in varied:
        eng.subscribe(b"v/+", s)
    for d in [0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile + 1, 3 * tile + 17]:
        nv = min(d // len(varied), 1200)
        n1 = d - nv * len(varied)
        T = [b"one/x"] * n1 + [b"v/%d" % i for i in range(nv)] + [b"nobody/home"]
        random.Random(d).shuffle(T)
        b = run(eng, T)
        got = b.inboxes()
        assert len(got[2]) == d, d
        assert b.inbox_info["passes"] == (4 if d else 0), d
        assert_inboxes(got, reference(b))
        if d == 0:
            assert len(got[0]) == 0 and got[1].tolist() == [0]
        b.free()
    b = run(eng, [])
    got = b.inboxes()
    assert [len(a) for a in got] == [0, 1, 0, 0] and got[1].tolist() == [0]
    assert b.inboxes_device()[:2] == (0, 0)
    b.free()
    eng.close()


def test_pass_count_and_digit_edges():
    ids = [0, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, 0xFFFFFFFE]
    eng = Engine(device=0)
    for k, s in enumerate(ids):
        eng.subscribe(b"k/#", s)
        eng.subscribe(b"own/%d" % k, s)
    T = [b"k/%d" % i for i in range(1200)] + [b"own/%d" % (i % 8) for i in range(1500)]
    random.Random(1).shuffle(T)
    b = run(eng, T)
    got = b.inboxes()
    assert b.inbox_info["passes"] == 4 and b.inbox_info["kernel_ms"] > 0
    assert len(got[2]) == 1200 * 8 + 1500 and got[0].tolist() == ids
    assert_inboxes(got, reference(b))
    b.free()
    eng.close()
    for top, passes in [(200, 1), (60_000, 2), (1 << 20, 3)]:
        eng = Engine(device=0)
        rng = random.Random(top)
        pids = sorted({top, 0} | {rng.randrange(top) for _ in range(300)})
        for s in pids:
            eng.subscribe(b"p/%d" % (s % 7), s)
            if s % 3 == 0:
                eng.subscribe(b"p/+", s)
        b = run(eng, [b"p/%d" % (i % 9) for i in range(400)])
        got = b.inboxes()
        assert b.inbox_info["passes"] == passes, top
        assert len(got[2]) > 2 * eng.L.tm_inbox_tile()
        assert_inboxes(got, reference(b))
        b.free()
        eng.close()


def test_skew_hash_subscribers_next_to_single_subscribers():
    """'#' with 20,000 subscribers beside 4,000 one-subscriber filters: whole
    tiles of one key next to tiles of all-different keys (~6M deliveries)."""
    p = replace(gen.C1, n_filters=4000)
    F = gen.gen_filters(p).tolist()
    T = gen.gen_topics(p, gen.Strings.from_list(F), 23, 300).tolist()
    eng = Engine(device=0)
    for i, f in enumerate(F):
        eng.subscribe(f, 1_000_000 + i)
    hot = 20_000
    for s in range(hot):
        eng.subscribe(b"#", s)
    b = run(eng, T)
    got = b.inboxes()
    assert b.inbox_info["passes"] == 3
    assert_inboxes(got, reference(b))
    subs, offs, pubs, fids = got
    plain = np.asarray([i for i, t in enumerate(T) if not t.startswith(b"$")], np.uint32)
    assert len(pubs) >= hot * len(plain) and len(plain) > 200
    # the '#' subscribers (the lowest ids) each hold every non-'$' publish, in order
    assert subs[:hot].tolist() == list(range(hot))
    assert np.array_equal(offs[:hot + 1], np.arange(hot + 1, dtype=np.uint32) * len(plain))
    assert np.array_equal(pubs[:hot * len(plain)].reshape(hot, len(plain)), np.broadcast_to(plain, (hot, len(plain))))
    assert {eng.filter_bytes(int(f)) for f in np.unique(fids[:hot * len(plain)])} == {b"#"}
    b.free()
    eng.close()


def test_stability_one_pid_through_three_filters():
    eng = Engine(device=0)
    for f in (b"a/+", b"a/#", b"a/b"):
        eng.subscribe(f, 5)
    eng.subscribe(b"a/b", 2)
    eng.subscribe(b"z", 9)
    eng.subscribe(b"a/#", 9)
    T = [b"a/b", b"z", b"a/b", b"q", b"a/c", b"a/b", b"z", b"a/b", b"a/b"]
    b = run(eng, T)
    subs, offs, pubs, fids = b.inboxes()
    assert_inboxes((subs, offs, pubs, fids), reference(b))
    r = subs.tolist().index(5)
    box = [(int(pubs[q]), eng.filter_bytes(int(fids[q]))) for q in range(int(offs[r]), int(offs[r + 1]))]
    want = []
    for i, t in enumerate(T):
        if t == b"a/b":
            want += [(i, b"a/#"), (i, b"a/+"), (i, b"a/b")]     # match (Erlang binary) order: '#' < '+' < 'b'
        elif t == b"a/c":
            want += [(i, b"a/#"), (i, b"a/+")]
    assert box == want
    b.free()
    eng.close()


def test_modes_and_lifetime():
    p = replace(gen.C1, n_filters=1500)
    F = gen.gen_filters(p).tolist()
    T = gen.gen_topics(p, gen.Strings.from_list(F), 31, 4000).tolist()

    def fill(eng):
        rng = random.Random(2)
        for f in F:
            for s in rng.sample(range(5000), rng.randint(0, 3)):
                eng.subscribe(f, s)
        for s in range(40):
            eng.subscribe(b"#", 100 * s)

    eng = Engine(device=0)
    fill(eng)
    b = eng.prepare(T)
    with pytest.raises(N.TmError) as ei:
        b.inboxes()                                     # not waited
    assert ei.value.rc == N.TM_EINVAL and b"waited" in eng.L.tm_last_error()
    b.launch()
    b.wait()
    first = b.inboxes()                                 # inboxes, then dispatch (inside reference), then inboxes
    want = reference(b)
    assert_inboxes(first, want)
    assert len(first[2]) > 3 * eng.L.tm_inbox_tile()
    assert_inboxes(b.inboxes(), want)
    offs, _, out = b.dispatch()                         # dispatch after inboxes: the publish-major form is intact
    _, _, out2 = b.dispatch()
    assert np.array_equal(out, out2) and int(offs[-1]) == len(want[2])
    r, d, ms, passes, d_sub, d_off, d_pub, d_fid = b.inboxes_device()
    assert (r, d, passes) == (len(want[0]), len(want[2]), 2) and ms > 0
    dev = [np.zeros(k, np.uint32) for k in (r, r + 1, d, d)]
    for dst, src in zip(dev, (d_sub, d_off, d_pub, d_fid)):
        _d2h(dst, src)
    assert_inboxes(dev, want)
    b.free()
    bd = run(eng, T[:500], dedup=True)                  # refused, and the batch stays usable
    with pytest.raises(N.TmError) as ei:
        bd.inboxes()
    assert ei.value.rc == N.TM_EINVAL and b"DEDUP" in eng.L.tm_last_error()
    offs, _, out = bd.dispatch()
    assert len(out) == int(offs[-1]) > 0
    bd.free()
    eng.close()
    two = Engine(devices=[0, 0])
    fill(two)
    for _ in range(2):                                  # round-robin: one batch on each replica
        b2 = run(two, T)
        assert_inboxes(b2.inboxes(), want)
        b2.free()
    two.close()


def test_nif_deliver_batch_on_the_device():
    from nif_harness import Nif
    nif = Nif()
    rng = random.Random(19)
    words = [b"a", b"b", b"c", b"+", b"#"]
    filters = set()
    while len(filters) < 120:
        ws = [rng.choice(words) for _ in range(rng.randint(1, 4))]
        if b"#" not in ws[:-1]:
            filters.add(b"/".join(ws))
    filters = sorted(filters)
    e, eng = nif.new(0), Engine(device=0)
    for f in filters:
        for s in rng.sample(range(2000), rng.randint(1, 4)):
            assert nif.call("subscribe", e, f, s, 0) == "ok"
            eng.subscribe(f, s)
    T = [b"/".join(rng.choice([b"a", b"b", b"c", b"d"]) for _ in range(rng.randint(1, 4))) for _ in range(400)]
    b = run(eng, T)
    subs, offs, pubs, fids = b.inboxes()
    want = [(int(s), [(int(pubs[q]), eng.filter_bytes(int(fids[q]))) for q in range(int(offs[r]), int(offs[r + 1]))])
            for r, s in enumerate(subs)]
    assert len(pubs) > 1000
    assert nif.call("deliver_batch", e, T) == want
    assert nif.call("deliver_batch", e, []) == []
    assert nif.call("deliver_batch", e, [b"$nobody/home"]) == []      # no filter here starts with '$'
    b.free()
    eng.close()
    nif.drop(e)
