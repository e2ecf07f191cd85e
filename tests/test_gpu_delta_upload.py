"""The delta uploads on the device, through the C ABI -- needs an MI355X.

tests/test_delta_shadow.py checks WHICH slots, nodes and keys the upload path
lists and which side of every full-or-delta switch it takes, against a shadow
in host memory.  Here the copies and the scatter kernels themselves are
checked: tm_debug_replica_diff copies the replica's seven tables back and
compares them with the host's element by element (so a slot no topic probes
counts too), and the rows of topics that touch the new filters are compared,
in order, with sorted(set(oracle.Trie.match)) -- Python's bytes order is the
rows' order.  The counters of tm_debug_upload_info say which path ran; they
count per replica, so every expectation is multiplied by the replicas.
"""

import pytest

from emqx_amd import _native as N
from emqx_amd.engine import Engine
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LIVE = [t for t in N.DIFF_TABLES if not t.endswith("_dead")]
REPLICAS = {1: [0], 2: [0, 0]}


def in_sync(d):
    return all(d[t] == (0, None) for t in LIVE)


def delta(u0, u1, *names):
    return tuple(u1[n] - u0[n] for n in names)


class Pair:
    """An engine on the device and the oracle trie, mutated together."""

    def __init__(self, nrep=1, **kw):
        self.e, self.t, self.nrep = Engine(devices=REPLICAS[nrep], **kw), O.Trie(), nrep

    def insert(self, f):
        self.e.insert(f)
        self.t.insert(f)

    def insert_many(self, F):
        assert self.e.insert_many(F) == len(F)
        for f in F:
            self.t.insert(f)

    def delete(self, f):
        self.e.delete(f)
        self.t.delete(f)

    def upload(self):
        """One upload; -> (upload info before, after).  Every replica then equals the host."""
        u0 = self.e.upload_info()
        for r in range(self.nrep):
            d = self.e.replica_diff(r, sync=True)
            assert in_sync(d), (r, d)
        return u0, self.e.upload_info()

    def rows_equal(self, T):
        offs, ids = self.e.match_batch(T)
        got = [[self.e.filter_bytes(int(i)) for i in ids[offs[k]:offs[k + 1]]] for k in range(len(T))]
        exp = [sorted(set(self.t.match(t))) for t in T]
        bad = [(T[k], got[k][:4], exp[k][:4]) for k in range(len(T)) if got[k] != exp[k]]
        assert not bad, bad[:3]
        return exp


def test_replica_diff_sees_a_stale_replica():
    p = Pair(init_slots=4096)
    p.insert_many([b"base/%d" % i for i in range(200)] + [b"base/+", b"#"])
    p.upload()
    for i in range(20):
        p.insert(b"late/%d/+" % i)
    d = p.e.replica_diff(0, sync=False)        # nothing uploaded since: the device is behind
    assert d["slots"][0] >= 20 and d["fbytes"][0] >= 20 * len(b"late/0/+") and d["flen"][0] == 20
    assert d["dkey"][0] >= 1 and d["tail"][0] == 1 and d["arena"][0] == len(b"late")    # (the one new word)
    assert in_sync(p.e.replica_diff(0, sync=True))
    assert in_sync(p.e.replica_diff(0, sync=False))
    p.rows_equal([b"late/3/x", b"base/7", b"late/19/", b"nothing"])


def test_the_shadow_refuses_an_engine_with_replicas():
    p = Pair()
    p.insert(b"a/+")
    with pytest.raises(N.TmError) as ei:       # the dirty sets are consumed once: by the replicas
        p.e.shadow_sync(apply=True)
    assert ei.value.rc == N.TM_EINVAL
    assert p.e.upload_info()["full_dirty"] == 1
    with pytest.raises(N.TmError) as ei:
        p.e.replica_diff(1, sync=False)
    assert ei.value.rc == N.TM_EINVAL
    p.upload()
    p.rows_equal([b"a/b"])


@pytest.mark.parametrize("nrep", [1, 2])
def test_slot_switch_on_the_device(nrep):
    """1,024 slots: 128 dirty slots are scattered, 129 copied whole (tests/test_delta_shadow.py)."""
    p = Pair(nrep)
    e = p.e
    p.upload()
    n = 0
    for target, whole in ((128, False), (129, True)):
        first = n
        while e.upload_info()["dirty"] < target:
            p.insert(b"s%d" % n)
            n += 1
        u0, u1 = p.upload()
        assert (u0["slots"], u0["dirty"], u0["full_dirty"]) == (1024, target, 0)
        if whole:
            assert delta(u0, u1, "uploads_full", "uploads_delta", "delta_slots") == (nrep, 0, 0)
        else:
            assert delta(u0, u1, "uploads_full", "uploads_delta", "delta_slots") == (0, nrep, nrep * target)
        assert delta(u0, u1, "fmeta_delta", "fmeta_nodes", "slots_realloc") == (nrep, nrep * u0["dirty_f"], 0)
        exp = p.rows_equal([b"s%d" % i for i in range(first, n)] + [b"s%d/x" % first, b"zz"])
        assert exp[0] == [b"s%d" % first]


@pytest.mark.parametrize("nrep", [1, 2])
@pytest.mark.parametrize("whole", [False, True])
def test_dictionary_switch_on_the_device(whole, nrep):
    """1,024 key slots: 128 listed keys are scattered, 129 copied whole."""
    p = Pair(nrep, init_slots=16384)
    e = p.e
    p.upload()
    target, n = 128 + (1 if whole else 0), 0
    while e.upload_info()["dict_dirty"] < target:
        p.insert(b"k%d" % n)
        n += 1
    u0, u1 = p.upload()
    assert (u0["dict_keys"], u0["dict_dirty"]) == (1024, target) and u0["dirty"] <= u0["slots"] // 8
    if whole:
        assert delta(u0, u1, "keys_full", "keys_delta", "keys_scattered") == (nrep, 0, 0)
    else:
        assert delta(u0, u1, "keys_full", "keys_delta") == (0, nrep)
        assert nrep * n <= u1["keys_scattered"] - u0["keys_scattered"] <= nrep * target
    assert delta(u0, u1, "dict_gen") == (0,)
    exp = p.rows_equal([b"k%d" % i for i in range(n)] + [b"k%d" % n, b"k"])   # tokenised on the device: the new keys
    assert exp[n - 1] == [b"k%d" % (n - 1)] and exp[n] == []


@pytest.mark.parametrize("nrep", [1, 2])
def test_scatter_kernels_block_tail(nrep):
    """Deltas of 1, 255, 256 and 257 slots, filter nodes and (at least as many)
    dictionary keys: the scatter kernels' last block empty but for one
    thread, one short, full, and one thread into the next."""
    p = Pair(nrep, init_slots=8192)
    e = p.e
    p.insert_many([b"w%d" % i for i in range(1100)])     # the key table grows to 8,192 slots: an eighth is 1,024
    p.upload()
    assert e.upload_info()["dict_keys"] == 8192
    n = 0
    for k in (1, 255, 256, 257):
        first = n
        while e.upload_info()["dirty"] < k:
            p.insert(b"t%d" % n)
            n += 1
        u0, u1 = p.upload()
        assert (u0["slots"], u0["dirty"], u0["dirty_f"], u0["full_dirty"]) == (8192, k, k, 0)
        assert k <= u0["dict_dirty"] <= 1024 and u0["dict_keys"] == 8192
        assert delta(u0, u1, "uploads_full", "uploads_delta", "delta_slots") == (0, nrep, nrep * k)
        assert delta(u0, u1, "fmeta_full", "fmeta_delta", "fmeta_nodes") == (0, nrep, nrep * k)
        assert delta(u0, u1, "keys_full", "keys_delta") == (0, nrep)
        assert nrep * k <= u1["keys_scattered"] - u0["keys_scattered"] <= nrep * u0["dict_dirty"]
        p.rows_equal([b"t%d" % i for i in range(first, n)] + [b"w7", b"t%d" % n])


def test_growth_under_captured_batches():
    """A rehash reallocates d_slots: an own-stream batch and an ordinary one,
    both launched before (their launch graphs hold the old address), are
    launched again and read the new table."""
    p = Pair()
    e = p.e
    p.insert_many([b"g%d/+" % i for i in range(300)] + [b"g1/#", b"+/x"])
    T = [b"g%d/x" % i for i in range(0, 450, 3)] + [b"new/1", b"new/40/x"]
    a, b = e.prepare(T, stream=True), e.prepare(T)

    def rows_of(batch):
        offs, ids = batch.result()
        return [[e.filter_bytes(int(i)) for i in ids[offs[k]:offs[k + 1]]] for k in range(len(T))]

    for _ in range(2):                         # the second launch replays the captured graph
        a.launch()
        b.launch()
        a.wait()
        b.wait()
    exp = [sorted(set(p.t.match(t))) for t in T]
    assert rows_of(a) == exp and rows_of(b) == exp
    u0 = e.upload_info()
    assert u0["slots"] == 1024
    n = 0
    while e.upload_info()["slots"] == 1024:    # through the 3/4-load rehash
        p.insert(b"new/%d/#" % n)
        n += 1
    assert e.upload_info()["full_dirty"] == 1
    a.launch()
    b.launch()
    a.wait()
    b.wait()
    exp2 = [sorted(set(p.t.match(t))) for t in T]
    assert n > 40 and exp[-1] == [] and exp2[-2:] == [[b"new/1/#"], [b"new/40/#"]]
    assert rows_of(a) == exp2 and rows_of(b) == exp2
    u1 = e.upload_info()
    assert delta(u0, u1, "slots_realloc", "uploads_full") == (1, 1) and u1["slots"] > 1024
    assert in_sync(e.replica_diff(0, sync=False))
    a.free()
    b.free()


def test_growth_with_two_replicas():
    p = Pair(2)
    e = p.e
    p.insert_many([b"g%d/+" % i for i in range(300)])
    p.upload()
    n = 0
    while e.upload_info()["slots"] == 1024:
        p.insert(b"new/%d/#" % n)
        n += 1
    for r in range(2):                         # a replica of another size is a difference, reported as an error
        with pytest.raises(N.TmError) as ei:
            e.replica_diff(r, sync=False)
        assert ei.value.rc == N.TM_EIO and b"1024 slots" in N.lib().tm_last_error()
    u0, u1 = p.upload()
    assert u0["full_dirty"] == 1 and delta(u0, u1, "slots_realloc", "uploads_full", "uploads_delta") == (2, 2, 0)
    p.rows_equal([b"g%d/x" % i for i in range(0, 400, 7)] + [b"new/%d/a/b" % i for i in range(n + 1)])
    p.insert(b"after/+")
    u0, u1 = p.upload()
    assert delta(u0, u1, "slots_realloc", "uploads_full", "uploads_delta") == (0, 0, 2)
    p.rows_equal([b"after/x", b"new/0"])


def test_repack_on_the_device():
    """70,000 filters in 1,048,576 slots (load 0.067 < 0.175): the upload
    re-packs the table to load 0.35, into a new buffer."""
    p = Pair(init_slots=1 << 20)
    e = p.e
    p.upload()                                 # the replica holds the sparse table first
    F = [b"r%d/s%d" % (i % 300, i) for i in range(70_000)]
    p.insert_many(F)
    for f in F[:300:3]:
        p.delete(f)
    edges = e.stats()["edges"]
    u = e.upload_info()
    assert edges > 65536 and u["slots"] == 1 << 20 and u["needs_repack"] == 1
    u0, u1 = p.upload()
    assert delta(u0, u1, "repacks", "uploads_full", "slots_realloc") == (1, 1, 1)
    assert u1["needs_repack"] == 0 and abs(edges / u1["slots"] - 0.35) < 0.01
    T = F[::35] + [b"r7/nope", b"nope/s7"]
    assert len(T) >= 2000
    exp = p.rows_equal(T)
    assert exp[0] == [] and exp[1] == [F[35]]


def test_appended_tails_pinned_regrown_and_pageable():
    p = Pair(init_slots=16384)
    e = p.e
    p.insert_many([b"base/%03d" % i for i in range(100)])
    u0, u1 = p.upload()
    # (the replica's buffers, by upload_to's rules: twice the need, a quarter more, at least 1,024)
    need = 2 * (u0["fbytes"] + 1)
    cap = max(need + need // 4, 1024)
    # an append that stays inside: three tails (filter bytes, dictionary tails, arena) through the pinned staging
    p.insert_many([b"in/%03d" % i for i in range(20)])
    u0, u1 = p.upload()
    assert u0["fbytes"] + 1 <= cap
    assert delta(u0, u1, "tail_pinned", "tail_pageable") == (3, 0)
    # across the capacity: a new buffer, recopied from byte 0 (the comparison covers the old bytes too)
    more = [b"across/%04d" % i for i in range(cap // 11 + 1)]
    p.insert_many(more)
    u0, u1 = p.upload()
    assert u0["fbytes"] + 1 > cap and delta(u0, u1, "tail_pinned", "tail_pageable") == (3, 0)
    p.rows_equal([b"base/007", b"in/019", more[-1], b"across/x"])
    # one delta above 8 MiB in all: pageable copies, waited for
    # (filters of four 1,000-byte words, the longest tests/long_words.py uses, the first one new each time:
    # 4,003 filter bytes and 1,000 arena bytes a filter)
    tail3 = b"/".join(c * 1000 for c in (b"x", b"y", b"z"))
    big = [b"%04d" % i + b"w" * 996 + b"/" + tail3 for i in range(1700)]
    was = e.upload_info()
    p.insert_many(big)
    u0, u1 = p.upload()
    appended = sum(delta(was, u0, "fbytes", "dict_arena"))
    assert appended == 1700 * (4003 + 1000) + 3000 > 8 << 20 and u0["slots"] == 16384
    assert delta(u0, u1, "tail_pinned", "tail_pageable") == (0, 3)
    p.rows_equal([big[0], big[-1], big[500][:-1] + b"q", b"base/099"])


DEEP = [b"d%d" % i for i in range(11)]


def test_filter_metadata_where_the_generic_path_reads_it():
    """A topic of 11 levels goes to the generic path, which orders its row by
    the filters' bytes on the device (d_foff, d_flen, d_fbytes): filters of
    the latest delta, and a filter id handed from one filter to another of
    other bytes and length, must sort where the oracle puts them."""
    p = Pair()
    e = p.e
    topic = b"/".join(DEEP)
    others = [topic + b"/x", b"/".join(DEEP[:10]), b"d0/zz"]
    p.insert_many([topic, b"d0/#", b"/".join([b"+"] + DEEP[1:]), b"/".join(DEEP[:5] + [b"+"] + DEEP[6:]), b"d0/zz"])
    exp = p.rows_equal([topic] + others)
    assert len(exp[0]) == 4
    # (a) filters the latest delta brought
    a = b"/".join(DEEP[:10] + [b"+"])
    for f in (a, b"/".join(DEEP[:9] + [b"+", b"+"]), b"/".join(DEEP[:3] + [b"#"]), b"#"):
        p.insert(f)
    u0 = e.upload_info()
    assert u0["dirty_f"] == 4 and not u0["full_f_dirty"]
    exp = p.rows_equal([topic] + others)
    assert len(exp[0]) == 8 and a in exp[0]
    # (b) a's id goes to another filter: held back while a batch launched before the delete lives
    live = e.prepare([topic]).launch().wait()
    fid = e.filter_id(a)
    p.delete(a)
    x = b"/".join(DEEP[:10] + [b"x"])
    p.insert(x)
    assert e.filter_id(x) != fid               # (pending: the live batch may still name it)
    p.rows_equal([topic] + others)
    live.free()
    b = topic + b"/#"                          # one new node, under d10: it takes the freed id
    p.insert(b)
    assert e.filter_id(b) == fid and len(b) != len(a) and e.filter_bytes(fid) == b
    u0 = e.upload_info()
    assert u0["dirty_f"] == 1 and not u0["full_f_dirty"]
    exp = p.rows_equal([topic] + others)
    assert len(exp[0]) == 8 and b in exp[0] and a not in exp[0] and b in exp[1]
    assert in_sync(e.replica_diff(0, sync=False))
