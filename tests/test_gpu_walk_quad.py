"""The walk's quad protocol at its edges, against the oracle -- the device
cases need an MI355X; the world's shape is proved on the host.

In the frontier loop a probe's owner lane p sits in the quad that reads its
bucket (round p & 3 of quad p >> 2).  The quad takes the bucket, the parent and
the word from the owner by DPP; the lane whose slot matches stores the slot
whole over the owner's stack entry, after the last slot's lane has stored that
slot's raw parent field into the entry's word field.  The owner tells "found"
from the child field (never its parent's id), the literal signature from the
key fields, "the run ends here" from SLOT_EMPTY in the word field.

The world (tests/probe_model.py places the keys in a 256-bucket table; the
shape is read back from the dumped table, test_world_has_the_shape_it_claims):

    slots     root keys found in slot 0, 1, 2 and 3 of their bucket: buckets of
              one, two and three keys (last slot free) and a full one, whose
              slot-3 key gets the tail word and the match in the same entry
    kinds     the four keys of the full bucket carry B_TOPIC alone, B_TOPIC |
              B_PLUS, a '#' child (B_HASH | B_HTERM), and all of them; children
              without a '#' child keep Bloom bits in the hash field
    misses    an absent key whose home bucket has a free last slot (1 read);
              absent keys homed in full buckets: continued into an empty
              bucket (2 reads), through two full ones (3), across the wrap (2)
    runs      keys found one and two buckets from home, and across the wrap
              from bucket 255 to bucket 0
    topics    from ROOT, '$'-rooted, a literal '#' last word (M_SKIPE), '+'
              edges, unknown words

Every row is compared with the oracle's; the batch's bucket reads with the
count read off the dumped table; visits, '#' hits, words and matches with the
oracle's own counters.  Batches of 1, 2, 3, 4, 5, 63, 64 and 65 topics walk
one-topic tiles (pops of one to three probes: partial quads); 512, 1,024 and
4,096 topics walk tiles of 2, 4 and 16 topics, whose pops hold any number of
probes and end in partial pops.  One more world overflows the probe stack.
"""

import itertools

import numpy as np
import pytest

import probe_model as M
from emqx_amd.engine import Engine
from oracle import pyoracle as P

NB = M.NB
B_FULL, B_ONE, B_TWO, B_THREE, B_RUN, B_LAST = 10, 20, 30, 40, 100, NB - 1
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 512, 1024, 4096]


def min_tiles():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "emqx_amd", "csrc", "tm_kernels.hip")).read()
    return int(re.search(r"#define TM_MIN_TILES (\d+)", src).group(1))


def tile_topics(n):
    tt = 64
    while tt > 1 and (n + tt - 1) // tt < min_tiles():
        tt >>= 1
    return tt


def quad_world(eng):
    """Fill eng; -> dict(filters, topics, and the keys by role)."""
    M.pool_ids(eng)
    M.pool_ids(eng, dollar=True)
    full = M.pick(eng, M.ROOT, B_FULL, 4)
    one = M.pick(eng, M.ROOT, B_ONE, 1)
    two = M.pick(eng, M.ROOT, B_TWO, 2)
    three = M.pick(eng, M.ROOT, B_THREE, 3)
    run = M.pick(eng, M.ROOT, B_RUN, 9)             # displacements 0 0 0 0 1 1 1 1 2
    wrap = M.pick(eng, M.ROOT, B_LAST, 6)           # four in bucket 255, two in bucket 0
    dl = M.pick(eng, M.ROOT, 60, 2, dollar=True)
    roots = full + one + two + three + run + wrap   # placed first, in this order
    absent = {
        "free": (M.pick(eng, M.ROOT, B_ONE, 1, skip=1)[0], 1),        # (word, bucket reads)
        "empty": (M.pick(eng, M.ROOT, B_FULL + 1, 1)[0], 1),
        "full": (M.pick(eng, M.ROOT, B_FULL, 1, skip=4)[0], 2),
        "full2": (M.pick(eng, M.ROOT, B_RUN, 1, skip=9)[0], 3),
        "wrap": (M.pick(eng, M.ROOT, B_LAST, 1, skip=6)[0], 2),
    }
    pool = M.pool_words()
    x, y, z = pool[11], pool[12], pool[13]
    below = [
        full[1] + b"/+",                                               # B_TOPIC | B_PLUS
        full[2] + b"/#",                                               # B_TOPIC, B_HASH | B_HTERM
        full[3] + b"/+", full[3] + b"/#", full[3] + b"/" + x, full[3] + b"/+/" + y,   # everything, in slot 3
        three[2] + b"/" + x + b"/#",                                   # '#' child without a topic of x's own
        run[8] + b"/#", run[8] + b"/+", run[8] + b"/" + y,
        run[4] + b"/" + x, run[4] + b"/" + y,                          # literal children only: Bloom bits
        wrap[5] + b"/+/" + z, wrap[4] + b"/" + z,
        b"+/" + z, b"+/+/" + y,                                        # root '+'
        dl[0], dl[0] + b"/" + x, dl[0] + b"/+", dl[1] + b"/#",         # '$' words
        one[0] + b"/#/" + x, one[0] + b"/#",                           # a literal '#' word in a topic
    ]
    filters = roots + below
    for f in filters:
        eng.insert(f)
    topics = [
        full[3] + b"/" + x, full[3], full[0], full[1] + b"/" + z, full[2] + b"/" + x + b"/" + y,
        one[0], two[1], three[2], three[2] + b"/" + x, three[2] + b"/" + x + b"/" + y, three[0] + b"/" + x,
        full[3] + b"/" + z + b"/" + y, full[3] + b"/" + y, full[1], full[2], two[0], three[1],
        absent["free"][0], absent["empty"][0], absent["full"][0], absent["full2"][0], absent["wrap"][0],
        absent["full"][0] + b"/" + z, absent["wrap"][0] + b"/" + x + b"/" + y,
        run[8], run[8] + b"/" + y, run[8] + b"/" + x, run[4], run[4] + b"/" + x, run[4] + b"/" + z, run[5], run[0],
        wrap[5] + b"/" + x + b"/" + z, wrap[4] + b"/" + z, wrap[4] + b"/" + y, wrap[0], wrap[3],
        dl[0], dl[0] + b"/" + x, dl[0] + b"/" + z, dl[1], dl[1] + b"/" + x + b"/" + y, b"$k59999", b"$k59999/" + x,
        one[0] + b"/#", one[0] + b"/#/" + x, one[0] + b"/#/" + z, full[2] + b"/#", two[0] + b"/#",
        b"neverseen", full[0] + b"/neverseen", full[3] + b"/neverseen/" + y, b"neverseen/" + z,
        run[1], run[2], run[3], run[6], run[7], wrap[1], wrap[2], three[0], one[0] + b"/" + z,
        z, z + b"/" + z, z + b"/" + x + b"/" + y,
    ]
    assert len(set(topics)) == len(topics) == 65
    return dict(filters=filters, topics=topics, full=full, one=one, two=two, three=three, run=run, wrap=wrap,
                absent=absent, max_probe=4)


def where(table, parent, wid):
    """(bucket, slot index, the slot) of a live key."""
    for b in range(table.nb):
        for k in range(M.BUCKET):
            p, w = int(table.s[b, k, 0]), int(table.s[b, k, 1])
            if p != M.EMPTY and (p & M.ID_MASK) == parent and (w & M.WID_MASK) == wid:
                return b, k, [int(v) for v in table.s[b, k]]
    raise AssertionError((parent, wid))


def check_quad_world(eng, w):
    """Everything the world claims, read from the dumped table; -> the Table."""
    t = M.Table(eng.debug_slots())
    assert t.nb == NB and t.max_disp() == eng.debug_check() == 2 and M.stepped(2) == w["max_probe"]
    root = lambda word: where(t, M.ROOT, M.word_id(eng, word))
    # a found edge in each slot of its bucket; slot 3 only in full buckets
    assert [root(k)[:2] for k in w["full"]] == [(B_FULL, i) for i in range(4)]
    assert root(w["one"][0])[:2] == (B_ONE, 0) and not t.full(B_ONE)
    assert [root(k)[:2] for k in w["two"]] == [(B_TWO, 0), (B_TWO, 1)] and not t.full(B_TWO)
    assert [root(k)[:2] for k in w["three"]] == [(B_THREE, i) for i in range(3)] and not t.full(B_THREE)
    # the summaries the full bucket's slots carry
    c = [root(k)[2] for k in w["full"]]
    topic, plus = [bool(s[2] & M.B_TOPIC) for s in c], [bool(s[2] & M.B_PLUS) for s in c]
    hsh, hterm = [bool(s[3] & M.B_HASH) for s in c], [bool(s[3] & M.B_HTERM) for s in c]
    assert topic == [True] * 4 and plus == [False, True, False, True]
    assert hsh == hterm == [False, False, True, True]
    s = root(w["three"][2])[2]                       # a node without a topic above a '#' child with one
    n = s[2] & M.ID_MASK
    s = where(t, n, M.word_id(eng, M.pool_words()[11]))[2]
    assert not s[2] & M.B_TOPIC and s[3] & M.B_HASH and s[3] & M.B_HTERM
    s = root(w["run"][4])[2]                         # literal children only: Bloom bits, no '#' flag
    assert not s[3] & M.B_HASH and s[3] != 0 and not s[2] & M.B_PLUS
    # a child's id is never its parent's (what "found" rests on)
    live = t.s[t.s[:, :, 0] != M.EMPTY]
    assert ((live[:, 0] & M.ID_MASK) != (live[:, 2] & M.ID_MASK)).all()
    # runs: one and two buckets on, and across the wrap
    assert [root(k)[0] - B_RUN for k in w["run"]] == [0, 0, 0, 0, 1, 1, 1, 1, 2]
    assert root(w["run"][7])[1] == 3 and root(w["run"][8])[1] == 0 and not t.full(B_RUN + 2)
    assert [root(k)[:2] for k in w["wrap"]] == [(B_LAST, 0), (B_LAST, 1), (B_LAST, 2), (B_LAST, 3), (0, 0), (0, 1)]
    # misses
    for word, reads in w["absent"].values():
        wid = M.word_id(eng, word)
        assert wid >= 4
        r = t.run(M.ROOT, wid, w["max_probe"])
        assert not r.found and r.reads == reads, (word, reads, r)
    assert t.full(B_FULL) and not t.full(B_FULL + 1) and t.full(B_RUN) and t.full(B_RUN + 1) and t.full(B_LAST)
    assert M.home_bucket(M.ROOT, M.word_id(eng, w["absent"]["wrap"][0])) == B_LAST
    return t


def test_world_has_the_shape_it_claims():
    eng = Engine(device=-1)
    w = quad_world(eng)
    t = check_quad_world(eng, w)
    # every kind of end a run can take occurs among the topics' probes
    ends = set()
    for ids, dollar in M.topic_ids(eng, w["topics"]):
        for p, wd, r in t.walk(ids, dollar, w["max_probe"])[1]:
            ends.add((r.found, r.disp))
    assert {(True, 0), (True, 1), (True, 2), (False, 0), (False, 1), (False, 2)} <= ends, ends
    eng.close()


class Checker:
    """The oracle over the world's filters: rows and counters of any batch."""

    def __init__(self, F):
        self.F = F
        self.orc = P.Oracle()
        for f in F:
            self.orc.register(f)
            self.orc.insert(f)

    def batch(self, T):
        buf, offs = P.pack(T)
        counts, idx, st = self.orc.match_batch(buf, offs, nthreads=2)
        cut = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        return [[self.F[int(j)] for j in idx[cut[i]:cut[i + 1]]] for i in range(len(T))], st


def device_rows(eng, T):
    b = eng.prepare(T)
    b.launch().wait()
    offs, ids = b.result()
    st = b.stats()
    b.free()
    cache = {}
    rows = [[cache.setdefault(int(i), eng.filter_bytes(int(i))) for i in ids[offs[k]:offs[k + 1]]]
            for k in range(len(offs) - 1)]
    return rows, st, len(ids)


def differing(T, got, exp):
    return [(T[i], got[i][:4], exp[i][:4]) for i in range(len(T)) if got[i] != exp[i]][:3]


@pytest.fixture(scope="module")
def world():
    eng = Engine(device=0)
    w = quad_world(eng)
    eng.sync()
    table = check_quad_world(eng, w)
    return eng, w, table, Checker(w["filters"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_rows_reads_and_counters(world, n):
    eng, w, table, chk = world
    U = w["topics"]
    # the larger batches start at another topic in every tile, so that a
    # tile's pops mix the kinds
    T = U[:n] if n <= len(U) else [U[(i + i // 16) % len(U)] for i in range(n)]
    assert tile_topics(n) == {512: 2, 1024: 4, 4096: 16}.get(n, 1)
    exp, ost = chk.batch(T)
    assert eng.debug_check() <= M.MAX_PROBE_DISP
    got, st, n_ids = device_rows(eng, T)
    assert not differing(T, got, exp)
    assert st["slow_topics"] == 0 and st["overflow_tiles"] == 0
    want = M.batch_reads(eng, table, T, w["max_probe"])
    print("n", n, "probes", st["probes"], "table-driven", want,
          {k: (st[k], ost[k]) for k in ("visits", "hash_hits", "words", "matches")})
    assert st["probes"] == want
    assert st["matches"] == ost["matches"] == n_ids == sum(len(r) for r in exp)
    assert st["visits"] == ost["visits"] and st["hash_hits"] == ost["hash_hits"] and st["words"] == ost["words"]


@pytest.mark.gpu
def test_a_tile_that_overflows_the_stack_leaves_by_the_early_exit():
    """16 topics of 8 words whose every level matches literally and by '+':
    a 16-topic tile holds 32, 64, 128, ... 384 probes and would push 448 at
    level 8, more than the 384-entry stack: the loop is left with entries
    written above the popped ones, and the tile's topics take the generic
    path (rows of 256 = 2 K entries)."""
    words = [b"g%d" % i for i in range(7)]
    U = [b"/".join(words + [b"end%02d" % i]) for i in range(16)]
    F = set()
    for t in U:
        ws = t.split(b"/")
        for mask in itertools.product((0, 1), repeat=8):
            F.add(b"/".join(b"+" if m else x for m, x in zip(mask, ws)))
    F = sorted(F)
    assert len(F) == 128 * 17
    T = U * 256
    assert len(T) == 4096 and tile_topics(len(T)) == 16
    eng = Engine(device=0)
    eng.insert_many(F)
    eng.sync()
    chk = Checker(F)
    exp, ost = chk.batch(U)
    assert all(len(r) == 256 for r in exp)
    got, st, n_ids = device_rows(eng, T)
    assert st["overflow_tiles"] == len(T) and st["slow_topics"] == len(T)
    assert not differing(T, got, exp * 256)
    assert st["matches"] == n_ids == 256 * ost["matches"]
    eng.close()
