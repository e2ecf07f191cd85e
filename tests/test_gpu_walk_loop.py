"""The tile walk's frontier loop against the oracle, through the C ABI -- needs
an MI355X.

The loop pops up to 64 probes per iteration; lanes without a probe ride along
on lane 0's entry, the quads report through the popped entries, continuations
re-push a probe whose key spilled past its home bucket, and a free last slot
ends a run.  Every case below compares the device's rows (filter bytes, in
order) with the oracle's on small worlds, each built once per module:

    edge      partial tiles (1 / 63 / 64 / 65 topics), $-topics, literal '#' and
              '+' last words, '' words, unknown words, depth 10 and 11
    probe     a table grown (seeded, filter by filter on the host) until some
              key sits two buckets from home: continuations and tail marks
    fan       seven levels matched by the literal and by '+' at every level
    rowcap    TM_ROWCAP = 4: rows of exactly K and K + 1 entries
    dedup     a TM_BATCH_DEDUP batch whose device-counted rows shrink the tile
"""

import itertools
import os
import random
import re

import numpy as np
import pytest

from emqx_amd.engine import Engine
from oracle import pyoracle as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QCAP = 384       # probe stack entries of the production walk
ROW_CAP = 128    # default K


def min_tiles():
    src = open(os.path.join(ROOT, "emqx_amd", "csrc", "tm_kernels.hip")).read()
    return int(re.search(r"#define TM_MIN_TILES (\d+)", src).group(1))


def tile_topics(n):
    tt = 64
    while tt > 1 and (n + tt - 1) // tt < min_tiles():
        tt >>= 1
    return tt


def oracle_rows(F, U):
    """Rows of the distinct topics U as lists of filter bytes (F: duplicate-free list)."""
    orc = P.Oracle()
    for f in F:
        orc.register(f)
        orc.insert(f)
    buf, offs = P.pack(U)
    counts, idx, _ = orc.match_batch(buf, offs, nthreads=4)
    orc.close()
    cut = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    return [[F[int(j)] for j in idx[cut[i]:cut[i + 1]]] for i in range(len(U))]


def device_rows(eng, T, batch=None):
    """Rows of the batch T as lists of filter bytes, and the batch's stats."""
    b = batch or eng.prepare(T)
    b.launch().wait()
    offs, ids = b.result()
    st = b.stats()
    cache = {}
    rows = [[cache.setdefault(int(i), eng.filter_bytes(int(i))) for i in ids[offs[k]:offs[k + 1]]]
            for k in range(len(offs) - 1)]
    if batch is None:
        b.free()
    return rows, st


def differing(T, got, exp):
    return [(T[i], got[i][:4], exp[i][:4]) for i in range(len(T)) if got[i] != exp[i]][:3]


# ---- edge world ------------------------------------------------------------------------------

DEEP = [b"d%d" % i for i in range(11)]
EDGE_FILTERS = [
    b"#", b"+", b"+/+", b"+/#", b"/", b"/#", b"+/", b"/+", b"a/", b"a//b", b"a/+/b", b"a//#", b"a/#", b"a/+", b"a",
    b"a/+/#", b"$SYS/#", b"$SYS/+/x", b"$SYS/b/x", b"$SYS/b/+", b"$SYS/+", b"$SYS", b"+/b/x",
    b"q/#", b"q/+", b"q/#/b", b"q/#/#", b"q/+/#", b"q/+/+", b"q/+/b",
    b"known/word", b"known/+/tail", b"known/#",
    b"/".join(DEEP[:10]), b"/".join(DEEP[:9] + [b"+"]), b"/".join(DEEP[:9] + [b"#"]), b"/".join(DEEP[:10] + [b"#"]),
    b"/".join(DEEP), b"/".join(DEEP[:10] + [b"+"]), b"d0/#", b"d0/+/d2/#",
]
EDGE_TOPICS = [
    b"a//b", b"/", b"a/", b"a", b"a/x", b"//", b"",
    b"$SYS/b/x", b"$SYS/b", b"$SYS/c/x", b"$SYS", b"$other/b/x",
    b"q/#", b"q/+", b"q/#/b", b"q/+/c", b"q/#/#", b"q/x/#", b"q/x/+",
    b"known/nope", b"nope/word", b"known/nope/tail", b"nope", b"nope/nope/nope",
    b"/".join(DEEP[:10]), b"/".join(DEEP), b"/".join(DEEP[:9]), b"/".join(DEEP[:9] + [b"zz"]),
]
assert len(EDGE_TOPICS) < 63


@pytest.fixture(scope="module")
def edge():
    rng = random.Random(11)
    words = [b"w%d" % i for i in range(12)]
    F = set(EDGE_FILTERS)
    while len(F) < 400:          # background: random 1..4-level filters over a small alphabet
        lv = [rng.choice(words + [b"+"]) for _ in range(rng.randint(1, 4))]
        if rng.random() < 0.2:
            lv.append(b"#")
        F.add(b"/".join(lv))
    F = sorted(F)
    U = list(EDGE_TOPICS)
    while len(U) < 65:
        t = b"/".join(rng.choice(words) for _ in range(rng.randint(1, 4)))
        if t not in U:
            U.append(t)
    eng = Engine(device=0)
    eng.insert_many(F)
    eng.sync()
    return eng, F, U, oracle_rows(F, U)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_partial_tiles(edge, n):
    """Batches of 1, 63, 64 and 65 topics: tile_topics < 64 and a last tile
    with idle lanes.  The first topics are the edge topics, so every one of
    them is walked in each size (n = 1: 'a//b' alone)."""
    eng, F, U, exp = edge
    assert tile_topics(n) < 64
    got, _ = device_rows(eng, U[:n])
    assert not differing(U[:n], got, exp[:n])


def test_edge_rows_are_what_the_reference_gives(edge):
    """The oracle's own rows for the edge topics, spelled out: '' words, a
    $-topic (no root '+' / '#'), literal '#' and '+' last words, unknown words."""
    _, F, U, exp = edge
    row = dict(zip(U, exp))
    assert row[b"a//b"] == sorted([b"#", b"+/#", b"a/#", b"a/+/#", b"a//#", b"a//b", b"a/+/b"])
    assert row[b"/"] == sorted([b"#", b"+/#", b"+/+", b"/", b"/#", b"+/", b"/+"])
    assert row[b"a/"] == sorted([b"#", b"+/#", b"+/+", b"+/", b"a/", b"a/#", b"a/+", b"a/+/#", b"a//#"])
    assert row[b"$SYS/b/x"] == sorted([b"$SYS/#", b"$SYS/+/x", b"$SYS/b/x", b"$SYS/b/+"])
    assert row[b"$SYS"] == sorted([b"$SYS", b"$SYS/#"])
    assert row[b"$other/b/x"] == []
    assert row[b"q/#"] == sorted([b"#", b"+/#", b"+/+", b"q/#", b"q/#/#", b"q/+", b"q/+/#"])
    assert row[b"q/+"] == sorted([b"#", b"+/#", b"+/+", b"q/#", b"q/+", b"q/+/#"])
    assert row[b"q/#/b"] == sorted([b"#", b"+/#", b"q/#", b"q/#/#", b"q/#/b", b"q/+/#", b"q/+/+", b"q/+/b"])
    assert row[b"known/nope"] == sorted([b"#", b"+/#", b"+/+", b"known/#"])
    assert row[b"nope/nope/nope"] == sorted([b"#", b"+/#"])
    assert b"/".join(DEEP[:10]) in row[b"/".join(DEEP[:10])] and b"/".join(DEEP) in row[b"/".join(DEEP)]


def test_depth_10_is_walked_by_tiles_and_depth_11_is_flagged_slow(edge):
    eng, F, U, exp = edge
    d10, d11 = b"/".join(DEEP[:10]), b"/".join(DEEP)
    pad = U[len(EDGE_TOPICS):][:30]       # background topics: none is flagged slow
    got, st = device_rows(eng, [d10] + pad)
    assert st["slow_topics"] == 0 and not differing([d10] + pad, got, [exp[U.index(t)] for t in [d10] + pad])
    got, st = device_rows(eng, [d11] + pad)
    assert st["slow_topics"] == 1 and not differing([d11] + pad, got, [exp[U.index(t)] for t in [d11] + pad])


# ---- probe runs past the home bucket ---------------------------------------------------------

@pytest.fixture(scope="module")
def probe():
    """Seeded filters go in, 500 at a time, until the host's table check
    (tm_debug_check, CPU) reports a key two or more buckets from home."""
    rng = random.Random(5)
    words = [b"p%d" % i for i in range(40)]
    eng = Engine(device=0)
    F, seen, disp = [], set(), 0
    while disp < 2 and len(F) < 20000:
        chunk = []
        while len(chunk) < 500:
            lv = [rng.choice(words) if rng.random() < 0.8 else b"+" for _ in range(rng.randint(2, 5))]
            if rng.random() < 0.15:
                lv.append(b"#")
            f = b"/".join(lv)
            if f not in seen:
                seen.add(f)
                chunk.append(f)
        eng.insert_many(chunk)
        F += chunk
        eng.sync()
        disp = eng.debug_check()
    # topics that walk the filters' own edges, and ones that leave them half way
    T = []
    for f in rng.sample(F, min(len(F), 3000)):
        lv = [w if w not in (b"+", b"#") else rng.choice(words) for w in f.split(b"/")]
        T.append(b"/".join(lv))
        if len(T) % 3 == 0:
            T.append(b"/".join(lv[:-1] + [rng.choice(words)]))
    T = T[:4096]
    U = sorted(set(T))
    F = sorted(F)
    return eng, F, T, dict(zip(U, oracle_rows(F, U))), disp


def test_continuations_and_tail_marks(probe):
    eng, F, T, exp, disp = probe
    assert disp >= 2 and len(F) <= 20000, (disp, len(F))
    got, st = device_rows(eng, T)
    assert not differing(T, got, [exp[t] for t in T])


# ---- a frontier that outgrows the stack ------------------------------------------------------

FAN_WORDS = [b"f%d" % i for i in range(6)]


@pytest.fixture(scope="module")
def fan():
    """64 topics f0/../f5/last_i; all 2^7 literal / '+' masks of each: every
    level matches both ways, 128 = K matches per topic."""
    U = [b"/".join(FAN_WORDS + [b"last%02d" % i]) for i in range(64)]
    F = set()
    for t in U:
        ws = t.split(b"/")
        for mask in itertools.product((0, 1), repeat=7):
            F.add(b"/".join(b"+" if m else w for m, w in zip(mask, ws)))
    F = sorted(F)
    assert len(F) == 64 * 64 + 64
    eng = Engine(device=0)
    eng.insert_many(F)
    eng.sync()
    exp = oracle_rows(F, U)
    assert all(len(r) == ROW_CAP for r in exp)
    return eng, F, U, exp


def test_full_tiles_overflow_the_stack_and_take_the_generic_path(fan):
    """A 64-topic tile starts with 128 probes and gains 64 per iteration: 448 >
    384 entries at level 6, so the whole tile goes to the generic path.  Tiles
    hold 64 topics only from 64 * TM_MIN_TILES topics on, hence this one large
    batch (the 64 distinct topics, repeated; the oracle walks the 64)."""
    eng, F, U, exp = fan
    reps = min_tiles()
    T = U * reps
    assert tile_topics(len(T)) == 64
    got, st = device_rows(eng, T)
    # (overflow_tiles counts the topics that tiles handed to the generic path)
    assert st["overflow_tiles"] == len(T) and st["slow_topics"] == len(T)
    assert not differing(T, got, exp * reps)


def test_16_topic_tiles_fill_the_stack_to_the_brim(fan):
    """4,096 topics make 16-topic tiles: 32 probes at level 1, 64 at level 2,
    then + 64 per iteration up to 256 + 128 = 384 = QCAP at level 7, which
    still fits: no tile overflows."""
    eng, F, U, exp = fan
    T = U * 64
    assert len(T) == 4096 and tile_topics(len(T)) == 16
    got, st = device_rows(eng, T)
    assert st["overflow_tiles"] == 0 and st["slow_topics"] == 0
    assert not differing(T, got, exp * 64)


# ---- the row stop ----------------------------------------------------------------------------

def test_rows_of_exactly_k_and_k_plus_one_entries():
    """TM_ROWCAP = 4: a row of K entries stays with the tile walk, a row of
    K + 1 goes to the generic path whole; both equal the oracle's."""
    K = 4
    os.environ["TM_ROWCAP"] = str(K)
    try:
        eng = Engine(device=0)
    finally:
        del os.environ["TM_ROWCAP"]
    F, U = [], []
    for i in range(40):
        a, b, c = b"r%da" % i, b"r%db" % i, b"r%dc" % i
        F += [b"/".join(x) for x in ((a, b, c), (a, b"+", c), (a, b, b"+"), (a, b"+", b"+"))]
        if i % 2:
            F.append(a + b"/#")           # the K + 1st
        if i % 4 == 3:
            F.append(a + b"/" + b + b"/#")   # K + 2
        U.append(b"/".join((a, b, c)))
    F = sorted(F)
    eng.insert_many(F)
    eng.sync()
    exp = oracle_rows(F, U)
    assert sorted(set(map(len, exp))) == [K, K + 1, K + 2]
    got, st = device_rows(eng, U)
    assert not differing(U, got, exp)
    assert st["slow_topics"] == sum(len(r) > K for r in exp)


# ---- device-counted rows ---------------------------------------------------------------------

def test_dedup_batch_whose_rows_shrink_the_tile(edge):
    """4,096 publishes of 65 distinct topics: the grid is sized for 4,096 rows,
    the device counts 65 and shrinks the tiles to one topic each."""
    eng, F, U, exp = edge
    rng = random.Random(3)
    pubs = U + [rng.choice(U) for _ in range(4096 - len(U))]
    b = eng.prepare(pubs, dedup=True)
    got, st = device_rows(eng, pubs, batch=b)
    row_of, n_rows = b.row_map()
    b.free()
    assert n_rows == len(U) and len(got) == n_rows
    for i, r in enumerate(row_of.tolist()):
        assert got[r] == exp[U.index(pubs[i])], pubs[i]
