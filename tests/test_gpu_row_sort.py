"""The tile epilogue's row sort against the oracle, through the C ABI -- needs
an MI355X.

A row of the fast walk is sorted either on 32-bit tagged keys (the path code's
high word with the entry's index in its free low bits) or, when the chunk's
codes reach too deep for the row's size class, by the u64 network.  Which one
runs depends on the deepest level any entry of the chunk emitted at, so the
batch below holds rows of every size-class edge at every depth tier, in tiles
that are all shallow and in tiles where one deep topic makes the whole tile
fall back.  One engine, one oracle run and one batch serve every test here.

Construction (as test_long_rows_every_generic_sort): for a topic of d unique
words the filters are seeded subsets of all literal/'+' masks at full depth,
the same masks with a trailing '#', and masks with '#' replacing the last
level; the first level stays literal so a topic's filters match it alone.  A
code's digit for level l sits at bit 61 - 3l; with words that sort above '+'
the digits are literal 4, '+' 3, '#' 2:

    tier   topic        deepest emitted level   free bits   tagged classes
    d7B    7 words, #   7                       8           all
    d8B    8 words, #   8 (digit 2)             6           all
    d9     9 words      8 (digit 3)             5           W <= 32
    d9B    9 words, #   9 (digit 2)             3           W <= 8
    d10    10 words     9 (digit 3)             2           W <= 4
    d10B   10 words, #  10                      0           none (u64)
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
LENGTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 100, 128, 129)
TIERS = (("d7B", 7, True), ("d8B", 8, True), ("d9", 9, False), ("d9B", 9, True), ("d10", 10, False),
         ("d10B", 10, True))
TILE = 64
STAGE = 1024      # u64 entries of a chunk: (384 stack entries * 16 B + 512 words * 4 B) / 8
ROW_CAP = 128     # default K

EDGE_FILTERS = [b"a//b", b"a/+/b", b"a//#", b"a/#", b"a/", b"a/+", b"a/+/#", b"a",
                b"P/", b"P/#", b"P/+", b"P",
                b"$SYS/#", b"$SYS/+/x", b"$SYS/b/x", b"$SYS/b/+", b"$SYS/+", b"+/+", b"+/+/+",
                b"q/#", b"q/+", b"q/#/b", b"q/#/#", b"q/+/#", b"q/+/+"]
EDGE_TOPICS = [b"a//b", b"a/", b"a", b"a/x", b"P/", b"P", b"P/y",
               b"$SYS/b/x", b"$SYS/b", b"$SYS/c/x",
               b"q/+", b"q/#", b"q/#/b", b"q/+/c", b"q/#/#"]


def min_tiles():
    """TM_MIN_TILES of the kernels: tile_topics(n) halves the tile until the
    batch has this many tiles."""
    src = open(os.path.join(ROOT, "emqx_amd", "csrc", "tm_kernels.hip")).read()
    return int(re.search(r"#define TM_MIN_TILES (\d+)", src).group(1))


def tile_topics(n):
    tt = 64
    while tt > 1 and (n + tt - 1) // tt < min_tiles():
        tt >>= 1
    return tt


def family(ws, with_hash):
    """-> (filters that emit at the tier's deepest level, the others)."""
    d = len(ws)
    full, tail, last = [], [], []
    for mask in itertools.product((0, 1), repeat=d - 1):
        lv = [ws[0]] + [b"+" if m else w for m, w in zip(mask, ws[1:])]
        full.append(b"/".join(lv))
        tail.append(b"/".join(lv + [b"#"]))
        last.append(b"/".join(lv[:-1] + [b"#"]))
    last = sorted(set(last))
    if with_hash:
        return tail, full + last
    plus_last = [f for f in full if f.endswith(b"/+")]    # digit 3 at the last level
    return plus_last, [f for f in full if not f.endswith(b"/+")] + last


def chunks_of(lengths):
    """Chunks the epilogue takes for a tile with these row lengths (whole rows, <= STAGE entries)."""
    n, fill = 0, 0
    for c in lengths:
        c = c if c <= ROW_CAP else 0    # a row past K leaves the tile for the generic path
        if n == 0 or fill + c > STAGE:
            n, fill = n + 1, 0
        fill += c
    return n


class World:
    pass


def build_world():
    """The filters, the batch and the oracle's rows (no GPU)."""
    rng = random.Random(7)
    w = World()
    F = set(EDGE_FILTERS)
    U = []                       # unique topics
    w.tier_topics = {}           # tier -> indices into U, one per length in LENGTHS
    for name, d, with_hash in TIERS:
        idx = []
        for L in LENGTHS:
            ws = [b"%s_%d_w%d" % (name.encode(), L, i) for i in range(d)]
            deep, rest = family(ws, with_hash)
            pick = [rng.choice(deep)]
            pick += rng.sample(sorted(set(deep + rest) - set(pick)), L - 1)
            assert len(set(pick)) == L
            F.update(pick)
            idx.append(len(U))
            U.append(b"/".join(ws))
        w.tier_topics[name] = idx
    w.edge = list(range(len(U), len(U) + len(EDGE_TOPICS)))
    U += EDGE_TOPICS
    F = sorted(F)

    shallow = w.tier_topics["d7B"]
    blocks, kinds = [], []

    def block(kind, members):
        assert len(members) == TILE
        blocks.append(members)
        kinds.append(kind)

    for name, _, _ in TIERS:                       # tiles of one tier, rows on two sets of lanes
        tt = w.tier_topics[name]
        for rot in (0, 5):
            block("aligned:" + name, [tt[(i + rot) % len(tt)] for i in range(TILE)])
    short = [t for t, L in zip(shallow, LENGTHS) if L <= 9]
    block("short", [short[i % len(short)] for i in range(TILE)])
    for name, _, _ in TIERS[1:]:                   # one deeper topic among shallow ones
        for j, deep_t in enumerate(w.tier_topics[name]):
            m = [shallow[(i + j) % len(shallow)] for i in range(TILE)]
            m[(7 * j + 3) % TILE] = deep_t
            block("mixed:" + name, m)
    for rot in (0, 1):                             # edge topics among shallow rows, and alone
        block("edge", [(w.edge + shallow)[(i + rot) % (len(w.edge) + len(shallow))] for i in range(TILE)])
    block("edge", [w.edge[i % len(w.edge)] for i in range(TILE)])
    reps = -(-min_tiles() // len(blocks))
    blocks, kinds = blocks * reps, kinds * reps
    w.blocks, w.kinds = blocks, kinds
    order = [t for b in blocks for t in b]
    w.order = np.asarray(order)
    T = [U[t] for t in order]

    orc = P.Oracle()
    for f in F:
        orc.register(f)
        orc.insert(f)
    buf, offs = P.pack(U)
    counts, idx, _ = orc.match_batch(buf, offs, nthreads=4)
    orc.close()
    cut = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    w.exp = [np.asarray(idx[cut[i]:cut[i + 1]], dtype=np.int64) for i in range(len(U))]   # indices into F
    w.U, w.F, w.T = U, F, T
    return w


@pytest.fixture(scope="module")
def world():
    w = build_world()
    F, T = w.F, w.T
    eng = Engine(device=0)
    eng.insert_many(F)
    eng.sync()
    roffs, ids = eng.match_batch(T)
    to_f = np.full(int(ids.max()) + 1, -1, dtype=np.int64)
    findex = {f: i for i, f in enumerate(F)}
    for i in np.unique(ids):
        to_f[int(i)] = findex[eng.filter_bytes(int(i))]
    w.got_offs = np.asarray(roffs, dtype=np.int64)
    w.got = to_f[ids]
    return w


def mismatches(w, which):
    bad = []
    for r in which:
        got = w.got[w.got_offs[r]:w.got_offs[r + 1]]
        exp = w.exp[w.order[r]]
        if not np.array_equal(got, exp):
            bad.append((r, w.kinds[r // TILE], w.T[r], [w.F[i] for i in got[:4]], [w.F[i] for i in exp[:4]]))
    return bad


def rows_of_kind(w, prefix):
    return [b * TILE + i for b, k in enumerate(w.kinds) if k.startswith(prefix) for i in range(TILE)]


def test_oracle_rows_cover_every_length_in_every_tier(world):
    w = world
    for name, _, _ in TIERS:
        assert [len(w.exp[t]) for t in w.tier_topics[name]] == list(LENGTHS), name
    # the K + 1 row is the generic path's, with the default K
    assert ROW_CAP + 1 in LENGTHS and os.environ.get("TM_ROWCAP") is None


def test_tiles_hold_64_topics_and_take_one_two_and_three_chunks(world):
    w = world
    assert tile_topics(len(w.T)) == TILE and len(w.T) % TILE == 0
    per_tile = [chunks_of([len(w.exp[t]) for t in b]) for b in w.blocks]
    assert {1, 2, 3} <= set(per_tile), sorted(set(per_tile))


@pytest.mark.parametrize("tier", [t[0] for t in TIERS])
def test_tiles_of_one_tier(world, tier):
    rows = rows_of_kind(world, "aligned:" + tier)
    assert rows and not mismatches(world, rows)


@pytest.mark.parametrize("tier", [t[0] for t in TIERS[1:]])
def test_one_deep_topic_among_shallow_ones(world, tier):
    rows = rows_of_kind(world, "mixed:" + tier)
    assert rows and not mismatches(world, rows)


def test_short_rows_single_chunk(world):
    rows = rows_of_kind(world, "short")
    assert rows and not mismatches(world, rows)


def test_edge_topics(world):
    """'' words (a//b, a trailing a/, P/ beside P/#), a $SYS topic, literal '+' and '#' words."""
    w = world
    rows = rows_of_kind(w, "edge")
    assert not mismatches(w, rows)
    by_topic = {w.U[t]: [w.F[i] for i in w.exp[t]] for t in w.edge}
    assert by_topic[b"P/"] == sorted([b"P/", b"P/#", b"P/+", b"+/+"])
    assert by_topic[b"$SYS/b"] == [b"$SYS/#", b"$SYS/+"]
    assert by_topic[b"a//b"] == sorted([b"a//b", b"a/+/b", b"a//#", b"a/#", b"a/+/#", b"+/+/+"])


def test_whole_batch(world):
    assert not mismatches(world, range(len(world.T)))[:3]
