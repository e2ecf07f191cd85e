"""The walk epilogue's row sort, four tagged keys per lane, at its edges,
against the oracle -- the device cases need an MI355X; the world's shape is
proved on the host.

A tile's 64 rows are sorted by size class.  With TM_SORT_KPL = 4 a row of c
entries whose chunk has `free` >= log2(W) zero low bits in every code's high
word sorts as tagged u32 keys, element e in lane e / 4, register e % 4:

    c = 1          stored directly
    c = 2..4       W = 4, inside the row's own lane (64 rows a pass)
    c = 5..16      W = 16, four lanes a row (16 rows a pass)
    c = 17..32     W = 32, 8 lanes (8 rows a pass)
    c = 33..64     W = 64, 16 lanes (4 rows a pass)
    c = 65..128    W = 128, 32 lanes (2 rows a pass)
    c > 128        the row leaves the fast path (TM_ROWCAP = 128)

and a class with log2(W) > free takes the u64 network (the rank count for
65..128) as before.  `free` of a chunk is the number of zero bits of the
codes' high words below the lowest digit any of its entries carries.  The
topic's word i (from 0) puts its digit at level i, a '#' after p words at
level p, and the digit of level l sits at bit key_shift(l) = 61 - 3 l of the
64-bit code; with words that sort above '+' the digits are literal 4, '+' 3,
'#' 2 (tests/test_gpu_row_sort.py has the same table):

    tier   topic         deepest level (digit)   free   tagged classes
    d7     7 words       6                       8      all (C2's shape)
    d9     9 words       8 ('+': 3)              5      W <= 32; 64 and 128 u64 in the same chunk
    d10    10 words      9 ('+': 3)              2      only the in-lane class
    d10B   10 words, #   10 ('#': 2)             0      none: bit 31, the level-10 digit's
                                                        lowest, is part of the code

The world: every topic has words of its own at every level (so its first word
is its own and rows are independent), and exactly c filters, the first c of a
fixed list of the literal / '+' / '#' patterns over its words that keep at
least one literal.  The list starts with the filters that carry the tier's
deepest digit (the all-literal one and the one with '+' at the last level; in
d10B all ten words and '#'), so every row of two or more entries holds it,
then goes on with the fewest '+' first, so that small rows have thin tries.
A row of 128 needs '+' at the first level too: with the first word literal a
topic of 7 words has only 127 filters of depth <= 7.

One batch of 256 tiles of 64 topics holds every case tile (repeated to fill
the batch); it is matched once and every row compared, in order, with the
oracle's.  Two shorter batches cut the same topics into tiles of 32 and leave
a last tile with fewer topics than lanes.
"""

import itertools
import os
import re
from dataclasses import replace

import numpy as np
import pytest

from emqx_amd.engine import Engine
from oracle import pyoracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 64
STAGE = 1024          # staged entries per chunk (TileLds<384>::STAGE)
ROWCAP = 128
EDGES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129]
# (lo, hi, rows per pass) of the tagged classes at four keys per lane: 64 * 4 / W
CLASSES = {4: (2, 4, 64), 16: (5, 16, 16), 32: (17, 32, 8), 64: (33, 64, 4), 128: (65, 128, 2)}


def source():
    return open(os.path.join(ROOT, "emqx_amd", "csrc", "tm_kernels.hip")).read()


def min_tiles():
    return int(re.search(r"#define TM_MIN_TILES (\d+)", source()).group(1))


def tile_topics(n):
    tt = TILE
    while tt > 1 and (n + tt - 1) // tt < min_tiles():
        tt >>= 1
    return tt


def key_shift(level):
    return 61 - 3 * level


DIGIT = {"literal": 4, "+": 3, "#": 2}     # of a word that sorts above '+' (dig_L / dig_P / dig_H, class C_ABOVE)


def free_of(level, digit):
    """`free` of a chunk whose lowest code bit is `digit`'s lowest at `level`
    (sort_rows_log: tz of the codes' bits 31..62 or-ed, capped at 9, minus 1,
    floor 0)."""
    low = key_shift(level) + (digit & -digit).bit_length() - 1
    tz = min(max(low - 31, 0), 9)
    return tz - 1 if tz else 0


def deepest(pattern):
    """(level, digit) of the lowest digit of a filter's code."""
    mask, hsh = pattern
    if hsh:
        return len(mask), DIGIT["#"]
    return len(mask) - 1, DIGIT["+" if mask[-1] else "literal"]


def patterns(depth, tail):
    """The filters of a topic of `depth` words, as (mask, hash): mask[i] = 1
    puts '+' at level i, hash ends the filter with '#' after len(mask) levels
    (after all `depth` of them only with `tail`).  At least one literal."""
    out = []
    for p in range(1, depth + 1):
        for mask in itertools.product((0, 1), repeat=p):
            if all(mask):
                continue
            if p == depth:
                out.append((mask, False))
            if p < depth or tail:
                out.append((mask, True))
    head = [((0,) * depth, False), ((0,) * (depth - 1) + (1,), False)]
    if tail:
        head = [((0,) * depth, True)] + head
    rest = sorted((x for x in out if x not in head), key=lambda x: (sum(x[0]), -len(x[0]) - x[1], x[0]))
    return head + rest


# tier -> (words of a topic, '#' after the last word too, free of a chunk that holds the tier's deepest digit)
TIERS = {"d7": (7, False, 8), "d9": (9, False, 5), "d10": (10, False, 2), "d10B": (10, True, 0)}
PATTERNS = {t: patterns(d, tail) for t, (d, tail, _) in TIERS.items()}
assert len(PATTERNS["d7"]) == 247 and all(len(m) + h <= 7 for m, h in PATTERNS["d7"])


def spread(rows, fill):
    """A tile's 64 row sizes: `rows` at lanes spread over the tile, lane 0 and
    lane 63 among them when there are two or more; the other lanes take the
    sizes of `fill` in turn."""
    n = len(rows)
    at = [0] if n == 1 else sorted({(i * 63) // (n - 1) for i in range(n)})
    assert len(at) == n
    tile, f = [None] * TILE, itertools.cycle(fill)
    for lane, c in zip(at, rows):
        tile[lane] = c
    return [next(f) if c is None else c for c in tile]


def class_rows(W, n):
    lo, hi, _ = CLASSES[W]
    return [(hi, lo, (lo + hi) // 2, hi - 1)[i % 4] for i in range(n)]


def case_tiles():
    """{name: (tier, the 64 row sizes)}"""
    small = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33]
    mixed = EDGES[:-1] + small * 4 + [2, 3, 4, 1]
    T = {"edges": ("d7", EDGES + [0, 1] * 23 + [0])}
    for W, (lo, hi, per) in CLASSES.items():
        for n in sorted({1, per, min(per + 1, TILE)}):
            T[f"class{W}_rows{n}"] = ("d7", spread(class_rows(W, n), [0, 1]))
    T["whole_c4"] = ("d7", [4] * TILE)
    T["whole_c32"] = ("d7", [32] * TILE)
    T["mixed"] = ("d7", mixed)
    # two chunks: 128 first in chunk 1, 64 last in it and filling it to the last place; 65 first and 128 last in chunk 2
    T["chunks2"] = ("d7", [128] + [32] * 26 + [64] + [65] + [16] * 34 + [128])
    # three chunks: chunk 1 one entry short of full (127 first); chunk 2 from 128 to 64, full; chunk 3 from 65 to 128
    T["chunks3"] = ("d7", [127] + [32] * 28 + [128] + [32] * 26 + [64] + [65] + [4] * 5 + [128])
    for tier in ("d9", "d10", "d10B"):
        T[f"{tier}_mixed"] = (tier, mixed)
    for tier, t in T.values():
        assert len(t) == TILE and max(t) <= len(PATTERNS[tier])
    return T


def chunks(tile):
    """The rows of each chunk of a tile (sort_rows_log: whole rows while the sum stays <= STAGE)."""
    out, cur = [], []
    for c in (c if c <= ROWCAP else 0 for c in tile):
        if sum(cur) + c > STAGE:
            out.append(cur)
            cur = []
        cur.append(c)
    return out + [cur]


class World:
    def __init__(self):
        self.cases = case_tiles()
        self.names = list(self.cases)
        self.filters, self.topics, self.sizes = [], [], []
        for t, name in enumerate(self.names):
            tier, tile = self.cases[name]
            for lane, c in enumerate(tile):
                words = [b"%x.%x.%x" % (t, lane, lv) for lv in range(TIERS[tier][0])]
                self.topics.append(b"/".join(words))
                self.sizes.append(c)
                for mask, hsh in PATTERNS[tier][:c]:
                    f = [b"+" if m else w for m, w in zip(mask, words)]
                    self.filters.append(b"/".join(f + [b"#"] if hsh else f))
        self.orc = P.Oracle()
        for f in self.filters:
            self.orc.register(f)
            self.orc.insert(f)

    def batch(self, n):
        """n topics: the case tiles in order, again and again."""
        return [self.topics[i % len(self.topics)] for i in range(n)]

    def expect(self, T):
        buf, offs = P.pack(T)
        counts, idx, st = self.orc.match_batch(buf, offs, nthreads=2)
        cut = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        return [[self.filters[int(j)] for j in idx[cut[i]:cut[i + 1]]] for i in range(len(T))], st


@pytest.fixture(scope="module")
def world():
    return World()


def test_world_has_the_shape_it_claims(world):
    w = world
    assert len(set(w.filters)) == len(w.filters) and len(set(w.topics)) == len(w.topics)
    exp, _ = w.expect(w.topics)
    assert [len(r) for r in exp] == w.sizes            # exactly c filters match, no row sees another's
    sizes = {name: tile for name, (_, tile) in w.cases.items()}
    assert set(EDGES) <= set(sizes["edges"])
    for W, (lo, hi, per) in CLASSES.items():
        for n in {1, per, min(per + 1, TILE)}:
            t = sizes[f"class{W}_rows{n}"]
            assert sum(lo <= c <= hi for c in t) == n and all(c <= 1 or lo <= c <= hi for c in t)
            assert n == 1 or (lo <= t[0] <= hi and lo <= t[63] <= hi)
    assert all(any(lo <= c <= hi for c in sizes["mixed"]) for lo, hi, _ in CLASSES.values())
    c2, c3 = chunks(sizes["chunks2"]), chunks(sizes["chunks3"])
    assert [sum(c) for c in c2] == [STAGE, 65 + 16 * 34 + 128] and (c2[0][0], c2[0][-1], c2[1][0], c2[1][-1]) == (128, 64, 65, 128)
    assert [sum(c) for c in c3] == [STAGE - 1, STAGE, 65 + 20 + 128]
    assert [(c[0], c[-1]) for c in c3] == [(127, 32), (128, 64), (65, 128)]
    # the free thresholds, as tests/test_gpu_row_sort.py tabulates them: 9 words
    # give level 8 and free 5, 10 words level 9 and free 2, "10 words, #" the
    # level-10 digit and free 0
    assert free_of(6, DIGIT["+"]) == free_of(7, DIGIT["#"]) == 8 and free_of(8, DIGIT["#"]) == 6
    assert (free_of(8, DIGIT["+"]), free_of(9, DIGIT["#"]), free_of(9, DIGIT["+"])) == (5, 3, 2)
    assert free_of(10, DIGIT["#"]) == free_of(10, DIGIT["+"]) == 0
    # free of every chunk of every case tile, from the filters its rows hold:
    # the tier's in all of them, so the classes that sort tagged there are
    tagged = {}
    for name, (tier, tile) in w.cases.items():
        lane = 0
        for ch in chunks(tile):
            pats = [q for c in tile[lane:lane + len(ch)] if c <= ROWCAP for q in PATTERNS[tier][:c]]
            lane += len(ch)
            assert pats and min(free_of(*deepest(q)) for q in pats) == TIERS[tier][2], (name, tier)
        tagged[tier] = [W for W in CLASSES if W.bit_length() - 1 <= TIERS[tier][2]]
    assert tagged == {"d7": [4, 16, 32, 64, 128], "d9": [4, 16, 32], "d10": [4], "d10B": []}
    assert deepest(PATTERNS["d10B"][0]) == (10, DIGIT["#"]) and PATTERNS["d10B"][0] == ((0,) * 10, True)


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


@pytest.fixture(scope="module")
def device(world):
    eng = Engine(device=0)
    eng.insert_many(world.filters)
    eng.sync()
    n = TILE * min_tiles()
    T = world.batch(n)
    assert tile_topics(n) == TILE
    exp, ost = world.expect(T)
    got, st, n_ids = device_rows(eng, T)
    return eng, T, exp, ost, got, st, n_ids


@pytest.mark.gpu
def test_the_batch_stays_on_the_fast_path(world, device):
    """Only the rows of 129 leave for the generic path (overflow_tiles counts
    the topics sent there, for a long row or with a whole tile whose stack
    overflowed): no tile overflows its stack, and the rows compared below were
    sorted by the tile epilogue."""
    eng, T, exp, ost, got, st, n_ids = device
    long_rows = sum(1 for r in exp if len(r) > ROWCAP)
    print({k: st[k] for k in ("overflow_tiles", "slow_topics", "matches")}, "rows > 128:", long_rows)
    assert st["overflow_tiles"] == st["slow_topics"] == long_rows > 0
    assert st["matches"] == ost["matches"] == n_ids == sum(len(r) for r in exp)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(case_tiles()))
def test_every_row_of_a_case_tile(world, device, name):
    eng, T, exp, ost, got, st, n_ids = device
    k = world.names.index(name)
    seen = 0
    for t in range(k, len(T) // TILE, len(world.names)):      # every copy of the tile in the batch
        for i in range(t * TILE, (t + 1) * TILE):
            assert got[i] == exp[i], (name, t, i - t * TILE, len(exp[i]), got[i][:3], exp[i][:3])
        seen += 1
    assert seen >= 1 and [len(r) for r in exp[k * TILE:(k + 1) * TILE]] == world.cases[name][1]


@pytest.mark.gpu
@pytest.mark.parametrize("n,tt,last", [(32 * min_tiles() - 22, 32, 10), (TILE * min_tiles() - 30, 64, 34)])
def test_short_tiles_and_a_last_tile_with_idle_lanes(world, device, n, tt, last):
    eng = device[0]
    assert tile_topics(n) == tt and n - (n - 1) // tt * tt == last
    T = world.batch(n)
    exp, ost = world.expect(T)
    got, st, n_ids = device_rows(eng, T)
    bad = [(i, len(exp[i]), got[i][:3], exp[i][:3]) for i in range(n) if got[i] != exp[i]][:3]
    assert not bad
    assert st["overflow_tiles"] == st["slow_topics"] == sum(1 for r in exp if len(r) > ROWCAP)
    assert st["matches"] == ost["matches"] == n_ids


@pytest.mark.gpu
def test_a_c2_miniature_through_the_default_build():
    """A miniature of the flagship workload (C2's filter shapes, depth <= 7, so
    free = 8 and every class up to 128 is due the tagged network) through the
    library as built by default, whose source sets four keys per lane: its
    rows equal the oracle's.  Compared with the oracle only: a second library
    with -DTM_SORT_KPL=1 takes a minute to build, far more than a test may.
    Which network sorted a row cannot be read off the rows -- both give the
    same order -- so this shows the default build right on the flagship's
    shapes, not that it took the tagged classes; the listing and the phase
    cycles show that."""
    from emqx_amd import _native as N
    from emqx_amd import build as B
    from emqx_amd import gen
    m = re.search(r"#define TM_SORT_KPL (\d+)", source())
    assert m and int(m.group(1)) == 4
    assert "EMQX_TM_LIB" not in os.environ and N.lib().tm_build_info().decode().endswith("src " + B.source_hash())
    p = replace(gen.C2, n_filters=100_000, vocab=64)   # 23.5 matches a topic (C2: 24.4), 79 rows of 65..128
    filters = gen.gen_filters(p)
    flist = filters.tolist()
    assert max(f.count(b"/") + 1 for f in flist) <= 7 and free_of(6, DIGIT["+"]) == 8    # 7 levels: the last is level 6
    n = TILE * min_tiles()
    topics = gen.gen_topics(p, filters, 1000, n)
    eng = Engine(device=0)
    orc = P.Oracle()
    for f in flist:
        orc.register(f)
        orc.insert(f)
    eng.insert_many(flist)
    eng.sync()
    b = eng.prepare(topics)
    b.launch().wait()
    offs, ids = b.result()
    st = b.stats()
    b.free()
    counts, oidx, _ = orc.match_batch(topics.buf, topics.offs)
    sizes = np.diff(offs.astype(np.int64))
    assert np.array_equal(sizes, counts.astype(np.int64))
    # the rows are worth sorting: every tagged class occurs, on the fast path
    print("rows per class", {W: int(((sizes >= lo) & (sizes <= hi)).sum()) for W, (lo, hi, _) in CLASSES.items()},
          {k: st[k] for k in ("overflow_tiles", "slow_topics")})
    assert all(((sizes >= lo) & (sizes <= hi)).any() for lo, hi, _ in CLASSES.values())
    assert st["slow_topics"] < n // 10
    cache = {}
    got = [cache.setdefault(int(i), eng.filter_bytes(int(i))) for i in ids]
    assert got == [flist[int(i)] for i in oidx]
    eng.close()
