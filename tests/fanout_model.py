"""A plain host model of the device fan-out (tm_batch_dispatch: tm_fan_scan_local
/ _scan_sums / _rows / _rows_stg / _tiles / _fill / _scan_add in
emqx_amd/csrc/tm_kernels.hip) and the layouts its edge tests share.  Nothing
here needs a GPU.

The geometry restated from the source (tests/test_fanout_model.py holds the
constants against the source text):

    FAN_BLOCK        threads per block of every fan-out kernel
    FAN_PER          CONSECUTIVE match entries per scan thread (`j0 = blockIdx.x *
                     FAN_SCAN_TILE + threadIdx.x * FAN_PER`): a thread loads its ids as
                     vectors when `j0 + 16 <= n_matches` and stores its offsets as
                     vectors when `j0 + 16 <= n_matches + 1` (the sentinel entry
                     n_matches has an offset and no id)
    FAN_SCAN_TILE    entries per scan block (256 * 16); a block whose deliveries
                     exceed the engine's limit (TM_FAN_BIG) keeps u64 offsets
    FAN_FILL_TILE    deliveries per fill block (256 * 8)
    FAN_LDS_ENTRIES  entries a fill tile can stage (3/4 of the tile); a tile that
                     covers more searches the offsets per delivery
    SCNT_SAT         the 1-byte run length's saturation: 255 means "read soff"
    TICKET_GROUPS    staging regions of the rows mode's virtual entry space

A layout is a list of run lengths, one per match entry: publish j matches
exactly one literal filter, so entry j is publish j and row_off is arange.  An
entry is an int r (one of POOL pooled filters of r subscribers, taken in turn,
so equal runs alternate between distinct filters; r = 0: a filter that was
inserted and never subscribed) or a pair (key, subscriber ids) for a filter of
its own.  A pooled subscriber id encodes (run length, pool index, position in
the run), so a misplaced delivery is visible.  Filter names and subscriber ids
do not depend on the layout: one engine can hold the filters of many layouts.

Every layout of tests/test_gpu_fanout_edges.py is built here, and
tests/test_fanout_model.py checks on the CPU that each one has the shape it is
named for, so a device test cannot pass on drifted inputs.
"""

from __future__ import annotations

import itertools

import numpy as np

FAN_BLOCK = 256
FAN_PER = 16
FAN_SCAN_TILE = FAN_BLOCK * FAN_PER
FAN_FILL_PER = 8
FAN_FILL_TILE = FAN_BLOCK * FAN_FILL_PER
FAN_LDS_ENTRIES = FAN_FILL_TILE * 3 // 4
SCNT_SAT = 255
TICKET_GROUPS = 8
DEFAULT_BIG_LIMIT = 0xFFFFFFFF

POOL = 3            # distinct filters per run length
POS_BITS = 13       # a pooled run is shorter than 2^13


def pooled_name(r: int, k: int) -> bytes:
    return b"r%d/%d" % (r, k)


def pooled_subs(r: int, k: int) -> list:
    assert 0 <= r < (1 << POS_BITS) and (r * POOL + k) < (1 << (31 - POS_BITS))
    return [((r * POOL + k) << POS_BITS) | pos for pos in range(r)]


def deliveries(roff, ids, tab_off, tab):
    """The fan-out of a result CSR (roff, ids) over the subscriber table
    (tab_off[f] .. tab_off[f + 1] of tab are filter f's subscribers, in
    subscription order) -> (row offsets u64[n + 1], match offsets u64[m + 1],
    subscribers u32[D])."""
    ids = np.asarray(ids, np.int64)
    tab_off = np.asarray(tab_off, np.int64)
    runs = tab_off[ids + 1] - tab_off[ids]
    moff = np.zeros(len(ids) + 1, np.int64)
    np.cumsum(runs, out=moff[1:])
    d = int(moff[-1])
    pos = np.arange(d, dtype=np.int64) - np.repeat(moff[:-1], runs)
    out = np.asarray(tab, np.uint32)[np.repeat(tab_off[ids], runs) + pos] if d else np.zeros(0, np.uint32)
    return moff[np.asarray(roff, np.int64)].astype(np.uint64), moff.astype(np.uint64), out.astype(np.uint32)


def block_totals(moff) -> np.ndarray:
    """Deliveries of every scan block over the n_matches + 1 entries (the
    sentinel delivers nothing, and may be alone in the last block)."""
    moff = np.asarray(moff, np.int64)
    m = len(moff) - 1
    nb = (m + 1 + FAN_SCAN_TILE - 1) // FAN_SCAN_TILE
    edges = np.minimum(np.arange(nb + 1, dtype=np.int64) * FAN_SCAN_TILE, m)
    return moff[edges[1:]] - moff[edges[:-1]]


def sums_per_thread(n_matches: int) -> int:
    """tm_fan_scan_sums: block sums per thread, `per = (nb + 255) / 256`."""
    nb = (n_matches + 1 + FAN_SCAN_TILE - 1) // FAN_SCAN_TILE
    return (nb + FAN_BLOCK - 1) // FAN_BLOCK


def entry_of(moff, p) -> np.ndarray:
    """fan_upper(0, m + 1, p) - 1: the last entry whose offset is <= p, i.e.
    among equal offsets the one that has the delivery."""
    return np.searchsorted(np.asarray(moff, np.int64), p, side="right") - 1


def tiles(moff) -> np.ndarray:
    """One row (jlo, jhi, ne, staged) per fill tile.  tm_fan_tiles gives tile k
    the entry of delivery k * FAN_FILL_TILE, and one more value, the entry of
    the last delivery; a tile's jhi is the NEXT tile's jlo, so the zero-run
    entries between two tiles count for the first."""
    moff = np.asarray(moff, np.int64)
    total = int(moff[-1])
    nt = (total + FAN_FILL_TILE - 1) // FAN_FILL_TILE
    if nt == 0:
        return np.zeros((0, 4), np.int64)
    p = np.r_[np.arange(nt, dtype=np.int64) * FAN_FILL_TILE, total - 1]
    tj = entry_of(moff, p)
    ne = tj[1:] - tj[:-1] + 1
    return np.stack([tj[:-1], tj[1:], ne, (ne <= FAN_LDS_ENTRIES).astype(np.int64)], axis=1)


class Layout:
    def __init__(self, name: str, spec, mid_limit=None):
        self.name = name
        self.mid_limit = mid_limit      # a TM_FAN_BIG between the layout's block totals
        self.filters = []               # (name, subscribers) in first-use order
        index, seen = {}, {}
        fidx = []
        for e in spec:
            if isinstance(e, tuple):
                key = (b"x/" + e[0], tuple(e[1]))
            else:
                k = seen.get(e, 0) % POOL
                seen[e] = seen.get(e, 0) + 1
                key = (pooled_name(e, k), tuple(pooled_subs(e, k)))
            if key[0] not in index:
                index[key[0]] = len(self.filters)
                self.filters.append(key)
            assert self.filters[index[key[0]]] == key, "one filter, two subscriber lists"
            fidx.append(index[key[0]])
        self.fidx = np.asarray(fidx, np.int64)
        self.n = len(fidx)
        self.topics = [self.filters[f][0] for f in fidx]
        lens = np.asarray([len(s) for _, s in self.filters], np.int64)
        self.tab_off = np.r_[0, np.cumsum(lens)].astype(np.int64)
        self.tab = np.asarray([s for _, subs in self.filters for s in subs], np.uint32)
        self.runs = lens[self.fidx] if self.n else np.zeros(0, np.int64)
        self.offs, self.moff, self.out = deliveries(np.arange(self.n + 1), self.fidx, self.tab_off, self.tab)
        self.total = int(self.moff[-1])

    def block_totals(self):
        return block_totals(self.moff)

    def big(self, limit=DEFAULT_BIG_LIMIT):
        return self.block_totals() > limit

    def tiles(self):
        return tiles(self.moff)

    def inboxes(self, ids):
        """(subscribers, offsets, publishes, filter ids) by a stable sort of the
        deliveries by subscriber; `ids` are the engine's filter ids per entry."""
        entry = np.repeat(np.arange(self.n, dtype=np.int64), self.runs)
        order = np.argsort(self.out, kind="stable")
        key = self.out[order]
        d = len(key)
        heads = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if d else np.zeros(0, np.int64)
        e = entry[order]
        return (key[heads].astype(np.uint32), np.r_[heads, d].astype(np.uint32), e.astype(np.uint32),
                np.asarray(ids, np.uint32)[e])


def naive(lay: Layout):
    """The same three arrays by a loop over the publishes."""
    offs, moff, out = [0], [], []
    for j in range(lay.n):
        moff.append(len(out))
        out.extend(lay.filters[int(lay.fidx[j])][1])
        offs.append(len(out))
    moff.append(len(out))
    return np.asarray(offs, np.uint64), np.asarray(moff, np.uint64), np.asarray(out, np.uint32)


# ------------------------------------------------------------------ the layouts

SCAN_TAIL_N = [15, 16, 17, 4079, 4080, 4081, 4095, 4096, 4097, 8191, 8192, 8193]
SCAN_TAIL_CYCLE = [1, 0, 2, 1, 3, 0, 0, 1]


def scan_tail(nm: int, last_zero: bool) -> Layout:
    """n_matches around the scan thread's 16 entries and the block's 4,096: the
    last thread's vector load and vector store conditions differ at n_matches
    = 16 k + 15, and at n_matches = 4,096 k the sentinel has a block of its own."""
    runs = [SCAN_TAIL_CYCLE[j % 8] for j in range(nm)]
    runs[-1] = 0 if last_zero else (runs[-1] or 1)
    return Layout("scan-tail-%d-%s" % (nm, "zero" if last_zero else "nonzero"), runs)


SATURATION_RUNS = [254, 255, 256, 257, 510]


def saturation() -> Layout:
    """Runs at the 1-byte count's saturation, each between runs of one: 254
    reads scnt, 255 and more read soff."""
    runs = [1]
    for r in SATURATION_RUNS:
        runs += [r, 1]
    return Layout("saturation", runs)


ONE_RUN_SUBS = [0x7FFFFFFF, 0x80000000, 0xFFFFFFFE]


def one_runs(search: bool) -> Layout:
    """Runs of one and of two whose subscribers have bit 31 set or are the
    largest id: the staged tile keeps a run of one as INT64_MIN + id.  `search`
    puts more than FAN_LDS_ENTRIES zero runs inside the (only) tile."""
    s = ONE_RUN_SUBS
    ones = [(b"one%d" % i, (s[i],)) for i in range(3)]
    twos = [(b"two%d" % i, (s[i], s[(i + 1) % 3])) for i in range(3)]
    mix = [ones[0], twos[0], ones[1], 1, twos[1], ones[2], twos[2], 2]
    spec = mix * 20 + ([0] * (FAN_LDS_ENTRIES + 64) if search else [0, 0]) + mix[::-1] * 20
    return Layout("one-runs-" + ("search" if search else "staged"), spec)


def units(total: int, unit: int) -> list:
    """`total` deliveries as runs of `unit` (and one run of one if it is odd)."""
    return [unit] * (total // unit) + [1] * (total % unit)


TILE_TOTALS = [1, 2047, 2048, 2049, 4095, 4096, 4097]
RUN_STARTS = [2047, 2048, 2049]
RUN_ENDS = [2048, 2049]             # one past the run's last delivery
BOUNDARY_ZEROS = [0, 1, 40]


def tile_edges() -> list:
    """Runs against the fill tile's boundary.  With runs of one a full tile
    covers 2,049 entries (the search path); the same totals of runs of two are
    staged."""
    T = FAN_FILL_TILE
    out = []
    for unit in (1, 2):
        for t in TILE_TOTALS:
            out.append(Layout("total-%d-of-%d" % (t, unit), units(t, unit)))
        for z in BOUNDARY_ZEROS:   # zero runs exactly between tile 0's last and tile 1's first delivery
            out.append(Layout("zeros-%d-of-%d" % (z, unit), units(T, unit) + [0] * z + units(100, unit)))
    for s in RUN_STARTS:
        out.append(Layout("run-starts-%d" % s, units(s, 2) + [300] + [1] * 5))
    for e in RUN_ENDS:
        out.append(Layout("run-ends-%d" % e, units(e - 300, 2) + [300] + [1] * 5))
    out.append(Layout("run-covers-tile", [1] * 10 + [5000] + [1] * 10))
    return out


STAGING_Z = [1532, 1533, 1534, 1535]


def staging_limit(z: int) -> Layout:
    """Tile 0 covers z + 3 entries: 1,535 and 1,536 are staged, 1,537 and 1,538
    searched.  The one scan block delivers 2,058: mid_limit makes it big by one."""
    return Layout("staging-%d" % z, [1] + [0] * z + [FAN_FILL_TILE - 1] + [1] * 10, mid_limit=FAN_FILL_TILE + 9)


STRADDLE_MID = 4500


def block_straddle(mirror: bool, search: bool) -> Layout:
    """Fill tile 2 (deliveries 4,096 .. 6,143) covers entries on both sides of
    scan-block entry 4,096; one block delivers 5,000 and more, the other less
    than STRADDLE_MID.  Staged: entries 4,090 .. 4,100 all deliver, so entry
    4,095's end offset is the next block's first.  Search: more than
    FAN_LDS_ENTRIES zero runs lie across entry 4,096."""
    S = FAN_SCAN_TILE
    if not mirror and not search:
        b0 = [1] * (S - 4) + [2] * 4                         # 4,100 deliveries
        b1 = [1] * 5 + [5000] + [1] * 10
    elif not mirror:
        b0 = [2] * 2050 + [0] * (S - 2050)                   # 4,100 deliveries
        b1 = [0] * 100 + [1] * 5 + [5000] + [1] * 10
    elif not search:
        b0 = [0] * 3000 + [1] * 100 + [5000] + [1] * (S - 3101)
        b1 = [1] * 5 + [2] * 1000 + [1] * 3
    else:
        b0 = [0] * 1000 + [1] * 100 + [5000] + [2] * 400 + [0] * (S - 1501)
        b1 = [0] * 50 + [2] * 1000 + [1] * 3
    assert len(b0) == S
    name = "straddle-%s-%s" % ("mirror" if mirror else "plain", "search" if search else "staged")
    return Layout(name, b0 + b1, mid_limit=STRADDLE_MID)


def straddles() -> list:
    return [block_straddle(m, s) for m in (False, True) for s in (False, True)]


def degenerate() -> dict:
    """Topic lists: no publish; publishes without a match; matches without a subscriber."""
    return {"empty": [], "no-match": [b"nobody/%d" % i for i in range(300)],
            "no-subscriber": Layout("no-subscriber", [0] * 5000)}


# many-blocks: n_matches + 1 = 2^20 is 256 scan blocks (one block sum per
# tm_fan_scan_sums thread), one entry more is 257 (two per thread)
MANY_TARGETS = [(1 << 20) - 1, 1 << 20]
# 2,049 scan blocks: nine sums per thread, one more than the sums loop loads at a time
MANY_RAGGED = 2048 * FAN_SCAN_TILE
WIDE_TOPIC = b"b/c/d/e"
SINGLE = b"$s/%d"       # a '$' topic: no root-level wildcard matches it


def wide_filters() -> list:
    """Every literal / '+' / '#' combination that matches WIDE_TOPIC."""
    lit = WIDE_TOPIC.split(b"/")
    F = []
    for k in range(len(lit) + 1):
        for pick in itertools.product((0, 1), repeat=k):
            ws = [lit[i] if pick[i] == 0 else b"+" for i in range(k)]
            F.append(b"/".join(ws + [b"#"]))
            if k == len(lit):
                F.append(b"/".join(ws))
    return sorted(set(F))


MANY_SUBSCRIBED = {b"b/c/d/e": [11, 12], b"b/+/d/#": [13], b"#": [14], SINGLE % 0: [15], SINGLE % 7: [16, 17, 18]}
MANY_SINGLES = 64


def many_blocks(n_matches: int):
    """-> (filters, topics): WIDE_TOPIC as often as fits and single-match
    publishes for the rest, the singles spread between the wide ones."""
    F = wide_filters()
    w = len(F)
    n_wide = (n_matches - MANY_SINGLES) // w
    n_single = n_matches - n_wide * w
    assert MANY_SINGLES <= n_single < MANY_SINGLES + w
    step = n_wide // n_single
    topics = []
    for i in range(n_single):
        topics.append(SINGLE % (i % MANY_SINGLES))
        topics.extend([WIDE_TOPIC] * (step if i + 1 < n_single else n_wide - step * (n_single - 1)))
    return F + [SINGLE % i for i in range(MANY_SINGLES)], topics


def refresh_steps():
    """[(op, filter, subscriber)] and, after each, the layout the same batch
    must dispatch as: run A goes 1 -> 2 -> 1 (sone, then soff, then sone with
    the OTHER subscriber), run B 254 -> 255 -> 256 -> 255 (scnt below, at and
    past its saturation)."""
    A, B = [0x80000001], list(range(5000, 5254))
    steps = [(None, None, None)]
    ops = [("sub", b"A", 7), ("unsub", b"A", 0x80000001), ("sub", b"B", 9001), ("sub", b"B", 9002),
           ("unsub", b"B", 5000)]
    lays = []

    def lay():
        a, b = (b"A", tuple(A)), (b"B", tuple(B))
        return Layout("refresh", [a, 1, b, a, a, 2, b, 0, a])
    lays.append(lay())
    for op, f, s in ops:
        v = A if f == b"A" else B
        if op == "sub":
            v.append(s)
        else:
            v.remove(s)
        steps.append((op, b"x/" + f, s))
        lays.append(lay())
    return list(zip(steps, lays))
