"""A plain host model of the device dedup (TM_BATCH_DEDUP: tm_dedup_claim /
_count / _compact / _rowmeta / _expand / _rowof / _sum in
emqx_amd/csrc/tm_kernels.hip) and the batches its edge tests share.  Nothing
here needs a GPU.

The geometry restated from the source (tests/test_dedup_model.py holds the
constants against the source text):

    DD_TILE         tm_internal.hpp `constexpr uint32_t DD_TILE = 1024`: publishes
                    per tm_dedup_count / tm_dedup_compact block
    DD_PT           tm_kernels.hip `DD_PT = DD_TILE / 256`: CONSECUTIVE publishes
                    per compact thread (`first = blockIdx.x * DD_TILE + tid * DD_PT`)
    DD_BLOCK        tm_kernels.hip `DD_BLOCK = 256`: publishes per claim block
    DD_LT           tm_kernels.hip `DD_LT = 512`: LDS election slots
    DD_EXPAND_TILE  tm_internal.hpp `DD_EXPAND_TILE = 2048`: publishes per
                    tm_dedup_expand block (one partial sum each)
    capacity(n)     tm_batch.cpp reserve_dedup: `cap = 1024; while (cap < n + n / 2)
                    cap <<= 1`
    weak_hash(len)  tm_dedup_claim under TM_DEDUP_WEAK_HASH: `len << 40 | len << 8 | 1`,
                    home `h & mask` (dd_claim), LDS slot `(h >> 7) & (DD_LT - 1)`

    Case(name, T)   a batch and what the device must make of it: row_of / n_rows
                    (dict.fromkeys: rows in first-occurrence order), the compacted
                    bytes and offsets, and per compact thread (mine, lo & 3, my_bytes)
    weak_slots()    the table slots a linear probe occupies under the weak hash

Every batch of tests/test_gpu_dedup_edges.py is built here, and
tests/test_dedup_model.py checks on the CPU that each one has the shape it is
named for, so a device test cannot pass on drifted inputs.
"""

from __future__ import annotations

from functools import lru_cache

import numpy as np

from emqx_amd import gen

DD_TILE = 1024
DD_PT = DD_TILE // 256
DD_BLOCK = 256
DD_LT = 512
DD_EXPAND_TILE = 2048
MAX_TOPIC_LEN = 4096       # include/emqx_tm.h TM_MAX_TOPIC_LEN


def capacity(n: int) -> int:
    """reserve_dedup: the power of two >= n + n / 2 (integer halves), at least 1,024."""
    cap = 1024
    while cap < n + n // 2:
        cap <<= 1
    return cap


def weak_hash(length: int) -> int:
    return (length << 40) | (length << 8) | 1


def weak_home(length: int, cap: int) -> int:
    return weak_hash(length) & (cap - 1)


def weak_lds_slot(length: int) -> int:
    return (weak_hash(length) >> 7) & (DD_LT - 1)


class Case:
    """One batch (T: list of bytes; `strings`: the packed form handed to the
    engine when it is not Strings.from_list(T)) and the model's view of it."""

    def __init__(self, name: str, T, strings: gen.Strings = None):
        self.name, self.T, self.strings = name, list(T), strings
        n = len(self.T)
        self.n = n
        self.rows = list(dict.fromkeys(self.T))           # distinct topics, first-occurrence order
        index = {t: r for r, t in enumerate(self.rows)}
        self.row_of = np.array([index[t] for t in self.T], np.uint32) if n else np.zeros(0, np.uint32)
        self.n_rows = len(self.rows)
        self.lens = np.array([len(t) for t in self.T], np.int64) if n else np.zeros(0, np.int64)
        self.offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        # the representative of a row: its first publish
        rep = np.zeros(n, bool)
        if n:
            _, first = np.unique(self.row_of, return_index=True)
            rep[first] = True
        self.rep = rep
        self.cbytes = b"".join(self.rows)
        self.coffs = np.concatenate([[0], np.cumsum([len(t) for t in self.rows])]).astype(np.int64)

    def pack(self) -> gen.Strings:
        return self.strings if self.strings is not None else gen.Strings.from_list(self.T)

    def cap(self) -> int:
        return capacity(self.n)

    def threads(self):
        """Per compact thread g (block g // 256, tid g % 256, publishes
        4g .. 4g + 3): (mine, lo, my_bytes) as tm_dedup_compact computes them --
        the mask of its representatives, the offset of its bytes in cbytes and
        their count.  int64 arrays [ceil(n / DD_PT)]."""
        g = -(-self.n // DD_PT)
        rep = np.zeros(g * DD_PT, np.int64)
        rep[:self.n] = self.rep
        rb = np.zeros(g * DD_PT, np.int64)
        rb[:self.n] = self.lens * self.rep
        mine = (rep.reshape(g, DD_PT) << np.arange(DD_PT)).sum(1)
        my_bytes = rb.reshape(g, DD_PT).sum(1)
        lo = np.concatenate([[0], np.cumsum(my_bytes)])[:-1]
        return mine, lo, my_bytes

    def weak_slots(self, cap: int = None):
        """Under the weak hash: (occupied slots, wrapped).  Every distinct topic
        takes the first free slot from its length's home, linear and circular;
        the occupied set does not depend on the claim order."""
        cap = cap or self.cap()
        used, wrapped = set(), False
        for t in self.rows:
            i = weak_home(len(t), cap)
            while i in used:
                wrapped |= i + 1 == cap
                i = (i + 1) & (cap - 1)
            used.add(i)
        return used, wrapped


# ------------------------------------------------------------------ topics

# no '+' / '#' (each topic is its own exact filter), no '$' first byte
_ALNUM = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-_.:", np.uint8)
_ALPHA = np.concatenate([_ALNUM, np.frombuffer(b"////", np.uint8)])      # ~6% level separators


class _Fresh:
    """Distinct random topics: never the same bytes twice from one instance."""

    def __init__(self, seed: int):
        self.rng = np.random.default_rng(seed)
        self.seen = set()

    def __call__(self, length: int, alpha=_ALPHA) -> bytes:
        for _ in range(10_000):
            t = self.rng.choice(alpha, length).tobytes()
            if t not in self.seen:
                self.seen.add(t)
                return t
        raise AssertionError(f"no fresh topic of {length} bytes left")

    def pool(self, count: int, lo: int, hi: int):
        """count distinct topics, lengths seeded in lo..hi (a length whose
        topics have run out is drawn again)."""
        out = []
        while len(out) < count:
            length = int(self.rng.integers(lo, hi + 1))
            t = self.rng.choice(_ALPHA, length).tobytes()
            if t not in self.seen:
                self.seen.add(t)
                out.append(t)
        return out


# ---- all publishes distinct

DISTINCT_N = [1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 3073]
CAPACITY_N = [682, 683, 684, 1365, 1366]      # n + n / 2 = 1023, 1024 | 1026 (2,048), 2047 | 2049 (4,096)


@lru_cache(maxsize=None)
def distinct_pool():
    return _Fresh(1).pool(max(DISTINCT_N), 1, 9)


def distinct(n: int) -> Case:
    return Case(f"distinct_{n}", distinct_pool()[:n])


# ---- every `mine` mask

MASK_N = 2 * DD_TILE
MASK_ROTATIONS = list(range(16))


@lru_cache(maxsize=None)
def mask_pool():
    return _Fresh(2).pool(MASK_N, 1, 9)


def mask_of(g: int, rot: int) -> int:
    """The mask meant for compact thread g of rotation rot (publish 0 is always
    a first occurrence, so thread 0 also has bit 0)."""
    return (g + rot) % 16 | (1 if g == 0 else 0)


def masks(rot: int) -> Case:
    """2,048 publishes: publish 4g + j is a first occurrence exactly where bit
    j of mask_of(g, rot) is set, otherwise a duplicate of an earlier publish.
    Over the 16 rotations every thread -- tids 63 / 64 of both blocks, tid 255
    and the next block's tid 0 among them -- holds every mask."""
    pool, rng, T, used = mask_pool(), np.random.default_rng(100 + rot), [], 0
    for g in range(MASK_N // DD_PT):
        m = mask_of(g, rot)
        for j in range(DD_PT):
            if m >> j & 1:
                T.append(pool[used])
                used += 1
            else:
                T.append(T[int(rng.integers(0, len(T)))])
    return Case(f"masks_{rot}", T)


# ---- empty topics

EMPTY_BOUNDARIES = [64, 256, 1024]            # a ballot, a 256-thread stride of the count, a DD_TILE


@lru_cache(maxsize=None)
def empty_pool():
    return _Fresh(3).pool(1100, 1, 9)


def _with_empties(name, n, at) -> Case:
    pool, at = empty_pool(), set(at)
    return Case(name, [b"" if t in at else pool[t] for t in range(n)])


def lone_empty(k: int) -> Case:
    """Thread 1's only representative is the empty topic (hi == lo, lo & 3 = k),
    between two threads that have bytes."""
    pool = empty_pool()
    head = [pool[0], pool[1], pool[2]]
    need = (k - sum(len(t) for t in head)) % 4 + 4            # 4..7 bytes: the thread's bytes = k (mod 4)
    head.append(next(t for t in pool[3:] if len(t) == need))
    tail = [t for t in pool[200:] if t not in head][:4]
    return Case(f"lone_empty_{k}", head + [b"", head[0], head[0], head[1]] + tail)


def empties():
    p = empty_pool()
    out = [Case("two_empties", [b"", b""]),
           Case("empty_after_nonempty", [p[0], b"", p[0], b""]),
           Case("first_empty_at_0", [b"", p[0], b"", p[1], b""]),
           Case("first_empty_later", [p[0], p[1], b"", b"", p[2], b""]),
           Case("only_empties_1", [b""]), Case("only_empties_2", [b""] * 2), Case("only_empties_1025", [b""] * 1025)]
    for B in EMPTY_BOUNDARIES:
        # the FIRST run of empties (the one at the slot's offset, where the
        # offs[t - 1] rule decides) straddles t = B - 1 / B; a later run follows
        out.append(_with_empties(f"empties_straddle_{B}", B + 40, list(range(B - 3, B + 3)) + [B + 10, B + 11]))
        # the first empty is publish B itself: its offs[t - 1] lies across the boundary
        out.append(_with_empties(f"empties_start_{B}", B + 40, [B, B + 1, B + 2, B + 20]))
    out += [lone_empty(k) for k in range(4)]
    return out


# ---- long topics

LONG_LENS = [63, 64, 65, 67, 127, 128, 129, 191, 192, 193, MAX_TOPIC_LEN]
PAIR_LENS = [64, 65, 67, 70, 127, 129, 133, 193, MAX_TOPIC_LEN]


def pair_positions(length: int):
    """The bytes a pair of `length`-byte topics differs in: byte 63, byte 64,
    the last byte, and one inside the last partial 8-byte group behind byte 64
    (dd_hash / dd_equal read those groups with dd_u64)."""
    pos = {63, length - 1}
    if length > 64:
        pos.add(64)
        k0 = 64 + 8 * ((length - 65) // 8)                     # the last group's first byte
        if (length - 64) % 8 and length - 2 >= k0:
            pos.add(length - 2)
    return sorted(pos)


def _long(fresh: _Fresh, length: int) -> bytes:
    return b"L/" + fresh(length - 2, _ALNUM)                   # two levels, one long word


@lru_cache(maxsize=None)
def long_topics() -> Case:
    """Per length of LONG_LENS, 16 threads: the long representative at
    j = 0..3 within its thread and at every alignment 0..3 of its first byte in
    cbytes, behind short representatives and followed by short ones; then the
    pairs; the longest topic stands last.  `placed` lists (publish, length, j);
    `pairs` lists (publish of X, publish of its variant, differing byte)."""
    fresh, T, seen, cb = _Fresh(4), [], set(), 0               # cb: compacted bytes so far
    placed, pairs = [], []

    def put(t):
        nonlocal cb
        if t not in seen:
            seen.add(t)
            cb += len(t)
        T.append(t)
    for length in LONG_LENS:
        for j in range(DD_PT):
            for a in range(4):
                pre = [fresh((2, 3, 5)[(j + i) % 3]) for i in range(j)]
                r = (a - sum(len(t) for t in pre) - cb) % 4
                for pad in (4 + r, 4, 4, 4):                   # one thread of short representatives
                    put(fresh(pad))
                assert len(T) % DD_PT == 0
                for t in pre:
                    put(t)
                assert cb % 4 == a
                placed.append((len(T), length, j))
                put(_long(fresh, length))
                for i in range(DD_PT - 1 - j):
                    put(fresh(2 + i % 2))
    for length in PAIR_LENS:
        x = _long(fresh, length)
        ix = len(T)
        put(x)
        for p in pair_positions(length):
            v = bytearray(x)
            v[p] = ord("!")                                    # ('!' is in no generated topic)
            pairs.append((ix, len(T), p))
            put(bytes(v))
        put(x)                                                 # equal bytes share the row
        for _, iv, _ in pairs[-2:]:
            put(T[iv])
    put(_long(fresh, MAX_TOPIC_LEN))                           # the reads at the end of the padded buffer
    c = Case("long_topics", T)
    c.placed, c.pairs = placed, pairs
    return c


# ---- zero-padded prefixes

ZERO_HEAD = b"H/" + bytes(range(ord("a"), ord("a") + 26)) * 2 + b"0123456789"      # 64 bytes


def zero_padded():
    """b"a", b"a\\0", b"a\\0\\0" and the same behind a 64-byte head: equal register
    images (dd_load64 zero-fills past len), three rows each.  Ascending and
    descending first occurrences."""
    z = [b"a", b"a\x00", b"a\x00\x00"]
    zz = [ZERO_HEAD + t for t in z]
    up = z + zz + z + zz
    down = z[::-1] + zz[::-1] + z + zz
    return [Case("zero_padded_up", up), Case("zero_padded_down", down)]


# ---- weak hash

WEAK_LEN = 7


def weak_election() -> Case:
    """One claim block of 256 distinct topics of one length (one LDS slot: 256
    election rounds), then a second block with the same topics reversed."""
    f = _Fresh(5)
    pool = [f(WEAK_LEN) for _ in range(DD_BLOCK)]
    return Case("weak_election", pool + pool[::-1])


WRAP_N = {1024: 600, 2048: 700}
WRAP_DISTINCT = 300


def weak_wrap(cap: int) -> Case:
    """300 distinct topics of one length whose probe run from the weak hash's
    home passes the table's last slot: 600 publishes for the 1,024-slot table,
    700 for the 2,048-slot one.  The length is the one in 1..9 with the highest
    home in that table."""
    n = WRAP_N[cap]
    length = max(range(1, 10), key=lambda k: (weak_home(k, cap), k))
    f = _Fresh(6)
    pool = [f(length) for _ in range(WRAP_DISTINCT)]
    rng = np.random.default_rng(cap)
    idx = np.concatenate([np.arange(WRAP_DISTINCT), rng.integers(0, WRAP_DISTINCT, n - WRAP_DISTINCT)])
    return Case(f"weak_wrap_{cap}", [pool[i] for i in rng.permutation(idx)])


# ---- first occurrence across claim blocks

def cross_blocks() -> Case:
    """64 topics; 8 claim blocks of 256 publishes, each holding all 64 (four
    times) in a permutation of its own: whichever block claims a topic first,
    the rows follow block 0's order (atomicMin lowers a later block's offset)."""
    pool, rng = _Fresh(7).pool(64, 1, 9), np.random.default_rng(7)
    T = []
    for _ in range(8):
        T += [pool[i] for i in rng.permutation(np.repeat(np.arange(64), 4))]
    return Case("cross_blocks", T)


# ---- rows versus publishes

ROWS_PUBLISHES = 5000
ROWS_DISTINCT = [1, 64, 65]           # the walk's 64-row tile: one row, a full tile, a tile and one row


@lru_cache(maxsize=None)
def rows_pool():
    return _Fresh(8).pool(max(ROWS_DISTINCT), 1, 9)


def rows_vs_publishes(k: int) -> Case:
    rng = np.random.default_rng(k)
    return Case(f"rows_{k}", [rows_pool()[i] for i in rng.integers(0, k, ROWS_PUBLISHES)])


# ---- table reuse

REUSE_N = 600


def reuse(weak: bool):
    """(A, B): two batches of 600 publishes over 300 distinct topics each, for
    one handle prepared twice (same count: same table, no memset between).  A
    slot of A that tm_dedup_rowmeta left behind would hold A's offset of

      * the empty topic: A has it at publish 1, B only late -- B's empty
        publishes would join the stale slot, whose lower offset no publish of B has;
      * X = A[0] (not under the weak hash, whose lengths are all equal): B[0] is
        X + b"!", so B's bytes at A's offset of X equal X, and X itself comes later.

    Either way the row would be lost.  All other topics of B are new."""
    f = _Fresh(9)
    mk = (lambda: f(WEAK_LEN)) if weak else (lambda: f(int(f.rng.integers(2, 10))))
    rng = np.random.default_rng(9)

    def deal(pool, n):
        idx = np.concatenate([np.arange(len(pool)), rng.integers(0, len(pool), n - len(pool))])
        return [pool[i] for i in rng.permutation(idx)]
    if weak:
        pa, pb = [mk() for _ in range(299)], [mk() for _ in range(299)]
        A = [pa[0], b""] + deal(pa, REUSE_N - 2)
        B = deal(pb, REUSE_N - 2)
        B = B[:400] + [b""] + B[400:] + [b""]
    else:
        x = f(7)
        pa, pb = [mk() for _ in range(298)], [mk() for _ in range(297)]
        A = [x, b""] + deal(pa, REUSE_N - 2)
        B = [x + b"!"] + deal(pb, REUSE_N - 5)
        B = B[:5] + [x] + B[5:400] + [b"", x] + B[400:] + [b""]
    return Case("reuse_A_weak" if weak else "reuse_A", A), Case("reuse_B_weak" if weak else "reuse_B", B)


# ---- a batch whose first offset is not 0

BASE = 37


def nonzero_base() -> Case:
    """A slice of a larger buffer: offs[0] = 37 (no multiple of 16), an empty
    first topic, duplicates, two DD_TILE blocks."""
    pool, rng = _Fresh(10).pool(300, 1, 9), np.random.default_rng(10)
    T = [b""] + [pool[i] for i in rng.integers(0, 300, 1099)]
    T[7] = T[500] = b""
    s = gen.Strings.from_list(T)
    junk, tail = rng.choice(_ALNUM, BASE), rng.choice(_ALNUM, 5)
    return Case("nonzero_base", T, gen.Strings(np.concatenate([junk, s.buf, tail]), s.offs + np.uint64(BASE)))


# ---- the batches also run through the host's dedup

def host_crosscheck():
    return [distinct(1025), masks(0), long_topics()]
