"""A plain numpy model of the filter-sharded partition (emqx_amd/csrc/tm_shard.cpp,
tm_tokens_shard / tm_part_* in tm_kernels.hip) and the grid workload its tests
share.  Nothing here needs a GPU.

    owners(words, toff, G)   tm_tokens_shard, vectorised: the shard of a publish's
                             first two words, or G when any shard resolves it
    effective(owner, n, G)   part_owner per publish: owner, or the slice-local
                             index mod G for the publishes dealt round-robin
    plan(owner, n, G)        G x G publishes of slice i walked by shard j; its
                             column sums are the step's part_topics
    grid_workload()          filters, unique topics U and the named cases (index
                             arrays into U) of tests/test_gpu_shard_partition.py

The scalar statement of the owner rule is edge_hash / shard_rule in
tests/sharded_worker.py; tests/test_shard_model.py holds the two together and
checks that every named case has the property it is named for.
"""

from __future__ import annotations

from functools import lru_cache

import numpy as np

from emqx_amd import gen

W_UNKNOWN, W_EMPTY, W_PLUS, W_HASH, W_FIRST = 0, 1, 2, 3, 4
WID_MASK = (1 << 29) - 1
PART_BLOCK = 1024      # tm_internal.hpp: publishes per partition block
SCAN_TILE = 4096       # tm_kernels.hip: entries per scan block (SCAN_BLOCK * SCAN_PER_THREAD)


def edge_hash_v(p: np.ndarray, w: np.ndarray) -> np.ndarray:
    """sharded_worker.edge_hash over uint64 arrays (the multiplies wrap)."""
    k = (p.astype(np.uint64) << np.uint64(32)) | w.astype(np.uint64)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xFF51AFD7ED558CCD)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xC4CEB9FE1A85EC53)
    k ^= k >> np.uint64(33)
    return k & np.uint64(0xFFFFFFFF)


def owners(words: np.ndarray, toff: np.ndarray, G: int) -> np.ndarray:
    """tm_tokens_shard: edge_hash(i0, i1) % G when depth >= 2 and neither id is
    W_UNKNOWN / W_PLUS / W_HASH, else G.  int64 [n]."""
    toff = np.asarray(toff).astype(np.int64)
    n = len(toff) - 1
    if n == 0:
        return np.zeros(0, np.int64)
    ids = np.asarray(words).astype(np.uint32) & np.uint32(WID_MASK)
    deep = np.diff(toff) >= 2
    at = np.where(deep, toff[:-1], 0)              # (shallow publishes read nothing)
    pad = np.concatenate([ids, np.zeros(2, np.uint32)])
    i0, i1 = pad[at], pad[at + 1]
    lit = deep
    for x in (W_UNKNOWN, W_PLUS, W_HASH):
        lit = lit & (i0 != x) & (i1 != x)
    h = (edge_hash_v(i0, i1) % np.uint64(G)).astype(np.int64)
    return np.where(lit, h, G)


def slice_bounds(n: int, G: int) -> np.ndarray:
    """lo_i = n * i // G, i = 0..G."""
    return np.array([n * i // G for i in range(G + 1)], np.int64)


def slice_of(n: int, G: int) -> np.ndarray:
    lo = slice_bounds(n, G)
    return np.repeat(np.arange(G, dtype=np.int64), np.diff(lo))


def effective(owner: np.ndarray, n: int, G: int) -> np.ndarray:
    """The shard that walks each publish: its owner, or slice-local t % G."""
    owner = np.asarray(owner, np.int64)
    assert len(owner) == n
    lo = slice_bounds(n, G)
    t_local = np.arange(n, dtype=np.int64) - lo[slice_of(n, G)]
    return np.where(owner < G, owner, t_local % G)


def plan(owner: np.ndarray, n: int, G: int) -> np.ndarray:
    """[i, j] = publishes of slice i walked by shard j."""
    eff = effective(owner, n, G)
    return np.bincount(slice_of(n, G) * G + eff, minlength=G * G).reshape(G, G)


def block_counts(owner: np.ndarray, depth: np.ndarray, n: int, G: int):
    """Per slice, the g-major arrays tm_part_count writes: (cnt, wcnt), each
    flat [G * nb] with entry g * nb + block."""
    eff = effective(owner, n, G)
    lo = slice_bounds(n, G)
    out = []
    for i in range(G):
        e, d = eff[lo[i]:lo[i + 1]], np.asarray(depth[lo[i]:lo[i + 1]], np.int64)
        nb = max(1, -(-len(e) // PART_BLOCK))
        key = e * nb + np.arange(len(e), dtype=np.int64) // PART_BLOCK
        out.append((np.bincount(key, minlength=G * nb), np.bincount(key, weights=d, minlength=G * nb).astype(np.int64)))
    return out


# ------------------------------------------------------------------ workload

NA, NB, NC, ND = 6, 5, 4, 2
HOT = b"a0/b0/c0/d0"


def hot_filters():
    """Every filter that matches HOT and is built from its own levels: each of
    the 4 levels literal or '+' (16), and every prefix of 0..4 such levels
    closed by '#' (1 + 2 + 4 + 8 + 16 = 31)."""
    lv = HOT.split(b"/")
    out = []
    for k in range(len(lv) + 1):
        for m in range(1 << k):
            pre = [lv[x] if m >> x & 1 else b"+" for x in range(k)]
            out.append(b"/".join(pre + [b"#"]))
            if k == len(lv):
                out.append(b"/".join(pre))
    return out


class Grid:
    """Filters F, unique topics U, and the index arrays of the named cases."""

    def __init__(self):
        A = [b"a%d" % i for i in range(NA)]
        B = [b"b%d" % j for j in range(NB)]
        Cw = [b"c%d" % k for k in range(NC)]
        D = [b"d%d" % x for x in range(ND)]
        self.vocab = A + B + Cw + D + [b"$SYS"]
        lit3 = [b"/".join((a, b, c)) for a in A for b in B for c in Cw]
        lit2 = [b"/".join((a, b)) for a in A for b in B]
        lit4 = [b"a1/b1/%s/d1" % c for c in Cw] + [HOT]
        odd = [b"", b"/", b"$SYS/b0"]
        unknown = [b"zz/" + b for b in B] + [a + b"/zz" for a in A]
        literal = lit3 + lit2 + A + lit4 + odd             # every literal topic is a filter
        wild = [a + b"/+" for a in A] + [b"+/" + b for b in B] + [p + b"/#" for p in lit2] + [b"#"]
        self.filters = sorted(set(literal + wild + hot_filters()))
        self.U = literal + unknown
        self.hot = self.U.index(HOT)
        S = gen.Strings.from_list(self.U)
        self._ubuf, self._uoffs = S.buf, S.offs.astype(np.int64)
        self._ulen = np.diff(self._uoffs)
        self._tok = None
        self._own = {}

    # -- tokens of U on a host engine (frozen dictionary, as the shards run)
    def engine(self):
        from emqx_amd.engine import Engine
        e = Engine(device=-1, frozen_dict=True)
        e.dict_load(self.vocab)
        return e

    def tokens(self):
        if self._tok is None:
            self._tok = self.engine().tokenize(self.U)
        return self._tok

    def depth_u(self) -> np.ndarray:
        return np.diff(self.tokens().toff.astype(np.int64))

    def own_u(self, G: int) -> np.ndarray:
        """owners() of every topic of U for G shards."""
        if G not in self._own:
            t = self.tokens()
            self._own[G] = owners(t.words, t.toff, G)
        return self._own[G]

    def round_robin_u(self) -> np.ndarray:
        """The topics of U no shard owns (unknown word, depth 1, '')."""
        return np.flatnonzero(self.own_u(2) == 2)

    def pair_u(self, pair: bytes) -> np.ndarray:
        """The topics of U under one literal prefix pair a<i>/b<j>."""
        return np.array([u for u, t in enumerate(self.U) if t == pair or t.startswith(pair + b"/")], np.int64)

    def pair_owned_by(self, G: int, shard: int) -> bytes:
        for u, t in enumerate(self.U):
            if t.count(b"/") == 1 and self.own_u(G)[u] == shard and t[:1] == b"a":
                return t
        raise AssertionError(f"no prefix pair on shard {shard} of {G}")

    # -- batches
    def strings(self, idx: np.ndarray) -> gen.Strings:
        """U[idx] as a packed batch, gathered by index (no Python list)."""
        idx = np.asarray(idx, np.int64)
        lens = self._ulen[idx]
        offs = np.zeros(len(idx) + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        pos = np.repeat(self._uoffs[idx] - offs[:-1], lens) + np.arange(int(offs[-1]), dtype=np.int64)
        return gen.Strings(self._ubuf[pos] if len(pos) else np.zeros(0, np.uint8), offs.astype(np.uint64))

    @staticmethod
    def _deal(pool: np.ndarray, n: int, seed: int) -> np.ndarray:
        """n draws from pool as shuffled rounds: any len(pool) consecutive
        publishes from a round's start hold every topic of the pool once."""
        pool = np.asarray(pool, np.int64)
        rounds = -(-n // len(pool)) if n else 0
        rng = np.random.default_rng(seed)
        return rng.permuted(np.tile(pool, (max(rounds, 1), 1)), axis=1).ravel()[:n]

    def case(self, name: str, G: int, n: int) -> np.ndarray:
        """Index array into U of a named case.
        mixed        every topic of U, shuffled: every shard owns publishes of every
                     slice, the hot topic and round-robin publishes among them
        one_pair     one literal prefix pair (rows differ below it): one owner,
                     every other shard's part batch is empty for the step
        no_middle    G = 3, owners 0 and 2 only: the middle part of the g-major
                     order is empty in every slice
        slice0_pair  slice 0 is one pair owned by shard 0, later slices mixed:
                     slice 0 sends nothing to shards > 0, whose parts then start at
                     base 0 with a zero-length piece in front
        round_robin  no publish has an owner: all are dealt by slice-local t % G
        """
        all_u = np.arange(len(self.U), dtype=np.int64)
        if name == "mixed":
            return self._deal(all_u, n, 11)
        if name == "one_pair":
            return self._deal(self.pair_u(b"a0/b0"), n, 12)
        if name == "no_middle":
            own = self.own_u(G)
            return self._deal(np.flatnonzero((own == 0) | (own == G - 1)), n, 13)
        if name == "slice0_pair":
            n0 = n // G
            head = self._deal(self.pair_u(self.pair_owned_by(G, 0)), n0, 14)
            return np.concatenate([head, self._deal(all_u, n - n0, 15)])
        if name == "round_robin":
            return self._deal(self.round_robin_u(), n, 16)
        raise KeyError(name)


@lru_cache(maxsize=None)
def grid_workload() -> Grid:
    return Grid()


def scan_tile_min(G: int) -> int:
    """The smallest n with G * ceil(ceil(n / G) / PART_BLOCK) > SCAN_TILE."""
    nb = SCAN_TILE // G + 1                       # blocks per slice: G * nb > SCAN_TILE
    return G * ((nb - 1) * PART_BLOCK) + 1        # ceil(n / G) = (nb - 1) * PART_BLOCK + 1


def scan_tile_n(G: int) -> int:
    """scan_tile_min plus a ragged remainder of about 1000 publishes per slice:
    every slice (floor bounds) crosses, and its last block -- one of the few
    entries read through the second block sum -- holds publishes of every owner."""
    return scan_tile_min(G) + 1000 * G + 1


# The shapes of tests/test_gpu_shard_partition.py, (case, G, n); the CPU test
# checks each one's property, so a device test cannot pass on drifted inputs.
BLOCK_EDGE_SIZES = [1023, 1024, 1025, 2048, 2049]
BLOCK_EDGE_N = [3 * s for s in BLOCK_EDGE_SIZES] + [3 * 1024 + 1, 3 * 1024 + 2]
EMPTY_PART_CASES = [("one_pair", 3, 3 * 1025 + 1), ("no_middle", 3, 3 * 1025 + 1), ("slice0_pair", 3, 3 * 1025 + 1),
                    ("round_robin", 3, 3 * 1025 + 1)]
SHARD_COUNTS = [2, 5, 8]
REPREPARE_STEPS = [("mixed", 3 * 2049), ("mixed", 7), ("mixed", 0), ("one_pair", 3 * 1025), ("mixed", 3 * 2049)]
