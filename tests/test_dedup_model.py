"""The host model of the device dedup (tests/dedup_model.py): its constants
against the source text, its rows against the host's own dedup, and every
batch of tests/test_gpu_dedup_edges.py against the shape it is named for -- so
a device test never passes on drifted inputs.  No GPU."""

import os
import re

import dedup_model as M
import numpy as np
import pytest
from test_gpu_parity import oracle_rows

from emqx_amd import _native as N
from emqx_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = [b"a/+", b"a/#", b"+/b", b"#", b"", b"/", b"+", b"a//b"]


def _src(name):
    with open(os.path.join(ROOT, "emqx_amd", "csrc", name)) as f:
        return f.read()


def _classes(case, only_reps=False):
    """{(lo & 3, class of my_bytes)} over the compact threads: 0, 1 (1..3), 4 (>= 4)."""
    mine, lo, mb = case.threads()
    keep = mine > 0 if only_reps else np.ones(len(mine), bool)
    return {(int(a), 0 if b == 0 else 1 if b < 4 else 4) for a, b in zip(lo[keep] & 3, mb[keep])}


# ------------------------------------------------------------------ the model

def test_constants_are_the_sources():
    hpp, hip, cpp = _src("tm_internal.hpp"), _src("tm_kernels.hip"), _src("tm_batch.cpp")
    assert int(re.search(r"constexpr uint32_t DD_TILE = (\d+);", hpp).group(1)) == M.DD_TILE == 1024
    assert int(re.search(r"constexpr uint32_t DD_EXPAND_TILE = (\d+);", hpp).group(1)) == M.DD_EXPAND_TILE == 2048
    assert int(re.search(r"constexpr uint32_t DD_BLOCK = (\d+);", hip).group(1)) == M.DD_BLOCK == 256
    assert int(re.search(r"constexpr uint32_t DD_LT = (\d+);", hip).group(1)) == M.DD_LT == 512
    assert "constexpr uint32_t DD_PT = DD_TILE / 256;" in hip and M.DD_PT == M.DD_TILE // 256 == 4
    # a compact thread's publishes are consecutive; a count thread's are strided by 256
    assert "const uint32_t first = blockIdx.x * DD_TILE + tid * DD_PT;" in hip
    assert "const uint32_t t = t0 + u * 256 + tid;" in hip
    # the capacity rule, the weak hash, its home and its LDS slot
    assert "uint64_t cap = 1024;" in cpp and "while (cap < (uint64_t)n + n / 2) cap <<= 1;" in cpp
    assert "if (a.weak_hash) h = ((uint64_t)len << 40) | ((uint64_t)len << 8) | 1ull;" in hip
    assert "uint64_t i = h & a.mask;" in hip and "s = (uint32_t)(h >> 7) & (DD_LT - 1);" in hip
    assert N.TM_MAX_TOPIC_LEN == M.MAX_TOPIC_LEN
    # the comment over tm_dedup_compact says what DD_PT is
    assert "16 consecutive publishes per thread" not in hip and "4 consecutive publishes per thread" in hip


def test_capacity_rule_at_its_steps():
    assert [M.capacity(n) for n in (0, 1, 682, 683)] == [1024] * 4           # 683 + 341 = 1,024: still fits
    assert [M.capacity(n) for n in (684, 1365)] == [2048] * 2               # 1365 + 682 = 2,047
    assert [M.capacity(n) for n in (1366, 2731, 2732, 3073)] == [4096, 4096, 8192, 8192]
    assert M.CAPACITY_N == [682, 683, 684, 1365, 1366]
    assert [M.capacity(n) for n in M.CAPACITY_N] == [1024, 1024, 2048, 2048, 4096]
    for n in range(1, 5000, 7):
        cap = M.capacity(n)
        assert cap >= max(1024, n + n // 2) and cap & (cap - 1) == 0 and (cap == 1024 or cap // 2 < n + n // 2)


def test_weak_hash_home_and_lds_slot():
    assert M.weak_hash(7) == (7 << 40) | (7 << 8) | 1
    assert M.weak_home(7, 1024) == 769 and M.weak_home(7, 2048) == 1793
    assert M.weak_lds_slot(7) == (7 << 1) and M.weak_lds_slot(0) == 0
    assert len({M.weak_hash(k) for k in range(M.MAX_TOPIC_LEN + 1)}) == M.MAX_TOPIC_LEN + 1


def test_model_of_a_batch_by_hand():
    c = M.Case("hand", [b"ab", b"", b"ab", b"c", b"", b"defgh"])
    assert c.row_of.tolist() == [0, 1, 0, 2, 1, 3] and c.n_rows == 4
    assert c.rep.tolist() == [True, True, False, True, False, True]
    assert c.cbytes == b"abcdefgh" and c.coffs.tolist() == [0, 2, 2, 3, 8]
    mine, lo, mb = c.threads()
    assert mine.tolist() == [0b1011, 0b0010] and lo.tolist() == [0, 3] and mb.tolist() == [3, 5]
    used, wrapped = c.weak_slots()
    assert used == {1, 257, 258, 513} and not wrapped          # (lengths 1 and 5 share home 257)
    e = M.Case("none", [])
    assert e.n_rows == 0 and len(e.row_of) == 0 and e.threads()[0].tolist() == []


def test_model_rows_are_the_host_dedups():
    eng = Engine(device=-1)
    for c in [M.distinct(1025), M.masks(3), M.long_topics(), M.cross_blocks(), M.nonzero_base()] + M.empties():
        b = eng.prepare(c.pack(), dedup=True)
        row_of, n_rows = b.row_map()
        assert np.array_equal(row_of, c.row_of) and n_rows == c.n_rows, c.name
        b.free()


def _all_cases():
    out = [M.distinct(n) for n in M.DISTINCT_N + M.CAPACITY_N] + [M.masks(r) for r in M.MASK_ROTATIONS]
    out += M.empties() + [M.long_topics()] + M.zero_padded() + [M.weak_election(), M.weak_wrap(1024), M.weak_wrap(2048)]
    out += [M.cross_blocks()] + [M.rows_vs_publishes(k) for k in M.ROWS_DISTINCT]
    out += list(M.reuse(False)) + list(M.reuse(True)) + [M.nonzero_base()]
    return out


def test_every_topic_is_its_own_exact_filter_and_batches_stay_small():
    names = set()
    for c in _all_cases():
        assert c.name not in names
        names.add(c.name)
        assert c.n <= 5000 and len(c.cbytes) < 200_000, c.name
        for t in c.rows:
            assert b"+" not in t and b"#" not in t and not t.startswith(b"$") and len(t) <= M.MAX_TOPIC_LEN
        assert c.pack().tolist() == c.T


@pytest.mark.parametrize("cases", [M.zero_padded(), M.empties()[:4] + [M.lone_empty(2)], [M.long_topics()]],
                         ids=["zero_padded", "empties", "long"])
def test_own_filter_rows_of_the_oracle(cases):
    """The shared check's premise: with every distinct topic inserted as a
    filter (NUL bytes and 4,096-byte words among them) the oracle's row of a
    publish holds its own topic, and no other topic of the batch."""
    filters = sorted(set(FILTERS) | {t for c in cases for t in c.rows})
    for c in cases:
        exp, _ = oracle_rows(filters, c.T)
        own = set(c.rows) - set(FILTERS)
        for t, row in zip(c.T, exp):
            assert t in row and set(row) & own <= {t}, (c.name, t)


# ------------------------------------------------------------------ the cases

def test_case_all_distinct():
    assert M.DISTINCT_N == [1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 3073]
    pool = M.distinct_pool()
    assert len(set(pool)) == len(pool) == 3073 and {len(t) for t in pool} == set(range(1, 10))
    for n in M.DISTINCT_N + M.CAPACITY_N:
        c = M.distinct(n)
        assert c.n == c.n_rows == n and np.array_equal(c.row_of, np.arange(n)) and c.rep.all()
        if n >= 682:    # thread byte ranges start at every alignment
            assert _classes(c) >= {(a, 4) for a in range(4)}
    # n = k * 1024 +- 1: the count / compact blocks and their ballots; 2047 / 2048 / 2049: the expansion's
    assert [-(-n // M.DD_TILE) for n in (1023, 1024, 1025, 2047, 2048, 2049, 3073)] == [1, 1, 2, 2, 2, 3, 4]
    assert [-(-n // M.DD_EXPAND_TILE) for n in (2047, 2048, 2049)] == [1, 1, 2]
    assert [-(-n // M.DD_PT) for n in (1, 3, 4, 5)] == [1, 1, 1, 2]
    assert [M.distinct(n).cap() for n in M.CAPACITY_N] == [1024, 1024, 2048, 2048, 4096]


def test_case_every_mine_mask():
    assert M.MASK_N == 2048 and M.MASK_ROTATIONS == list(range(16))
    at = {g: set() for g in (10, 63, 64, 255, 256, 256 + 63, 256 + 64, 511)}
    classes, inside_one_dword = set(), False
    for rot in M.MASK_ROTATIONS:
        c = M.masks(rot)
        mine, lo, mb = c.threads()
        assert c.n == M.MASK_N and len(mine) == 512
        assert mine.tolist() == [M.mask_of(g, rot) for g in range(512)]
        for g in at:
            at[g].add(int(mine[g]))
        # a publish that is no first occurrence duplicates an EARLIER one
        first = {}
        for t, topic in enumerate(c.T):
            assert c.rep[t] == (topic not in first)
            first.setdefault(topic, t)
        classes |= _classes(c, only_reps=True)
        assert {int(a) for a in lo[mine == 0] & 3} == {0, 1, 2, 3}          # hi == lo at every alignment
        inside_one_dword |= bool((((lo & 3) > 0) & (mb > 0) & ((lo & 3) + mb < 4)).any())
    # an ordinary thread, tids 63 / 64 of both blocks (a wave boundary), tid 255
    # and the next block's tid 0 (g = 256), the batch's last thread: all 16 masks each
    for g, seen in at.items():
        assert seen == set(range(16)), g
    # a thread holding 1 to 4 representatives, at every alignment, with 1..3 and >= 4 bytes
    assert classes >= {(a, k) for a in range(4) for k in (1, 4)}
    assert inside_one_dword                   # a thread whose bytes lie inside one dword shared with both neighbours


def test_case_empty_topics():
    cases = {c.name: c for c in M.empties()}
    assert M.EMPTY_BOUNDARIES == [64, 256, 1024]
    assert cases["two_empties"].T == [b"", b""] and cases["two_empties"].n_rows == 1
    for c in cases.values():
        e = [t for t, x in enumerate(c.T) if x == b""]
        assert e and c.rep[e[0]] and not c.rep[e[1:]].any(), c.name      # one representative: the first empty
    c = cases["empty_after_nonempty"]
    assert c.T[0] != b"" and c.T[1] == b"" and c.row_of.tolist() == [0, 1, 0, 1]
    assert cases["first_empty_at_0"].T[0] == b"" and cases["first_empty_at_0"].T.count(b"") == 3
    c = cases["first_empty_later"]
    assert c.T.index(b"") == 2 and c.T[3] == b"" and c.offs[2] == c.offs[3] == c.offs[4] > 0
    for n in (1, 2, 1025):
        c = cases[f"only_empties_{n}"]
        assert c.n == n and c.n_rows == 1 and c.cbytes == b"" and set(c.T) == {b""}
    for B in M.EMPTY_BOUNDARIES:
        c = cases[f"empties_straddle_{B}"]
        e = [t for t, x in enumerate(c.T) if x == b""]
        # the first run holds the lowest offset (the slot's) on both sides of the boundary
        assert e[:6] == list(range(B - 3, B + 3)) and len({int(c.offs[t]) for t in e[:6]}) == 1
        assert c.T[B - 4] != b"" and c.T[B + 3] != b"" and len(e) == 8 and c.offs[e[6]] > c.offs[e[0]]
        c = cases[f"empties_start_{B}"]
        e = [t for t, x in enumerate(c.T) if x == b""]
        assert e == [B, B + 1, B + 2, B + 20] and c.T[B - 1] != b"" and c.offs[B - 1] != c.offs[B]
        assert c.n > B + 20 and c.n_rows == c.n - 3
    for k in range(4):
        c = cases[f"lone_empty_{k}"]
        mine, lo, mb = c.threads()
        assert mine.tolist() == [15, 1, 15] and c.T[4] == b""
        assert mb[1] == 0 and lo[1] & 3 == k and mb[0] > 0 and mb[2] > 0


def test_case_long_topics():
    c = M.long_topics()
    assert M.LONG_LENS == [63, 64, 65, 67, 127, 128, 129, 191, 192, 193, N.TM_MAX_TOPIC_LEN]
    assert M.DD_TILE < c.n < 3000
    seen = {}
    src_align = set()
    for p, length, j in c.placed:
        assert len(c.T[p]) == length and p % M.DD_PT == j and c.rep[p]
        a = int(c.coffs[c.row_of[p]] & 3)
        seen.setdefault(length, set()).add((j, a))
        src_align.add(int(c.offs[p] & 15))
        # behind short representatives (the thread in front is all short ones), followed by short ones
        assert all(c.rep[q] and 1 <= len(c.T[q]) <= 7 for q in range(p - j - 4, p))
        assert all(c.rep[q] and 1 <= len(c.T[q]) <= 3 for q in range(p + 1, p - j + 4))
    assert set(seen) == set(M.LONG_LENS)
    for length, s in seen.items():
        assert s == {(j, a) for j in range(4) for a in range(4)}, length
    assert len(src_align) == 16                          # dd_load64's 16-B window at every offset
    # the pairs
    by_len = {}
    for ix, iv, p in c.pairs:
        x, v = c.T[ix], c.T[iv]
        assert len(x) == len(v) and [i for i in range(len(x)) if x[i] != v[i]] == [p]
        assert c.row_of[ix] != c.row_of[iv]
        assert c.T.count(x) == 2
        by_len.setdefault(len(x), set()).add(p)
    assert by_len == {length: set(M.pair_positions(length)) for length in M.PAIR_LENS}
    assert by_len[64] == {63} and by_len[65] == {63, 64} and by_len[67] == {63, 64, 65, 66}
    assert by_len[70] == {63, 64, 68, 69} and by_len[133] == {63, 64, 131, 132}
    assert by_len[N.TM_MAX_TOPIC_LEN] == {63, 64, N.TM_MAX_TOPIC_LEN - 1}
    assert sum(c.T.count(c.T[iv]) == 2 for _, iv, _ in c.pairs) >= len(M.PAIR_LENS)      # variants repeated too
    # the longest topic stands last, a representative: its bytes end the padded buffer
    assert len(c.T[-1]) == N.TM_MAX_TOPIC_LEN and c.rep[-1] and c.row_of[-1] == c.n_rows - 1


def test_case_zero_padded_prefixes():
    up, down = M.zero_padded()
    assert len(M.ZERO_HEAD) == 64 and up.T[:3] == [b"a", b"a\x00", b"a\x00\x00"]
    for c in (up, down):
        assert c.n_rows == 6 and c.n == 12
        short = [t for t in c.rows if len(t) <= 3]
        long_ = [t for t in c.rows if len(t) > 64]
        assert sorted(map(len, short)) == [1, 2, 3] and sorted(map(len, long_)) == [65, 66, 67]
        # equal register images: only the length tells them apart
        assert len({t.ljust(64, b"\x00") for t in short}) == 1
        assert len({t.ljust(128, b"\x00") for t in long_}) == 1
    assert [len(t) for t in down.T[:3]] == [3, 2, 1]


def test_case_weak_hash_election_and_wrap():
    c = M.weak_election()
    assert c.n == 2 * M.DD_BLOCK and c.n_rows == M.DD_BLOCK and set(c.lens.tolist()) == {M.WEAK_LEN}
    assert c.T[:256] == c.T[256:][::-1] and len(set(c.T[:256])) == 256
    assert np.array_equal(c.row_of[256:], np.arange(256)[::-1])
    assert len({M.weak_lds_slot(len(t)) for t in c.T}) == 1               # one LDS slot: 256 rounds
    # 1,024 slots, home 769: 300 topics reach slot 44 past slot 1,023
    c = M.weak_wrap(1024)
    assert c.n == 600 and c.n_rows == 300 and c.cap() == 1024 and set(c.lens.tolist()) == {7}
    used, wrapped = c.weak_slots()
    assert M.weak_home(7, 1024) == 769 and wrapped
    assert used == set(range(769, 1024)) | set(range(0, 45))
    # 2,048 slots
    c = M.weak_wrap(2048)
    assert c.n == 700 and c.n_rows == 300 and c.cap() == 2048 and len(set(c.lens.tolist())) == 1
    used, wrapped = c.weak_slots()
    home = M.weak_home(int(c.lens[0]), 2048)
    assert wrapped and home + 300 > 2048 and used == set(range(home, 2048)) | set(range(0, home + 300 - 2048))
    # with `i + 1` for `(i + 1) & a.mask` in dd_claim, both runs would index past the table
    assert max(M.weak_home(7, 1024) + 299, home + 299) >= 1024


def test_case_first_occurrence_across_claim_blocks():
    c = M.cross_blocks()
    assert c.n == 8 * M.DD_BLOCK and c.n_rows == 64
    blocks = [c.T[k * 256:(k + 1) * 256] for k in range(8)]
    for blk in blocks:
        assert len(set(blk)) == 64 and all(blk.count(t) == 4 for t in set(blk))
    orders = [tuple(dict.fromkeys(blk)) for blk in blocks]
    assert len(set(orders)) == 8 and list(orders[0]) == c.rows        # the rows follow block 0
    assert not c.rep[256:].any()


def test_case_rows_versus_publishes():
    assert M.ROWS_DISTINCT == [1, 64, 65] and M.ROWS_PUBLISHES == 5000
    for k in M.ROWS_DISTINCT:
        c = M.rows_vs_publishes(k)
        assert c.n == 5000 and c.n_rows == k


@pytest.mark.parametrize("weak", [False, True])
def test_case_table_reuse(weak):
    A, B = M.reuse(weak)
    assert A.n == B.n == M.REUSE_N and A.cap() == B.cap() == 1024 and A.n_rows == B.n_rows == 300
    # the empty topic: early in A, late only in B -- a stale slot's offset is below every empty publish of B
    ea, eb = A.T.index(b""), B.T.index(b"")
    assert ea == 1 and eb > 300 and B.offs[eb] > A.offs[ea] and B.T.count(b"") == 2
    if weak:
        assert set(A.lens.tolist()) == set(B.lens.tolist()) == {0, M.WEAK_LEN}
        assert set(A.rows) & set(B.rows) == {b""}
    else:
        x = A.T[0]
        assert B.T[0] == x + b"!" and x not in B.T[:5] and B.T[5] == x and B.T.count(x) == 2
        assert B.pack().buf[:len(x)].tobytes() == x and A.offs[0] == 0       # B's bytes at A's offset of X
        assert set(A.rows) & set(B.rows) == {b"", x}


def test_case_nonzero_base():
    c = M.nonzero_base()
    s = c.pack()
    assert int(s.offs[0]) == M.BASE == 37 and M.BASE % 16 and len(s) == c.n == 1100
    assert s.tolist() == c.T and len(s.buf) > int(s.offs[-1])            # a slice inside a larger buffer
    assert c.T[0] == b"" and c.T.count(b"") == 3 and c.n_rows < c.n // 2


def test_host_crosscheck_batches():
    assert [c.name for c in M.host_crosscheck()] == ["distinct_1025", "masks_0", "long_topics"]
