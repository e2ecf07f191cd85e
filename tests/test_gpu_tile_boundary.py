"""What a wave carries from one tile to the next, against the oracle -- needs
an MI355X.

After a tile's frontier loop the walk loads the next tile's offsets and flags
into registers, and after the first read-back its words; the next prologue
writes LDS from them.  The prefetch is pending on every way out of a tile
(the epilogue, the stack-overflow return, a staging region that is full) and
across tiles of either word copy.  That only shows when one wave walks
several tiles, so the cases run in a fresh child process with
TM_WAVES_PER_CU=1 (256 waves; match_waves reads it once per process): 65,536
topics are 1,024 tiles of 64, two round-robin and two ticket tiles per wave.
Every row of every case is compared with the oracle's, and the batch's match
count (summed per tile by the walk) with the number of ids.

    partial   65,536 + 37 gen.C1 topics: a partial last tile, waves with and
              without a next tile
    words     blocks of 256 tiles alternate between <= 7-word topics (<= 448
              words, staged in LDS) and 9-word topics (576 > 512: read from
              HBM), so every wave switches copies from tile to tile
    fan       a block of tiles that overflow the probe stack (the fan world of
              test_gpu_walk_loop) between ordinary blocks: the early return
              with a prefetch pending
    mix       a world of its own with exact row sizes: tiles without a match,
              tiles of depth-11 topics (all flagged slow), tiles of 2,560
              entries (three chunks), and tiles whose log is one below, at and
              one above the half, the whole and twice the read-back step
    dedup     65,536 publishes of 4,000 distinct topics: the device counts the
              rows and shrinks the tile to 2 topics, eight tiles per wave

One more case runs in this process at the default grid: two tiles per wave
plus one topic (the case-one topics repeated, so the oracle is not run again).
"""

import itertools
import json
import os
import random
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TILE = 64
STAGE = 1024      # u64 entries of an epilogue chunk
ROW_CAP = 128     # default K
WCAP = 512        # words of a tile staged in LDS
WAVES = 256       # TM_WAVES_PER_CU=1 on 256 CUs
N_BASE = 65536
CASES = ("partial", "words", "fan", "mix", "dedup")


def kernel_define(name):
    src = open(os.path.join(ROOT, "emqx_amd", "csrc", "tm_kernels.hip")).read()
    return int(re.search(r"#define %s (\d+)" % name, src).group(1))


# ---- comparing a whole batch with the oracle, vectorised ------------------------------------

class Rows:
    """The oracle's rows of the distinct topics U over the filters F (indices into F)."""

    def __init__(self, F, U):
        from oracle import pyoracle as P
        orc = P.Oracle()
        for f in F:
            orc.register(f)
            orc.insert(f)
        buf, offs = P.pack(U)
        counts, idx, _ = orc.match_batch(buf, offs, nthreads=4)
        orc.close()
        self.F, self.U = F, U
        self.counts = counts.astype(np.int64)
        self.cut = np.concatenate([[0], np.cumsum(self.counts)])
        self.idx = np.asarray(idx, dtype=np.int64)

    def expected(self, order):
        """(counts, flat ids) of the batch [U[i] for i in order]."""
        order = np.asarray(order, dtype=np.int64)
        cnt = self.counts[order]
        tot = int(cnt.sum())
        starts = np.repeat(self.cut[order], cnt)
        within = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        return cnt, self.idx[starts + within]


def compare(eng, rows, order, offs, ids):
    """'' when the device's CSR equals the oracle's rows, else what differs first."""
    findex = {f: i for i, f in enumerate(rows.F)}
    ids = np.asarray(ids, dtype=np.int64)
    to_f = np.full(int(ids.max()) + 1 if ids.size else 1, -1, dtype=np.int64)
    for i in np.unique(ids):
        to_f[int(i)] = findex[eng.filter_bytes(int(i))]
    got = to_f[ids]
    cnt, exp = rows.expected(order)
    got_cnt = np.diff(np.asarray(offs, dtype=np.int64))
    if len(got_cnt) != len(cnt):
        return "rows %d != %d" % (len(got_cnt), len(cnt))
    if not np.array_equal(got_cnt, cnt):
        r = int(np.flatnonzero(got_cnt != cnt)[0])
        return "row %d (tile %d) %r: %d entries, oracle %d" % (r, r // TILE, rows.U[order[r]], got_cnt[r], cnt[r])
    if not np.array_equal(got, exp):
        k = int(np.flatnonzero(got != exp)[0])
        r = int(np.searchsorted(np.cumsum(cnt), k, side="right"))
        return "row %d (tile %d) %r: entry %d is %r, oracle %r" % (
            r, r // TILE, rows.U[order[r]], k - int(np.cumsum(cnt)[r] - cnt[r]), rows.F[got[k]], rows.F[exp[k]])
    return ""


def run_batch(eng, rows, order, dedup=False):
    T = [rows.U[i] for i in order]
    b = eng.prepare(T, dedup=dedup)
    b.launch().wait()
    offs, ids = b.result()
    st = b.stats()
    if dedup:
        row_of, n_rows = b.row_map()
        first = np.full(n_rows, -1, dtype=np.int64)      # a publish of every result row
        first[row_of[::-1]] = np.arange(len(order) - 1, -1, -1)
        assert (first >= 0).all()
        order = [order[i] for i in first]
    b.free()
    diff = compare(eng, rows, order, offs, ids)
    return {"diff": diff, "rows": len(offs) - 1, "matches": int(st["matches"]), "ids": int(len(ids)),
            "slow_topics": int(st["slow_topics"]), "overflow_tiles": int(st["overflow_tiles"])}


# ---- the C1 world: cases partial, words, fan, dedup -----------------------------------------

FAN_WORDS = [b"f%d" % i for i in range(6)]


def c1_world():
    """gen.C1's 10k filters + the fan filters; topics: 65,573 C1 topics (1 to 9
    words, about 300 a tile), 9-word topics made from them, the 64 fan topics."""
    from emqx_amd import gen
    filters = gen.gen_filters(gen.C1)
    topics = gen.gen_topics(gen.C1, filters, 1001, N_BASE + 37).tolist()
    fan_u = [b"/".join(FAN_WORDS + [b"last%02d" % i]) for i in range(64)]
    F = set(filters.tolist())
    for t in fan_u:
        ws = t.split(b"/")
        for mask in itertools.product((0, 1), repeat=7):
            F.add(b"/".join(b"+" if m else w for m, w in zip(mask, ws)))
    F = sorted(F)
    index, U, base = {}, [], []
    for t in topics:
        base.append(index.setdefault(t, len(index)))
        if index[t] == len(U):
            U.append(t)
    # 9-word topics: a C1 topic's words, padded
    U9 = [b"/".join((t.split(b"/") + [b"pad%d" % j for j in range(9)])[:9]) for t in U[:4096]]
    nine = list(range(len(U), len(U) + len(U9)))
    fan = list(range(len(U) + len(U9), len(U) + len(U9) + 64))
    return F, U + U9 + fan_u, base, nine, fan


def block_of(members, tiles):
    return [members[i % len(members)] for i in range(tiles * TILE)]


def c1_cases(eng, rows, base, nine, fan):
    out = {}
    # 1: the C1 topics as they come, 65,536 + 37
    out["partial"] = run_batch(eng, rows, base)
    out["partial"]["n"] = len(base)
    # 2: 256-tile blocks, <= 448 words and 576 words in turn
    order = []
    for blk in range(4):
        src = base[blk * 256 * TILE:(blk + 1) * 256 * TILE] if blk % 2 == 0 else block_of(nine, 256)
        order += src
    assert len(order) == N_BASE
    words = np.asarray([rows.U[i].count(b"/") + 1 for i in order]).reshape(-1, TILE).sum(axis=1).reshape(4, 256)
    assert (words[0::2] <= WCAP).all() and (words[1::2] == 9 * TILE).all() and 9 * TILE > WCAP
    out["words"] = run_batch(eng, rows, order)
    # 3: ordinary, overflowing, ordinary, ordinary blocks (an overflowing tile
    # in a wave's second round-robin slot; the ticket tiles follow it)
    order = base[:256 * TILE] + block_of(fan, 256) + base[256 * TILE:768 * TILE]
    assert len(order) == N_BASE
    out["fan"] = run_batch(eng, rows, order)
    out["fan"]["fan_topics"] = 256 * TILE
    # 5: 65,536 publishes of 4,000 distinct topics
    rng = random.Random(3)
    distinct = sorted(set(base))[:4000]
    pubs = distinct + [rng.choice(distinct) for _ in range(N_BASE - len(distinct))]
    out["dedup"] = run_batch(eng, rows, pubs, dedup=True)
    out["dedup"]["distinct"] = len(distinct)
    return out


# ---- the mix world: exact row sizes ---------------------------------------------------------

def family(ws):
    """Filters that match the 7-word topic ws alone (its first word stays literal)."""
    full, tail, last = [], [], []
    for mask in itertools.product((0, 1), repeat=len(ws) - 1):
        lv = [ws[0]] + [b"+" if m else w for m, w in zip(mask, ws[1:])]
        full.append(b"/".join(lv))
        tail.append(b"/".join(lv + [b"#"]))
        last.append(b"/".join(lv[:-1] + [b"#"]))
    return full + tail + sorted(set(last))


def mix_world():
    """-> F, U, {kind: [64 indices into U]}, {kind: entries of the tile's log}."""
    rng = random.Random(17)
    step = TILE * kernel_define("TM_LOG_U")
    F, U, tiles, totals = set(), [], {}, {}

    def sized_tile(kind, total):
        idx = []
        for i in range(TILE):
            L = total // TILE + (1 if i < total % TILE else 0)
            assert 0 < L <= ROW_CAP
            ws = [b"%s_%d_w%d" % (kind.encode(), i, j) for j in range(7)]
            F.update(rng.sample(family(ws), L))
            idx.append(len(U))
            U.append(b"/".join(ws))
        tiles[kind], totals[kind] = idx, total

    for name, n in (("half", step // 2), ("step", step), ("two", 2 * step)):
        for tag, d in (("m1", -1), ("p0", 0), ("p1", 1)):
            sized_tile(name + tag, n + d)
    sized_tile("three", 2560)                      # > 2 * STAGE: three chunks
    tiles["none"], totals["none"] = list(range(len(U), len(U) + TILE)), 0
    U += [b"$nomatch%d/x/y" % i for i in range(TILE)]
    tiles["deep"], totals["deep"] = list(range(len(U), len(U) + TILE)), 0
    for i in range(TILE):
        ws = [b"deep%d" % i] + [b"l%d" % j for j in range(10)]
        U.append(b"/".join(ws))
        F.update([ws[0] + b"/#", b"/".join(ws), b"/".join(ws[:10] + [b"+"])])
    # half a tile without a match, a quarter slow, a quarter of long rows
    tiles["mixed"] = tiles["none"][:32] + tiles["deep"][:16] + tiles["three"][:16]
    totals["mixed"] = None
    return sorted(F), U, tiles, totals


def mix_case():
    from emqx_amd.engine import Engine
    F, U, tiles, totals = mix_world()
    rows = Rows(F, U)
    for kind, total in totals.items():          # the oracle's own sizes are the constructed ones
        if total is not None and kind != "deep":
            assert int(rows.counts[tiles[kind]].sum()) == total, kind
    assert (rows.counts[tiles["deep"]] == 3).all() and -(-totals["three"] // STAGE) == 3
    kinds = sorted(tiles)
    rng = random.Random(23)
    seq = kinds * (-(-N_BASE // TILE // len(kinds)))
    rng.shuffle(seq)                                # any kind may follow any other on a wave
    seq = seq[:N_BASE // TILE]
    order = [t for k in seq for t in tiles[k]]
    eng = Engine(device=0)
    eng.insert_many(F)
    eng.sync()
    res = run_batch(eng, rows, order)
    res["deep_topics"] = sum(TILE if k == "deep" else 16 if k == "mixed" else 0 for k in seq)
    res["kinds"] = len(kinds)
    eng.close()
    return res


def worker(path):
    from emqx_amd.engine import Engine
    F, U, base, nine, fan = c1_world()
    rows = Rows(F, U)
    eng = Engine(device=0)
    eng.insert_many(F)
    eng.sync()
    out = c1_cases(eng, rows, base, nine, fan)
    eng.close()
    out["mix"] = mix_case()
    with open(path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    worker(sys.argv[1])
    sys.exit(0)


import pytest  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def child():
    """The five cases, run once in a child process with one wave per CU."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cases.json")
        env = dict(os.environ, TM_WAVES_PER_CU="1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        with open(path) as f:
            return json.load(f)


@pytest.mark.parametrize("case", CASES)
def test_every_row_equals_the_oracles(child, case):
    r = child[case]
    assert r["diff"] == "", r
    assert r["matches"] == r["ids"], r          # the walk's own sum of the row sizes


def test_shapes_are_the_ones_meant(child):
    """Several tiles per wave in every case, and each case's special tiles took the path meant."""
    assert child["partial"]["n"] == N_BASE + 37 and child["partial"]["rows"] == N_BASE + 37
    assert N_BASE // TILE == 4 * WAVES
    assert child["partial"]["overflow_tiles"] == 0 and child["words"]["overflow_tiles"] == 0
    # every fan topic left its tile for the generic path; of the ordinary
    # topics (all of them in case one) at most those that did there
    for key in ("overflow_tiles", "slow_topics"):
        assert 0 <= child["fan"][key] - child["fan"]["fan_topics"] <= child["partial"][key], key
    assert child["mix"]["slow_topics"] == child["mix"]["deep_topics"] > 0 and child["mix"]["overflow_tiles"] == 0
    # 4,000 rows on 256 waves: the kernel halves the tile down to 2 topics (2,000 tiles >= 4 * 256)
    assert child["dedup"]["rows"] == child["dedup"]["distinct"] == 4000


def test_default_grid_two_tiles_per_wave_plus_one_topic():
    """In this process, every resident wave: 2 * 4,096 tiles + 1 topic (16 waves on
    each of 256 CUs), the case-one topics repeated."""
    from emqx_amd.engine import Engine
    F, U, base, _, _ = c1_world()
    rows = Rows(F, U)
    n = 2 * 4096 * TILE + 1
    order = (base * (-(-n // len(base))))[:n]
    eng = Engine(device=0)
    eng.insert_many(F)
    eng.sync()
    r = run_batch(eng, rows, order)
    eng.close()
    assert r["diff"] == "" and r["rows"] == n and r["matches"] == r["ids"], r
