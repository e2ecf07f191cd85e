"""Long and prefix-sharing words through the device dictionary mirror and the
two tokeniser paths -- needs an MI355X.

The mirror (tm_kernels.hip ck_match / dict_find / tok_lookup) decides a word
by its length and first 8 bytes in the cuckoo key, then bytes 8-15 in the
tail record, then bytes 16 and up in the arena; the word hash exists on the
host, in the lane-per-topic path's 4-byte loop and in the LDS path's 8-byte
chunks.  The inputs of long_words.py make the later stages decide (families
of equal-length words sharing 8 to 36 leading bytes, half of them subscribed)
and run every partial-chunk size at every alignment (a word of each length
1..40 at each offset mod 16, words of 100, 255 and 1,000 bytes).  Expected:
the host tokeniser's tokens (pinned by test_long_words.py) and the oracle's
rows (src/emqx_trie.erl restated)."""

import os

import numpy as np
import pytest
from test_gpu_parity import assert_same, engine_rows, oracle_rows, rows_of

import long_words as LW
from emqx_amd.engine import Engine, _d2h

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def torch_first():
    """torch's HIP runtime must initialise before the engine's (the device
    tokens come back as torch tensors)."""
    import torch
    torch.zeros(1, device="cuda")
    yield


@pytest.fixture(scope="module")
def world():
    """One engine holding every filter, the probes on the LDS path and their
    oracle rows: computed once, read by every test."""
    filters = LW.all_filters()
    eng = Engine(device=0)
    for f in filters:
        eng.insert(f)
    P = LW.lds_batch()
    exp, _ = oracle_rows(filters, P.topics, nthreads=16)
    return eng, filters, P, exp


def assert_tokens_equal(eng, topics):
    host = eng.tokenize(topics)
    dw, dt, df = eng.tokenize_device(topics)
    dw, dt, df = dw.cpu().numpy().view(np.uint32), dt.cpu().numpy().view(np.uint32), df.cpu().numpy()
    assert np.array_equal(dt, host.toff)
    assert np.array_equal(df, host.tflags)
    bad = np.nonzero(dw != host.words)[0]
    print(f"{len(topics)} topics, {len(host.words)} words: {bad.size} differ")
    assert bad.size == 0, (bad.size, bad[:5], dw[bad[:5]], host.words[bad[:5]])
    return host


def row_names(eng, offs, ids):
    names = {int(i): None for i in np.unique(ids)}
    for i in names:
        names[i] = eng.filter_bytes(i)
    return [[names[int(i)] for i in r] for r in rows_of(offs, ids)]


# ---- a. tokens -------------------------------------------------------------------
def test_tokens_on_the_lds_path_the_lane_per_topic_path_and_both(world):
    eng = world[0]
    LW.assert_floors()     # the model alone, before any device call: the probes bite
    for P in (LW.lds_batch(), LW.global_batch(), LW.mixed_batch()):
        P.assert_every_alignment()
        assert_tokens_equal(eng, P.topics)


# ---- b. rows ---------------------------------------------------------------------
def test_rows_equal_the_oracle_and_unknown_probes_match_only_the_root_wildcard(world):
    eng, filters, P, exp = world
    got = engine_rows(eng, P.topics)
    assert_same(P.topics, got, exp)
    for t, w, known, row in zip(P.topics, P.word, P.known, got):
        lit = [b"+/" + w] + ([b"f/" + w + b"/#"] if t.startswith(b"f/") else [])
        assert row == [b"#"] + (lit if known else []), (t, row)


# ---- c. window and word-count boundaries -------------------------------------------
POOL = [fam[i] for i in (0, 1, 2, 3, 748, 749, 1498, 1499) for fam in LW.FAMILY_WORDS]
W29 = LW.FAMILY_WORDS[3][1498]    # known, 29 bytes, sharing 24 with its family


def fill_topic(nbytes, last):
    """a topic of exactly nbytes that ends in `last`: family words, subscribed
    and not, behind a first word of b"x" that takes up the rest"""
    ws, left, i = [last], nbytes - len(last), 0
    while left - (len(POOL[i % len(POOL)]) + 1) >= 2:
        ws.insert(0, POOL[i % len(POOL)])
        left -= len(ws[0]) + 1
        i += 1
    ws.insert(0, b"x" * (left - 1))
    t = b"/".join(ws)
    assert len(t) == nbytes and left >= 2
    return t


def boundary_batch(tile, lead):
    """128 topics in tiles of 4 (the rule for small batches): 16 tiles of
    short probes, `tile`, 15 more -- `tile` starting `lead` bytes past a
    16-byte boundary.  -> (topics, index of `tile`)"""
    short = LW.base_probes().topics
    head = short[:63]
    pad = (lead - sum(len(t) for t in head) - 3) % 16 + 1
    head.append(b"x" * pad + b"/" + POOL[0][:1])     # pad + 2 bytes
    topics = head + tile + short[64:124]
    assert sum(len(t) for t in head) % 16 == lead and len(topics) == 128
    return topics, 16


def window_tile(window, lead):
    """four topics whose tile window (from the 16-byte boundary before the
    first) is `window` bytes, the last ending in a subscribed 29-byte word"""
    nbytes = window - lead
    q = nbytes // 4
    return [fill_topic(q + (nbytes - 4 * q if j == 0 else 0), W29) for j in range(4)]


def words_tile(nwords):
    """four topics of nwords words in all: one-byte words, a 29-byte family
    word (subscribed or not) after every 15 of them"""
    out = []
    for j in range(4):
        k = nwords // 4 + (nwords % 4 if j == 3 else 0)
        ws = [LW.FAMILY_WORDS[3][1400 + 16 * j + i // 16] if i % 16 == 15 else b"a" for i in range(k - 1)] + [W29]
        out.append(b"/".join(ws))
    assert sum(t.count(b"/") + 1 for t in out) == nwords
    return out


@pytest.mark.parametrize("case,lds", [("window3072", True), ("window3073", False), ("words512", True),
                                      ("words513", False)])
@pytest.mark.parametrize("lead", [0, 9])
def test_tiles_at_the_lds_window_and_word_limits(world, case, lds, lead):
    eng = world[0]
    tile = window_tile(int(case[6:]), lead) if case.startswith("window") else words_tile(int(case[5:]))
    topics, at = boundary_batch(tile, lead)
    tt, paths = LW.tile_paths(topics)
    assert tt == 4 and paths[at] is lds and all(paths[:at] + paths[at + 1:]), (tt, paths)
    if case.startswith("window"):
        o = sum(len(t) for t in topics[:4 * at])
        assert sum(len(t) for t in tile) + o % 16 == int(case[6:]) and topics[4 * at + 3].endswith(b"/" + W29)
    host = assert_tokens_equal(eng, topics)
    LW.check_tokens(host, topics, set(LW.dictionary_order()))


# ---- d. deltas -------------------------------------------------------------------
def test_dictionary_deltas_with_long_words_between_prepare_and_launch(world):
    _, filters, P, exp = world
    words = LW.known_words()
    bounds = LW.step_bounds(len(words))
    rebuilds, arena = LW.step_model(words, bounds)
    # the model: the cuckoo table is rebuilt (uploaded whole) at some steps and
    # patched slot by slot at others; the arena's block is outgrown (replaced,
    # filled from 0) at nearly every step, and appended to at the others
    assert rebuilds >= 2 and arena[-1] >= 60_000
    assert LW.regrowths([0] + arena) - 1 >= 10
    eng = Engine(device=0)
    eng.insert(b"#")
    b = eng.prepare(P.topics)                       # bytes only: words resolved at launch
    assert_tokens_equal(eng, P.topics)              # (the arena's first, empty block)
    for lo, hi in zip([0] + bounds, bounds):
        for f in LW.filters_of(words[lo:hi]):
            eng.insert(f)
        assert_tokens_equal(eng, P.topics)
    b.launch().wait()
    offs, ids = b.result()
    got = row_names(eng, offs, ids)
    b.free()
    assert_same(P.topics, got, exp)


# ---- e. replicas -------------------------------------------------------------------
def test_second_replica_appends_tails_and_arena(world, device_pair):
    one, filters, P, exp = world
    rep = Engine(devices=device_pair)
    assert rep.replicas == 2
    half = len(filters) // 2
    for f in filters[:half]:
        rep.insert(f)
    e1, _ = oracle_rows(filters[:half], P.topics[:2000])
    for _ in range(2):                               # a small batch on each replica: both hold the first half
        assert_same(P.topics[:2000], engine_rows(rep, P.topics[:2000]), e1)
    for f in filters[half:]:
        rep.insert(f)
    n = 70_000                                       # >= 65,536 publishes: one slice per replica
    T = (P.topics * (n // len(P.topics) + 1))[:n]
    o1, i1 = one.match_batch(T)
    o1, r1 = o1.copy(), row_names(one, o1, i1)
    o2, i2 = rep.match_batch(T)
    assert np.array_equal(o1, o2)
    r2 = row_names(rep, o2, i2)
    assert_same(T, r2, r1)
    lo = n // 2 - 1500                               # 3,000 rows across the slices' boundary
    assert_same(T[lo:lo + 3000], r2[lo:lo + 3000], [exp[i % len(P.topics)] for i in range(lo, lo + 3000)])
    rep.close()


# ---- f. dedup ----------------------------------------------------------------------
W36, W24, W16 = LW.FAMILY_WORDS[4], LW.FAMILY_WORDS[3], LW.FAMILY_WORDS[2]


def dedup_topic(d):
    """93 bytes; topics of one d % 5 share their first 67 bytes and more,
    any two their first 41: past the 64 bytes the dedup holds in registers"""
    return b"t/" + W36[d % 5] + b"/" + W24[(d // 5) % 9] + b"/" + W16[d]


def pair_topic(n, last):
    return (b"pair-" + b"0123456789" * 8)[:n - 1] + last


DEDUP_FILTERS = ([b"#", b"", b"+"] + [b"t/" + W36[i] + b"/#" for i in (0, 2, 4)] +
                 [b"t/+/" + W24[i] + b"/+" for i in range(0, 9, 2)] +
                 [b"+/+/+/" + W16[d] for d in range(0, 500, 2)] +
                 [b"t/" + W36[1] + b"/" + W24[1] + b"/" + W16[d] for d in range(6, 500, 45)] +
                 [pair_topic(n, b"a") for n in range(56, 81, 2)])


def dedup_publishes(runs):
    """~4,000 publishes of 550 distinct topics: every topic twice in a row,
    then all of them in turn twice (equal topics 500 apart: other workgroups
    of 256), then blocks of 50 four times over (50 apart: mostly the same
    workgroup); pairs of every length 56..80 differing in the last byte,
    adjacent and far apart; runs of b"" at the start, in the middle and at
    the end."""
    D = [dedup_topic(d) for d in range(500)]
    pairs = [pair_topic(n, c) for n in range(56, 81) for c in (b"a", b"b")]
    T = [b""] * runs[0]
    T += [t for t in D for _ in range(2)] + pairs
    T += D + D
    T += [b""] * runs[1]
    T += [t for c in range(0, 500, 50) for _ in range(4) for t in D[c:c + 50]]
    T += pairs[::-1]
    T += [b""] * runs[2]
    return T


@pytest.mark.parametrize("runs,weak", [((1, 2, 5), False), ((2, 5, 1), False), ((5, 1, 2), False),
                                       ((0, 2, 5), False), ((1, 2, 5), True)])
def test_dedup_of_long_topics_sharing_their_heads(runs, weak):
    if weak:
        os.environ["TM_DEDUP_WEAK_HASH"] = "1"   # the hash is the length: every two 93-byte topics collide
    try:
        eng = Engine(device=0)
    finally:
        os.environ.pop("TM_DEDUP_WEAK_HASH", None)
    for f in DEDUP_FILTERS:
        eng.insert(f)
    T = dedup_publishes(runs)
    assert 3900 <= len(T) <= 4200 and len(set(T)) == 551 and len({len(dedup_topic(d)) for d in range(500)}) == 1
    exp, _ = oracle_rows(DEDUP_FILTERS, T)
    b = eng.prepare(T, dedup=True)
    b.launch().wait()
    row_of, n_rows = b.row_map()
    offs, ids = b.result()
    st = b.stats()
    assert n_rows == len(set(T)) and len(offs) == n_rows + 1
    assert st["publishes"] == len(T) and st["topics"] == n_rows
    # rows in first-occurrence order, equal bytes on an equal row
    first = {}
    for i, t in enumerate(T):
        first.setdefault(t, len(first))
    assert row_of.tolist() == [first[t] for t in T]
    rows = row_names(eng, offs, ids)
    assert_same(T, [rows[r] for r in row_of.tolist()], exp)
    # every publish's expanded row in HBM is its row's; delivered = their sum
    cnt_p, start_p, ids_p, delivered = b.publish_rows_device()
    pc, ps = np.zeros(len(T), np.uint32), np.zeros(len(T), np.uint64)
    _d2h(pc, cnt_p)
    _d2h(ps, start_p)
    cnt_r, start_r, _ = b.rows(n_rows)
    assert np.array_equal(pc, cnt_r[row_of]) and np.array_equal(ps, start_r[row_of])
    assert delivered == st["delivered"] == int(pc.sum()) == sum(len(e) for e in exp)
    b.free()
