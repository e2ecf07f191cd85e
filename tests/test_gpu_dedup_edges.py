"""TM_BATCH_DEDUP on the device at its thread, block, dword and table edges
(tm_dedup_claim / _count / _compact / _rowmeta / _expand / _rowof / _sum).
Every batch is built by tests/dedup_model.py, whose CPU test checks that it has
the shape it is named for.  Every batch goes through one check: row_of and
n_rows equal the model's (rows in first-occurrence order, dict.fromkeys), and
every publish's row equals the oracle's with every distinct topic of the batch
inserted as a filter of its own -- a byte that tm_dedup_compact lost, doubled
or shifted changes a word, so the row misses its exact filter -- needs an
MI355X."""

import os

import dedup_model as M
import numpy as np
import pytest
import test_gpu_dedup as D

from emqx_amd.engine import Engine

pytestmark = pytest.mark.gpu


def engine_for(cases, weak=False, **kw):
    """An engine holding FILTERS and every distinct topic of `cases`."""
    if weak:
        os.environ["TM_DEDUP_WEAK_HASH"] = "1"
    try:
        eng = Engine(device=0, **kw)
    finally:
        os.environ.pop("TM_DEDUP_WEAK_HASH", None)
    eng.own = sorted({t for c in cases for t in c.rows} - set(D.FILTERS))
    eng.insert_many(list(D.FILTERS) + eng.own)
    return eng


def check(eng, b, case):
    """test_gpu_dedup._check (per-publish rows against the oracle, the expanded
    (count, start), delivered) with the engine's own-topic filters, then the
    model's exact row_of."""
    D.extra_filters[:] = eng.own
    try:
        row_of, n_rows = D._check(eng, b, case.T)
    finally:
        D.extra_filters.clear()
    assert n_rows == case.n_rows, case.name
    assert np.array_equal(row_of, case.row_of), case.name


def run(eng, case):
    b = eng.prepare(case.pack(), dedup=True)
    b.launch().wait()
    check(eng, b, case)
    b.free()


@pytest.fixture(scope="module")
def distinct_engine():
    return engine_for([M.distinct(max(M.DISTINCT_N))])


@pytest.mark.parametrize("n", M.DISTINCT_N + M.CAPACITY_N)
def test_all_publishes_distinct(distinct_engine, n):
    """Every publish a representative: thread byte ranges at every alignment,
    repbits / bcount at n = k * 1024 +- 1, the expansion's block sums at
    2047 / 2048 / 2049, the table's capacity rule at its steps."""
    case = M.distinct(n)
    run(distinct_engine, case)
    assert np.array_equal(case.row_of, np.arange(n))


@pytest.fixture(scope="module")
def mask_engine():
    return engine_for([M.Case("pool", M.mask_pool())])


@pytest.mark.parametrize("rot", M.MASK_ROTATIONS)
def test_every_mine_mask(mask_engine, rot):
    """Compact thread g holds the representatives mask_of(g, rot): over the
    rotations every mask in ordinary threads, at tids 63 / 64, at tid 255 and
    at the next block's tid 0."""
    run(mask_engine, M.masks(rot))


def test_empty_topics():
    """The first empty publish at the slot's offset is the representative:
    across a ballot, a 256-thread and a DD_TILE boundary, alone in a batch,
    alone in a thread (hi == lo) between threads that have bytes."""
    cases = M.empties()
    eng = engine_for(cases)
    for c in cases:
        run(eng, c)


def test_long_topics():
    """The 64-byte chunk loop of dd_load64 / dd_put at 63 .. 193 and 4,096
    bytes, at j = 0..3 and every alignment; pairs differing in byte 63, 64, the
    last one or inside the last 8-byte group; the longest topic last."""
    c = M.long_topics()
    eng = engine_for([c])
    run(eng, c)


@pytest.mark.parametrize("weak", [False, True])
def test_zero_padded_prefixes(weak):
    cases = M.zero_padded()
    eng = engine_for(cases, weak=weak)
    for c in cases:
        run(eng, c)
        assert c.n_rows == 6


def test_weak_hash_election_and_table_wrap():
    """Every topic of one length collides: 256 election rounds in one claim
    block, and a probe run that wraps past the table's last slot (1,024 and
    2,048 slots)."""
    cases = [M.weak_election(), M.weak_wrap(1024), M.weak_wrap(2048)]
    assert all(c.weak_slots()[1] for c in cases[1:])
    eng = engine_for(cases, weak=True)
    for c in cases:
        run(eng, c)


def test_first_occurrence_across_claim_blocks():
    c = M.cross_blocks()
    eng = engine_for([c])
    run(eng, c)
    run(eng, c)


def test_rows_versus_publishes():
    """5,000 publishes over 1, 64 and 65 rows: the walk's tile edges over the compacted rows."""
    cases = [M.rows_vs_publishes(k) for k in M.ROWS_DISTINCT]
    eng = engine_for(cases)
    for c in cases:
        run(eng, c)


@pytest.mark.parametrize("weak", [False, True])
def test_table_reuse(weak):
    """A second pass on the table that tm_dedup_rowmeta cleared (same handle,
    same count: no memset), with other topics; then two fresh passes with no
    wait between (the dirty table's memset)."""
    A, B = M.reuse(weak)
    eng = engine_for([A, B], weak=weak)
    b = eng.prepare(A.pack(), dedup=True)
    b.launch().wait()
    check(eng, b, A)
    b.reprepare(B.pack(), dedup=True)
    b.launch().wait()
    check(eng, b, B)
    b.retokenize().launch()
    b.retokenize().launch().wait()
    check(eng, b, B)
    b.retokenize().launch().wait()          # and a clean table again
    check(eng, b, B)
    b.free()


def test_nonzero_base():
    """offs[0] = 37: every kernel subtracts the batch's base."""
    c = M.nonzero_base()
    assert int(c.pack().offs[0]) == M.BASE
    eng = engine_for([c])
    run(eng, c)


def test_host_dedup_gives_the_same_row_map():
    cases = M.host_crosscheck()
    dev, host = Engine(device=0), Engine(device=0, host_tokenize=True)
    for eng in (dev, host):
        eng.insert_many(list(D.FILTERS))
    for c in cases:
        maps = []
        for eng in (dev, host):
            b = eng.prepare(c.pack(), dedup=True)
            b.launch().wait()
            maps.append(b.row_map())
            b.free()
        assert maps[0][1] == maps[1][1] == c.n_rows, c.name
        assert np.array_equal(maps[0][0], maps[1][0]) and np.array_equal(maps[0][0], c.row_of), c.name
