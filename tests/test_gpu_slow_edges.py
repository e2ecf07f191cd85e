"""The generic match path (tm_match_slow) at its stack, sort and scratch edges,
through the C ABI -- needs an MI355X.

The kernel is a chain of size regimes: the probe stack in LDS (SLOW_SQ = 512
entries, or TM_SLOW_LDS) or, after a restart, in global scratch; a row not
sorted at all, sorted in LDS as u64 (up to 1,024), as two LDS runs merged by
rank (up to 2,048), as filter ids by bytes (up to 2,048) or in global scratch;
a row past s_ocap (16,384) or past the staging area answered by a relaunch;
and one wave that serves item after item in the same 8 KB of LDS.  Every case
here puts rows on both sides of one of these edges, beside a few ordinary
topics, and compares every row of the batch, as filter bytes in order, with
sorted(filters of the row's layout): Python's bytes order is Erlang's binary
order, so the expectation needs neither the model nor the oracle.  Nothing is
skipped or filtered: every comparison covers every row of its batch.

tests/slow_model.py builds the layouts and restates the kernel's loop;
tests/test_slow_model.py checks there, without a GPU, that each layout has
the row length, the sort regime, the stack peak and the restart this file
names for it, and that the expectation equals the oracle's row.

The checked build runs first: an index past an array is then reported by the
bounds check before any other case could meet it as a fault.
"""

import functools
import os
import random

import pytest
import slow_model as S
from test_gpu_walk_loop import device_rows, differing, tile_topics

from emqx_amd.engine import Engine

pytestmark = pytest.mark.gpu

# name -> (depth, matches, with '#' filters, seed): slow_model.layout
LAYOUTS = {
    "deep0": (11, 0, False, 1), "deep1": (11, 1, False, 2), "deep2": (11, 2, False, 3),
    "p1023": (10, 1023, True, 4), "p1024": (10, 1024, True, 5), "p1025": (10, 1025, True, 6),
    "p1026": (10, 1026, True, 7), "p2047": (10, 2047, True, 8), "p2048": (10, 2048, True, 9),
    "p2049": (10, 2049, True, 10),
    "k128": (8, 128, True, 11), "k129": (8, 129, True, 12),
    "b1024": (11, 1024, True, 13), "b1025": (11, 1025, True, 14), "b2048": (11, 2048, True, 15),
    "b2049": (11, 2049, True, 16), "b4097": (11, 4097, True, 17),
    # deep rows whose stack peaks at exactly 64 and 65 entries beside the other layouts (found by search)
    "s64": (11, 44, False, 113), "s65": (11, 37, False, 135),
}
BRIM_DEPTH = 13            # the full product: 8,192 matches, a stack of exactly SLOW_SQ
PAST_PLUS_UNDER = [8190]   # slow_model.find_past_brim(14, SLOW_SQ + 1)
ROW_LEN = {"brim": 1 << BRIM_DEPTH, "past": (1 << BRIM_DEPTH) + 1}

ORD_FILTERS = [b"ord/a", b"ord/+", b"ord/#", b"ord/a/b", b"ord/+/b", b"$SYS/ord/#"]
ORD = {b"ord/a": [b"ord/#", b"ord/+", b"ord/a"], b"ord/a/b": [b"ord/#", b"ord/+/b", b"ord/a/b"],
       b"ord/x/b": [b"ord/#", b"ord/+/b"], b"ord": [b"ord/#"], b"nothing/here": [], b"$SYS/ord/x": [b"$SYS/ord/#"]}

SORT_EDGE = ["p1023", "p1024", "p1025", "p1026", "p2047", "p2048", "p2049",
             "b1024", "b1025", "b2048", "b2049", "b4097"]
# case -> [(layout, its row's sort regime)]
CASES = {
    "no_sort": [("deep0", "none"), ("deep1", "none"), ("deep2", "lds_bytes")],
    "lds_to_two_runs": [("p1023", "lds64"), ("p1024", "lds64"), ("p1025", "two_runs"), ("p1026", "two_runs")],
    "two_runs_to_global": [("p2047", "two_runs"), ("p2048", "two_runs"), ("p2049", "global")],
    "k_to_generic": [("k128", None), ("k129", "lds64")],       # (128 = K stays with the tile walk)
    "bytes_lds_to_global": [("b1024", "lds_bytes"), ("b1025", "lds_bytes"), ("b2048", "lds_bytes"),
                            ("b2049", "global"), ("b4097", "global")],
    "brim": [("brim", "global")],
    "past_brim": [("past", "global")],
    "global_stack": [("s64", "lds_bytes"), ("s65", "lds_bytes")],
}
SCRATCH = (13, S.S_OCAP + 1, True, 18)     # its first S_OCAP filters, then the one more


class World:
    """The filters of an engine, its topics by name, and each topic's expected row."""

    def __init__(self, layouts, extra_filters, extra_rows):
        self.topic, self.row = {}, dict(extra_rows)
        F = list(extra_filters)
        for name, (t, fl) in layouts.items():
            self.topic[name] = t
            self.row[t] = sorted(fl)
            F += fl
        assert len(set(F)) == len(F)
        self.F = F

    def batch(self, names):
        """-> (topics, expected rows): the named topics with the ordinary ones between and around them."""
        T = [self.topic[n] for n in names]
        o = list(ORD)
        for i, t in enumerate(o):
            T.insert(min(len(T), 2 * i), t)
        return T, [self.row[t] for t in T]

    def generic(self, T):
        """Topics of T that the generic path serves: deeper than 10 levels, or a row longer than K."""
        return [t for t in T if t.count(b"/") >= 10 or len(self.row[t]) > S.ROW_CAP]


@functools.lru_cache(maxsize=None)
def main_world():
    lay = {n: S.layout(*spec) for n, spec in LAYOUTS.items()}
    lay["brim"] = S.brim_layout(BRIM_DEPTH)
    lay["past"] = S.past_brim_layout(BRIM_DEPTH + 1, PAST_PLUS_UNDER)
    return World(lay, ORD_FILTERS, ORD)


@functools.lru_cache(maxsize=None)
def scratch_world():
    """-> (world of the first S_OCAP filters, the one more, the row with it)."""
    t, fl = S.layout(*SCRATCH)
    return World({"edge": (t, fl[:S.S_OCAP])}, ORD_FILTERS, ORD), fl[S.S_OCAP], sorted(fl)


@functools.lru_cache(maxsize=None)
def main_model():
    return S.SlowModel(main_world().F)


@functools.lru_cache(maxsize=None)
def walked(topic, lcap):
    return main_model().walk(topic, lcap=lcap)


def restarts(T, lcap=S.SLOW_SQ):
    """The model's count of walks of batch T that start again in global scratch."""
    return sum(walked(t, lcap).restarted for t in main_world().generic(T))


def engine(F, **env):
    os.environ.update(env)
    try:
        eng = Engine(device=0)
    finally:
        for k in env:
            del os.environ[k]
    eng.insert_many(F)
    eng.sync()
    return eng


@pytest.fixture(scope="module")
def main():
    return engine(main_world().F)


def check_case(eng, case, lcap=S.SLOW_SQ):
    """The case's batch on eng: the row lengths and regimes named above, then
    every row exact, every generic row counted, and the model's restarts."""
    w = main_world()
    names = [n for n, _ in CASES[case]]
    T, exp = w.batch(names)
    for n, reg in CASES[case]:
        row = w.row[w.topic[n]]
        assert len(row) == (LAYOUTS[n][1] if n in LAYOUTS else ROW_LEN[n]), n
        if reg is None:
            assert w.topic[n] not in w.generic(T), n
        else:
            assert w.topic[n] in w.generic(T) and S.regime(len(row), w.topic[n].count(b"/") >= 10) == reg, n
    assert tile_topics(len(T)) == 1     # no tile shares its stack: only long rows leave the tile walk
    b = eng.prepare(T)
    got, st = device_rows(eng, T, batch=b)
    info = b.slow_info
    b.free()
    assert len(got) == len(T) and not differing(T, got, exp)
    assert st["slow_topics"] == len(w.generic(T))
    assert info["restarts"] == restarts(T, lcap)
    assert info["s_ocap"] == S.S_OCAP and info["s_qcap"] == S.S_QCAP and info["s_waves"] == S.SLOW_WAVES_SMALL
    return info


# ---- the checked build, first ----------------------------------------------------------------

def test_checked_build_reports_no_index_past_an_array():
    """TM_CHECKED=1: the sort-edge rows, the rows that peak at 64 and 65, the
    brim and the row one past it; wait() fails on the first index out of bounds."""
    eng = engine(main_world().F, TM_CHECKED="1")
    w = main_world()
    T, exp = w.batch(SORT_EDGE + ["s64", "s65", "brim", "past"])
    got, st = device_rows(eng, T)
    assert not differing(T, got, exp)
    assert st["slow_topics"] == len(w.generic(T)) == len(T) - len(ORD)


# ---- the sort regimes ------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["no_sort", "lds_to_two_runs", "two_runs_to_global", "k_to_generic",
                                  "bytes_lds_to_global"])
def test_sort_edges(main, case):
    """no_sort: a deep topic with 0, 1 and 2 matches.  lds_to_two_runs: 1,024
    entries fill the LDS sort, 1,025 make a second run of one entry (not
    sorted), 1,026 one of two.  two_runs_to_global: 2,048 = two full runs,
    2,049 sorts in global scratch padded to 4,096.  k_to_generic: K = 128
    entries stay with the tile walk, 129 take the generic path.
    bytes_lds_to_global: rows ordered by bytes fill the LDS sort at 2,048 ids;
    4,097 pad to 8,192."""
    check_case(main, case)


# ---- the probe stack -------------------------------------------------------------------------

def test_stack_filled_to_the_brim_does_not_restart(main):
    """The full depth-13 product: 8,192 entries ordered by bytes in global
    scratch after a walk whose stack peaks at 512 = SLOW_SQ, sq[511] included."""
    w = walked(main_world().topic["brim"], S.SLOW_SQ)
    assert w.peak == S.SLOW_SQ and not w.restarted and len(w.emissions) == 1 << BRIM_DEPTH
    assert check_case(main, "brim")["restarts"] == 0


def test_one_entry_past_the_brim_restarts_in_global_scratch(main):
    w = walked(main_world().topic["past"], S.SLOW_SQ)
    assert w.peak == S.SLOW_SQ + 1 and w.restarted and not w.error
    assert check_case(main, "past_brim")["restarts"] == 1


@pytest.mark.parametrize("lcap", [64, 65])
def test_same_rows_with_the_stack_cut_to_64_and_65(lcap):
    """TM_SLOW_LDS = 64 and 65: the sort-edge rows and two rows whose stacks
    peak at exactly 64 and 65.  The first restarts under neither, the second
    under 64 alone; the longer rows restart under both.  Rows as before."""
    w = main_world()
    assert walked(w.topic["s64"], lcap).peak == 64 and walked(w.topic["s65"], lcap).peak == 65
    assert not walked(w.topic["s64"], lcap).restarted and walked(w.topic["s65"], lcap).restarted == (lcap == 64)
    eng = engine(w.F, TM_SLOW_LDS=str(lcap))
    check_case(eng, "global_stack", lcap)
    names = SORT_EDGE + ["s64", "s65"]
    T, exp = w.batch(names)
    assert 0 < restarts(T, lcap) == len(SORT_EDGE) + (lcap == 64)
    b = eng.prepare(T)
    got, st = device_rows(eng, T, batch=b)
    info = b.slow_info
    b.free()
    assert not differing(T, got, exp)
    assert st["slow_topics"] == len(names) and info["restarts"] == restarts(T, lcap)


# ---- scratch and staging ---------------------------------------------------------------------

def test_row_of_exactly_s_ocap_entries_and_one_more():
    """16,384 entries fill a wave's row scratch: no relaunch, the sizes stay.
    One more filter: the walk reports the miss, the host multiplies both sizes
    by 4 and launches again.  The result is read twice, and further batches on
    the engine, on a new handle and on the grown one, are exact."""
    w, one_more, row_more = scratch_world()
    t = w.topic["edge"]
    sm = S.SlowModel(w.F)
    at = sm.walk(t)
    assert len(w.row[t]) == len(at.emissions) == S.S_OCAP and not at.error
    assert S.regime(S.S_OCAP, True) == "global"
    eng = engine(w.F)
    T, exp = w.batch(["edge"])
    b = eng.prepare(T)
    got, st = device_rows(eng, T, batch=b)
    assert not differing(T, got, exp) and st["slow_topics"] == 1
    assert (b.slow_info["s_qcap"], b.slow_info["s_ocap"]) == (S.S_QCAP, S.S_OCAP)
    b.free()

    sm.insert(one_more)
    assert sm.walk(t).error and len(row_more) == S.S_OCAP + 1
    grown = sm.walk(t, qcap=4 * S.S_QCAP, ocap=4 * S.S_OCAP)
    assert not grown.error and len(grown.emissions) == S.S_OCAP + 1
    assert S.regime(S.S_OCAP + 1, True, 4 * S.S_OCAP) == "global"
    eng.insert(one_more)
    eng.sync()
    exp = [row_more if x == t else w.row[x] for x in T]
    b = eng.prepare(T)
    got, st = device_rows(eng, T, batch=b)
    assert not differing(T, got, exp) and st["slow_topics"] == 1
    assert (b.slow_info["s_qcap"], b.slow_info["s_ocap"]) == (4 * S.S_QCAP, 4 * S.S_OCAP)
    first, again = b.result(), b.result()
    assert all((x == y).all() for x, y in zip(first, again))
    got, _ = device_rows(eng, T, batch=b)          # the grown handle: no miss this time
    assert not differing(T, got, exp)
    assert (b.slow_info["s_qcap"], b.slow_info["s_ocap"]) == (4 * S.S_QCAP, 4 * S.S_OCAP)
    b.free()
    got, _ = device_rows(eng, T[::-1])             # a new handle: the miss and the relaunch again
    assert not differing(T[::-1], got, exp[::-1])


def test_rows_that_do_not_fit_staging_are_written_after_the_relaunch():
    """TM_STAGING_MIN = 64: a batch of 8 topics starts with 32 staging entries
    per topic, far less than its rows of 2,048 (two full runs, merged straight
    into staging) and 2,049 entries: the first launch writes neither."""
    w = main_world()
    eng = engine(w.F, TM_STAGING_MIN="64")
    T, exp = w.batch(["p2048", "p2049"])
    assert [len(r) for r in exp if len(r) > 3] == [2048, 2049] and 32 * len(T) < 2048
    b = eng.prepare(T)
    for _ in range(2):                             # and again on the grown buffers
        got, st = device_rows(eng, T, batch=b)
        assert not differing(T, got, exp) and st["slow_topics"] == 2
    T2, exp2 = w.batch(["p2049", "p1025", "p2048"])
    b.reprepare(T2)
    got, st = device_rows(eng, T2, batch=b)
    b.free()
    assert not differing(T2, got, exp2) and st["slow_topics"] == 3


# ---- one wave, item after item ---------------------------------------------------------------

def test_waves_change_regime_between_items(main):
    """192 generic-path items (the 12 sort-edge topics, 16 times over, shuffled)
    on 64 waves: whatever order the device lists them in, every wave serves
    three, so the same LDS is stack, u64 sort area, id sort area and stack
    again.  Every row compared, twice on the same handle."""
    w = main_world()
    T = [w.topic[n] for n in SORT_EDGE] * 16 + list(ORD)
    random.Random(192).shuffle(T)
    exp = [w.row[t] for t in T]
    assert len(w.generic(T)) == 192 == 3 * S.SLOW_WAVES_SMALL and tile_topics(len(T)) == 1
    b = main.prepare(T)
    for _ in range(2):
        got, st = device_rows(main, T, batch=b)
        assert len(got) == len(T) and not differing(T, got, exp)
        assert st["slow_topics"] == 192 and b.slow_info["s_waves"] == S.SLOW_WAVES_SMALL
        assert b.slow_info["restarts"] == 0 == restarts(T)
    b.free()
