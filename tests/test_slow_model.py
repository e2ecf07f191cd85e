"""tests/slow_model.py (the generic match path restated) and the layouts of
tests/test_gpu_slow_edges.py, without a GPU: the constants against the
sources, the expectation sorted(filters) against the oracle and against the
model's own emissions, the rank merge against sorted(), and for every GPU case
the shape it is there for -- the regime its rows sort in, the stack's peak,
whether the walk restarts and whether it runs out of scratch."""

import random

import pytest
import slow_model as S
import test_gpu_slow_edges as G
from test_gpu_walk_loop import oracle_rows


def test_constants_are_the_sources():
    assert S.source_constants() == {k: getattr(S, k) for k in
                                    ("SLOW_SQ", "SORT_LDS", "S_QCAP", "S_OCAP", "SLOW_WAVES_SMALL", "ROW_CAP")}


def by_bytes(t):
    return t.count(b"/") >= 10


def model_row(walk, t):
    """The model's emissions in the order the kernel's sort gives them."""
    if by_bytes(t):
        return sorted(f for _, f in walk.emissions)
    assert len({k for k, _ in walk.emissions}) == len(walk.emissions)      # codes of a row are distinct
    return [f for _, f in sorted(walk.emissions, key=lambda e: e[0])]


@pytest.fixture(scope="module")
def main_oracle():
    w = G.main_world()
    U = list(w.row)
    return dict(zip(U, oracle_rows(sorted(w.F), U)))


def test_expected_rows_are_the_oracles_and_the_models(main_oracle):
    w = G.main_world()
    assert set(G.LAYOUTS) | {"brim", "past"} == set(w.topic) and len(w.row) == len(w.topic) + len(G.ORD)
    for t, row in w.row.items():
        assert row == main_oracle[t], t
        assert row == model_row(G.main_model().walk(t, qcap=1 << 30, ocap=1 << 30), t), t
    for n, spec in G.LAYOUTS.items():
        assert len(w.row[w.topic[n]]) == spec[1] and w.topic[n].count(b"/") + 1 == spec[0]


def test_scratch_edge_rows_are_the_oracles_and_the_models():
    w, one_more, row_more = G.scratch_world()
    t = w.topic["edge"]
    sm = S.SlowModel(w.F)
    U = list(w.row)
    assert [w.row[u] for u in U] == oracle_rows(sorted(w.F), U)
    at = sm.walk(t)
    assert len(at.emissions) == S.S_OCAP and not at.error and w.row[t] == model_row(at, t)
    assert S.regime(S.S_OCAP, True) == "global"
    sm.insert(one_more)
    past = sm.walk(t)
    assert past.error and len(past.emissions) <= S.S_OCAP       # the first launch: the row does not fit
    grown = sm.walk(t, qcap=4 * S.S_QCAP, ocap=4 * S.S_OCAP)
    assert not grown.error and row_more == model_row(grown, t) and len(row_more) == S.S_OCAP + 1
    assert S.regime(S.S_OCAP + 1, True, 4 * S.S_OCAP) == "global"
    assert S.regime(S.S_OCAP + 1, True) == "scratch_error"
    assert row_more == oracle_rows(sorted(w.F + [one_more]), [t])[0]
    assert max(at.peak, grown.peak) <= S.S_QCAP


@pytest.mark.parametrize("nb", [1, 2, 63, 64, 65, 1023, 1024])
def test_merge_runs_is_sorted(nb):
    rng = random.Random(nb)
    keys = rng.sample(range(1 << 40), S.SORT_LDS + nb)
    a, b = sorted(keys[:S.SORT_LDS]), sorted(keys[S.SORT_LDS:])
    assert S.merge_runs(a, b) == sorted(keys)
    # and with run B wholly below and wholly above run A
    for b2 in ([-nb + i for i in range(nb)], [(1 << 41) + i for i in range(nb)]):
        assert S.merge_runs(a, b2) == sorted(a + b2)


def test_regime_edges():
    L = S.SORT_LDS
    assert [S.regime(n, False) for n in (0, 1, 2, L, L + 1, 2 * L, 2 * L + 1, S.S_OCAP)] == \
        ["none", "none", "lds64", "lds64", "two_runs", "two_runs", "global", "global"]
    assert [S.regime(n, True) for n in (0, 1, 2, 2 * L, 2 * L + 1, S.S_OCAP, S.S_OCAP + 1)] == \
        ["none", "none", "lds_bytes", "lds_bytes", "global", "global", "scratch_error"]


def test_every_gpu_case_has_the_shape_it_is_there_for():
    w = G.main_world()
    for case, rows in G.CASES.items():
        T, _ = w.batch([n for n, _ in rows])
        assert len(T) == len(rows) + len(G.ORD) and not any(by_bytes(t) or len(w.row[t]) > S.ROW_CAP for t in G.ORD)
        for n, reg in rows:
            t = w.topic[n]
            at = G.walked(t, S.SLOW_SQ)
            assert not at.error and at.peak <= S.S_QCAP, n
            assert len(at.emissions) == (G.LAYOUTS[n][1] if n in G.LAYOUTS else G.ROW_LEN[n]), n
            if reg is None:
                assert t not in w.generic(T) and len(at.emissions) == S.ROW_CAP, n
            else:
                assert t in w.generic(T) and S.regime(len(at.emissions), by_bytes(t)) == reg, (n, reg)
            assert at.restarted == (n == "past"), n
    # every sort edge of the issue is a row here, and the padded sizes are the named ones
    lens = {n: len(w.row[w.topic[n]]) for n in w.topic}
    assert [lens[n] for n in G.SORT_EDGE] == [1023, 1024, 1025, 1026, 2047, 2048, 2049, 1024, 1025, 2048, 2049, 4097]
    assert [lens[n] for n in ("deep0", "deep1", "deep2", "k128", "k129")] == [0, 1, 2, 128, 129]
    assert all(by_bytes(w.topic[n]) == (n[0] != "p") for n in G.SORT_EDGE)


def test_stack_cut_to_64_and_65_restarts_exactly_the_rows_past_it():
    w = G.main_world()
    for lcap in (64, 65):
        a, b = G.walked(w.topic["s64"], lcap), G.walked(w.topic["s65"], lcap)
        assert (a.peak, a.restarted) == (64, False) and (b.peak, b.restarted) == (65, lcap == 64)
        for n in G.SORT_EDGE:
            at = G.walked(w.topic[n], lcap)
            assert at.restarted and not at.error and at.peak > 65, n
            assert at.emissions == G.walked(w.topic[n], S.SLOW_SQ).emissions      # the second walk is the same walk
        T, _ = w.batch(G.SORT_EDGE + ["s64", "s65"])
        assert G.restarts(T, lcap) == len(G.SORT_EDGE) + (lcap == 64)
        assert G.restarts(T) == 0


def test_two_run_rows_interleave():
    """In emission order the first 1,024 entries (run A) hold a key above the
    rest's (run B's) smallest and one below its largest: the merge has to
    weave them, appending would be wrong."""
    w = G.main_world()
    two = [n for rows in G.CASES.values() for n, reg in rows if reg == "two_runs"]
    assert sorted(two) == ["p1025", "p1026", "p2047", "p2048"]
    for n in two:
        keys = [k for k, _ in G.walked(w.topic[n], S.SLOW_SQ).emissions]
        a, b = keys[:S.SORT_LDS], keys[S.SORT_LDS:]
        assert len(b) == len(keys) - S.SORT_LDS >= 1
        assert max(a) > min(b) and min(a) < max(b), n
        assert S.merge_runs(sorted(a), sorted(b)) == sorted(keys)


def test_the_brim_and_one_past_it():
    """Full products peak at 128 + 64 per level past the seventh: 512 = SLOW_SQ
    at depth 13 with no restart, 576 at depth 14.  The depth-14 product pruned
    to literal last words peaks at 512 too; the search finds the one '+' child
    that makes it 513."""
    for depth, peak in ((10, 320), (11, 384), (12, 448), (13, 512), (14, 576)):
        t, F = S.brim_layout(depth)
        at = S.SlowModel(F).walk(t)
        assert (at.peak, at.restarted, at.error, len(at.emissions)) == (peak, peak > S.SLOW_SQ, False, 1 << depth)
    t, F = S.past_brim_layout(G.BRIM_DEPTH + 1, [])
    assert S.SlowModel(F).walk(t).peak == S.SLOW_SQ
    t, F = S.past_brim_layout(G.BRIM_DEPTH + 1, [0])      # a '+' child under the prefix popped last: no higher
    assert S.SlowModel(F).walk(t).peak == S.SLOW_SQ
    found, tried = S.find_past_brim(G.BRIM_DEPTH + 1, S.SLOW_SQ + 1)
    assert found == G.PAST_PLUS_UNDER, tried
    # and beside every other layout of the engine
    w = G.main_world()
    brim, past = G.walked(w.topic["brim"], S.SLOW_SQ), G.walked(w.topic["past"], S.SLOW_SQ)
    assert (brim.peak, brim.restarted, brim.error) == (S.SLOW_SQ, False, False)
    assert (past.peak, past.restarted, past.error) == (S.SLOW_SQ + 1, True, False)
    assert (len(brim.emissions), len(past.emissions)) == (8192, 8193)


def test_unknown_words_push_no_literal_probe():
    sm = S.SlowModel([b"a/+/c", b"a/b/c", b"+/b/#"])
    at = sm.walk(b"a/zz/c")
    assert [f for _, f in at.emissions] == [b"a/+/c"] and at.peak == 2
    assert sorted(f for _, f in sm.walk(b"a/b/c").emissions) == [b"+/b/#", b"a/+/c", b"a/b/c"]
