"""The numpy model of the sharded partition (tests/shard_model.py) against the
scalar rule of tests/sharded_worker.py and the engine's host tm_filter_shard,
and every named case of the grid workload against the property it is named
for -- so tests/test_gpu_shard_partition.py never passes on drifted inputs.
No GPU."""

import numpy as np
import pytest
import shard_model as M
from sharded_worker import WID_MASK, shard_rule, workload

from emqx_amd.engine import Engine
from oracle import pyoracle as P

GS = [1, 2, 3, 5, 8]


def scalar_owners(tok, G):
    w, o = tok.words, tok.toff
    return np.array([shard_rule([int(x) & WID_MASK for x in w[o[t]:o[t + 1]][:2]], G) for t in range(len(o) - 1)],
                    np.int64)


@pytest.fixture(scope="module")
def grid():
    return M.grid_workload()


@pytest.mark.parametrize("G", GS)
def test_owners_equal_the_scalar_rule_on_the_irregular_workload(G):
    F, T, vocab = workload(5)
    eng = Engine(device=-1, frozen_dict=True)
    eng.dict_load(vocab)
    tok = eng.tokenize(T)
    got = M.owners(tok.words, tok.toff, G)
    assert np.array_equal(got, scalar_owners(tok, G))
    if G > 1:
        assert (got == G).any() and (got < G).any()     # both kinds of publish occur
    # filters: the same rule on the filter side is the engine's tm_filter_shard
    ftok = eng.tokenize(F)
    assert np.array_equal(M.owners(ftok.words, ftok.toff, G), [eng.filter_shard(f, G) for f in F])


@pytest.mark.parametrize("G", GS)
def test_owners_equal_the_scalar_rule_on_the_grid(grid, G):
    tok = grid.tokens()
    assert np.array_equal(grid.own_u(G), scalar_owners(tok, G))
    eng = grid.engine()
    ftok = eng.tokenize(grid.filters)
    assert (ftok.words & WID_MASK != M.W_UNKNOWN).all()            # the vocabulary covers every filter word
    assert np.array_equal(M.owners(ftok.words, ftok.toff, G), [eng.filter_shard(f, G) for f in grid.filters])


def test_owners_of_no_publishes():
    assert len(M.owners(np.zeros(0, np.uint32), np.zeros(1, np.uint32), 3)) == 0


def test_grid_rows_tell_every_topic_apart(grid):
    """Every topic's row is unlike every other topic's (so a misplaced or
    permuted row shows), the hot topic's row is its 47 filters -- owned and
    replicated ones mixed, three trips of a 16-lane loop -- and the odd topics
    are there."""
    F, U = grid.filters, grid.U
    assert len(set(F)) == len(F) and len(set(U)) == len(U) and 100 < len(U) < 400
    orc = P.Oracle()
    for f in F:
        orc.register(f)
        orc.insert(f)
    buf, offs = P.pack(U)
    counts, idx, _ = orc.match_batch(buf, offs)
    cut = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    rows = [tuple(F[int(j)] for j in idx[cut[i]:cut[i + 1]]) for i in range(len(U))]
    assert len(set(rows)) == len(rows) and min(len(r) for r in rows) >= 1
    hot = rows[grid.hot]
    assert sorted(hot) == sorted(M.hot_filters()) and len(hot) == 47 and len(set(hot)) == 47
    eng = grid.engine()
    kinds = {eng.filter_shard(f, 3) == 3 for f in hot}
    assert kinds == {True, False}
    for t in (b"", b"/", b"$SYS/b0", b"zz/b0", b"a0/zz", b"a0", M.HOT):
        assert t in U
    # round-robin topics: unknown first word, unknown second word, depth 1, ''
    rr = {U[u] for u in grid.round_robin_u()}
    assert {b"zz/b1", b"a1/zz", b"a2", b""} <= rr and b"/" not in rr and M.HOT not in rr
    for G in GS:
        assert (grid.own_u(G)[grid.round_robin_u()] == G).all()


def test_strings_are_the_topics_gathered_by_index(grid):
    idx = grid.case("mixed", 3, 1000)
    S = grid.strings(idx)
    assert S.tolist() == [grid.U[i] for i in idx]
    E = grid.strings(np.zeros(0, np.int64))
    assert len(E) == 0 and E.tolist() == []


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("n", [0, 1, 7, 3 * 1024 + 1, 8 * 1025 + 3])
def test_plan_conserves_publishes(grid, G, n):
    own = grid.own_u(G)[grid.case("mixed", G, n)]
    pl = M.plan(own, n, G)
    assert pl.shape == (G, G) and pl.sum() == n
    assert np.array_equal(pl.sum(1), np.diff(M.slice_bounds(n, G)))
    eff = M.effective(own, n, G)
    assert ((eff >= 0) & (eff < G)).all() and np.array_equal(eff[own < G], own[own < G])
    assert np.array_equal(np.bincount(eff, minlength=G), pl.sum(0))


def test_round_robin_is_slice_local():
    """t % G counts from the slice's first publish, not the batch's."""
    n, G = 10, 3                                   # slices [0,3) [3,6) [6,10)
    eff = M.effective(np.full(n, G), n, G)
    assert eff.tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 2, 0]
    n = 11                                         # slices [0,3) [3,7) [7,11): local != global from slice 2 on
    assert M.effective(np.full(n, G), n, G).tolist() == [0, 1, 2, 0, 1, 2, 0, 0, 1, 2, 0]


# ---- each named case has the property it is named for

def _plan(grid, name, G, n):
    idx = grid.case(name, G, n)
    assert len(idx) == n
    own = grid.own_u(G)[idx]
    return idx, own, M.plan(own, n, G)


@pytest.mark.parametrize("n", M.BLOCK_EDGE_N)
def test_case_block_edges_mixed(grid, n):
    idx, own, pl = _plan(grid, "mixed", 3, n)
    sizes = np.diff(M.slice_bounds(n, 3)).tolist()
    assert (pl > 0).all()                          # every slice sends to every shard
    assert (own == 3).any() and (idx == grid.hot).any()
    assert len(np.unique(idx)) == len(grid.U)      # every topic of U occurs
    if n % 3 == 0:
        assert sizes == [n // 3] * 3 and n // 3 in M.BLOCK_EDGE_SIZES
    else:
        assert len(set(sizes)) == 2 and min(sizes) == 1024     # ragged: 1024 / 1025 publishes
    # the block count of the partition is the one the size is named for
    assert [-(-s // M.PART_BLOCK) for s in sizes] == [{1023: 1, 1024: 1, 1025: 2, 2048: 2, 2049: 3}[s] for s in sizes]


def test_block_edge_sizes_cover_one_two_and_three_blocks():
    assert sorted(M.BLOCK_EDGE_N) == sorted([3069, 3072, 3073, 3074, 3075, 6144, 6147])
    assert max(M.BLOCK_EDGE_N) + 1 > M.SCAN_TILE    # tm_unpart_rows' scans over n + 1 pass one scan tile


@pytest.mark.parametrize("name,G,n", M.EMPTY_PART_CASES)
def test_case_empty_parts(grid, name, G, n):
    idx, own, pl = _plan(grid, name, G, n)
    cols = pl.sum(0)
    assert G == 3 and n == 3 * 1025 + 1 and (np.diff(M.slice_bounds(n, G)) > M.PART_BLOCK).all()   # nb = 2 per slice
    if name == "one_pair":
        # one owner: two shards get an empty part batch for the whole step
        assert len(set(own.tolist())) == 1 and own[0] < G
        assert sorted(cols.tolist()) == [0, 0, n]
        assert len(np.unique(idx)) == len(grid.pair_u(b"a0/b0")) >= 5 and (idx == grid.hot).any()
    elif name == "no_middle":
        # owner 1 receives nothing, in any slice; owners 0 and 2 do in every slice
        assert (pl[:, 1] == 0).all() and (pl[:, 0] > 0).all() and (pl[:, 2] > 0).all()
    elif name == "slice0_pair":
        # slice 0 sends nothing to shards 1 and 2; the later slices send to all:
        # zero-length pieces in front of non-zero pieces at base 0
        assert pl[0].tolist() == [n // 3, 0, 0] and (pl[1:] > 0).all()
    else:
        # every effective owner comes from round-robin
        assert name == "round_robin" and (own == G).all()
        sizes = np.diff(M.slice_bounds(n, G))
        assert np.array_equal(pl, [[(s - j + G - 1) // G for j in range(G)] for s in sizes])
        # slice-local and batch-global t % G disagree here, so a global index would show
        eff = M.effective(own, n, G)
        assert (eff != np.arange(n) % G).any()
        assert not np.array_equal(np.bincount(np.arange(n) % G, minlength=G), cols)
        kinds = {grid.U[u] for u in np.unique(idx)}
        assert {b"zz/b0", b"a0/zz", b"a0", b""} <= kinds


@pytest.mark.parametrize("G", M.SHARD_COUNTS)
def test_case_shard_counts(grid, G):
    n = G * 1025 + 3
    idx, own, pl = _plan(grid, "mixed", G, n)
    assert (pl.sum(0) > 0).all() and (own == G).any()
    assert set(own[own < G].tolist()) == set(range(G))            # every shard owns a prefix pair
    assert (np.diff(M.slice_bounds(n, G)) > M.PART_BLOCK).all()   # two blocks per slice
    assert len(set(np.diff(M.slice_bounds(n, G)).tolist())) == 2  # ragged


def test_case_scan_tile_crossing(grid):
    G = 3
    n = M.scan_tile_n(G)
    assert G * -(-(-(-n // G)) // M.PART_BLOCK) > M.SCAN_TILE
    n_min = M.scan_tile_min(G)
    assert G * -(-(-(-n_min // G)) // M.PART_BLOCK) > M.SCAN_TILE >= G * -(-(-(-(n_min - 1) // G)) // M.PART_BLOCK)
    assert n_min < n <= n_min + 1001 * G           # the smallest such n plus a ragged remainder
    sizes = np.diff(M.slice_bounds(n, G))
    assert (G * -(-sizes // M.PART_BLOCK) > M.SCAN_TILE).all() and len(set(sizes.tolist())) == 2
    idx, own, pl = _plan(grid, "mixed", G, n)
    assert (pl > 0).all() and (own == G).any() and (idx == grid.hot).any()
    # every scan block of both g-major arrays holds non-zero counts
    for cnt, wcnt in M.block_counts(own, grid.depth_u()[idx], n, G):
        assert len(cnt) > M.SCAN_TILE
        for a in (cnt, wcnt):
            pad = np.concatenate([a, np.zeros(-len(a) % M.SCAN_TILE, a.dtype)]).reshape(-1, M.SCAN_TILE)
            assert len(pad) == 2 and (pad.sum(1) > 0).all()
            assert (a[M.SCAN_TILE:] > 0).all()     # the entries read through the second block sum


def test_case_reprepare_steps(grid):
    assert [n for _, n in M.REPREPARE_STEPS] == [3 * 2049, 7, 0, 3 * 1025, 3 * 2049]
    assert M.REPREPARE_STEPS[0] == M.REPREPARE_STEPS[-1]
    for name, n in M.REPREPARE_STEPS:
        idx, own, pl = _plan(grid, name, 3, n)
        if name == "one_pair":
            assert sorted(pl.sum(0).tolist()) == [0, 0, n]
        elif n >= 3 * 1025:
            assert (pl > 0).all()
