"""The sharded group's partition and reassembly kernels (tm_tokens_shard,
tm_part_count / tm_part_segs / tm_part_scatter over their two g-major scans,
tm_export, tm_unpart_counts / tm_unpart_rows; emqx_amd/csrc/tm_shard.cpp) at
the shapes where they can go wrong -- needs an MI355X.

Several partition blocks per slice (PART_BLOCK = 1024) under every link kind,
empty parts, publishes dealt round-robin, 2 to 8 shards, a g-major scan longer
than one scan tile (SCAN_TILE = 4096), rows longer than tm_unpart_rows' 16
lanes, and one batch handle re-prepared.  Every publish of every batch is
compared: the expected rows are the oracle's over the grid workload's unique
topics (tests/shard_model.py) expanded by index, and the shard that walked
each publish is pinned twice, by the step's part_topics against the numpy
model's plan and by every global id's shard (gid % G)."""

from functools import lru_cache

import numpy as np
import pytest
import shard_model as M
from test_gpu_parity import assert_same, oracle_rows

from emqx_amd.engine import ShardedGroup

pytestmark = pytest.mark.gpu
# this module never imports torch: the in-process sharded group is torch-free

LINKS = ("same", "staged", "peer")


@lru_cache(maxsize=None)
def expected():
    """(oracle rows of the unique topics, their lengths): computed once, never changed."""
    g = M.grid_workload()
    rows, _ = oracle_rows(g.filters, g.U)
    return rows, np.array([len(r) for r in rows], np.int64)


def group(G, monkeypatch, link="same"):
    g = M.grid_workload()
    if link != "same":
        monkeypatch.setenv("TM_SHARD_LINK", link)
    grp = ShardedGroup([0] * G)
    monkeypatch.delenv("TM_SHARD_LINK", raising=False)
    if G > 1:
        assert {grp.link(i, j) for i in range(G) for j in range(G)} == {link}
    grp.dict_load(g.vocab)
    grp.insert_many(g.filters)
    return grp


def check(grp, b, idx):
    """Every publish of the batch U[idx] against the oracle and the model."""
    g = M.grid_workload()
    G, n = len(grp), len(idx)
    exp_u, len_u = expected()
    st = b.stats()
    offs, ids = b.result()
    assert len(offs) == n + 1
    offs = offs.astype(np.int64)
    lens = np.diff(offs)
    # the partition: who walked how many
    own = g.own_u(G)[idx]
    assert st["part_topics"] == M.plan(own, n, G).sum(0).tolist()
    assert st["host_waits"] == 1
    # row lengths of the whole batch, and the CSR's ends
    assert np.array_equal(lens, len_u[idx])
    assert offs[0] == 0 and int(offs[-1]) == len(ids) == st["matches"]
    if n == 0:
        return offs, ids
    # every id of a publish's row lives on the shard the model says walked it
    eff = M.effective(own, n, G)
    assert np.array_equal(ids.astype(np.int64) % G, np.repeat(eff, lens))
    # Every occurrence's id row equals its first occurrence's.  A replicated
    # filter has one global id per shard (local id * G + shard), so a topic
    # dealt round-robin has one id row per shard that walked it: occurrences
    # are grouped by (topic, shard).  One gather over ids, no loop over publishes.
    key = idx.astype(np.int64) * G + eff
    uniq, first = np.unique(key, return_index=True)
    first_of = np.zeros(len(g.U) * G, np.int64)
    first_of[uniq] = first
    src = offs[first_of[key]]
    within = np.arange(len(ids), dtype=np.int64) - np.repeat(offs[:-1], lens)
    assert np.array_equal(ids, ids[np.repeat(src, lens) + within])
    # each first occurrence, as filter bytes, is the oracle's row
    cache = {}

    def fb(x):
        x = int(x)
        if x not in cache:
            cache[x] = grp.filter_bytes(x)
        return cache[x]
    topics = [g.U[int(k) // G] for k in uniq]
    got = [[fb(x) for x in ids[offs[p]:offs[p + 1]]] for p in first]
    assert_same(topics, got, [exp_u[int(k) // G] for k in uniq])
    return offs, ids


def run_checked(grp, idx, runs=1):
    b = grp.prepare(M.grid_workload().strings(idx))
    for _ in range(runs):
        b.run()
        res = check(grp, b, idx)
    b.free()
    return res


@pytest.mark.parametrize("n", M.BLOCK_EDGE_N)
def test_block_edges_under_every_link(monkeypatch, n):
    """Slices of 1023 .. 2049 publishes (one, two and three partition blocks;
    ragged at 3 * 1024 + 1 and + 2), three shards, mixed ownership, two steps
    per batch, under the same-device, staged and peer links: every publish is
    right and the three links give the same arrays.  From n = 3 * 2049 the
    scans of tm_unpart_rows pass one scan tile too."""
    idx = M.grid_workload().case("mixed", 3, n)
    res = {}
    for link in LINKS:
        grp = group(3, monkeypatch, link)
        res[link] = run_checked(grp, idx, runs=2)
        grp.close()
    for link in LINKS[1:]:
        assert np.array_equal(res[link][0], res["same"][0]) and np.array_equal(res[link][1], res["same"][1])


@pytest.mark.parametrize("link", ["same", "staged"])
@pytest.mark.parametrize("name,G,n", M.EMPTY_PART_CASES)
def test_empty_parts(monkeypatch, name, G, n, link):
    """Shards that walk nothing for a whole step (one_pair), an empty part in
    the middle of the g-major order (no_middle), zero-length pieces in front of
    later slices' pieces (slice0_pair), and publishes no shard owns, dealt by
    their slice-local index (round_robin)."""
    grp = group(G, monkeypatch, link)
    run_checked(grp, M.grid_workload().case(name, G, n), runs=2)
    grp.close()


@pytest.mark.parametrize("G", M.SHARD_COUNTS)
def test_shard_counts(monkeypatch, G):
    """2, 5 (% G by a non-power of two) and 8 shards (the node's shape), two
    blocks per ragged slice, mixed ownership."""
    grp = group(G, monkeypatch)
    run_checked(grp, M.grid_workload().case("mixed", G, G * 1025 + 3), runs=2)
    grp.close()


def test_scan_tile_crossing(monkeypatch):
    """G * nb > SCAN_TILE in every slice: the g-major scans of the partition
    take tm_scan_sums, and scan_at reads cnt_bs[1] / w_bs[1].  PART_BLOCK and
    SCAN_TILE are compile-time constants, so this is the smallest such batch."""
    G = 3
    n = M.scan_tile_n(G)
    assert G * -(-(-(-n // G)) // M.PART_BLOCK) > M.SCAN_TILE
    assert (G * -(-np.diff(M.slice_bounds(n, G)) // M.PART_BLOCK) > M.SCAN_TILE).all()
    grp = group(G, monkeypatch)
    run_checked(grp, M.grid_workload().case("mixed", G, n))
    grp.close()


def test_reprepare_on_one_handle(monkeypatch):
    """One batch handle re-prepared through large, tiny, empty, one-owner and
    large batches again (what bench.py does every step): each step is right,
    and the first and last, the same publishes, give the same arrays."""
    g = M.grid_workload()
    grp = group(3, monkeypatch)
    b = grp.prepare([])
    res = []
    for name, n in M.REPREPARE_STEPS:
        idx = g.case(name, 3, n)
        b.reprepare(g.strings(idx)).run()
        res.append(check(grp, b, idx))
    assert np.array_equal(res[0][0], res[-1][0]) and np.array_equal(res[0][1], res[-1][1])
    b.free()
    grp.close()
