"""Lifetime of a batch's device and pinned buffers: three rounds of engine ->
batches -> every per-batch call -> free -> close in one process, batch sizes
64, 5,000 and 300 (first allocation, regrowth past the 1,024-element minimum,
reuse without growth), every result checked against the oracle and the host
mirrors, and the device memory the process keeps after round three compared
with what it kept after round one."""

from collections import Counter
from dataclasses import replace

import numpy as np
import pytest
import torch
from test_gpu_parity import _widen

from emqx_amd import emqx_broker as B
from emqx_amd import emqx_router as R
from emqx_amd import emqx_shared_sub as S
from emqx_amd import gen
from oracle import pyoracle as P

pytestmark = pytest.mark.gpu

SIZES = (64, 5000, 300)
# The largest buffer of the 5,000-publish round is the walk's wave-private
# rows (reserve_rows): one u64 per row slot, waves * topics per tile * K slots
# and an eighth on top, grown by a quarter when reserved.  5,000 topics make
# 313 tiles of 16 (tiles halve from 64 until there are 256 of them), one wave
# each, K = 128.  (The staging area and the dense ids, 32 u32 per publish, are
# 0.8 MB each; the runtime hands memory out in 2 MiB pieces.)
_ROW_SLOTS = 313 * 16 * 128
LARGEST_ROUND2 = (_ROW_SLOTS + _ROW_SLOTS // 8 + 8) * 5 // 4 * 8


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _tables():
    """About 200 filters: a third routed to one or two nodes, a third with one
    to three plain subscribers, the rest routed to this node; two $share
    groups, one on '#' (every publish outside '$' gets a delivery)."""
    B.clear_tables()                                       # a fresh engine; the old one is closed
    F = sorted(set(gen.gen_filters(replace(gen.C1, n_filters=200)).tolist()))
    for i, f in enumerate(F):
        if i % 3 == 0:
            for d in range(1 + i % 2):
                R.add_route(f, "n%d" % d)
        elif i % 3 == 1:
            for s in range(1 + i % 3):
                B.subscribe(f, "p%d.%d" % (i, s))
        else:
            R.add_route(f)
    wild = [f for f in F if b"+" in f or f.endswith(b"#")]
    for m in ("a", "b", "c"):
        S.subscribe("g1", b"#", m)
    for m in ("x", "y"):
        S.subscribe("g2", wild[0], m)
    return F


def _rows(eng, offs, ids):
    return [[eng.filter_bytes(int(x)) for x in ids[offs[i]:offs[i + 1]]] for i in range(len(offs) - 1)]


def _round(n_pub, seed):
    F = _tables()
    eng = R.engine()
    p = replace(gen.C1, n_filters=200)
    T = gen.gen_topics(p, gen.Strings.from_list(F), seed, n_pub).tolist()
    live = sorted(R._routes)                               # every topic in the trie, Erlang binary order
    orc = P.Oracle()
    for f in live:
        orc.register(f)
        orc.insert(f)
    buf, o = P.pack(T)
    counts, idx, _ = orc.match_batch(buf, o)
    cut = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    want = [[live[int(j)] for j in idx[cut[t]:cut[t + 1]]] for t in range(len(T))]
    assert sum(len(r) for r in want) > n_pub // 2          # '#' alone matches every publish outside '$'

    b = eng.prepare(T).launch().wait()
    offs, ids = b.result()
    offs, ids = offs.copy(), ids.copy()
    assert _rows(eng, offs, ids) == want
    po, pids, ib = b.result_packed()
    assert ib == 3 and np.array_equal(po, offs) and np.array_equal(_widen(pids, ib), ids)
    pick = list(range(0, n_pub, 7))[::-1]
    so, si = b.sample(pick)
    assert _rows(eng, so, si) == [want[i] for i in pick]

    roffs, rfids, rdests = b.routes()
    for t in range(len(T)):
        exp = [(f, R.aggregate(d)) for f in want[t] for d in R._routes[f]]
        got = [(eng.filter_bytes(int(rfids[k])), R._agg_of[int(rdests[k])]) for k in range(roffs[t], roffs[t + 1])]
        assert got == exp, T[t]

    doffs, _, dsubs = b.dispatch()
    for t in range(len(T)):
        exp = [pid for f in want[t] for pid in B._order.get(f, [])]
        assert [B._terms[int(s)] for s in dsubs[doffs[t]:doffs[t + 1]]] == exp, T[t]

    keys = [(i * 2654435761) & 0xFFFFFFFF for i in range(n_pub)]
    for strategy in ("hash", "round_robin"):
        goffs, gfids, ggrp, gsubs = b.dispatch_shared(strategy, keys=keys)
        got = [[(eng.filter_bytes(int(gfids[k])), R._agg_of[int(ggrp[k])][1], B._terms[int(gsubs[k])])
                for k in range(int(goffs[i]), int(goffs[i + 1]))] for i in range(n_pub)]
        mirror = S.dispatch_batch_mirror(T, strategy, keys=keys)
        assert sum(len(r) for r in mirror) > n_pub // 2
        if strategy == "hash":
            assert got == mirror
        else:                                              # tickets within one batch are unordered
            assert [[x[:2] for x in r] for r in got] == [[x[:2] for x in r] for r in mirror]
            assert Counter(x for r in got for x in r) == Counter(x for r in mirror for x in r)
    b.free()

    d = eng.prepare(T, dedup=True).launch().wait()
    row_of, n_rows = d.row_map()
    assert n_rows == len(set(T))
    doffs, dids = d.result()
    drows = _rows(eng, doffs, dids)
    assert len(drows) == n_rows and all(drows[int(row_of[i])] == want[i] for i in range(n_pub))
    d.free()
    eng.close()
    R._engine = None
    R._routes.clear()
    S.clear()


def test_three_rounds_keep_no_per_round_memory():
    torch.cuda.init()
    before = _free_bytes()
    kept = []
    for rnd, n_pub in enumerate(SIZES):
        _round(n_pub, 31 + rnd)
        kept.append(before - _free_bytes())
    print("device bytes kept after rounds 1..3:", kept)
    # the runtime keeps some memory of its own after the first round; a buffer
    # that every round left behind would add round two's share on top of it
    assert kept[2] - kept[0] <= LARGEST_ROUND2, kept
