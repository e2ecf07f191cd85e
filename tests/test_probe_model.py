"""The probe-run model (tests/probe_model.py) against the host engine, and the
probe bound (MAX_PROBE_DISP = 48 buckets) on the host -- no device.

    model     the placement simulation and Table(dump) agree with the engine on
              insert-only worlds: per-bucket key sets, largest displacement
    worlds    every world test_gpu_probe_edges.py walks has the shape it claims,
              read from the dumped table alone: the exact displacement of each
              probed key, the reads of each absent key, the wrapped keys' home
              and stored buckets
    bound     a key placed more than 48 buckets from home makes the insert
              re-pack before it returns -- by single inserts, by insert_many
              and by the parallel edge phase -- and stays found; an insert
              that may not re-pack (TM_PROBE_TRIES = 0) returns TM_EOVERFLOW
    churn     seeded insert / delete churn over clustered words keeps the bound
              after every operation and the lookups equal to the oracle trie's
"""

import random

import numpy as np
import pytest

import probe_model as M
from emqx_amd import _native as N
from emqx_amd.engine import Engine
from oracle import oracle as O


# ---- model -----------------------------------------------------------------------------------

def test_hash_restated_matches_the_dump():
    """Every stored key's home bucket, by the restated hash, lies at most
    debug_check() buckets before its bucket, its run full in between."""
    e = Engine(device=-1)
    rng = random.Random(3)
    ws = [b"h%d" % i for i in range(30)]
    for _ in range(600):
        e.insert(b"/".join(rng.choice(ws) for _ in range(rng.randint(1, 4))))
    md = e.debug_check()
    t = M.Table(e.debug_slots())
    assert t.max_disp() == md
    n = 0
    for b, ks in enumerate(t.keys()):
        for p, w in ks:
            h = M.home_bucket(p, w, t.nb)
            assert all(t.full(x) for x in range(h, h + (b - h) % t.nb))
            r = t.run(p, w, M.stepped(md))
            assert r.found and r.disp == (b - h) % t.nb
            n += 1
    assert n == e.stats()["edges"]


@pytest.mark.parametrize("D,bucket", M.STEP_CASES)
def test_simulation_matches_the_engine(D, bucket):
    e = Engine(device=-1)
    w = M.build(e, M.step_world(e, D, bucket))
    t = M.Table(e.debug_slots())
    # the cluster's keys are root keys; the 'w/#' edges hang under three of them
    keys = []
    for f in w["filters"]:
        ws = f.split(b"/")
        if len(ws) == 1:
            keys.append((M.ROOT, M.word_id(e, f)))
        else:
            keys.append((t.node(e, ws[:1]), M.W_HASH))
    buckets, disp = M.simulate(keys)
    assert [set(b) for b in buckets] == t.keys()
    assert max(disp.values()) == D == e.debug_check() == t.max_disp()


# ---- worlds ----------------------------------------------------------------------------------

@pytest.mark.parametrize("D,bucket", M.STEP_CASES)
def test_step_worlds_bite(D, bucket):
    e = Engine(device=-1)
    w = M.build(e, M.step_world(e, D, bucket))
    t = M.check_world(e, w)
    assert w["max_probe"] == {4: 4, 5: 8, 8: 8, 9: 16, 16: 16, 17: 48, 48: 48}[D]
    last = w["found"][-1]
    assert last[3] == D and sorted({f[3] for f in w["found"]}) == list(range(D + 1))
    assert (len(w["wrap"]) > 0) == (bucket + D >= M.NB)
    assert {a[2] for a in w["absent"]} >= {1, 2, D + 1}
    if D == w["max_probe"]:     # the key on the last allowed continuation; an absent run of max_probe reads
        assert t.run(M.ROOT, M.word_id(e, last[0]), D - 1).found is False
        assert D in {a[2] for a in w["absent"]}


@pytest.mark.parametrize("max_probe,first", [(4, 200), (8, 200), (4, 253)])
def test_absent_worlds_bite(max_probe, first):
    e = Engine(device=-1)
    w = M.build(e, M.absent_world(e, max_probe, first))
    t = M.check_world(e, w)
    assert [a[2] for a in w["absent"]] == [max_probe + 1, max_probe, 2, 1]
    assert all(t.full(first + j) for j in range(max_probe + 1)) and not t.full(first + max_probe + 1)
    # the cut run saw no free last slot: one more read would have
    assert t.run(M.ROOT, M.word_id(e, w["absent"][0][0]), max_probe + 1).reads == max_probe + 2
    # no key of the run is displaced: the bound alone cuts it
    assert all(d == 0 for _, _, _, d in w["found"][-4 * (max_probe + 1):])


def test_wrap_world_bites():
    e = Engine(device=-1)
    w = M.build(e, M.wrap_world(e))
    t = M.check_world(e, w)
    homes = {M.home_bucket(M.ROOT, M.word_id(e, x)) for x in w["wrap"]}
    assert homes == {M.NB - 2, M.NB - 1}
    assert {t.where(M.ROOT, M.word_id(e, x))[1] for x in w["wrap"]} == {0, 1, 2, 3, 4, 5}


def test_kinds_world_bites():
    e = Engine(device=-1)
    w = M.kinds_world(e)
    M.check_world(e, w)
    kinds = [(len(path), x) for _, path, x, d in w["found"] if d == M.KIND_D]
    assert (0, b"+") in kinds and (0, b"#") in kinds and (1, b"+") in kinds and (9, b"l10") in kinds
    assert (0, w["dollar_last"]) in kinds and sum(1 for n, x in kinds if n == 1) == 2


def test_change_world_bites():
    e = Engine(device=-1)
    w = M.change_world(e)
    for f in w["first"]:
        e.insert(f)
    assert e.debug_check() == 4
    for f in w["more"]:
        e.insert(f)
    t = M.Table(e.debug_slots())
    assert e.debug_check() == 5 and t.run(M.ROOT, M.word_id(e, w["more"][-1]), 8).disp == 5
    for f in w["gone"]:
        e.delete(f)
    t = M.Table(e.debug_slots())
    # 17 keys of one home bucket, packed again: four full buckets and one key; the probed key moved home-wards
    assert e.debug_check() == 4 and t.run(M.ROOT, M.word_id(e, w["more"][-1]), 8).disp < 5
    # every run of the batch ends at a free last slot: its reads do not depend on the step
    for x in w["topics"]:
        assert t.run(M.ROOT, M.word_id(e, x), 4).reads == t.run(M.ROOT, M.word_id(e, x), 8).reads


# ---- the bound -------------------------------------------------------------------------------

def run_of_70(e):
    """70 neighbouring buckets of the fresh table filled by four keys of their
    own each, then one more key homed in the first: placed 70 buckets out."""
    fs = []
    for j in range(70):
        fs += M.pick(e, M.ROOT, 10 + j, 4)
    return fs + M.pick(e, M.ROOT, 10, 1, skip=4)


def check_bound(e, fs):
    assert e.debug_check() <= M.MAX_PROBE_DISP
    t = M.Table(e.debug_slots())
    assert t.max_disp() <= M.MAX_PROBE_DISP and t.nb > M.NB
    for f in fs:
        assert e.lookup(f) == (0, f), f
        assert t.run(M.ROOT, M.word_id(e, f), M.MAX_PROBE_DISP).found


def test_bound_by_single_insert():
    e = Engine(device=-1)
    fs = run_of_70(e)
    buckets, disp = M.simulate([(M.ROOT, M.word_id(e, f)) for f in fs])
    assert disp[(M.ROOT, M.word_id(e, fs[-1]))] == 70       # what the 256-bucket table would hold
    for f in fs[:-1]:
        e.insert(f)
    assert e.debug_check() == 0 and e.debug_slots()[1] == M.NB
    e.insert(fs[-1])
    check_bound(e, fs)


def test_bound_by_insert_many():
    e = Engine(device=-1)
    fs = run_of_70(e)
    assert e.insert_many(fs) == len(fs)
    check_bound(e, fs)


def test_bound_given_up_is_an_error_and_the_next_insert_recovers(monkeypatch):
    """TM_PROBE_TRIES = 0: the insert may not double the table.  It returns
    TM_EOVERFLOW, its filter stays, the table check fails; the next insert
    re-packs first and the bound holds again."""
    monkeypatch.setenv("TM_PROBE_TRIES", "0")
    e = Engine(device=-1)
    monkeypatch.delenv("TM_PROBE_TRIES")
    fs = run_of_70(e)
    for f in fs[:-1]:
        e.insert(f)
    with pytest.raises(N.TmError) as err:
        e.insert(fs[-1])
    assert err.value.rc == N.TM_EOVERFLOW
    assert b"70 buckets from home" in N.lib().tm_last_error()
    assert e.lookup(fs[-1]) == (0, fs[-1]) and e.debug_slots()[1] == M.NB
    assert M.Table(e.debug_slots()).max_disp() == 70
    with pytest.raises(N.TmError) as err:
        e.debug_check()
    assert err.value.rc == N.TM_EIO and "exceeds the probe bound" in str(err.value)
    e.insert(b"one/more")
    check_bound(e, fs)


def test_bound_by_the_parallel_edge_phase(monkeypatch, capfd):
    """2,048 filters into a trie of 9,000 take the parallel path (its trace
    says so).  468-odd of them are the pool's words from one narrow range of
    the hash: neighbours in a table of any size, so one doubling is not
    enough and the edge phase doubles until the bound holds."""
    monkeypatch.setenv("TM_PAR_TRACE", "1")
    e = Engine(device=-1, host_threads=4)
    words, ids = M.pool_ids(e)
    assert e.insert_many([b"b%06d" % i for i in range(9000)]) == 9000
    h = np.array([M.edge_hash(M.ROOT, i) for i in ids.tolist()], dtype=np.int64)
    lo = 1 << 30
    cluster = [w for w, x in zip(words, h) if lo <= x < lo + (1 << 25)]       # 1/128 of the hash range
    rest = [w for w, x in zip(words, h) if not (lo - (1 << 27) <= x < lo + (1 << 28))]
    assert 400 <= len(cluster) <= 540
    # in the table the batch is placed into, the cluster alone overruns the bound
    fs = rest[:2048 - len(cluster)] + cluster
    capfd.readouterr()
    assert e.insert_many(fs) == 2048
    assert "[par edges" in capfd.readouterr().err
    assert e.debug_check() <= M.MAX_PROBE_DISP
    t = M.Table(e.debug_slots())
    nb0 = (int((9000 + 2048) / 0.55) + 3) // 4          # the re-pack ahead of the inserts
    assert t.nb >= 4 * nb0, (t.nb, nb0)                 # two doublings at least
    for f in cluster:
        assert e.lookup(f) == (0, f)


# ---- churn -----------------------------------------------------------------------------------

def test_clustered_churn_keeps_the_bound():
    """Insert / delete churn over words of three narrow hash ranges (long runs
    in a table of any size): the bound holds after every operation, the table
    invariants with it, and lookups equal the oracle trie's."""
    rng = random.Random(17)
    e, t = Engine(device=-1), O.Trie()
    words, ids = M.pool_ids(e)
    h = np.array([M.edge_hash(M.ROOT, i) for i in ids.tolist()], dtype=np.int64)
    pool = []
    for lo in (1 << 28, 3 << 30, (1 << 32) - (1 << 24)):        # the last range ends at the table's end
        pool += [w for w, x in zip(words, h) if lo <= x < lo + (1 << 24)]
    assert len(pool) > 600
    pool += [a + b"/" + b for a, b in zip(pool[:200], pool[200:400])]
    live, worst = set(), 0
    for step in range(2500):
        f = rng.choice(pool)
        if f in live and rng.random() < 0.6:
            e.delete(f)
            t.delete(f)
            live.discard(f)
        else:
            e.insert(f)
            t.insert(f)
            live.add(f)
        md = e.debug_check()
        assert md <= M.MAX_PROBE_DISP
        worst = max(worst, md)
    assert worst > 16, worst        # the runs did get long: max_probe reached its top step
    for g in pool:
        exp, got = t.lookup(g), e.lookup(g)
        assert (got is None) == (not exp), g
        if got is not None:
            assert got == (exp[0][1], exp[0][2]), g
