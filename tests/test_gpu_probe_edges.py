"""The walks' probe runs at their displacement steps, wrap and tail edges --
needs an MI355X.

A key that did not fit its home bucket sits up to max_disp buckets further
on; the tile walk follows it by re-pushing the probe as a continuation
(displacement + 1 in the entry's meta word), the generic walk by looping in
probe(), both for at most max_probe + 1 buckets: max_disp stepped up to 4, 8,
16 or 48.  The worlds of tests/probe_model.py put keys at chosen
displacements in a 256-bucket table (test_probe_model.py proves their shape
on the host); here every case compares

    rows    with the oracle's (filter bytes, in order), and
    reads   stats()["probes"] with the bucket reads counted off the dumped
            table (probe_model.Table), wherever the whole batch stays on the
            tile path -- which shows that a found key, a free last slot and the
            bound each end a run where they should.

    steps     a key at displacement 4, 5, 8, 9, 16, 17 and 48 (max_probe 4, 8,
              8, 16, 16, 48, 48) with its neighbours at every smaller one, and
              absent keys whose runs end after 1, 2, max_probe, D + 1 reads
    absent    max_probe + 1 full buckets of undisplaced keys: cut by the bound
    wrap      clusters homed in the last two buckets, stored in buckets 0 .. 5
    kinds     continued '+', '#' (M_SKIPE), $-start (M_DSTART), non-root and
              level-10 probes, each five buckets from home
    tiles     16,448 / 65 / 1 topics: whole tiles of continuing lanes
    generic   the same root keys as first words of 11-word and '+x' topics
    change    max_probe 4 -> 8 -> 4 between launches of one prepared batch

No launch here runs against a table above the bound: every one is preceded by
the host's check (tm_debug_check <= 48).
"""

import pytest

import probe_model as M
from emqx_amd.engine import Engine
from test_gpu_walk_loop import device_rows, differing, oracle_rows, tile_topics

pytestmark = pytest.mark.gpu


def guarded_rows(eng, T, batch=None):
    """device_rows behind the host's check of the bound."""
    assert eng.debug_check() <= M.MAX_PROBE_DISP
    return device_rows(eng, T, batch=batch)


def check_batch(eng, table, F, T, max_probe, batch=None):
    """Rows against the oracle and, the batch being all on the tile path, the
    bucket reads against the table-driven count; -> stats."""
    U = sorted(set(T))
    exp = dict(zip(U, oracle_rows(sorted(F), U)))
    got, st = guarded_rows(eng, T, batch=batch)
    assert not differing(T, got, [exp[t] for t in T])
    assert st["slow_topics"] == 0 and st["overflow_tiles"] == 0
    want = M.batch_reads(eng, table, T, max_probe)
    print("probes", st["probes"], "table-driven", want)
    assert st["probes"] == want
    return st


# ---- steps -----------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=M.STEP_CASES, ids=lambda c: "D%d" % c[0])
def step(request):
    D, bucket = request.param
    eng = Engine(device=0)
    w = M.build(eng, M.step_world(eng, D, bucket))
    eng.sync()
    return eng, w


def test_steps_found_at_every_displacement(step):
    """The cluster's 4 D + 1 keys sit at displacements 0 .. D, the last on
    continuation D (for D = max_probe the last one allowed); the absent keys'
    runs end at the cluster's tail bucket."""
    eng, w = step
    table = M.check_world(eng, w)
    check_batch(eng, table, w["filters"], [w["found"][-1][0]], w["max_probe"])     # the deepest key alone
    check_batch(eng, table, w["filters"], w["topics"], w["max_probe"])


def test_steps_generic_path_walks_the_same_runs(step):
    """The displaced, absent and wrapped root keys as first words of 11-word
    topics and of topics with an irregular '+x' word: probe() follows the
    runs; 'w/#' gives the found ones their rows."""
    eng, w = step
    M.check_world(eng, w)       # (the '#' edges did not move the keys under test)
    firsts = w["deep"] + [a[0] for a in w["absent"]] + w["wrap"][-2:]
    tail = b"/".join(b"g%d" % i for i in range(10))
    T = [f + b"/" + tail for f in firsts] + [f + b"/+x" for f in firsts]
    exp = oracle_rows(sorted(w["filters"]), T)
    assert [r for r in exp if r] and [r for r in exp if not r]
    got, st = guarded_rows(eng, T)
    assert st["slow_topics"] == len(T)
    assert not differing(T, got, exp)


# ---- absent keys cut by the bound ------------------------------------------------------------

@pytest.mark.parametrize("max_probe,first", [(4, 200), (8, 200), (4, 253)])
def test_absent_runs_tail_cut_and_wrap(max_probe, first):
    eng = Engine(device=0)
    w = M.build(eng, M.absent_world(eng, max_probe, first))
    eng.sync()
    table = M.check_world(eng, w)
    check_batch(eng, table, w["filters"], w["topics"], max_probe)
    # the absent keys alone: max_probe + 1, max_probe, 2 and 1 reads
    T = [a[0] for a in w["absent"]]
    st = check_batch(eng, table, w["filters"], T, max_probe)
    assert st["probes"] == 2 * max_probe + 4


# ---- wrap ------------------------------------------------------------------------------------

def test_wrapped_clusters():
    eng = Engine(device=0)
    w = M.build(eng, M.wrap_world(eng))
    eng.sync()
    table = M.check_world(eng, w)
    assert len(w["wrap"]) >= 20
    check_batch(eng, table, w["filters"], w["topics"], w["max_probe"])


# ---- continued probe kinds -------------------------------------------------------------------

def test_continued_probe_kinds():
    eng, twin = Engine(device=0), Engine(device=0, host_tokenize=True)
    w = M.kinds_world(eng, twin)
    eng.sync()
    twin.sync()
    table = M.check_world(eng, w)
    M.check_world(twin, w)
    T = w["topics"]
    st = check_batch(eng, table, w["filters"], T, w["max_probe"])
    got2, st2 = guarded_rows(twin, T)
    got, _ = guarded_rows(eng, T)
    assert got == got2
    assert st["visits"] == st2["visits"] and st["probes"] == st2["probes"]
    # each kind alone in a batch of its own: the continued probe is the batch
    for t in (b"k00000", b"#", w["dollar_last"], w["dollar_last"] + b"/x", T[10], T[13]):
        check_batch(eng, table, w["filters"], [t], w["max_probe"])


# ---- tile shapes -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def d9():
    eng = Engine(device=0)
    w = M.build(eng, M.step_world(eng, 9, 250))
    eng.sync()
    return eng, w


def test_whole_tiles_of_continuing_lanes(d9):
    """16,448 topics: 64-topic tiles.  Tiles of the deepest key alone (all 64
    lanes continue in the same iteration, nine times over), tiles that
    alternate it with a key found at home, tiles over the whole cluster."""
    eng, w = d9
    table = M.check_world(eng, w)
    deep, home = w["found"][-1][0], w["found"][0][0]
    T = [deep] * 128 + [deep, home] * 64 + [deep] * 63 + [home]
    T += [w["topics"][i % len(w["topics"])] for i in range(16448 - len(T))]
    assert len(T) == 16448 and tile_topics(len(T)) == 64
    check_batch(eng, table, w["filters"], T, w["max_probe"])


@pytest.mark.parametrize("n", [1, 65])
def test_small_batches_of_continuing_lanes(d9, n):
    eng, w = d9
    table = M.check_world(eng, w)
    deep, home = w["found"][-1][0], w["found"][0][0]
    T = ([deep, home, w["absent"][-1][0]] * 22)[:n]
    assert tile_topics(n) < 64
    check_batch(eng, table, w["filters"], T, w["max_probe"])


# ---- the step changes under a prepared batch -------------------------------------------------

def test_step_change_between_launches_of_one_batch():
    eng = Engine(device=0)
    w = M.change_world(eng)
    for f in w["first"]:
        eng.insert(f)
    eng.sync()
    T = w["topics"]
    b = eng.prepare(T)
    F = list(w["first"])
    assert eng.debug_check() == 4
    check_batch(eng, M.Table(eng.debug_slots()), F, T, 4, batch=b)
    for f in w["more"]:
        eng.insert(f)
    F += w["more"]
    assert eng.debug_check() == 5
    table = M.Table(eng.debug_slots())
    assert table.run(M.ROOT, M.word_id(eng, w["more"][-1]), 8).disp == 5
    u0 = eng.stats()["uploads_delta"]
    check_batch(eng, table, F, T, 8, batch=b)
    assert eng.stats()["uploads_delta"] == u0 + 1       # the delta upload carried the slots
    for f in w["gone"]:
        eng.delete(f)
    F = [f for f in F if f not in w["gone"]]
    table = M.Table(eng.debug_slots())
    assert table.run(M.ROOT, M.word_id(eng, w["more"][-1]), 8).disp < 5
    # (every run of the batch ends at a free last slot: the count is the same under either step)
    assert M.batch_reads(eng, table, T, 4) == M.batch_reads(eng, table, T, 8)
    check_batch(eng, table, F, T, 8, batch=b)
    b.free()
