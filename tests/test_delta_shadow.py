"""The delta-upload path's host logic against a shadow replica -- no GPU.

tm_engine::sync_device gathers the dirty slots, filter-metadata nodes and
dictionary keys once, applies them to every replica, then empties the dirty
sets.  tm_debug_shadow_sync runs the same gather and consume stages around a
host-memory stand-in for a replica (the seven tables, grown and recopied by
the replicas' rules, a regrown buffer losing its contents) and compares it
with the host tables element by element.  So a forgotten mark_dirty, a stale
*_uploaded mark or the wrong side of a full-or-delta switch shows here as a
non-zero difference, whichever slot it hits -- no topic has to probe it.

Every case asserts its precondition from tm_debug_upload_info first (exact
threshold hits, needs_repack, displacement >= 2, >= 8,192 dirty slots), then
that the comparison SEES the mutation before the apply (a comparison that
cannot see a stale table proves nothing), then that the apply leaves no
difference, tm_debug_check passes and lookups equal oracle.Trie's.

Not covered here: the copies and the scatter kernels themselves
(tests/test_gpu_delta_upload.py reads the device's tables back).
"""

import functools

import pytest

from emqx_amd import _native as N
from emqx_amd.engine import Engine
from oracle import oracle as O

LIVE = [t for t in N.DIFF_TABLES if not t.endswith("_dead")]


def in_sync(d):
    """No difference in any table (metadata of nodes that are no filter is never read)."""
    return all(d[t] == (0, None) for t in LIVE)


def settle(e):
    """One apply; -> (the comparison before it, the upload info before it, the info after)."""
    before, u0 = e.shadow_sync(apply=False), e.upload_info()
    after = e.shadow_sync(apply=True)
    assert in_sync(after), after
    u1 = e.upload_info()
    assert (u1["dirty"], u1["full_dirty"], u1["dirty_f"], u1["full_f_dirty"], u1["dict_dirty"]) == (0, 0, 0, 0, 0)
    assert in_sync(e.shadow_sync(apply=False))
    return before, u0, u1


def delta(u0, u1, *names):
    return tuple(u1[n] - u0[n] for n in names)


def same_lookups(e, t, nodes):
    for g in nodes:
        exp, got = t.lookup(g), e.lookup(g)
        assert (got is None) == (not exp), g
        if got is not None:
            assert got == (exp[0][1], exp[0][2]), g


class Pair:
    """An engine and the oracle trie, mutated together."""

    def __init__(self, **kw):
        self.e, self.t, self.seen = Engine(device=-1, **kw), O.Trie(), set()

    def insert(self, f):
        self.e.insert(f)
        self.t.insert(f)
        self.seen.add(f)

    def delete(self, f):
        self.e.delete(f)
        self.t.delete(f)

    def check(self):
        same_lookups(self.e, self.t, self.seen)
        return self.e.debug_check()


def fresh(**kw):
    """A settled engine: the first apply (everything whole) is behind it."""
    p = Pair(**kw)
    u = p.e.upload_info()
    assert u["full_dirty"] == 1 and u["full_f_dirty"] == 1      # a new engine uploads whole
    before, _, u1 = settle(p.e)
    assert before["slots"][0] == u["slots"] and before["dkey"][0] == u["dict_keys"]   # the shadow started empty
    assert (u1["uploads_full"], u1["fmeta_full"], u1["keys_full"], u1["slots_realloc"]) == (1, 1, 1, 1)
    return p


# ---- the 1/8 switches ---------------------------------------------------------------------------

def test_slot_switch_exactly_an_eighth_is_a_delta_and_one_more_is_whole():
    p = fresh()
    e = p.e
    slots = e.upload_info()["slots"]
    assert slots == 1024                       # the smallest table: 256 buckets x 4
    n = 0
    for target, whole in ((slots // 8, False), (slots // 8 + 1, True)):
        while e.upload_info()["dirty"] < target:        # one-word filters under the root: the finest step
            p.insert(b"s%d" % n)
            n += 1
        before, u0, u1 = settle(e)
        assert u0["dirty"] == target and u0["slots"] == slots and not u0["full_dirty"]
        assert before["slots"][0] == target
        if whole:
            assert delta(u0, u1, "uploads_full", "uploads_delta", "delta_slots", "slots_realloc") == (1, 0, 0, 0)
        else:
            assert delta(u0, u1, "uploads_full", "uploads_delta", "delta_slots", "slots_realloc") == (0, 1, target, 0)
        # the filter metadata went with it, as a scatter of exactly the new filters
        assert delta(u0, u1, "fmeta_full", "fmeta_delta", "fmeta_nodes") == (0, 1, u0["dirty_f"])
        assert before["flen"][0] == u0["dirty_f"]
        p.check()


@pytest.mark.parametrize("whole", [False, True])
def test_dictionary_switch_an_eighth_of_the_key_slots(whole):
    p = fresh(init_slots=16384)                # (the edge hash stays far below its own switch)
    e = p.e
    keys = e.upload_info()["dict_keys"]
    assert keys == 1024
    target = keys // 8 + (1 if whole else 0)
    n = 0
    while e.upload_info()["dict_dirty"] < target:
        p.insert(b"k%d" % n)                   # a new word each: one key slot, or a few when keys are evicted
        n += 1
    before, u0, u1 = settle(e)
    assert u0["dict_dirty"] == target and u0["dict_keys"] == keys and u0["dirty"] <= u0["slots"] // 8
    assert before["dkey"][0] >= n              # every new word's key differs before the apply
    if whole:
        assert delta(u0, u1, "keys_full", "keys_delta", "keys_scattered") == (1, 0, 0)
    else:
        # (a slot written twice is listed twice and scattered once)
        assert delta(u0, u1, "keys_full", "keys_delta") == (0, 1)
        assert n <= u1["keys_scattered"] - u0["keys_scattered"] <= target
    assert delta(u0, u1, "dict_gen") == (0,)
    p.check()


def test_dictionary_rebuild_and_the_tails_across_their_capacities():
    p = fresh(init_slots=65536)
    e = p.e
    u = e.upload_info()
    gen, n, rounds = u["dict_gen"], 0, []
    # rounds of 150 new 17-byte words (arena bytes past the inline 16): the
    # key table is rebuilt when a quarter full (257 words in 1,024 slots,
    # then 513, 1,025, ...), the tails' buffer starts at 1,024 entries and the
    # arena's at 1,024 bytes
    for rnd in range(16):
        for _ in range(150):
            p.insert(b"longish-word-%04d" % n)
            n += 1
        before, u0, u1 = settle(e)
        assert before["dkey"][0] and before["tail"][0] and before["arena"][0] and before["fbytes"][0]
        rebuilt = u0["dict_gen"] != gen
        gen = u0["dict_gen"]
        if rebuilt:                            # a rebuild is a whole copy however few keys are listed
            assert delta(u0, u1, "keys_full", "keys_delta") == (1, 0)
        rounds.append((rebuilt, u0["dict_keys"], u0["dict_dirty"], delta(u0, u1, "keys_full")[0]))
        assert delta(u0, u1, "tail_pinned", "tail_pageable") == (3, 0)     # filter bytes, tails, arena: small
    u = e.upload_info()
    assert u["dict_tails"] > 2 * 1024 and u["dict_arena"] > 16 * 1024     # both buffers regrown several times
    assert sum(r[0] for r in rounds) >= 3                                  # 1,024 -> 2,048 -> 4,096 -> ... slots
    assert any(not r[0] and r[3] == 0 for r in rounds)                     # and rounds that scattered keys
    p.check()


# ---- every path that changes a slot ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def crowded_filters():
    return [b"p%d/q%d" % (i % 37, i) for i in range(700)]


def crowded():
    """1,024 slots at load 0.72, just under the growth threshold of 3/4: keys sit buckets away from home."""
    p = fresh(init_slots=1024)
    for f in crowded_filters():
        p.insert(f)
    settle(p.e)
    assert p.e.upload_info()["slots"] == 1024
    assert p.check() >= 2
    return p


SLOT_PATHS = {
    "insert": [("insert", b"p5/new")],
    "delete": [("delete", b"p5/q5")],
    "hash_leaf": [("insert", b"p7/#"), ("delete", b"p7/#")],                  # set_topic rewrites p7's summary
    "plus_chain": [("insert", b"+/+/+"), ("insert", b"p9/+/+/x"), ("delete", b"+/+/+"), ("delete", b"p9/+/+/x")],
    "last_child": [("insert", b"solo/only/leaf"), ("delete", b"solo/only/leaf")],   # the parents die with it
    "root_hash": [("insert", b"#"), ("delete", b"#")],
    "subscribe": [("subscribe", b"p3/+/sub"), ("unsubscribe", b"p3/+/sub")],
}


@pytest.mark.parametrize("path", sorted(SLOT_PATHS))
def test_every_slot_changing_path_reaches_the_shadow(path):
    p = crowded()
    e = p.e
    for op, f in SLOT_PATHS[path]:
        if op == "insert":
            p.insert(f)
        elif op == "delete":
            p.delete(f)
        elif op == "subscribe":                # the broker's entry points reach the trie through the route table
            e.subscribe(f, 7)
            p.t.insert(f)
            p.seen.add(f)
        else:
            assert e.unsubscribe(f, 7)
            p.t.delete(f)
        u = e.upload_info()
        assert u["slots"] == 1024 and not u["full_dirty"], (op, f)     # still the crowded table, and a delta
        before, u0, u1 = settle(e)
        if f != b"#":                          # (the root's record is no slot: it is rebuilt at every launch)
            assert before["slots"][0] >= 1 and before["slots"][0] == u0["dirty"], (op, f)
            assert delta(u0, u1, "uploads_delta", "delta_slots") == (1, u0["dirty"])
        assert p.check() >= 2, (op, f)


def test_backward_shift_deletion_moves_reach_the_shadow():
    """Deleting from full buckets pulls later keys back across buckets (move_slot):
    both ends of every move must be listed."""
    p = crowded()
    e = p.e
    most = 0
    for f in crowded_filters()[:120]:
        p.delete(f)
        before, u0, u1 = settle(e)
        assert u0["slots"] == 1024 and not u0["full_dirty"]
        assert before["slots"][0] == u0["dirty"] >= 1
        most = max(most, u0["dirty"])
    # a leaf's delete without a move lists its slot and its parent's: more means moves
    assert most >= 5
    assert p.check() >= 1
    for f in crowded_filters()[:60]:           # and back in, through the holes
        p.insert(f)
        settle(e)
    assert p.check() >= 2


def test_growth_reallocates_and_recopies():
    p = crowded()
    e = p.e
    n = 0
    while e.upload_info()["slots"] == 1024:    # through the 3/4-load rehash
        p.insert(b"grow/%d" % n)
        n += 1
    before, u0, u1 = settle(e)
    assert u0["slots"] > 1024 and u0["full_dirty"] == 1 and u0["dirty"] == 0
    assert before["slots"][0] >= 1024 // 2     # the keys moved to other slots; the shadow has no room for the rest
    assert delta(u0, u1, "slots_realloc", "uploads_full", "uploads_delta") == (1, 1, 0)
    p.check()
    p.insert(b"grow/after")                    # and deltas go on in the new table
    before, u0, u1 = settle(e)
    assert delta(u0, u1, "slots_realloc", "uploads_full", "uploads_delta") == (0, 0, 1)


# ---- re-pack, both sides; parallel batches on the re-packed table -----------------------------------

N_BULK = 70_000
REPACK = {"dense": 131_072, "sparse": 1_048_576}      # loads 0.54 > 0.525 and 0.067 < 0.175


@functools.lru_cache(maxsize=None)
def bulk_filters():
    return [b"r%d/s%d" % (i % 300, i) for i in range(N_BULK)]


def repacked(side, threads):
    e, t = Engine(device=-1, init_slots=REPACK[side], host_threads=threads), O.Trie()
    F = bulk_filters()
    assert e.insert_many(F) == N_BULK
    for f in F:
        t.insert(f)
    gone = F[:300:3]                           # literal children deleted before the re-pack: stale signature bits
    for f in gone:
        e.delete(f)
        t.delete(f)
    u = e.upload_info()
    edges = e.stats()["edges"]
    assert edges > 65536 and u["slots"] == REPACK[side] and u["needs_repack"] == 1
    before, u0, u1 = settle(e)
    assert before["slots"][0] == u["slots"]
    assert delta(u0, u1, "repacks", "uploads_full", "slots_realloc") == (1, 1, 1)
    assert u1["needs_repack"] == 0 and abs(edges / u1["slots"] - 0.35) < 0.01      # target_load
    e.debug_check()
    same_lookups(e, t, F[::50] + F[:300])
    return e, t, F


@pytest.mark.parametrize("side", ["dense", "sparse"])
def test_repack_both_sides(side):
    e, t, F = repacked(side, 1)
    # a literal child goes after the re-pack: its slot's and its parent's change reach the shadow
    e.delete(F[301])
    t.delete(F[301])
    before, u0, u1 = settle(e)
    assert before["slots"][0] >= 1 and delta(u0, u1, "repacks", "uploads_delta") == (0, 1)
    e.debug_check()
    same_lookups(e, t, F[::50] + F[:302])


@pytest.mark.parametrize("threads", [1, 4])
def test_parallel_batches_gather_on_the_workers(threads):
    """insert_many / delete_many / apply_many of 9,000 filters on the re-packed table
    (200,860 slots): at least 8,192 dirty slots, so with 4 host threads the
    gather runs in chunks on the workers, and at most slots / 8, so it is a delta."""
    e, t, F = repacked("sparse", threads)
    add = [b"r%d/n%d" % (i % 300, i) for i in range(9000)]
    more = [b"r%d/m%d/+" % (i % 300, i) for i in range(4500)]
    probe = F[::50] + add[::9] + more[::9] + F[1000:1100]
    steps = [
        ("insert_many", lambda: e.insert_many(add), add, []),
        ("delete_many", lambda: e.delete_many(add), [], add),
        ("apply_many", lambda: e.apply_many(F[1000:5500], more), more, F[1000:5500]),   # deletes and inserts, planned together
    ]
    for name, run, ins, dels in steps:
        done = run()
        assert done in (9000, (4500, 4500)), name
        for f in dels:
            t.delete(f)
        for f in ins:
            t.insert(f)
        u = e.upload_info()
        assert 8192 <= u["dirty"] <= u["slots"] // 8 and not u["full_dirty"], (name, u["dirty"])
        before, u0, u1 = settle(e)
        assert before["slots"][0] == u0["dirty"], name
        assert delta(u0, u1, "uploads_delta", "delta_slots", "uploads_full") == (1, u0["dirty"], 0), name
        if ins:
            assert u0["dirty_f"] >= len(ins) and delta(u0, u1, "fmeta_delta", "fmeta_nodes") == (1, u0["dirty_f"])
        e.debug_check()
        same_lookups(e, t, probe)


# ---- a filter id handed to another filter -----------------------------------------------------------

def test_reused_filter_id_carries_the_new_offset_and_length():
    p = fresh()
    e = p.e
    a = b"reuse/this/filter/id"
    for f in (b"keep/one", a, b"keep/two"):
        p.insert(f)
    settle(e)
    fid = e.filter_id(a)
    p.delete(a)                                # no batch is live on a host-only engine: the id is free at once
    settle(e)
    for i in range(8):                         # shorter, of other bytes; one of them takes the id
        b = b"b%d" % i
        p.insert(b)
        if e.filter_id(b) == fid:
            break
        settle(e)                              # (the ids of A's dead parents go first)
    assert e.filter_id(b) == fid and e.filter_bytes(fid) == b and len(b) != len(a)
    before = e.shadow_sync(apply=False)
    # the shadow still holds A's (offset, length) under that id, and lacks B's bytes
    assert before["foff"] == (1, fid) and before["flen"] == (1, fid) and before["fbytes"][0] == len(b)
    _, u0, u1 = settle(e)
    assert delta(u0, u1, "fmeta_delta", "fmeta_nodes", "fmeta_full") == (1, 1, 0)
    p.check()


# ---- the hooks themselves ---------------------------------------------------------------------------

def test_upload_info_reads_only_and_names_every_field():
    e = Engine(device=-1)
    e.insert(b"a/b")
    u = e.upload_info()
    assert list(u) == list(N.UPLOAD_INFO) and e.upload_info() == u
    assert (u["full_dirty"], u["nodes"], u["fbytes"], u["uploads_full"]) == (1, 3, 3, 0)
    d = e.shadow_sync(apply=False)
    assert list(d) == list(N.DIFF_TABLES) and e.upload_info() == u
    with pytest.raises(N.TmError) as ei:       # no replica to read back
        e.replica_diff(0, sync=False)
    assert ei.value.rc == N.TM_ENODEV
