"""The host model of the device fan-out (tests/fanout_model.py): its constants
against the source text, its arrays against a loop over the publishes, and
every layout of tests/test_gpu_fanout_edges.py against the shape it is named
for -- so a device test never passes on drifted inputs.  Where a kernel line
cannot be mutated safely on a device (a wrong index there reads or writes
outside an array), the test here shows that a layout reaches the line.  No GPU."""

import os
import re

import fanout_model as M
import numpy as np
import pytest

from emqx_amd import emqx_topic as T
from emqx_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    with open(os.path.join(ROOT, "emqx_amd", "csrc", name)) as f:
        return f.read()


def _entries(lay, k):
    jlo, jhi, ne, staged = (int(x) for x in lay.tiles()[k])
    return jlo, jhi, ne, bool(staged)


# ------------------------------------------------------------------ the model

def test_constants_are_the_sources():
    hip, cpp, hpp = _src("tm_kernels.hip"), _src("tm_fanout.cpp"), _src("tm_internal.hpp")
    assert int(re.search(r"constexpr uint32_t FAN_BLOCK = (\d+);", hip).group(1)) == M.FAN_BLOCK == 256
    assert int(re.search(r"constexpr uint32_t FAN_PER = (\d+);", hip).group(1)) == M.FAN_PER == 16
    assert "constexpr uint32_t FAN_SCAN_TILE = FAN_BLOCK * FAN_PER;" in hip and M.FAN_SCAN_TILE == 4096
    assert int(re.search(r"#define TM_FAN_FILL_PER (\d+)", hip).group(1)) == M.FAN_FILL_PER == 8
    assert "constexpr uint32_t FAN_FILL_TILE = FAN_BLOCK * FAN_FILL_PER;" in hip and M.FAN_FILL_TILE == 2048
    assert "constexpr uint32_t FAN_LDS_ENTRIES = FAN_FILL_TILE * 3 / 4;" in hip and M.FAN_LDS_ENTRIES == 1536
    assert int(re.search(r"constexpr uint32_t TICKET_GROUPS = (\d+),", hpp).group(1)) == M.TICKET_GROUPS == 8
    # a scan thread's entries are consecutive; its vector load and store conditions
    assert "const uint64_t j0 = (uint64_t)blockIdx.x * FAN_SCAN_TILE + (uint64_t)threadIdx.x * FAN_PER;" in hip
    assert "if (j0 + FAN_PER <= a.n_matches) {" in hip and "if (!big && j0 + FAN_PER <= a.n_matches + 1) {" in hip
    # the 1-byte run length and its saturation, on the host and on the device
    assert "(uint8_t)std::min<uint64_t>(h_soff[i + 1] - h_soff[i], 255);" in cpp
    assert "c[k] = s1 < 255 ? s1 : a.soff[f[k] + 1] - a.soff[f[k]];" in hip and M.SCNT_SAT == 255
    # the inline subscriber of a run of one, and who reads it back
    assert "if (h_soff[i + 1] - h_soff[i] == 1) h_sone[i] = h_subs[h_soff[i]];" in cpp
    assert hip.count("m1[u] - m0[u] == 1 ? INT64_MIN + (int64_t)a.sone[f[u]]") == 1
    assert hip.count("m1 - m0 == 1 ? INT64_MIN + (int64_t)a.sone[f[u]]") == 1
    assert "r[u] = bs < INT64_MIN + (1ll << 33) ? (uint32_t)(bs - INT64_MIN)" in hip
    # the width of a block's offsets, the staging threshold, the tile search and its tie rule
    assert "const bool big = total > a.big_limit;" in hip and hip.count("a.total > a.big_limit") == 2
    assert "if (ne > FAN_LDS_ENTRIES) {" in hip
    assert "a.tile_j[k] = fan_upper(a, 0, a.n_matches + 1, p) - 1;" in hip
    assert "const uint64_t p = k < ntiles ? k * FAN_FILL_TILE : a.total - 1;" in hip
    assert "if (fan_moff(a, m) > p) hi = m;" in hip
    assert "const uint64_t m1 = r1[u] + ((j + 1) / FAN_SCAN_TILE != sb0 ? bs1 : bs0);" in hip
    assert "const uint32_t per = (nb + FAN_BLOCK - 1) / FAN_BLOCK;" in hip
    assert "(nm + 1 + fan_scan_tile() - 1) / fan_scan_tile()" in cpp
    # TM_FAN_BIG: set to 0 is a limit, not "unset"
    assert "k.fan_big_set = true;" in hpp and "if (kn.fan_big_set) fan_big_limit = kn.fan_big;" in _src("tm_pipeline.cpp")
    assert "uint64_t fan_big_limit = 0xFFFFFFFFull;" in _src("tm_engine_impl.hpp") and M.DEFAULT_BIG_LIMIT == 0xFFFFFFFF


@pytest.mark.parametrize("value, limit", [(None, 0xFFFFFFFF), ("0", 0), ("1", 1), ("4500", 4500),
                                          ("99999999999", 0xFFFFFFFF)])
def test_fan_big_knob_is_applied_when_set(value, limit, monkeypatch):
    """TM_FAN_BIG=0 used to be taken for "unset": the engine kept 2^32 - 1."""
    monkeypatch.delenv("TM_FAN_BIG", raising=False)
    if value is not None:
        monkeypatch.setenv("TM_FAN_BIG", value)
    assert Engine(device=-1).fan_big_limit == limit


def test_model_by_hand():
    lay = M.Layout("hand", [2, 0, 1, (b"own", (70, 80, 90)), 2, 2, 2, 2])
    assert lay.topics == [b"r2/0", b"r0/0", b"r1/0", b"x/own", b"r2/1", b"r2/2", b"r2/0", b"r2/1"]
    assert lay.runs.tolist() == [2, 0, 1, 3, 2, 2, 2, 2]
    assert lay.moff.tolist() == lay.offs.tolist() == [0, 2, 2, 3, 6, 8, 10, 12, 14]
    s = M.pooled_subs
    assert lay.out.tolist() == s(2, 0) + s(1, 0) + [70, 80, 90] + s(2, 1) + s(2, 2) + s(2, 0) + s(2, 1)
    assert len({x for r in (1, 2, 300) for k in range(M.POOL) for x in s(r, k)}) == 3 * 303
    assert lay.block_totals().tolist() == [14] and lay.big(13).tolist() == [True] and lay.big(14).tolist() == [False]
    assert lay.tiles().tolist() == [[0, 7, 8, 1]]
    # among equal offsets the entry that has the delivery: delivery 2 is entry 2's, not zero-run entry 1's
    assert M.entry_of(lay.moff, [0, 1, 2, 3, 13]).tolist() == [0, 0, 2, 3, 7]
    subs, offs, pubs, fids = lay.inboxes(100 + lay.fidx)
    assert subs.tolist() == sorted(set(lay.out.tolist())) and offs[-1] == 14
    k = subs.tolist().index(s(2, 0)[1])
    assert pubs[offs[k]:offs[k + 1]].tolist() == [0, 6] and fids[offs[k]:offs[k + 1]].tolist() == [100, 100]
    e = M.Layout("none", [])
    assert e.n == 0 and e.moff.tolist() == [0] and len(e.out) == 0 and len(e.tiles()) == 0
    assert e.block_totals().tolist() == [0]


def _small_layouts():
    return ([M.scan_tail(n, z) for n in (15, 17, 4097) for z in (False, True)] + [M.saturation(), M.one_runs(False)]
            + [M.staging_limit(1533)] + M.tile_edges()[:6] + [lay for _, lay in M.refresh_steps()])


def test_model_is_the_loop_over_the_publishes():
    for lay in _small_layouts() + M.straddles():
        offs, moff, out = M.naive(lay)
        assert np.array_equal(offs, lay.offs) and np.array_equal(moff, lay.moff) and np.array_equal(out, lay.out), lay.name
        assert lay.offs.dtype == lay.moff.dtype == np.uint64 and lay.out.dtype == np.uint32


def test_tiles_are_the_search_per_delivery():
    """tiles() against a plain scan for the entry of a delivery."""
    for lay in [M.staging_limit(1535), M.block_straddle(True, True), M.tile_edges()[9]]:
        owner = np.repeat(np.arange(lay.n), lay.runs)
        for k, (jlo, jhi, ne, staged) in enumerate(lay.tiles().tolist()):
            nxt = min((k + 1) * M.FAN_FILL_TILE, lay.total - 1)
            assert jlo == owner[k * M.FAN_FILL_TILE] and jhi == owner[nxt] and ne == jhi - jlo + 1, (lay.name, k)
            assert bool(staged) == (ne <= 1536)


# ------------------------------------------------------------------ the layouts

def test_scan_tail_sizes_hit_both_vector_conditions():
    assert M.SCAN_TAIL_N == [15, 16, 17, 4079, 4080, 4081, 4095, 4096, 4097, 8191, 8192, 8193]
    seen = set()
    for nm in M.SCAN_TAIL_N:
        for z in (False, True):
            lay = M.scan_tail(nm, z)
            assert lay.n == nm and (lay.runs[-1] == 0) == z
            assert lay.runs[:-1].tolist() == [M.SCAN_TAIL_CYCLE[j % 8] for j in range(nm - 1)]
        j0 = nm // 16 * 16                       # the thread that owns the sentinel
        seen.add((j0 + 16 <= nm, j0 + 16 <= nm + 1, nm % 4096 == 0))
        if nm % 16 == 15:                        # the thread's ids are 15, its offsets 16: scalar load, vector store
            assert not j0 + 16 <= nm and j0 + 16 <= nm + 1
    # (load, store) of the sentinel's thread: both scalar; scalar load with vector store; the sentinel alone in a block
    assert seen == {(False, False, False), (False, True, False), (False, False, True)}
    # ... and the thread before it is the last with a vector load, except at the smallest sizes
    assert [nm for nm in M.SCAN_TAIL_N if nm >= 16 and (nm // 16 - 1) * 16 + 16 <= nm] == M.SCAN_TAIL_N[1:]
    assert [len(M.scan_tail(nm, False).block_totals()) for nm in (4095, 4096, 8191, 8192)] == [1, 2, 2, 3]
    assert M.scan_tail(4096, False).block_totals()[-1] == 0


def test_saturation_runs_straddle_255():
    lay = M.saturation()
    assert lay.runs.tolist() == [1, 254, 1, 255, 1, 256, 1, 257, 1, 510, 1]
    assert [min(r, 255) for r in M.SATURATION_RUNS] == [254, 255, 255, 255, 255]
    assert all(s for s in lay.tiles()[:, 3])


def test_one_runs_reach_the_inline_subscriber_in_a_staged_tile():
    """The `m1 - m0 == 1` line and the `bs < INT64_MIN + 2^33` line are not
    mutated on a device (a wrong answer there indexes subs[] with a
    subscriber id): this shows the staged layout reaches both with ids of 2^31
    and more, next to longer runs that take the other branch."""
    for search in (False, True):
        lay = M.one_runs(search)
        assert len(lay.tiles()) == 1 and _entries(lay, 0)[3] == (not search)
        one = {int(lay.out[lay.moff[j]]) for j in range(lay.n) if lay.runs[j] == 1}
        two = {tuple(lay.out[int(lay.moff[j]):int(lay.moff[j + 1])].tolist()) for j in range(lay.n) if lay.runs[j] == 2}
        assert one >= {0x7FFFFFFF, 0x80000000, 0xFFFFFFFE}
        assert two >= {(0x7FFFFFFF, 0x80000000), (0x80000000, 0xFFFFFFFE), (0xFFFFFFFE, 0x7FFFFFFF)}
    assert _entries(M.one_runs(True), 0)[2] > M.FAN_LDS_ENTRIES


def test_tile_edge_layouts_have_their_boundaries():
    T_ = M.FAN_FILL_TILE
    by = {lay.name: lay for lay in M.tile_edges()}
    assert len(by) == len(M.tile_edges()) == 2 * (7 + 3) + 3 + 2 + 1
    for unit in (1, 2):
        for t in M.TILE_TOTALS:
            lay = by["total-%d-of-%d" % (t, unit)]
            assert lay.total == t and len(lay.tiles()) == -(-t // T_) and set(lay.runs.tolist()) <= {1, unit}
            full = [bool(s) for (_, _, ne, s) in lay.tiles().tolist() if ne > 1100]
            assert all(f == (unit == 2) for f in full)          # full tiles: searched (ones), staged (twos)
        for z in M.BOUNDARY_ZEROS:
            lay = by["zeros-%d-of-%d" % (z, unit)]
            j = int(M.entry_of(lay.moff, T_ - 1))               # the entry of tile 0's last delivery
            assert int(lay.moff[j + 1]) == T_ and lay.runs[j + 1:j + 1 + z].tolist() == [0] * z and lay.runs[j + 1 + z] > 0
            # z + 1 equal offsets: the tile search's tie goes to the last, tile 0 counts the zero runs
            assert np.count_nonzero(lay.moff == T_) == z + 1
            assert _entries(lay, 0)[1] == _entries(lay, 1)[0] == j + 1 + z
            assert _entries(lay, 0)[3] == (unit == 2)
    for s in M.RUN_STARTS:
        lay = by["run-starts-%d" % s]
        j = lay.runs.tolist().index(300)
        assert int(lay.moff[j]) == s and all(st for st in lay.tiles()[:, 3])
        # 2,047: the run starts in tile 0 and enters tile 1 from before it (mark at 0); 2,048: on the boundary
        assert _entries(lay, 1)[0] == (j if s <= T_ else j - 1)
    for e in M.RUN_ENDS:
        lay = by["run-ends-%d" % e]
        j = lay.runs.tolist().index(300)
        assert int(lay.moff[j + 1]) == e and _entries(lay, 0)[1] == (j + 1 if e == T_ else j)
    lay = by["run-covers-tile"]
    assert _entries(lay, 1) == (10, 10, 1, True) and int(lay.moff[10]) < T_ and int(lay.moff[11]) > 2 * T_


def test_staging_sweep_has_two_tiles_on_each_path():
    ne = [_entries(M.staging_limit(z), 0)[2] for z in M.STAGING_Z]
    assert ne == [1535, 1536, 1537, 1538]
    assert [_entries(M.staging_limit(z), 0)[3] for z in M.STAGING_Z] == [True, True, False, False]
    for z in M.STAGING_Z:
        lay = M.staging_limit(z)
        assert lay.runs.tolist() == [1] + [0] * z + [2047] + [1] * 10 and len(lay.tiles()) == 2
        t = int(lay.block_totals()[0])
        assert len(lay.block_totals()) == 1 and t == 2058 and t - 1 == lay.mid_limit   # big by one


def test_block_straddle_tiles_cross_entry_4096():
    """The block-boundary term `(j + 1) / FAN_SCAN_TILE != sb0` of the staging
    loop is not mutated on a device: this shows that the staged layouts apply
    it to entry 4,095 with a non-zero run, and that every limit of the device
    test puts the tile's two blocks on the intended sides."""
    S = M.FAN_SCAN_TILE
    for lay in M.straddles():
        mirror, search = "mirror" in lay.name, "search" in lay.name
        jlo, jhi, ne, staged = _entries(lay, 2)
        assert jlo < S <= jhi and staged == (not search), lay.name
        tot = lay.block_totals()
        assert len(tot) == 2 and min(tot) < lay.mid_limit == M.STRADDLE_MID < max(tot)
        assert lay.big(lay.mid_limit).tolist() == [mirror, not mirror]
        assert lay.big(1).tolist() == lay.big(0).tolist() == [True, True] and not lay.big().any()
        if not search:
            assert ne <= M.FAN_LDS_ENTRIES and np.all(lay.runs[4090:4101] > 0)
            # entry 4,095 has deliveries in tile 2, and its end offset is block 1's first
            assert lay.moff[S - 1] < lay.moff[S] and lay.moff[S] > 2 * M.FAN_FILL_TILE
        else:
            z = np.flatnonzero(lay.runs == 0)
            across = z[(z > jlo) & (z < jhi)]
            assert len(across) > M.FAN_LDS_ENTRIES and S in across and S - 1 in across
        if not mirror:
            assert int(tot[0]) == 4100 and 5000 in lay.runs[S:]
        else:
            assert 5000 in lay.runs[:S] and 5000 not in lay.runs[S:]


def test_many_blocks_sizes_give_one_and_two_sums_per_thread():
    F = M.wide_filters()
    assert len(F) == len(set(F)) == 47 and all(T.match(M.WIDE_TOPIC, f) for f in F)
    assert [M.sums_per_thread(nm) for nm in M.MANY_TARGETS] == [1, 2]
    assert [(nm + 1 + 4095) // 4096 for nm in M.MANY_TARGETS] == [256, 257]
    assert "constexpr uint32_t U = 8;" in _src("tm_kernels.hip") and M.sums_per_thread(M.MANY_RAGGED) == 9
    assert M.sums_per_thread(M.MANY_RAGGED - 1) == 8
    for nm in M.MANY_TARGETS + [M.MANY_RAGGED]:
        filters, topics = M.many_blocks(nm)
        singles = [t for t in topics if t != M.WIDE_TOPIC]
        assert len(singles) + 47 * (len(topics) - len(singles)) == nm
        # a single matches its own filter only
        assert all(sum(T.match(t, f) for f in filters) == 1 for t in set(singles))
        assert set(M.MANY_SUBSCRIBED) <= set(filters)
    assert M.sums_per_thread(255 * 4096 - 1) == 1 and M.sums_per_thread(256 * 4096) == 2


def test_degenerate_and_refresh_layouts():
    d = M.degenerate()
    assert d["empty"] == [] and d["no-subscriber"].total == 0 and d["no-subscriber"].n == 5000
    assert len(d["no-subscriber"].block_totals()) == 2
    steps = M.refresh_steps()
    a = [int(lay.runs[0]) for _, lay in steps]
    b = [int(lay.runs[2]) for _, lay in steps]
    assert a == [1, 2, 1, 1, 1, 1] and b == [254, 254, 254, 255, 256, 255]
    assert steps[0][1].out[0] == 0x80000001 and steps[2][1].out[0] == 7      # the run of one: another subscriber
    assert steps[-1][1].out[int(steps[-1][1].moff[2])] == 5001                 # B lost its first subscriber
    assert [s[0] for s, _ in steps] == [None, "sub", "unsub", "sub", "sub", "unsub"]
