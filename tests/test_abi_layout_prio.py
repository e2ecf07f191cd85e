"""The C ABI of the priority tables without a device: the new ctypes mirrors
against include/emqx_tm.h by a compiled sizeof / offsetof program,
tm_ptable_create's errors and tm_ptable_classes' order on a host-only engine,
and every argument check of tm_batch_window_prio that needs no device."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from emqx_amd import _native as N
from emqx_amd import emqx_mqueue as MQ
from emqx_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNB = N.TM_SESS_UNBOUNDED
INF = N.TM_PRIO_INFINITY

PAIRS = [("tm_session_prio", N.SessionPrio), ("tm_window_prio_opts", N.WindowPrioOpts),
         ("tm_prio_record", N.PrioRecord), ("tm_window_prio", N.WindowPrio)]
CONSTS = ["TM_PRIO_INFINITY", "TM_PRIO_MAX_CLASSES", "TM_PRIO_MAX_TABLES", "TM_PRIO_NOCLASS"]


@pytest.mark.skipif(not shutil.which("gcc"), reason="needs gcc")
def test_ctypes_mirrors_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "emqx_tm.h"', "int main(void) {"]
    for cname, py in PAIRS:
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    for c in CONSTS:
        lines.append(f'printf("const {c} %llu\\n", (unsigned long long){c});')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        k1, k2, v = ln.split()
        got[(k1, k2)] = int(v)
    for cname, py in PAIRS:
        assert got[(cname, "size")] == C.sizeof(py), cname
        for f in py._fields_:
            assert got[(cname, f[0])] == getattr(py, f[0]).offset, (cname, f[0])
    for c in CONSTS:
        assert got[("const", c)] == getattr(N, c), c
        if hasattr(MQ, c):
            assert got[("const", c)] == getattr(MQ, c), c
    assert C.sizeof(N.SessionPrio) == 40 and C.sizeof(N.WindowPrioOpts) == 32 and C.sizeof(N.PrioRecord) == 8
    assert C.sizeof(N.WindowPrio) == 24


def _last_error(L) -> str:
    return (L.tm_last_error() or b"").decode()


def _create(eng, keys, prios, default):
    buf = np.frombuffer(b"".join(keys) or b"\0", np.uint8).copy()
    offs = np.cumsum([0] + [len(k) for k in keys]).astype(np.uint64)
    pr = np.asarray(prios or [0], np.uint16)
    h = C.c_void_p()
    rc = eng.L.tm_ptable_create(eng.h, buf.ctypes.data, offs.ctypes.data, pr.ctypes.data, len(keys), default, C.byref(h))
    return rc, h


def test_ptable_create_errors_and_class_order_host_only():
    eng = Engine(device=-1)
    L = eng.L
    # the classes: distinct priorities with the default, descending, infinity first
    t = eng.ptable({b"t1": 1, b"t2": 2, b"t3": 3})
    assert t.classes == [3, 2, 1, 0]
    assert eng.ptable({b"t1": 1}, default="highest").classes == ["infinity", 1]
    assert eng.ptable({}, default="highest").classes == ["infinity"]
    assert eng.ptable({}).classes == [0]
    assert eng.ptable({b"a": "infinity", b"b": 255, b"c": 0, b"d": 255}, default=7).classes == ["infinity", 255, 7, 0]
    assert eng.ptable({b"k%d" % i: i % 7 + 1 for i in range(1000)}).classes == [7, 6, 5, 4, 3, 2, 1, 0]   # 8 classes
    # a repeated key keeps its last priority (maps:put): 9 is gone, so is the class it alone would make
    rc, h = _create(eng, [b"a", b"b", b"a"], [9, 4, 5], 0)
    assert rc == N.TM_OK
    out = (C.c_uint16 * N.TM_PRIO_MAX_CLASSES)()
    assert L.tm_ptable_classes(h, out) == 3 and list(out)[:3] == [5, 4, 0]
    assert L.tm_ptable_classes(h, None) == 3 and L.tm_ptable_classes(None, out) == 0
    L.tm_ptable_free(eng.h, h)
    L.tm_ptable_free(eng.h, None)
    # the mirror names the same classes
    for entries, default in (({b"t1": 1, b"t2": 2}, "lowest"), ({b"x": "infinity", b"y": 3}, 200), ({}, "highest")):
        assert eng.ptable(entries, default).classes == MQ.classes_of({"priorities": entries, "default_priority": default})
    # the errors
    for keys, prios, default, word in (
            ([b"a"], [256], 0, "key 0: priority 256"),
            ([b"a", b"b"], [1, 0xFFFE], 0, "key 1: priority 65534"),
            ([], [], 256, "default priority 256"),
            ([], [], 0x10000, "default priority 65536"),
            ([b"k%d" % i for i in range(8)], list(range(1, 9)), 0, "9 classes"),
            ([b"k%d" % i for i in range(8)], list(range(8)), INF, "9 classes"),
            ([b"a", b"x" * 4097], [1, 1], 0, "key 1 of 4097 bytes")):
        rc, h = _create(eng, keys, prios, default)
        assert rc == N.TM_EINVAL and word in _last_error(L), (word, _last_error(L))
    rc, h = _create(eng, [b"x" * 4096] + [b"k%d" % i for i in range(7)], list(range(8)), 0)   # both at their limits
    assert rc == N.TM_OK
    L.tm_ptable_free(eng.h, h)
    with pytest.raises(N.TmError) as ei:
        eng.ptable({b"a": 300})
    assert ei.value.rc == N.TM_EINVAL and "priority 300" in str(ei.value)
    with pytest.raises(ValueError):
        eng.ptable({b"a": -1})
    offs = np.asarray([3, 1], np.uint64)
    pr = np.asarray([1], np.uint16)
    h = C.c_void_p()
    assert L.tm_ptable_create(eng.h, b"abc", offs.ctypes.data, pr.ctypes.data, 1, 0, C.byref(h)) == N.TM_EINVAL
    assert "monotone" in _last_error(L)
    assert L.tm_ptable_create(None, None, None, None, 0, 0, C.byref(h)) == N.TM_EINVAL
    assert L.tm_ptable_create(eng.h, None, None, None, 0, 0, None) == N.TM_EINVAL
    t.free()
    t.free()
    with pytest.raises(RuntimeError):
        t.h
    eng.close()


def test_window_prio_validation_host_only():
    """Every TM_EINVAL of tm_batch_window_prio that needs no device, each
    message naming the offender, and TM_ENODEV."""
    eng, other = Engine(device=-1), Engine(device=-1)
    L = eng.L
    T3 = eng.ptable({b"t1": 1, b"t2": 2})            # classes 2 1 0
    T1 = eng.ptable({})                              # class 0
    foreign = other.ptable({})
    do, out, pout = N.DeliverOpts(), N.SessionWindow(), N.WindowPrio()

    def wopts(sessions=(), **dflt):
        wo = N.WindowOpts()
        wo.defaults = N.SessionState(**dict({"next_pkt_id": 1, "inflight_free": UNB}, **dflt))
        arr = (N.SessionState * max(len(sessions), 1))(*[N.SessionState(*s) for s in sessions])
        wo.sessions = C.cast(arr, C.POINTER(N.SessionState))
        wo.n_sessions = len(sessions)
        return wo, arr

    def popts(tables=(), prio=(), default_table=N.TM_NONE):
        po = N.WindowPrioOpts()
        tarr = (C.c_void_p * max(len(tables), 1))(*[t if t is None or isinstance(t, int) else t.h.value for t in tables])
        po.tables, po.n_tables = C.cast(tarr, C.POINTER(C.c_void_p)), len(tables)
        parr = (N.SessionPrio * max(len(prio), 1))(*[
            N.SessionPrio(s, t, (C.c_uint32 * 8)(*(list(pl) + [0] * (8 - len(pl))))) for s, t, pl in prio])
        po.prio, po.n_prio = C.cast(parr, C.POINTER(N.SessionPrio)), len(prio)
        po.default_table = default_table
        return po, (tarr, parr)

    def call(wo, po):
        return L.tm_batch_window_prio(eng.h, None, C.byref(do), C.byref(wo), C.byref(po), C.byref(out), C.byref(pout))

    S3, S4 = (3, 1, 0, UNB, 0, 0), (4, 65535, 1, 0, 5, 3)          # S4: 5 queued against max_len 3: legal with a table
    wo, _k = wopts([S3, S4])
    po, _p = popts([T3], [(4, 0, [3, 2])])
    assert call(wo, po) == N.TM_ENODEV
    assert L.tm_batch_window_prio(None, None, C.byref(do), C.byref(wo), C.byref(po), C.byref(out), C.byref(pout)) == N.TM_EINVAL
    assert L.tm_batch_window_prio(eng.h, None, C.byref(do), C.byref(wo), None, C.byref(out), C.byref(pout)) == N.TM_EINVAL
    assert "popts is NULL" in _last_error(L)
    assert L.tm_batch_window_prio(eng.h, None, C.byref(do), C.byref(wo), C.byref(po), C.byref(out), None) == N.TM_EINVAL
    assert "pout is NULL" in _last_error(L)
    assert L.tm_batch_window_prio(eng.h, None, C.byref(do), C.byref(wo), C.byref(po), None, C.byref(pout)) == N.TM_EINVAL
    assert "out is NULL" in _last_error(L)
    # without a table S4 is refused as tm_batch_window refuses it
    pn, _p = popts()
    assert call(wo, pn) == N.TM_EINVAL and "mqueue_len above mqueue_max" in _last_error(L)
    pn, _p = popts([T3], [(4, N.TM_NONE, [])])
    assert call(wo, pn) == N.TM_EINVAL and "mqueue_len above mqueue_max" in _last_error(L)
    ok, _k2 = wopts([S3, (4, 1, 0, UNB, 2, 3)])
    assert call(ok, pn) == N.TM_ENODEV                               # an entry naming no table: plen ignored
    cases = [
        (([S3, S4], {}), ([T3] * 17, [], N.TM_NONE), "n_tables = 17"),
        (([S3, S4], {}), ([T3, None], [], N.TM_NONE), "tables[1] is NULL"),
        (([S3, S4], {}), ([T3, foreign], [], N.TM_NONE), "tables[1] is a table of another engine"),
        (([S3], {}), ([T3], [], 1), "default_table = 1"),
        (([S3, S4], {}), ([T3], [(4, 0, [3, 2]), (3, 0, [])], N.TM_NONE), "prio[1] (subscriber 3) not above prio[0] (4)"),
        (([S3, S4], {}), ([T3], [(3, 0, []), (3, 0, [])], N.TM_NONE), "not above"),
        (([S3, S4], {}), ([T3], [(4, 1, [3, 2])], N.TM_NONE), "prio[0] (subscriber 4): table = 1"),
        (([S3, S4], {}), ([T3], [(4, 0, [3, 2]), (9, 0, [])], N.TM_NONE), "prio[1] (subscriber 9) is not in wopts->sessions"),
        (([S3], {}), ([T3], [(9, 0, [])], N.TM_NONE), "subscriber 9) is not in"),
        (([S3, S4], {}), ([T3], [(4, 0, [3, 1])], N.TM_NONE), "subscriber 4): sum of plen 4 is not mqueue_len 5"),
        (([S3, S4], {}), ([T3], [(4, 0, [4, 1])], N.TM_NONE), "subscriber 4): plen[0] = 4 above mqueue_max 3"),
        (([S3, S4], {}), ([T3], [(4, 0, [2, 2, 0, 1])], N.TM_NONE), "subscriber 4): plen[3] = 1 for a class its table lacks"),
        (([S3, S4], {}), ([T3, T1], [(4, 1, [3, 2])], N.TM_NONE), "plen[1] = 2 for a class its table lacks (1 classes)"),
        (([S3, (4, 1, 0, 0, 2, 3)], {}), ([T3], [], 0), "subscriber 4) has a priority table and mqueue_len = 2 but no prio entry"),
        (([S3], {"mqueue_len": 1}), ([T3], [], 0), "defaults (subscriber 0) has a priority table and mqueue_len = 1"),
        (([S3], {"mqueue_len": 2, "mqueue_max": 1}), ([T3], [], N.TM_NONE), "defaults: mqueue_len above mqueue_max"),
        (([S4, S3], {}), ([T3], [(4, 0, [3, 2])], N.TM_NONE), "sessions[1] (subscriber 3) not above"),
        (([(3, 0, 0, 0, 0, 0)], {}), ([T3], [], 0), "next_pkt_id"),
    ]
    for (sessions, dflt), (tables, prio, dt), word in cases:
        wo, _k = wopts(sessions, **dflt)
        po, _p = popts(tables, prio, dt)
        assert call(wo, po) == N.TM_EINVAL and word in _last_error(L), (word, _last_error(L))
        assert "tm_batch_window_prio" in _last_error(L)
    # TM_SESS_HOST wins over a table: such a session needs no prio entry and its plen is not looked at
    wo, _k = wopts([S3, (4, 1, N.TM_SESS_HOST, 0, 5, 3)])
    for prio in ([], [(4, 0, [9, 9, 9, 9])]):
        po, _p = popts([T3], prio, 0)
        assert call(wo, po) == N.TM_ENODEV
    po, _p = popts([T3], [(4, 0, [3, 2])])
    po.pad0 = 1
    assert call(wo, po) == N.TM_EINVAL and "pad0" in _last_error(L)
    po, _p = popts([T3], [(4, 0, [3, 2])])
    po.prio = None
    assert call(wo, po) == N.TM_EINVAL and "prio is NULL" in _last_error(L)
    # through the wrapper
    b = eng.prepare([b"a"])
    for fn in (b.window_prio, b.window_prio_device):
        with pytest.raises(N.TmError) as ei:
            fn([dict(subscriber=4, mqueue_len=5, mqueue_max=3)], None, [T3], [dict(subscriber=4, table=0, plen=[3, 2])])
        assert ei.value.rc == N.TM_ENODEV
    with pytest.raises(ValueError):
        b.window_prio([], None, [T3], [dict(subscriber=4, table=0, plen=[0] * 9)])
    b.free()
    for t in (T3, T1, foreign):
        t.free()
    eng.close()
    other.close()
