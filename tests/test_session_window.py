"""The session's send window (tm_batch_window) without a device: the host
mirror's literal folds (emqx_session.window_one: deliver/2, enqueue/2,
emqx_mqueue:in/2 with a real deque) against the reference's known answers and
against the header's closed form, the ctypes mirrors against the header, and
the argument checks that need no device."""

import ctypes as C
import os
import shutil
import subprocess

import pytest
from conftest import load_golden
from hypothesis import given, settings
from hypothesis import strategies as st

from emqx_amd import _native as N
from emqx_amd import emqx_session as S
from emqx_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNB = N.TM_SESS_UNBOUNDED


def kat_cases():
    """The KATs with `repeat` and `first_packet_id` spelled out."""
    out = []
    for c in load_golden("kat_session_window.json")["cases"]:
        k = c.get("repeat", 1)
        qos, disp = c["qos"] * k, c["disp"] * k
        if c["packet_ids"] is None:
            pids = [c["first_packet_id"] + i for i in range(len(qos))]
        else:
            pids = c["packet_ids"] * k
        assert len(qos) == len(disp) == len(pids), c["name"]
        out.append((c["name"], c["state"], qos, list(zip(disp, pids)), tuple(c["record"])))
    return out


def test_kat_file_covers_the_cases_asked_for():
    names = {c[0] for c in kat_cases()}
    assert names >= {"t_deliver_qos0", "t_deliver_qos1", "t_deliver_qos2", "t_deliver_one_msg",
                     "t_deliver_when_inflight_is_full", "t_enqueue", "t_in", "t_in_qos0", "t_simple_mqueue",
                     "t_infinity_simple_mqueue", "t_dropped", "pkt_id_wrap", "inflight_max_size_0"}
    for c in load_golden("kat_session_window.json")["cases"]:
        assert c["cite"].split(":")[0] in ("test/emqx_session_SUITE.erl", "test/emqx_mqueue_SUITE.erl",
                                           "src/emqx_session.erl", "src/emqx_inflight.erl", "src/emqx_mqueue.erl")


@pytest.mark.parametrize("name,state,qos,want,record", kat_cases(), ids=[c[0] for c in kat_cases()])
def test_mirror_against_the_kats(name, state, qos, want, record):
    got, rec = S.window_one(qos, state)
    assert got == want and rec == record


def test_mirror_pieces():
    """mqueue_in, next_pkt_id, deliver_msg on their own."""
    mq = S.new_mqueue(2, store_qos0=False)
    m = [{"qos": q, "k": k} for k, q in enumerate([0, 1, 2, 1])]
    assert S.mqueue_in(m[0], mq) is m[0] and mq["len"] == 0 and mq["dropped"] == 0   # :149-150, not counted
    assert S.mqueue_in(m[1], mq) is None and S.mqueue_in(m[2], mq) is None and mq["len"] == 2
    assert S.mqueue_in(m[3], mq) is m[1] and mq["len"] == 2 and mq["dropped"] == 1 and list(mq["q"]) == [m[2], m[3]]
    s = S.new_session(0xFFFF)
    S.next_pkt_id(s)
    assert s["next_pkt_id"] == 1
    S.next_pkt_id(s)
    assert s["next_pkt_id"] == 2
    s = S.new_session(5, inflight_max=1)
    assert S.deliver_msg({"qos": 0}, s) == ([(None, {"qos": 0})], []) and s["next_pkt_id"] == 5
    assert S.deliver_msg({"qos": 2}, s) == ([(5, {"qos": 2})], []) and s["next_pkt_id"] == 6 and s["inflight"] == [5]
    assert S.inflight_is_full(s)
    assert S.deliver_msg({"qos": 1}, s) == ([], []) and s["mqueue"]["len"] == 1 and s["next_pkt_id"] == 6
    assert not S.inflight_is_full(S.new_session(1, inflight_max=0, inflight=list(range(100))))


def closed_form(qos, st_):
    """The header's closed form (include/emqx_tm.h, tm_batch_window), restated."""
    P, F, L, M, fl = st_["next_pkt_id"], st_["inflight_free"], st_["mqueue_len"], st_["mqueue_max"], st_["flags"]
    if fl & N.TM_SESS_HOST:
        return [(N.TM_DISP_HOST, 0)] * len(qos), (P, 0, 0, 0)
    disc = bool(fl & N.TM_SESS_DISCONNECTED)
    enters = [q > 0 or (disc and bool(fl & N.TM_SESS_STORE_QOS0)) for q in qos]
    A = sum(enters)
    nsend = 0 if disc else min(F, A)
    E = A - nsend
    drops = max(0, L + E - M) if M > 0 else 0
    old = min(drops, L)
    out, a = [], 0
    for q, e in zip(qos, enters):
        if not e:
            out.append((N.TM_DISP_DROP_QOS0 if disc else N.TM_DISP_SEND0, 0))
            continue
        if a < nsend:
            out.append((N.TM_DISP_SEND, (P - 1 + a) % 65535 + 1))
        else:
            out.append((N.TM_DISP_DROP_FULL if a - nsend < drops - old else N.TM_DISP_QUEUED, 0))
        a += 1
    return out, ((P - 1 + nsend) % 65535 + 1, nsend, E - (drops - old), old)


states = st.builds(
    lambda p, f, m, l, disc, store: {"next_pkt_id": p, "inflight_free": f, "mqueue_max": m,
                                     "mqueue_len": min(l, m) if m else l,
                                     "flags": (N.TM_SESS_DISCONNECTED if disc else 0) | (N.TM_SESS_STORE_QOS0 if store else 0)},
    st.one_of(st.integers(65520, 65535), st.integers(1, 65535)),
    st.sampled_from([0, 1, 2, 3, 7, UNB]), st.sampled_from([0, 1, 2, 5]), st.integers(0, 6),
    st.booleans(), st.booleans())


@settings(max_examples=600, deadline=None)
@given(st.lists(st.integers(0, 2), max_size=40), states)
def test_closed_form_equals_the_literal_fold(qos, state):
    assert S.window_one(qos, state) == closed_form(qos, state)


def test_closed_form_on_the_kats_and_host_sessions():
    for name, state, qos, want, record in kat_cases():
        assert closed_form(qos, state) == (want, record), name
    host = {"next_pkt_id": 77, "flags": N.TM_SESS_HOST | N.TM_SESS_DISCONNECTED, "inflight_free": 0, "mqueue_len": 3,
            "mqueue_max": 3}
    assert S.window_one([0, 1, 2], host) == closed_form([0, 1, 2], host) == ([(N.TM_DISP_HOST, 0)] * 3, (77, 0, 0, 0))


def test_session_window_over_session_inboxes():
    boxes = {5: [(0, b"a", 1, 0), (1, b"a", 0, 0), (2, b"a", 2 | 4, 9)], 9: [(1, b"b", 8, 0)]}
    states_ = {5: {"next_pkt_id": 65535, "flags": 0, "inflight_free": 1, "mqueue_len": 0, "mqueue_max": 0}}
    got = S.session_window(boxes, states_, {"flags": N.TM_SESS_DISCONNECTED})
    assert got == {5: ([(1, 65535), (0, 0), (2, 0)], (1, 1, 1, 0)), 9: ([(3, 0)], (1, 0, 0, 0))}


PAIRS = [("tm_session_state", N.SessionState), ("tm_window_opts", N.WindowOpts), ("tm_window_record", N.WindowRecord),
         ("tm_session_window", N.SessionWindow), ("tm_session_inboxes", N.SessionInboxes)]


@pytest.mark.skipif(not shutil.which("gcc"), reason="needs gcc")
def test_ctypes_mirrors_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "emqx_tm.h"', "int main(void) {"]
    for cname, py in PAIRS:
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    consts = ["TM_SESS_DISCONNECTED", "TM_SESS_STORE_QOS0", "TM_SESS_HOST", "TM_SESS_UNBOUNDED", "TM_WINDOW_DEVICE",
              "TM_DISP_SEND0", "TM_DISP_SEND", "TM_DISP_QUEUED", "TM_DISP_DROP_QOS0", "TM_DISP_DROP_FULL",
              "TM_DISP_HOST", "TM_DISP_COUNT"]
    for c in consts:
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
    for c in consts:
        assert got[("const", c)] == getattr(N, c), c
        if hasattr(S, c):
            assert got[("const", c)] == getattr(S, c), c
    assert C.sizeof(N.SessionState) == 24 and C.sizeof(N.WindowOpts) == 40 and C.sizeof(N.WindowRecord) == 16


def _last_error(L) -> str:
    return (L.tm_last_error() or b"").decode()


def test_abi_validation_host_only():
    """Every TM_EINVAL of tm_batch_window that needs no device, and TM_ENODEV."""
    eng = Engine(device=-1)
    L = eng.L
    do, out = N.DeliverOpts(), N.SessionWindow()

    def wopts(sessions=(), wflags=0, **dflt):
        wo = N.WindowOpts()
        wo.flags = wflags
        wo.defaults = N.SessionState(**dict({"next_pkt_id": 1, "inflight_free": UNB}, **dflt))
        arr = (N.SessionState * max(len(sessions), 1))(*[N.SessionState(*s) for s in sessions])
        wo.sessions = C.cast(arr, C.POINTER(N.SessionState))
        wo.n_sessions = len(sessions)
        return wo, arr

    def call(wo):
        return L.tm_batch_window(eng.h, None, C.byref(do), C.byref(wo), C.byref(out))

    good, _k0 = wopts([(3, 1, 0, UNB, 0, 0), (4, 65535, 7, 0, 5, 5)])
    assert L.tm_batch_window(None, None, C.byref(do), C.byref(good), C.byref(out)) == N.TM_EINVAL
    assert L.tm_batch_window(eng.h, None, C.byref(do), C.byref(good), None) == N.TM_EINVAL and "out is NULL" in _last_error(L)
    assert L.tm_batch_window(eng.h, None, None, C.byref(good), C.byref(out)) == N.TM_EINVAL and "dopts is NULL" in _last_error(L)
    assert L.tm_batch_window(eng.h, None, C.byref(do), None, C.byref(out)) == N.TM_EINVAL and "wopts is NULL" in _last_error(L)
    assert call(good) == N.TM_ENODEV
    cases = [
        ([(4, 1, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0)], 0, {}, "not above"),
        ([(3, 1, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0)], 0, {}, "not above"),
        ([(3, 0, 0, 0, 0, 0)], 0, {}, "next_pkt_id"),
        ([(3, 65536, 0, 0, 0, 0)], 0, {}, "next_pkt_id"),
        ([], 0, {"next_pkt_id": 0}, "defaults"),
        ([], 0, {"next_pkt_id": 70000}, "defaults"),
        ([(3, 1, 0, 0, 6, 5)], 0, {}, "mqueue_len"),
        ([], 0, {"mqueue_len": 2, "mqueue_max": 1}, "mqueue_len"),
        ([(3, 1, 8, 0, 0, 0)], 0, {}, "session flag"),
        ([], 0, {"flags": 16}, "session flag"),
        ([], 2, {}, "window flag"),
    ]
    for sessions, flags, dflt, word in cases:
        wo, _keep = wopts(sessions, flags, **dflt)
        assert call(wo) == N.TM_EINVAL and word in _last_error(L), (sessions, flags, dflt, _last_error(L))
    wo, _keep = wopts([])
    wo.sessions = None
    wo.n_sessions = 2
    assert call(wo) == N.TM_EINVAL and "sessions is NULL" in _last_error(L)
    do.flags = 16
    assert call(good) == N.TM_EINVAL and "deliver flag" in _last_error(L)
    do.flags = 0
    # mqueue_len above a max of 0 (infinity) is fine; so is the largest subscriber id
    wo, _keep = wopts([(0, 1, 0, 0, 9, 0), (0xFFFFFFFF, 65535, 3, UNB, 0, 0)])
    assert call(wo) == N.TM_ENODEV
    b = eng.prepare([b"a"])
    for fn in (b.window, b.window_device):
        with pytest.raises(N.TmError) as ei:
            fn()
        assert ei.value.rc == N.TM_ENODEV
    with pytest.raises(ValueError):
        b.window([{"subscriber": 1, "nonsense": 2}])
    with pytest.raises(ValueError):
        b.window([{"subscriber": 1 << 32}])
    b.free()
    eng.close()


def test_nif_session_window_terms():
    """session_window_batch/4 against the runtime stand-in: arity, the dirty
    flag, badargs, {error, enodev} on a host-only engine."""
    from nif_harness import Nif
    nif = Nif()
    assert nif.flags("session_window_batch", 4) == 2   # ERL_NIF_DIRTY_JOB_IO_BOUND
    e = nif.new(-1)
    pub = (3, 1, True, False, b"a/b")
    dflt = (0, 1, [], "unbounded", 0, 0)
    ok = (dflt, [(3, 65535, ["disconnected", "store_qos0"], 4, 1, 2), (9, 7, ["host"], "unbounded", 0, 0)])
    for bad in [dflt, (dflt,), (dflt, (3, 1, [], 0, 0, 0)), (dflt[:5], []), (dflt, [dflt[:5]]), (dflt + (0,), []),
                ((0, 1, ["sticky"], 0, 0, 0), []), ((0, 1, "host", 0, 0, 0), []), ((0, 1, [], "infinity", 0, 0), []),
                ((0, 1, [], 0xFFFFFFFF, 0, 0), []), ((b"0", 1, [], 0, 0, 0), []), ((0, b"1", [], 0, 0, 0), []),
                (dflt, [(3, 1, [], 0, b"0", 0)]), (dflt, [(3, 1, [], 0, 0, -1)]), (dflt, [dflt, b"x"]), [dflt, []]]:
        assert nif.call("session_window_batch", e, [pub], bad, []) == ("#badarg",), bad
    for bad in [("session_window_batch", e, [pub], ok, ["sticky"]), ("session_window_batch", e, pub, ok, []),
                ("session_window_batch", e, [pub[:4]], ok, []), ("session_window_batch", b"e", [pub], ok, [])]:
        assert nif.call(*bad) == ("#badarg",), bad[2:]
    for flags in ([], ["upgrade_qos"], ["nl_all", "upgrade_qos"]):
        assert nif.call("session_window_batch", e, [pub, ("none", 0, False, True, b"a/c")], ok, flags) == ("error", "enodev")
    assert nif.call("session_window_batch", e, [], (dflt, []), []) == ("error", "enodev")
    nif.drop(e)
