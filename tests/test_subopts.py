"""Subscription options (the ?SUBOPTION table) and the session's per-delivery
steps, the parts that need no device: the known answers through the host
mirrors (emqx_session.py, emqx_broker.py) and a host-only Engine, a random
walk of the table against a dict model, the ABI's argument checks and the
ctypes layouts.  The device path (tm_batch_deliver) is in test_gpu_subopts.py."""

import ctypes as C
import os
import random
import shutil
import subprocess

import pytest
from conftest import lb, load_golden

from emqx_amd import _native as N
from emqx_amd import emqx_broker as B
from emqx_amd import emqx_router as R
from emqx_amd import emqx_session as S
from emqx_amd.engine import Engine

DIRTY_IO = 2
DEFAULTS = {"qos": 0, "nl": 0, "rap": 0, "rh": 0, "subid": 0}


@pytest.fixture
def host_broker():
    """The broker mirror on a host-only engine; afterwards the mirror picks
    its engine anew (a device engine where there is a device)."""
    R.use(Engine(device=-1))
    B.clear_tables()
    yield
    B.clear_tables()
    R.engine().close()
    R.use(None)


def _last_error(L) -> str:
    return (L.tm_last_error() or b"").decode()


def test_kat_file_is_cited_and_complete():
    kat = load_golden("kat_subopts.json")
    for case in kat["broker"] + kat["session"]:
        assert ".erl:" in case["cite"] or ".hrl:" in case["cite"], case["name"]
    names = " ".join(c["name"] for c in kat["broker"] + kat["session"])
    for must in ("t_subopts", "t_subscriptions", "t_handle_deliver:", "t_handle_deliver_nl", "t_subscribe_no_local"):
        assert must in names, must


def test_kat_session_mirror():
    """ignore_local/3 + enrich_subopts/3 of every session case, per mode."""
    kat = load_golden("kat_subopts.json")
    assert len(kat["session"]) >= 10
    for case in kat["session"]:
        subs = {lb(t): o for t, o in case["subs"].items()}
        delivers = [(lb(to), dict(S.msg_of(byte, fr), i=i)) for i, (to, fr, byte) in enumerate(case["delivers"])]
        for exp in case["expect"]:
            left, dropped = S.ignore_local(delivers, case["subscriber"], subs, exp["nl_all"])
            out = S.enrich(left, subs, exp["upgrade_qos"])
            got = [[m["i"], S.byte_of(e), e["subid"] or 0] for (_, m), (_, e) in zip(left, out)]
            assert got == exp["left"] and dropped == exp["dropped"], (case["name"], exp)
        # the batch form over a one-pid mailbox agrees
        pid = case["subscriber"]
        box = {pid: [(i, lb(to)) for i, (to, _, _) in enumerate(case["delivers"])]}
        fr = [d[1] for d in case["delivers"]]
        by = [d[2] for d in case["delivers"]]
        for exp in case["expect"]:
            got, dropped = S.session_inboxes(box, {pid: subs}, fr, by, exp["upgrade_qos"], exp["nl_all"])
            want = [(i, lb(case["delivers"][i][0]), b, s) for i, b, s in exp["left"]]
            assert got == ({pid: want} if want else {}) and dropped == exp["dropped"], case["name"]


def _full(o):
    return None if o is None else dict(DEFAULTS, **o)


def test_kat_broker_mirror_and_host_engine(host_broker):
    """t_subopts / t_subscriptions through emqx_broker.py on a host-only engine."""
    kat = load_golden("kat_subopts.json")
    for case in kat["broker"]:
        B.clear_tables()
        assert R.engine().device == -1
        for op in case["ops"]:
            name, args, want = op[0], op[1:-1], op[-1]
            if name == "set_subopts":
                got = B.set_subopts(lb(args[0]), args[2], args[1])
            elif name == "get_subopts":
                got = B.get_subopts(args[1], lb(args[0]))
                want = _full(want)
            elif name == "subscribe":
                got = B.subscribe(lb(args[0]), args[1], args[2])
            elif name == "unsubscribe":
                got = B.unsubscribe(lb(args[0]), args[1])
            elif name == "subscriber_down":
                got = B.subscriber_down(args[0])
            elif name == "subscriptions":
                got = B.subscriptions(args[0])
                want = [(lb(t), _full(o)) for t, o in want]
            else:
                raise AssertionError(name)
            assert got == want, (case["name"], op)


def test_random_walk_against_a_dict_model(host_broker):
    """20,000 random subscribe_opts / subscribe / set_subopts / unsubscribe /
    subscriber_down calls: get_subopts of every live and dead pair every 2,500
    steps, and the bag order (B.subscribers) against the model's."""
    rng = random.Random(77)
    assert R.engine().device == -1
    topics = [b"t/%d" % i for i in range(40)] + [b"w/+/%d" % i for i in range(10)] + [b"#"]
    pids = list(range(25))
    model = {}                       # (topic, pid) -> opts
    order = {t: [] for t in topics}  # topic -> pids in subscription order

    def rand_opts(partial):
        o = {"qos": rng.randrange(3), "nl": rng.randrange(2), "rap": rng.randrange(2), "rh": rng.randrange(3),
             "subid": rng.choice([0, 0, 1, 7, rng.randrange(1, N.TM_SUBID_MAX + 1), N.TM_SUBID_MAX])}
        if partial:
            o = {k: v for k, v in o.items() if rng.random() < 0.5}
        return o

    def check_all():
        for t in topics:
            assert B.subscribers(t) == order[t], t
            for p in pids:
                assert B.get_subopts(p, t) == model.get((t, p)), (t, p)

    for step in range(20000):
        t, p, r = rng.choice(topics), rng.choice(pids), rng.random()
        key = (t, p)
        if r < 0.35:
            o = rand_opts(rng.random() < 0.5)
            B.subscribe(t, p, o)
            if key in model:     # merge: flags replaced (missing = default), subid only when non-zero
                old = model[key]
                model[key] = dict(dict(DEFAULTS, **o), subid=o.get("subid") or old["subid"])
            else:
                model[key] = dict(DEFAULTS, **o)
                order[t].append(p)
        elif r < 0.45:
            B.subscribe(t, p)
            if key in model:
                model[key] = dict(DEFAULTS, subid=model[key]["subid"])
            else:
                model[key] = dict(DEFAULTS)
                order[t].append(p)
        elif r < 0.65:
            o = rand_opts(True)
            assert B.set_subopts(t, o, p) == (key in model)
            if key in model:
                model[key].update(o)
        elif r < 0.98:
            B.unsubscribe(t, p)
            if model.pop(key, None) is not None:
                order[t].remove(p)
        else:
            n = B.subscriber_down(p)
            gone = [k for k in model if k[1] == p]
            assert n == len(gone)
            for k in gone:
                del model[k]
                order[k[0]].remove(p)
        if (step + 1) % 2500 == 0:
            check_all()
    assert model and any(v["nl"] for v in model.values())


def test_abi_validation_host_only():
    """Every TM_EINVAL / TM_ENOENT of the table calls and of tm_batch_deliver
    that needs no device, and TM_ENODEV."""
    eng = Engine(device=-1)
    L = eng.L
    ok = N.SubOpts(1, 1, 1, 2, N.TM_SUBID_MAX)
    out = N.SubOpts()
    t = b"a/b"
    assert L.tm_set_subopts(eng.h, t, 3, 9, N.TM_SUBOPT_QOS, C.byref(ok)) == N.TM_ENOENT
    assert L.tm_get_subopts(eng.h, t, 3, 9, C.byref(out)) == N.TM_ENOENT
    for bad, what in [(N.SubOpts(3, 0, 0, 0, 0), "qos"), (N.SubOpts(0, 2, 0, 0, 0), "nl"),
                      (N.SubOpts(0, 0, 2, 0, 0), "rap"), (N.SubOpts(0, 0, 0, 3, 0), "rh"),
                      (N.SubOpts(0, 0, 0, 0, N.TM_SUBID_MAX + 1), "subid")]:
        assert L.tm_subscribe_opts(eng.h, t, 3, 9, 0, C.byref(bad)) == N.TM_EINVAL and what in _last_error(L), what
    assert L.tm_get_subopts(eng.h, t, 3, 9, C.byref(out)) == N.TM_ENOENT   # a refused subscribe subscribed nothing
    assert L.tm_subscribe_opts(eng.h, t, 3, 9, 0, C.byref(ok)) == 0
    assert L.tm_get_subopts(eng.h, t, 3, 9, C.byref(out)) == 0 and out.asdict() == ok.asdict()
    assert L.tm_subscribe_opts(eng.h, t, 3, 9, 0, None) == 0            # NULL = the defaults; the subid stays
    assert L.tm_get_subopts(eng.h, t, 3, 9, C.byref(out)) == 0
    assert out.asdict() == dict(DEFAULTS, subid=N.TM_SUBID_MAX)
    for bad, mask, what in [(N.SubOpts(3, 0, 0, 0, 0), N.TM_SUBOPT_QOS, "qos"), (N.SubOpts(0, 2, 0, 0, 0), N.TM_SUBOPT_NL, "nl"),
                            (N.SubOpts(0, 0, 2, 0, 0), N.TM_SUBOPT_RAP, "rap"), (N.SubOpts(0, 0, 0, 3, 0), N.TM_SUBOPT_RH, "rh"),
                            (N.SubOpts(0, 0, 0, 0, 1 << 28), N.TM_SUBOPT_SUBID, "subid")]:
        assert L.tm_set_subopts(eng.h, t, 3, 9, mask, C.byref(bad)) == N.TM_EINVAL and what in _last_error(L), what
    # a field outside the mask is not looked at
    assert L.tm_set_subopts(eng.h, t, 3, 9, N.TM_SUBOPT_RAP, C.byref(N.SubOpts(3, 2, 1, 3, 1 << 28))) == 0
    assert L.tm_set_subopts(eng.h, t, 3, 9, 32, C.byref(ok)) == N.TM_EINVAL and "mask" in _last_error(L)
    assert L.tm_set_subopts(eng.h, t, 3, 9, N.TM_SUBOPT_QOS, None) == N.TM_EINVAL and "NULL" in _last_error(L)
    assert L.tm_get_subopts(eng.h, t, 3, 9, None) == N.TM_EINVAL and "NULL" in _last_error(L)
    assert L.tm_get_subopts(eng.h, t, 3, 9, C.byref(out)) == 0 and out.asdict() == dict(DEFAULTS, rap=1, subid=N.TM_SUBID_MAX)
    # removal deletes the options with the subscription
    assert eng.unsubscribe(t, 9) is True and eng.get_subopts(t, 9) is None
    eng.subscribe_opts(t, 9, {"qos": 2})
    assert eng.subscriber_down(9) == 1 and eng.get_subopts(t, 9) is None
    with pytest.raises(ValueError):
        eng.subscribe_opts(t, 9, {"retain": 1})
    # a value past the field's width is refused, not wrapped into a valid one
    for bad in ({"qos": 256}, {"nl": 258}, {"rap": -1}, {"rh": 1 << 16}, {"subid": 1 << 32}, {"subid": N.TM_SUBID_MAX + 1}):
        with pytest.raises(ValueError):
            eng.subscribe_opts(t, 9, bad)
        with pytest.raises(ValueError):
            eng.set_subopts(t, 9, bad)
    with pytest.raises(N.TmError) as ei:
        eng.subscribe_opts(t, 9, {"qos": 255})
    assert ei.value.rc == N.TM_EINVAL and eng.get_subopts(t, 9) is None

    o, si = N.DeliverOpts(), N.SessionInboxes()
    assert L.tm_batch_deliver(None, None, C.byref(o), C.byref(si)) == N.TM_EINVAL
    assert L.tm_batch_deliver(eng.h, None, C.byref(o), None) == N.TM_EINVAL and "out is NULL" in _last_error(L)
    assert L.tm_batch_deliver(eng.h, None, None, C.byref(si)) == N.TM_EINVAL and "opts is NULL" in _last_error(L)
    o.flags = 16
    assert L.tm_batch_deliver(eng.h, None, C.byref(o), C.byref(si)) == N.TM_EINVAL and "unknown flag" in _last_error(L)
    o.flags = N.TM_DELIVER_NL_ALL | N.TM_DELIVER_SUBIDS
    assert L.tm_batch_deliver(eng.h, None, C.byref(o), C.byref(si)) == N.TM_ENODEV
    b = eng.prepare([b"a"])
    for call in (b.deliver, b.deliver_device):
        with pytest.raises(N.TmError) as ei:
            call()
        assert ei.value.rc == N.TM_ENODEV
    b.free()
    eng.close()


def test_nif_subopts_terms():
    """subscribe/5 and get_subopts/3 against the runtime stand-in: arities,
    the dirty flag, badargs, the merge."""
    from nif_harness import Nif
    nif = Nif()
    assert nif.flags("subscribe", 5) == DIRTY_IO and nif.flags("get_subopts", 3) == DIRTY_IO
    assert nif.flags("subscribe", 4) == DIRTY_IO
    e = nif.new(-1)
    assert nif.call("get_subopts", e, b"a/+", 3) == "undefined"
    assert nif.call("subscribe", e, b"a/+", 3, 0, (1, 1, 0, 2, 77)) == "ok"
    assert nif.call("get_subopts", e, b"a/+", 3) == ("ok", (1, 1, 0, 2, 77))
    assert nif.call("subscribe", e, b"a/+", 3, 0, (2, 0, 1, 0, 0)) == "ok"       # merge: SubIdent 0 keeps 77
    assert nif.call("get_subopts", e, b"a/+", 3) == ("ok", (2, 0, 1, 0, 77))
    assert nif.call("subscribe", e, b"a/+", 3, 0) == "ok"                        # subscribe/4: the defaults
    assert nif.call("get_subopts", e, b"a/+", 3) == ("ok", (0, 0, 0, 0, 77))
    for bad in [(3, 0, 0, 0, 0), (0, 2, 0, 0, 0), (0, 0, 2, 0, 0), (0, 0, 0, 3, 0), (0, 0, 0, 0, 1 << 28),
                (0, 0, 0, 0), (0, 0, 0, 0, 0, 0), (0, 0, 0, 0, b"x"), [0, 0, 0, 0, 0], b"opts"]:
        assert nif.call("subscribe", e, b"a/+", 3, 0, bad) == ("#badarg",), bad
    for bad in [("get_subopts", e, "a", 3), ("get_subopts", e, b"a", b"3"), ("get_subopts", b"e", b"a", 3),
                ("subscribe", e, "a", 3, 0, (0, 0, 0, 0, 0)), ("subscribe", b"e", b"a", 3, 0, (0, 0, 0, 0, 0))]:
        assert nif.call(*bad) == ("#badarg",), bad[2:]
    assert nif.call("get_subopts", e, b"a/+", 3) == ("ok", (0, 0, 0, 0, 77))
    # session_deliver_batch/3: arity, dirty flag, badargs, {error, enodev} on a host-only engine
    assert nif.flags("session_deliver_batch", 3) == DIRTY_IO
    pub = (3, 1, True, False, b"a/b")
    for bad in [("session_deliver_batch", e, [pub], ["sticky"]), ("session_deliver_batch", e, [pub], "nl_all"),
                ("session_deliver_batch", e, [pub], [b"nl_all"]), ("session_deliver_batch", e, pub, []),
                ("session_deliver_batch", e, [b"a/b"], []), ("session_deliver_batch", e, [pub[:4]], []),
                ("session_deliver_batch", e, [pub + (0,)], []),
                ("session_deliver_batch", e, [("nobody", 1, True, False, b"a/b")], []),
                ("session_deliver_batch", e, [(b"3", 1, True, False, b"a/b")], []),
                ("session_deliver_batch", e, [(0xFFFFFFFF, 1, True, False, b"a/b")], []),
                ("session_deliver_batch", e, [(3, 3, True, False, b"a/b")], []),
                ("session_deliver_batch", e, [(3, 1, 1, False, b"a/b")], []),
                ("session_deliver_batch", e, [(3, 1, True, "no", b"a/b")], []),
                ("session_deliver_batch", e, [(3, 1, True, False, "a/b")], []),
                ("session_deliver_batch", e, [pub, b"x"], []), ("session_deliver_batch", b"e", [pub], [])]:
        assert nif.call(*bad) == ("#badarg",), bad[2:]
    for flags in ([], ["upgrade_qos"], ["nl_all", "upgrade_qos"]):
        assert nif.call("session_deliver_batch", e, [pub, ("none", 0, False, True, b"a/c")], flags) == ("error", "enodev")
    assert nif.call("session_deliver_batch", e, [], []) == ("error", "enodev")
    assert nif.call("unsubscribe", e, b"a/+", 3, 0) == "ok"
    assert nif.call("get_subopts", e, b"a/+", 3) == "undefined"
    nif.drop(e)


@pytest.mark.skipif(not shutil.which("gcc"), reason="needs gcc")
def test_ctypes_mirrors_match_the_header(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = [("tm_subopts", N.SubOpts, {}), ("tm_deliver_opts", N.DeliverOpts, {"from_": "from"}),
               ("tm_session_inboxes", N.SessionInboxes, {})]
    consts = ["TM_SUBOPT_QOS", "TM_SUBOPT_NL", "TM_SUBOPT_RAP", "TM_SUBOPT_RH", "TM_SUBOPT_SUBID", "TM_SUBID_MAX",
              "TM_MSG_RETAIN", "TM_MSG_RETAINED", "TM_MSG_NL", "TM_DELIVER_DEVICE", "TM_DELIVER_UPGRADE_QOS",
              "TM_DELIVER_NL_ALL", "TM_DELIVER_SUBIDS"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "emqx_tm.h"', "int main(void) {"]
    for cname, cls, ren in structs:
        lines.append(f'printf("{cname}.size %zu\\n", sizeof({cname}));')
        for f in cls._fields_:
            lines.append(f'printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {ren.get(f[0], f[0])}));')
    for c in consts:
        lines.append(f'printf("{c} %u\\n", (unsigned){c});')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    for cname, cls, _ in structs:
        assert int(got[f"{cname}.size"]) == C.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got[f"{cname}.{f[0]}"]) == getattr(cls, f[0]).offset, (cname, f[0])
    for c in consts:
        assert int(got[c]) == getattr(N, c), c
    assert S.TM_MSG_RETAIN == N.TM_MSG_RETAIN and S.TM_MSG_RETAINED == N.TM_MSG_RETAINED and S.TM_MSG_NL == N.TM_MSG_NL
