"""Shared by test_shared_dispatch.py (CPU) and test_gpu_shared_dispatch.py: the
known answers of tests/golden/kat_shared_sub.json run through the
emqx_shared_sub mirror, whose engine is a host-only one or the device's."""

from conftest import lb, load_golden

from emqx_amd import emqx_router as R
from emqx_amd import emqx_shared_sub as S


def kat():
    return load_golden("kat_shared_sub.json")


def has_route(topic: bytes, group) -> bool:
    """The (topic, {Group, node()}) route, in the host table and in the engine
    (a KAT case gives a topic no other route, so its filter exists with it)."""
    host = (group, R.NODE) in R._routes.get(topic, [])
    try:
        R.engine().filter_id(topic)
        eng = True
    except KeyError:
        eng = False
    assert host == eng, (topic, group, host, eng)
    return host


def run_case(case, dispatchers):
    """Runs one KAT case; every publish goes through each of `dispatchers`
    ((topic_list, strategy, keys=) -> rows), which keep separate pick state."""
    strategy = case["strategy"]
    for k, op in enumerate(case["ops"]):
        where = (case["name"], k, op)
        kind = op["op"]
        topic = lb(op["topic"]) if "topic" in op else None
        if kind == "subscribe":
            assert S.subscribe(op["group"], topic, op["pid"]) == "ok", where
        elif kind == "unsubscribe":
            assert S.unsubscribe(op["group"], topic, op["pid"]) == "ok", where
        elif kind == "down":
            assert S.member_down(op["pid"]) == op["expect"], where
        elif kind == "route":
            assert has_route(topic, op["group"]) == op["expect"], where
        elif kind == "members":
            assert S.subscribers(op["group"], topic) == op["expect"], where
            gid = R._agg_id((op["group"], R.NODE))
            from emqx_amd import emqx_broker as B
            assert [B._terms[s] for s in R.engine().shared_members(topic, gid)] == op["expect"], where
        elif kind == "publish":
            exp = [(lb(to), g, pid) for to, g, pid in op["expect"]]
            for d in dispatchers:
                assert d([topic], strategy, keys=[op["key"]])[0] == exp, where
        else:
            raise ValueError(kind)
