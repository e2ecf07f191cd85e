"""The options of shared subscriptions in the ?SUBOPTION table
(tm_shared_subscribe_opts) on a host-only engine, the host restatement of the
merged mailboxes (emqx_broker.mailboxes_shared), and the argument checks of
tm_batch_shared_mode / tm_batch_inbox_groups that need no device.

The reference keeps one ?SUBOPTION entry per {SubPid, Topic}, shared or not
(src/emqx_broker.erl:145-163); a subscribe/3 on a key that exists only merges
the options (`true -> %% Existed`, :129-135); do_unsubscribe/3 deletes the entry
of a shared subscription (:179-183)."""

import ctypes as C

import pytest

from emqx_amd import _native as N
from emqx_amd import emqx_broker as B
from emqx_amd.engine import Engine

DEFAULTS = {"qos": 0, "nl": 0, "rap": 0, "rh": 0, "subid": 0}
G, H = 70, 71


@pytest.fixture
def eng():
    e = Engine(device=-1)
    yield e
    e.close()


def opts(**kw):
    return dict(DEFAULTS, **kw)


def test_shared_subscribe_stores_options_and_joins(eng):
    eng.shared_subscribe_opts(b"a/+", G, 5, {"qos": 2, "nl": 1, "subid": 9})
    assert eng.shared_members(b"a/+", G) == [5]
    assert eng.get_subopts(b"a/+", 5) == opts(qos=2, nl=1, subid=9)
    eng.shared_subscribe_opts(b"a/+", G, 6)                      # opts = NULL: the defaults
    assert eng.shared_members(b"a/+", G) == [5, 6] and eng.get_subopts(b"a/+", 6) == DEFAULTS
    eng.shared_subscribe(b"a/+", G, 7)                           # tm_shared_subscribe stores none
    assert eng.shared_members(b"a/+", G) == [5, 6, 7] and eng.get_subopts(b"a/+", 7) is None
    # a plain member that subscribes with options later gets them; its membership is unchanged
    eng.shared_subscribe_opts(b"a/+", G, 7, {"qos": 1})
    assert eng.shared_members(b"a/+", G) == [5, 6, 7] and eng.get_subopts(b"a/+", 7) == opts(qos=1)
    # get / set on a shared-owned entry
    assert eng.set_subopts(b"a/+", 5, {"qos": 0, "rap": 1})
    assert eng.get_subopts(b"a/+", 5) == opts(qos=0, nl=1, rap=1, subid=9)
    assert not eng.set_subopts(b"a/#", 5, {"qos": 1})
    # the options are not a non-shared subscription
    assert not eng.unsubscribe(b"a/+", 5)
    assert eng.get_subopts(b"a/+", 5) is not None


def test_existed_branch_both_ways_round(eng):
    # non-shared first: the shared subscribe only merges, the pid joins no group
    eng.subscribe_opts(b"t", 1, {"qos": 1, "subid": 4})
    eng.shared_subscribe_opts(b"t", G, 1, {"qos": 2, "rap": 1})
    assert eng.shared_members(b"t", G) == []
    assert eng.get_subopts(b"t", 1) == opts(qos=2, rap=1, subid=4)         # subid 0 keeps the old one
    assert eng.unsubscribe(b"t", 1) and eng.get_subopts(b"t", 1) is None   # still the non-shared subscription's
    # shared first: the non-shared subscribe only merges, nothing is subscribed
    eng.shared_subscribe_opts(b"u", G, 2, {"qos": 2, "nl": 1})
    eng.subscribe_opts(b"u", 2, {"qos": 1, "subid": 3})
    assert eng.get_subopts(b"u", 2) == opts(qos=1, subid=3)
    assert not eng.unsubscribe(b"u", 2)                                    # no non-shared subscription came of it
    eng.subscribe(b"u", 2)                                                 # tm_subscribe: the defaults, subid kept
    assert eng.get_subopts(b"u", 2) == opts(subid=3) and not eng.unsubscribe(b"u", 2)
    # shared first, a second group on the same topic: merges, does not join
    eng.shared_subscribe_opts(b"u", H, 2, {"rap": 1})
    assert eng.shared_members(b"u", H) == [] and eng.shared_members(b"u", G) == [2]
    assert eng.get_subopts(b"u", 2) == opts(rap=1, subid=3)


def test_options_deleted_with_the_membership(eng):
    eng.shared_subscribe_opts(b"x/#", G, 3, {"qos": 1})
    eng.shared_subscribe_opts(b"y", G, 3, {"qos": 2})
    eng.shared_subscribe_opts(b"y", H, 4, {"nl": 1})
    eng.subscribe_opts(b"z", 3, {"qos": 2})
    assert eng.shared_unsubscribe(b"x/#", G, 3)
    assert eng.get_subopts(b"x/#", 3) is None and eng.get_subopts(b"y", 3) == opts(qos=2)
    assert not eng.shared_unsubscribe(b"x/#", G, 3)
    assert eng.shared_member_down(3) == 1
    assert eng.get_subopts(b"y", 3) is None and eng.get_subopts(b"y", 4) == opts(nl=1)
    assert eng.get_subopts(b"z", 3) == opts(qos=2)               # a non-shared subscribe stored these
    # ... and neither call deletes options a non-shared subscribe stored under the member's key
    eng.subscribe_opts(b"w", 8, {"qos": 1})
    eng.shared_subscribe(b"w", G, 8)                             # a member as well, without options of its own
    assert eng.shared_unsubscribe(b"w", G, 8) and eng.get_subopts(b"w", 8) == opts(qos=1)
    eng.shared_subscribe(b"w", G, 8)
    assert eng.shared_member_down(8) == 1 and eng.get_subopts(b"w", 8) == opts(qos=1)
    # subscriber_down leaves the shared-owned entry alone (that is shared_member_down's)
    eng.shared_subscribe_opts(b"v", G, 9, {"qos": 2})
    eng.subscribe(b"v2", 9)
    assert eng.subscriber_down(9) == 1 and eng.get_subopts(b"v", 9) == opts(qos=2)
    # a member that comes back starts from the defaults
    eng.shared_subscribe_opts(b"y", G, 3)
    assert eng.get_subopts(b"y", 3) == DEFAULTS


def test_validation_host_only(eng):
    for bad in ({"qos": 3}, {"nl": 2}, {"rap": 2}, {"rh": 3}):
        with pytest.raises(N.TmError) as ei:
            eng.shared_subscribe_opts(b"a", G, 1, bad)
        assert ei.value.rc == N.TM_EINVAL and b"tm_shared_subscribe_opts" in eng.L.tm_last_error()
    assert eng.shared_members(b"a", G) == [] and eng.get_subopts(b"a", 1) is None
    # tm_batch_shared_mode checks its options before it asks for a device
    o = N.SharedOpts()
    o.strategy = 9
    assert eng.L.tm_batch_shared_mode(eng.h, None, C.byref(o)) == N.TM_EINVAL and b"strategy" in eng.L.tm_last_error()
    o.strategy = N.TM_SHARED_HASH
    assert eng.L.tm_batch_shared_mode(eng.h, None, C.byref(o)) == N.TM_EINVAL and b"keys" in eng.L.tm_last_error()
    o.strategy, o.flags = N.TM_SHARED_RANDOM, N.TM_SHARED_COUNT_ONLY
    assert eng.L.tm_batch_shared_mode(eng.h, None, C.byref(o)) == N.TM_EINVAL
    o.flags = 0
    assert eng.L.tm_batch_shared_mode(eng.h, None, C.byref(o)) == N.TM_ENODEV
    assert eng.L.tm_batch_shared_mode(eng.h, None, None) == N.TM_ENODEV
    assert eng.L.tm_batch_inbox_groups(eng.h, None, 0, None) == N.TM_EINVAL
    p = C.POINTER(C.c_uint32)()
    assert eng.L.tm_batch_inbox_groups(eng.h, None, 0, C.byref(p)) == N.TM_ENODEV


def test_mailboxes_shared_is_mailboxes_without_groups():
    rows = [[(b"a/#", "p"), (b"a/+", "q"), (b"a/+", "p")], [], [(b"b", "q")]]
    none = [[], [], []]
    plain = B.mailboxes(rows)
    assert B.mailboxes_shared(rows, none) == {pid: [(i, to, None) for i, to in box] for pid, box in plain.items()}
    srows = [[(b"a/#", "g", "q"), (b"a/+", "h", "p"), (b"a/b", "g", "r")], [(b"c", "g", "p")], []]
    assert B.mailboxes_shared(rows, srows) == {
        "p": [(0, b"a/#", None), (0, b"a/+", None), (0, b"a/+", "h"), (1, b"c", "g")],
        "q": [(0, b"a/#", "g"), (0, b"a/+", None), (2, b"b", None)],
        "r": [(0, b"a/b", "g")]}


def test_nif_shared_subscribe_5_and_flag_terms():
    """shared_subscribe/5 and the strategy flags against the runtime stand-in:
    arities, the dirty flag, badargs, the Existed merge, {error, enodev} on a
    host-only engine."""
    from nif_harness import Nif
    nif = Nif()
    dirty = nif.flags("shared_subscribe", 4)
    assert nif.flags("shared_subscribe", 5) == dirty and nif.flags("deliver_batch", 3) == nif.flags("deliver_batch", 2)
    e = nif.new(-1)
    assert nif.call("shared_subscribe", e, b"a/+", G, 3, (1, 1, 0, 2, 77)) == "ok"
    assert nif.call("get_subopts", e, b"a/+", 3) == ("ok", (1, 1, 0, 2, 77))
    assert nif.call("shared_subscribe", e, b"a/+", H, 3, (2, 0, 1, 0, 0)) == "ok"      # Existed: merges, SubIdent 0 keeps 77
    assert nif.call("get_subopts", e, b"a/+", 3) == ("ok", (2, 0, 1, 0, 77))
    assert nif.call("shared_subscribe", e, b"a/+", G, 4) == "ok"                       # shared_subscribe/4 stores none
    assert nif.call("get_subopts", e, b"a/+", 4) == "undefined"
    for bad in [(3, 0, 0, 0, 0), (0, 2, 0, 0, 0), (0, 0, 0, 0, 1 << 28), (0, 0, 0, 0), [0, 0, 0, 0, 0], b"opts"]:
        assert nif.call("shared_subscribe", e, b"a/+", G, 5, bad) == ("#badarg",), bad
    assert nif.call("shared_unsubscribe", e, b"a/+", G, 3) == "ok"
    assert nif.call("get_subopts", e, b"a/+", 3) == "undefined"
    pub = (3, 1, True, False, b"a/b")
    for flags in (["shared_round_robin"], [("shared_random", 7)], [("shared_hash", [5])], ["nl_all", ("shared_hash", [5])]):
        assert nif.call("session_deliver_batch", e, [pub], flags) == ("error", "enodev"), flags
    for flags in ([("shared_hash", [5, 6])], [("shared_hash", 5)], [("shared_random", b"7")], [("shared_sticky", 1)],
                  ["shared_round_robin", ("shared_random", 7)], [("shared_hash", [5], 0)]):
        assert nif.call("session_deliver_batch", e, [pub], flags) == ("#badarg",), flags
        assert nif.call("deliver_batch", e, [b"a/b"], flags) == ("#badarg",), flags
    assert nif.call("deliver_batch", e, [b"a/b"], ["nl_all"]) == ("#badarg",)
    assert nif.call("deliver_batch", e, [b"a/b"], [("shared_hash", [5])]) == ("error", "enodev")
    nif.drop(e)
