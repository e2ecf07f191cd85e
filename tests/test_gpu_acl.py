"""Batched ACL check on the device (Engine.acl_check, kernel tm_acl_check):
verdict and deciding rule index equal the Python mirror's on the reference's
known answers, the directed table of its clauses, a randomised batch and the
shapes at which the kernel takes another path."""

import numpy as np
import pytest

import acl_cases as K
from emqx_amd import _native as N
from emqx_amd import emqx_access_rule as R
from emqx_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(device=0)
    yield e
    e.close()


def device(eng, terms, clients, requests):
    acl = eng.acl_create(terms)
    try:
        v, r = eng.acl_check(acl, clients, requests)
    finally:
        acl.close()
    return v.tolist(), r.tolist()


def same_as_mirror(eng, terms, clients, requests):
    mv, mr, _ = K.mirror_batch(terms, clients, requests)
    dv, dr = device(eng, terms, clients, requests)
    bad = [(i, requests[i], (dv[i], dr[i]), (mv[i], mr[i])) for i in range(len(requests))
           if (dv[i], dr[i]) != (mv[i], mr[i])]
    assert not bad, bad[:5]


def test_known_answers(eng):
    kat = K.kat()
    for case in kat["match"]:
        client = K.full_client(K.dec_client(kat["clients"][case["client"]]))
        terms = [K.dec_rule(case["rule"])]
        exp = N.TM_ACL_NOMATCH if case["expect"] == "nomatch" else K.CODE[case["expect"][1]]
        for access in ("publish", "subscribe"):       # emqx_access_rule:match/3 ignores the rule's access
            if len(terms[0]) == 4 and terms[0][2] not in (access, "pubsub"):
                continue
            v, r = device(eng, terms, [client], [(0, access, case["topic"].encode())])
            assert v == [exp], case["src"]
            assert r == [N.TM_NONE if exp == N.TM_ACL_NOMATCH else 0], case["src"]
    sec = kat["mod_acl_internal"]
    client = K.full_client(K.dec_client(kat["clients"][sec["client"]]))
    # the two split lists of the suite as one ordered list with access masks
    terms = [("allow", R.ALL, "publish", ["#"]), ("deny", R.ALL, "subscribe", ["#"])]
    v, r = device(eng, terms, [client], [(0, "publish", b"t"), (0, "subscribe", b"t")])
    assert (v, r) == ([N.TM_ACL_ALLOW, N.TM_ACL_DENY], [0, 1])
    conf = [K.dec_rule(x) for x in kat["acl_conf"]["rules"]]
    clients = [{"clientid": b"d", "username": b"dashboard", "peerhost": "10.1.1.1"},
               {"clientid": b"l", "username": b"x", "peerhost": "127.0.0.1"},
               {"clientid": b"o", "username": None, "peerhost": "10.1.1.1"}]
    reqs = [(0, "subscribe", b"$SYS/brokers"), (0, "subscribe", b"#"), (1, "subscribe", b"#"),
            (1, "publish", b"$SYS/x"), (2, "subscribe", b"$SYS/x"), (2, "subscribe", b"a/#"), (2, "publish", b"$SYS/x")]
    v, r = device(eng, conf, clients, reqs)
    A, D = N.TM_ACL_ALLOW, N.TM_ACL_DENY
    assert (v, r) == ([A, D, A, A, D, A, A], [0, 2, 1, 1, 2, 3, 3])
    same_as_mirror(eng, conf, clients, reqs)
    # acl_nomatch folded in (emqx_access_control:do_check_acl/3)
    acl = eng.acl_create([("allow", R.ALL, "publish", ["a"])])
    for default, code in (("deny", D), ("allow", A)):
        v, r = eng.acl_check(acl, clients, [(0, "publish", b"a"), (0, "publish", b"b")], nomatch=default)
        assert v.tolist() == [A, code] and r.tolist() == [0, N.TM_NONE]


def test_directed_table(eng):
    for terms, client, access, topic, verdict, idx in K.directed():
        v, r = device(eng, terms, [client], [(0, access, topic)])
        assert (v, r) == ([verdict], [idx]), (terms, client, access, topic)


def test_randomised_parity(eng):
    terms, clients, requests = K.gen_random(K.SEED)
    assert (len(requests), len(terms), len(clients)) == (3000, 40, 64)
    mv, mr, mk = K.mirror_batch(terms, clients, requests)
    K.assert_floors(mv, mr, mk)                       # from the mirror alone, before the device runs
    dv, dr = device(eng, terms, clients, requests)
    assert dv == mv
    assert dr == mr


def _small_rules(r, seed=5):
    terms, clients, requests = K.gen_random(seed, n_req=300, n_rules=max(r, 1), n_clients=16)
    return terms[:r], clients, requests


@pytest.mark.parametrize("n", [1, 257])
def test_block_tail(eng, n):
    terms, clients, requests = _small_rules(40)
    same_as_mirror(eng, terms, clients, (requests * 2)[:n])


@pytest.mark.parametrize("r", [0, 1, 70])
def test_rule_counts(eng, r):
    terms, clients, requests = _small_rules(r)
    if r == 0:
        v, rr = device(eng, [], clients, requests)
        assert set(v) == {N.TM_ACL_NOMATCH} and set(rr) == {N.TM_NONE}
    same_as_mirror(eng, terms, clients, requests)


def test_no_requests_and_empty_names(eng):
    acl = eng.acl_create([("allow", R.ALL, "pubsub", ["", "+/b"]), ("deny", R.ALL)])
    c = [{"clientid": b"c", "username": b"u", "peerhost": None}]
    v, r = eng.acl_check(acl, c, [])
    assert len(v) == 0 and len(r) == 0
    v, r = eng.acl_check(acl, [], [])
    assert len(v) == 0
    reqs = [(0, "publish", b""), (0, "publish", b"a"), (0, "publish", b"/b"), (0, "subscribe", b"")]
    v, r = eng.acl_check(acl, c, reqs)
    assert v.tolist() == [N.TM_ACL_ALLOW, N.TM_ACL_DENY, N.TM_ACL_ALLOW, N.TM_ACL_ALLOW]
    assert r.tolist() == [0, 1, 0, 0]
    same_as_mirror(eng, [("allow", R.ALL, "pubsub", ["", "+/b"]), ("deny", R.ALL)], c, reqs)


def test_one_long_name_takes_the_global_path(eng):
    """One TM_MAX_TOPIC_LEN-byte name among 255 short ones: the block's byte
    range (> 16 KB, the kernel's LDS stage) is read from global memory; the
    last block, short names only, stages again."""
    long_name = b"/".join([b"seg"] * 1024)
    assert len(long_name) == 4095
    long_name += b"x"
    assert len(long_name) == N.TM_MAX_TOPIC_LEN
    long_hash = b"/".join([b"seg"] * 1023) + b"/#"
    terms = [("deny", R.ALL, "pubsub", [("eq", long_name.decode())]),
             ("allow", ("client", "c1"), "publish", [long_hash.decode(), "s/%c/+/+"]),
             ("deny", R.ALL, "pubsub", ["s/#"])]
    clients = [{"clientid": b"c1", "username": None, "peerhost": None},
               {"clientid": b"c2", "username": None, "peerhost": None}]
    short = [(i % 2, "publish", b"s/c1/%d/" % i + b"p" * 48) for i in range(255)]
    requests = short[:100] + [(0, "publish", long_name)] + short[100:] + \
        [(0, "publish", long_name[:-1] + b"y"), (1, "publish", long_name[:-1] + b"y")] + short + short
    stage = 16384
    assert sum(len(t) for _c, _a, t in requests[:256]) > stage > sum(len(t) for _c, _a, t in requests[512:768])
    mv, mr, _ = K.mirror_batch(terms, clients, requests)
    assert (mv[100], mr[100]) == (N.TM_ACL_DENY, 0) and (mv[256], mr[256]) == (N.TM_ACL_ALLOW, 1)
    assert (mv[257], mr[257]) == (N.TM_ACL_NOMATCH, N.TM_NONE)
    dv, dr = device(eng, terms, clients, requests)
    assert (dv, dr) == (mv, mr)
    with pytest.raises(N.TmError) as ei:                     # one byte more is refused
        device(eng, terms, clients, [(0, "publish", long_name + b"z")])
    assert ei.value.rc == N.TM_EINVAL and "request 0" in str(ei.value)


def test_rule_set_larger_than_the_scalar_cache(eng):
    """The kernel stages no rules: it reads the compiled block through the
    scalar cache (16 KB), so a block far larger than that -- 400 rules with
    distinct 120-byte filters, > 100 KB -- takes the same path."""
    terms = [("allow" if j % 2 else "deny", R.ALL if j % 3 else ("client", "c%d" % (j % 5)), "pubsub",
              ["big/%04d/" % j + "w" * 100 + "/%c", ("eq", "big/%04d/" % j + "e" * 110)]) for j in range(400)]
    clients = [{"clientid": b"c%d" % i, "username": None, "peerhost": None} for i in range(5)]
    requests = []
    for i in range(150):
        j = (i * 37) % 430                                   # some past the last rule: nomatch
        c = i % 5
        requests.append((c, "publish", b"big/%04d/" % j + b"w" * 100 + b"/c%d" % (c if i % 7 else (c + 1) % 5)))
        requests.append((c, "subscribe", b"big/%04d/" % j + b"e" * 110))
    mv, mr, _ = K.mirror_batch(terms, clients, requests)
    assert len(set(mr)) > 100 and N.TM_ACL_NOMATCH in mv
    dv, dr = device(eng, terms, clients, requests)
    assert (dv, dr) == (mv, mr)


def test_bad_requests_are_refused(eng):
    acl = eng.acl_create([("allow", R.ALL)])
    c = [{"clientid": b"c", "username": None, "peerhost": None}]
    with pytest.raises(N.TmError) as ei:
        eng.acl_check(acl, c, [(0, "publish", b"a"), (1, "publish", b"a")])
    assert ei.value.rc == N.TM_EINVAL and "request 1" in str(ei.value)
    buf = np.frombuffer(b"a", np.uint8).copy()
    offs = np.array([0, 1], np.uint64)
    cof = np.zeros(1, np.uint32)
    ver, rule = np.zeros(1, np.uint8), np.zeros(1, np.uint32)
    from emqx_amd import acl as A
    cs, keep = A.encode_clients(c)
    import ctypes as C
    for access in (0, 3):
        acc = np.array([access], np.uint8)
        rc = eng.L.tm_acl_check(eng.h, acl.h, C.byref(cs), buf.ctypes.data, offs.ctypes.data, cof.ctypes.data,
                                acc.ctypes.data, 1, ver.ctypes.data, rule.ctypes.data)
        assert rc == N.TM_EINVAL


def test_two_replicas_split_a_large_batch(eng, device_pair):
    terms, clients, requests = K.gen_random(K.SEED)
    big = (requests * 24)[:70000]
    rep = Engine(devices=device_pair)
    try:
        assert rep.replicas == 2
        acl2, acl1 = rep.acl_create(terms), eng.acl_create(terms)
        v2, r2 = rep.acl_check(acl2, clients, big)
        v1, r1 = eng.acl_check(acl1, clients, big)
        assert np.array_equal(v1, v2) and np.array_equal(r1, r2)
        mv, mr, _ = K.mirror_batch(terms, clients, requests)
        # a 3,000-request sample across the slice boundary (35,000) against the mirror
        lo = 35000 - 1500
        for i in range(lo, lo + 3000):
            assert (v2[i], r2[i]) == (mv[i % 3000], mr[i % 3000]), i
        v2s, r2s = rep.acl_check(acl2, clients, requests)      # below the split threshold: one replica
        assert v2s.tolist() == mv and r2s.tolist() == mr
    finally:
        rep.close()


def test_nif_path():
    from nif_harness import Nif, Raw
    nif = Nif()
    e = nif.new(0)
    terms, clients, requests = K.gen_random(K.SEED, n_req=200)
    t = nif.call_raw("acl_new", e, K.nif_rules(terms))
    assert nif.decode(t)[0] == "ok"
    acl = Raw(nif.L.mock_tuple_elem(t, 1))
    got = nif.call("acl_check", e, acl, K.nif_clients(clients), [(c, a, tp) for c, a, tp in requests])
    mv, mr, _ = K.mirror_batch(terms, clients, requests)
    names = {N.TM_ACL_ALLOW: "allow", N.TM_ACL_DENY: "deny", N.TM_ACL_NOMATCH: "nomatch"}
    assert got == [(names[v], "none" if r == N.TM_NONE else r) for v, r in zip(mv, mr)]
    assert len({g[0] for g in got}) == 3
    nif.drop(acl)
    nif.drop(e)
