"""The batched ACL check (tm_acl_check: acl_lane, acl_who, the compiler in
tm_acl.cpp) at the edges of its LDS stage, its who stack, its address
compare, its level walk, its wave logic and its slice base.  Every comparison
is exact: verdict and deciding rule index per request against the mirror
(acl_cases.mirror_batch), and where a plain computation exists, against that
too.  The builders are in acl_cases.py; what they must exercise is asserted on
the CPU in test_acl.py and again here before the device runs."""

import ctypes as C

import numpy as np
import pytest

import acl_cases as K
from emqx_amd import _native as N
from emqx_amd import acl as A
from emqx_amd.engine import Engine

pytestmark = pytest.mark.gpu

NOMATCH = (N.TM_ACL_NOMATCH, N.TM_NONE)


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
    return list(zip(v.tolist(), r.tolist()))


def mirror(terms, clients, requests):
    v, r, _ = K.mirror_batch(terms, clients, requests)
    return list(zip(v, r))


def assert_same(got, exp, requests):
    assert len(got) == len(exp) == len(requests)
    bad = [(i, requests[i][:2], requests[i][2][-24:], got[i], exp[i]) for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (len(bad), bad[:5])


# ---- 1. stage boundary ---------------------------------------------------------------
@pytest.mark.parametrize("form", ["eq", "pattern"])
@pytest.mark.parametrize("width", [K.STAGE, K.STAGE + 1])
@pytest.mark.parametrize("lead", [0, 1, 15])
def test_stage_boundary(eng, lead, width, form):
    """Block 1 spans exactly `width` bytes from the 16-byte boundary before it
    (staged at 16,384, global at 16,385) and starts `lead` bytes past that
    boundary; its first and last names, and the last names of blocks 0 and 2
    (the last 16-byte line a block stages), turn on their first and last byte."""
    terms, clients, requests, edges = K.stage_case(lead, width, form, tag=b"%d%d" % (lead, width & 1))
    assert len(requests) == 700
    spans = K.block_spans(requests)                   # from the lengths alone: the kernel does not say which path it took
    (_, e0, _), (b0, b1, a0), (c0, c1, ca) = spans
    assert e0 == 4096 + lead and b0 - a0 == lead and b1 - a0 == width
    assert c1 - ca <= K.STAGE and (c1 - ca) % 16 != 0
    exp = mirror(terms, clients, requests)
    assert [exp[i] for i in edges] == [(N.TM_ACL_ALLOW, 1), (N.TM_ACL_ALLOW, 3), (N.TM_ACL_ALLOW, 5),
                                       (N.TM_ACL_ALLOW, 7)]
    empty_last = [i for i, q in enumerate(requests) if q[2] == b"m/k1/x/"]
    assert len(empty_last) == 1 and 256 < empty_last[0] < 511
    assert exp[empty_last[0]] == (N.TM_ACL_ALLOW, 8) and exp[empty_last[0] + 1] == (N.TM_ACL_DENY, 11)
    assert_same(device(eng, terms, clients, requests), exp, requests)


# ---- 2. who programs -------------------------------------------------------------------
def test_who_stack_depth_and_width(eng):
    """Leaves at depth 32 under alternating 'and' / 'or' (the stack word is
    full), a sibling whose bit is the oldest on the stack, and 40-wide nodes,
    alone and at depth 10: the device, the mirror and all / any agree."""
    terms, clients, requests, labels, plain = K.who_case()
    depths = [K.who_depth(t[1]) for t in terms]
    assert max(depths) == N.TM_ACL_MAX_WHO_DEPTH == 32 and depths.count(32) >= 8
    assert len({p[0] for p in plain[0::2]}) == 2       # client k1 passes some trees and not others
    exp = mirror(terms, clients, requests)
    assert exp == plain
    got = device(eng, terms, clients, requests)
    bad = [(labels[i // 2], requests[i][0], got[i], exp[i]) for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, bad[:5]


def test_who_depth_33_is_refused(eng):
    for outer in ("and", "or"):
        deep = K.who_chain(N.TM_ACL_MAX_WHO_DEPTH + 1, K.TRUE_LEAF, outer)
        assert K.who_depth(deep) == 33
        with pytest.raises(N.TmError) as ei:
            eng.acl_create([("allow", K.TRUE_LEAF, "pubsub", ["t"]), ("allow", deep, "pubsub", ["t"])])
        assert ei.value.rc == N.TM_EINVAL
        assert "rule 1" in str(ei.value) and "nested deeper" in str(ei.value)
    # the engine is usable afterwards, and the limit itself is accepted
    terms = [("allow", K.who_chain(N.TM_ACL_MAX_WHO_DEPTH, K.TRUE_LEAF), "pubsub", ["t"])]
    requests = [(0, "publish", b"t"), (1, "publish", b"t")]
    assert device(eng, terms, K.WHO_CLIENTS, requests) == [(N.TM_ACL_ALLOW, 0), NOMATCH]


# ---- 3. address ranges -------------------------------------------------------------------
def test_address_ranges(eng):
    """Ranges that vary in one 32-bit word only, for each word of a v6 address
    and for v4, the word from {0, 1, 0x01000000, 0x7FFFFFFF, 0x80000000,
    0xFFFFFFFF}, probed around both ends; lo == hi; lo > hi; the other family;
    no peerhost.  Expected: lo <= int(ip_address(h)) <= hi within one family."""
    terms, clients, requests, plain, ranges = K.ip_case()
    assert {f for _lo, _hi, f in ranges} == {4, 6}
    assert sum(lo == hi for lo, hi, _f in ranges) >= 12 and sum(lo > hi for lo, hi, _f in ranges) >= 4
    per_rule = {}
    for q, p in zip(requests, plain):
        per_rule.setdefault(int(q[2][2:]), set()).add(p[0])
    for j, (lo, hi, _f) in enumerate(ranges):          # inside and outside, except where nobody is inside
        assert per_rule[j] == ({N.TM_ACL_ALLOW, N.TM_ACL_NOMATCH} if lo <= hi else {N.TM_ACL_NOMATCH}), j
    exp = mirror(terms, clients, requests)
    assert exp == plain
    got = device(eng, terms, clients, requests)
    bad = [(ranges[int(requests[i][2][2:])], clients[requests[i][0]]["peerhost"], got[i], exp[i])
           for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (len(bad), [(hex(lo), hex(hi), f, h, g, e) for (lo, hi, f), h, g, e in bad[:5]])


# ---- 4. levels and variables ----------------------------------------------------------------
def test_level_cross_product(eng):
    """Every filter of 1 to 3 levels over {a, '', +, #, %c, %u} against every
    name of 1 to 3 levels over {a, '', +, #, cid, b} (and the spellings an unfed
    %c / %u equals), as a pattern and as {eq, _}, for a client with both fields
    and with either undefined: one rule set per filter."""
    assert len(K.LEVEL_FILTERS) == 258 and len(K.LEVEL_NAMES) == 258
    matches = {"pattern": 0, "eq": 0}
    unfed = 0
    for f in K.LEVEL_FILTERS:
        terms, clients, requests = K.level_case(f)
        exp = mirror(terms, clients, requests)
        got = device(eng, terms, clients, requests)
        bad = [(f, clients[requests[i][0]], requests[i][1:], got[i], exp[i]) for i in range(len(exp))
               if got[i] != exp[i]]
        assert not bad, (len(bad), bad[:5])
        for (c, acc, x), e in zip(requests, exp):
            if e != NOMATCH:
                matches["pattern" if acc == "publish" else "eq"] += 1
                unfed += c != 0 and acc == "publish" and (b"%c" in x or b"%u" in x)
    # (the shares are asserted in test_acl.py; here: the loop above compared more than nomatch with nomatch)
    assert matches["pattern"] >= 2800 and matches["eq"] >= 3 * 84 and unfed > 0, (matches, unfed)


@pytest.fixture(scope="module")
def max_shape():
    terms, clients, requests = K.max_shape_case()
    return terms, clients, requests, mirror(terms, clients, requests)


def test_max_shape_in_one_block(eng, max_shape):
    """4,095- and 4,096-byte names of 2,048 levels against 2,048-level filters,
    64 requests in one block: far past the stage, read from global memory."""
    terms, clients, requests, exp = max_shape
    assert K.block_spans(requests)[0][1] > 15 * K.STAGE
    assert {e[1] for e in exp} == {0, 1, 2, 3, 4, N.TM_NONE}      # every filter decides somewhere, and none
    ids = [c["clientid"] for c in clients]
    for want_id, name_len in ((b"a", 4095), (b"aa", 4096), (b"ab", 4096)):       # %c last: the id is the last level
        hits = [i for i, (c, _a, x) in enumerate(requests) if exp[i][1] == 2 and ids[c] == want_id and len(x) == name_len]
        assert len(hits) == 2, (want_id, hits)
    assert all(ids[requests[i][0]] in (b"a", b"aa", b"ab") for i in range(len(exp)) if exp[i][1] == 2)
    assert_same(device(eng, terms, clients, requests), exp, requests)


def test_max_shape_one_request_at_a_time(eng, max_shape):
    """The same requests alone: 4,096 bytes fit the stage, and the answers are
    those of the global path."""
    terms, clients, requests, exp = max_shape
    acl = eng.acl_create(terms)
    try:
        got = []
        for q in requests:
            assert len(q[2]) <= K.STAGE
            v, r = eng.acl_check(acl, clients, [q])
            got.append((int(v[0]), int(r[0])))
    finally:
        acl.close()
    assert_same(got, exp, requests)


# ---- 5. waves and tails -------------------------------------------------------------------
@pytest.mark.parametrize("final", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 511, 513])
def test_lanes_decide_at_different_rules(eng, n, final):
    terms, clients, requests = K.wave_case(n, final)
    assert len(terms) == K.WAVE_RULES + final and len(requests) == n
    exp = mirror(terms, clients, requests)
    for w in range(0, n - 62, 64):                      # each full wave: 48 deciding rules, and the client no rule admits
        rules = {e[1] for e in exp[w:w + 64]}
        assert len(rules) >= 49 - (w + 64 == n), (w, len(rules))
        assert (K.WAVE_RULES if final else N.TM_NONE) in rules
    assert exp[-1] == ((N.TM_ACL_DENY, K.WAVE_RULES) if final else NOMATCH)       # under no filter: the last rule or none
    assert_same(device(eng, terms, clients, requests), exp, requests)


def test_no_rules_at_a_block_tail(eng):
    _terms, clients, requests = K.wave_case(257)
    assert device(eng, [], clients, requests) == [NOMATCH] * 257


# ---- 6. non-zero base ------------------------------------------------------------------------
def raw_check(eng, acl, clients, requests, base, junk):
    """tm_acl_check through the C ABI with offsets[0] == base and `junk` before the first name."""
    cs, keep = A.encode_clients(clients)
    buf, offs, cof, acc = A.encode_requests(requests)
    buf = np.concatenate([np.frombuffer(junk, np.uint8), buf]).copy()
    offs = (offs + np.uint64(base)).astype(np.uint64)
    n = len(requests)
    ver, rule = np.full(n, 9, np.uint8), np.full(n, 9, np.uint32)
    rc = eng.L.tm_acl_check(eng.h, acl.h, C.byref(cs), buf.ctypes.data, offs.ctypes.data, cof.ctypes.data,
                            acc.ctypes.data, n, ver.ctypes.data, rule.ctypes.data)
    assert rc == N.TM_OK
    del keep
    return list(zip(ver.tolist(), rule.tolist()))


@pytest.mark.parametrize("base", [5, 21, 4096 + 7])
def test_names_that_start_past_the_buffer_start(eng, base):
    """offsets[0] != 0, off a 16-byte boundary, junk before the first name:
    the answers are those of the same requests at base 0."""
    terms, clients, requests, _edges = K.stage_case(1, K.STAGE, "pattern", tag=b"b%d" % base)
    wt, wc, wq = K.wave_case(65)
    acl, wacl = eng.acl_create(terms), eng.acl_create(wt)
    try:
        junk = (b"s/k0/#E/+" * (base // 9 + 1))[:base]
        assert len(junk) == base and base % 16 != 0
        for a, tm, cl, rq in ((acl, terms, clients, requests), (wacl, wt, wc, wq)):
            at0 = raw_check(eng, a, cl, rq, 0, b"")
            assert_same(at0, mirror(tm, cl, rq), rq)
            assert_same(raw_check(eng, a, cl, rq, base, junk), at0, rq)
    finally:
        acl.close()
        wacl.close()


def test_two_replicas_on_one_device_split_mid_line(eng):
    """70,000 requests (the wave and the stage patterns repeated) over two
    replicas on device 0: the second slice starts at request 35,000, inside a
    16-byte line and inside a repetition, with a base of its own."""
    terms, clients, requests, period = K.slice_case(70000)
    assert len(requests) == 70000 and period == 1213 and 35000 % period != 0
    offs = np.cumsum([0] + [len(q[2]) for q in requests])
    assert offs[35000] % 16 != 0
    exp = mirror(terms, clients, requests[:period])
    assert len({e[1] for e in exp}) >= 55 and (N.TM_ACL_DENY, len(terms) - 1) in exp
    rep = Engine(devices=[0, 0])
    try:
        assert rep.replicas == 2
        acl2, acl1 = rep.acl_create(terms), eng.acl_create(terms)
        v2, r2 = rep.acl_check(acl2, clients, requests)
        v1, r1 = eng.acl_check(acl1, clients, requests)
        acl1.close()
    finally:
        rep.close()
    assert np.array_equal(v1, v2) and np.array_equal(r1, r2)
    got = list(zip(v2.tolist(), r2.tolist()))
    lo = 35000 - 1500
    assert_same(got[lo:lo + 3000], [exp[i % period] for i in range(lo, lo + 3000)], requests[lo:lo + 3000])
    ev = np.array([e[0] for e in exp], np.uint8)[np.arange(70000) % period]      # and, cheaply, on all of them
    er = np.array([e[1] for e in exp], np.uint32)[np.arange(70000) % period]
    assert np.array_equal(v2, ev) and np.array_equal(r2, er)
