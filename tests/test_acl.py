"""ACL check on the CPU: the Python mirrors of emqx_access_rule /
emqx_mod_acl_internal / emqx_access_control against the reference's known
answers and a directed table of its clauses, and the host side of the C ABI
(tm_acl_create's validation on a host-only engine, struct layouts)."""

import ctypes as C
import os
import shutil
import subprocess

import pytest

import acl_cases as K
from emqx_amd import _native as N
from emqx_amd import acl as A
from emqx_amd import emqx_access_control as AC
from emqx_amd import emqx_access_rule as R
from emqx_amd import emqx_mod_acl_internal as M
from emqx_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- known answers ------------------------------------------------------------
def test_kat_compile():
    kat = K.kat()
    assert len(kat["compile"]) == 4
    for case in kat["compile"]:
        assert R.compile(K.dec_rule(case["rule"])) == K.dec_compiled(case["compiled"]), case["src"]


def test_kat_match():
    kat = K.kat()
    assert len(kat["match"]) == 16
    for case in kat["match"]:
        client = K.dec_client(kat["clients"][case["client"]])
        exp = case["expect"] if case["expect"] == "nomatch" else tuple(case["expect"])
        got = R.match(client, case["topic"].encode(), R.compile(K.dec_rule(case["rule"])))
        assert got == exp, case["src"]


def test_kat_mod_acl_internal_and_access_control():
    kat = K.kat()
    sec = kat["mod_acl_internal"]
    rules = {k: [R.compile(K.dec_rule(r)) for r in v] for k, v in sec["rules"].items()}
    client = K.dec_client(kat["clients"][sec["client"]])
    for access, topic, exp in sec["cases"]:
        got = M.check_acl(client, access, topic.encode(), rules)
        assert got == (exp if exp == "ok" else tuple(exp)), (sec["src"], access)
    sec = kat["access_control"]
    client = K.dec_client(kat["clients"][sec["client"]])
    for case in sec["cases"]:
        got = AC.check_acl(client, case["pubsub"], case["topic"].encode(), sec["rules"], case["acl_nomatch"])
        assert got == case["expect"], sec["src"]
    # a hook's {ok, deny} beats acl_nomatch = allow; anything but allow denies
    deny_all = M.rules([("deny", R.ALL)])
    assert AC.check_acl(client, "publish", b"t", deny_all, "allow") == "deny"
    assert AC.check_acl(client, "publish", b"t", M.rules([("allow", R.ALL)]), "deny") == "allow"


def test_stock_acl_conf():
    """etc/acl.conf:19-25 decided by the mirror: the split keeps the file's order."""
    terms = [K.dec_rule(r) for r in K.kat()["acl_conf"]["rules"]]
    rules = M.rules(terms)
    assert len(rules["publish"]) == 2 and len(rules["subscribe"]) == 4
    dash = {"clientid": b"d", "username": b"dashboard", "peerhost": "10.1.1.1"}
    local = {"clientid": b"l", "username": b"x", "peerhost": "127.0.0.1"}
    other = {"clientid": b"o", "username": None, "peerhost": "10.1.1.1"}
    compiled = [R.compile(t) for t in terms]
    for client, access, topic, verdict, idx in [
            (dash, "subscribe", b"$SYS/brokers", "allow", 0),
            (dash, "subscribe", b"#", "deny", 2),            # {eq, "#"}
            (local, "subscribe", b"#", "allow", 1),
            (local, "publish", b"$SYS/x", "allow", 1),
            (other, "subscribe", b"$SYS/x", "deny", 2),
            (other, "subscribe", b"a/#", "allow", 3),        # {eq, "#"} is literal
            (other, "publish", b"$SYS/x", "allow", 3)]:
        assert M.check_acl(client, access, topic, rules) == ("ok", verdict)
        assert K.decide(compiled, client, access, topic)[:2] == (K.CODE[verdict], idx)


def test_compile_rejects_what_the_reference_has_no_clause_for():
    for bad in [("allow", b"client1", "pubsub", ["t"]),          # a bare binary who: in the type, not in compile/2
                ("permit", R.ALL), ("allow", R.ALL, "connect", ["t"]), ("allow", R.ALL, "pubsub", "t"),
                ("allow", ("client",), "pubsub", ["t"]), ("allow", ("and", ("client", "x")), "pubsub", ["t"])]:
        with pytest.raises(R.RuleError):
            R.compile(bad)
    assert R.compile(("allow", ("client", "all"), "pubsub", [])) == ("allow", ("client", b"all"), "pubsub", [])
    assert R.compile(("allow", ("client", R.ALL), "pubsub", []))[1] == ("client", R.ALL)


# ---- directed table -----------------------------------------------------------------
def test_directed_table_mirror():
    table = K.directed()
    assert len(table) > 120
    for terms, client, access, topic, verdict, idx in table:
        compiled = [R.compile(t) for t in terms]
        assert K.decide(compiled, client, access, topic)[:2] == (verdict, idx), (terms, client, access, topic)
        got = M.check_acl(client, access, topic, M.rules(terms))     # the split lists give the same answer
        exp = "ok" if verdict == N.TM_ACL_NOMATCH else ("ok", "allow" if verdict == N.TM_ACL_ALLOW else "deny")
        assert got == exp, (terms, client, access, topic)


def test_feed_var_keeps_the_value_one_word():
    c = {"clientid": b"a/b", "username": None, "peerhost": None}
    assert R.feed_var(c, R.compile_topic("x/%c/%u")[1]) == [b"x", b"a/b", b"%u"]
    assert R.feed_var({"clientid": b"+"}, [b"%c"]) == [b"+"] and R.feed_var({"clientid": b"+"}, [b"%c"])[0] is not \
        R.T.PLUS


def test_random_generator_meets_the_floors():
    """The randomised GPU parity test's inputs exercise every outcome (the
    floors are asserted from the mirror's output alone, there and here)."""
    rules, clients, requests = K.gen_random(K.SEED)
    v, r, k = K.mirror_batch(rules, clients, requests)
    K.assert_floors(v, r, k)


# ---- the edge builders' conditions (test_gpu_acl_edges.py runs them on the device) -------------
@pytest.mark.parametrize("form", ["eq", "pattern"])
@pytest.mark.parametrize("width", [K.STAGE, K.STAGE + 1])
@pytest.mark.parametrize("lead", [0, 1, 15])
def test_stage_case_arithmetic(lead, width, form):
    """Block 1 starts `lead` bytes past a 16-byte boundary and spans `width`
    from it; the last block is partial and ends inside a 16-byte line; the edge
    names are decided by their own rule, which a changed first or last byte
    turns into the deny before it."""
    terms, clients, requests, edges = K.stage_case(lead, width, form, tag=b"%d%d" % (lead, width & 1))
    assert len(requests) == 2 * K.BLOCK + 188 and edges == [255, 256, 511, 699]
    (a0, a1, aa), (b0, b1, ba), (c0, c1, ca) = K.block_spans(requests)
    assert (a0, aa, a1) == (0, 0, 4096 + lead) and a1 - aa <= K.STAGE
    assert b0 % 16 == lead and ba == b0 - lead and b1 - ba == width
    assert c1 - ca <= K.STAGE and (c1 - ca) % 16 != 0
    assert all(len(q[2]) < 256 for q in requests)
    compiled = [R.compile(t) for t in terms]
    kinds = set()
    for k, i in enumerate(edges):
        c, access, name = requests[i]
        client = K.full_client(clients[c])
        v, j, kind = K.decide(compiled, client, access, name)
        assert (v, j) == (N.TM_ACL_ALLOW, 2 * k + 1)
        kinds.add(kind)
        for at in (0, -1):
            assert K.decide(compiled, client, access, K._flip(name, at))[:2] == (N.TM_ACL_DENY, 2 * k)
        for cut in (name[1:], name[:-1]):               # a dropped edge byte: neither
            assert K.decide(compiled, client, access, cut)[1] not in (2 * k, 2 * k + 1)
    assert kinds == {form}
    at = [q[2] for q in requests].index(b"m/k1/x/")
    assert K.BLOCK < at < 2 * K.BLOCK - 1
    assert K.decide(compiled, K.full_client(clients[1]), "publish", b"m/k1/x/")[:2] == (N.TM_ACL_ALLOW, 8)
    assert terms[8][3] == ["m/%c/x/+"]
    assert K.decide(compiled, K.full_client(clients[1]), "publish", b"m/k1/x")[:2] == (N.TM_ACL_DENY, 11)
    _v, r, _k = K.mirror_batch(terms, clients, requests)
    assert set(r) == {1, 3, 5, 7, 8, 9, 10, 11}


def test_who_trees_plain_evaluation_equals_the_mirror():
    terms, clients, requests, labels, plain = K.who_case()
    trees = K.who_trees()
    assert sum(K.who_depth(t) == N.TM_ACL_MAX_WHO_DEPTH for t in trees.values()) >= 8
    assert max(K.who_depth(t) for t in trees.values()) == N.TM_ACL_MAX_WHO_DEPTH
    assert K.who_depth(K.who_chain(33, K.TRUE_LEAF)) == 33
    assert K.who_depth(trees["wide or under and at depth 10"]) == 11
    for k in ("wide or", "wide and"):
        assert len(trees[k][1]) == 40
    # only the last child decides the wide nodes
    assert [K.who_plain(c, b"k1") for c in trees["wide or"][1]] == [False] * 39 + [True]
    assert [K.who_plain(c, b"k1") for c in trees["wide and"][1]] == [True] * 39 + [False]
    v, r, _ = K.mirror_batch(terms, clients, requests)
    assert list(zip(v, r)) == plain
    k1 = {labels[i // 2]: p[0] == N.TM_ACL_ALLOW for i, p in enumerate(plain) if i % 2 == 0}
    assert k1["deep and true"] and k1["deep or true"] and not k1["deep and false"] and not k1["deep or false"]
    assert k1["deep or sibling first"] and not k1["deep and sibling first"]
    assert k1["wide or"] and not k1["wide and"] and k1["wide and every"] and not k1["wide or none"]
    assert all(p == (N.TM_ACL_NOMATCH, N.TM_NONE) for p in plain[1::2])       # client k0 passes none of them


def test_address_table_integer_compare_equals_the_mirror():
    import ipaddress
    terms, clients, requests, plain, ranges = K.ip_case()
    v, r, _ = K.mirror_batch(terms, clients, requests)
    assert list(zip(v, r)) == plain
    # each word of a v6 address, and v4, varies alone in some range, with every pair of word values
    seen = set()
    for lo, hi, fam in ranges:
        if lo < hi:
            diff = lo ^ hi
            words = [q for q in range(4) if (diff >> (32 * (3 - q))) & 0xFFFFFFFF] if fam == 6 else ["v4"]
            if len(words) == 1:
                sh = 0 if fam == 4 else 32 * (3 - words[0])
                seen.add((words[0], (lo >> sh) & 0xFFFFFFFF, (hi >> sh) & 0xFFFFFFFF))
    pairs = [(a, b) for a in K.IP_WORDS for b in K.IP_WORDS if a < b]
    assert len(pairs) == 15
    for w in (0, 1, 2, 3, "v4"):
        assert all((w, a, b) in seen for a, b in pairs), w
    # both ends and their neighbours are probed, in the range's own family
    asked = {}
    for (c, _a, t), p in zip(requests, plain):
        h = clients[c]["peerhost"]
        asked.setdefault(int(t[2:]), set()).add(None if h is None else
                                                (ipaddress.ip_address(h).version, int(ipaddress.ip_address(h))))
    for j, (lo, hi, fam) in enumerate(ranges):
        top = (1 << (32 if fam == 4 else 128)) - 1
        for p in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1):
            assert not 0 <= p <= top or (fam, p) in asked[j], (j, hex(p))
        assert None in asked[j] and any(x is not None and x[0] != fam for x in asked[j])
    assert sum(p[0] == N.TM_ACL_ALLOW for p in plain) > 300 and sum(p[0] == N.TM_ACL_NOMATCH for p in plain) > 300


def test_level_table_match_share():
    """The cross product's pattern form for the client with both fields: 2 to
    10 % of the pairs match, among them filters ending in '#', holding '+',
    holding %c and holding an empty level."""
    assert len(K.LEVEL_FILTERS) == len(set(K.LEVEL_FILTERS)) == 258
    assert len(K.LEVEL_NAMES) == len(set(K.LEVEL_NAMES)) == 258
    client = K.full_client(K.LEVEL_CLIENTS[0])
    assert (client["clientid"], client["username"]) == (b"cid", b"b")
    hits = []
    for f in K.LEVEL_FILTERS:
        rule = R.compile(("allow", R.ALL, "publish", [f.decode()]))
        hits += [f for x in K.LEVEL_NAMES if R.match(client, x, rule) != "nomatch"]
    share = len(hits) / (258 * 258)
    assert 0.02 <= share <= 0.10, share
    assert any(f.endswith(b"#") for f in hits) and any(b"+" in f.split(b"/") for f in hits)
    assert any(b"%c" in f.split(b"/") for f in hits) and any(b"" in f.split(b"/") for f in hits)
    # an undefined field leaves %c / %u literal: it equals a name level spelled the same
    terms, clients, requests = K.level_case(b"a/%c")
    v, _r, _k = K.mirror_batch(terms, clients, requests)
    got = {(c, acc, x) for (c, acc, x), y in zip(requests, v) if y != N.TM_ACL_NOMATCH}
    assert got == {(0, "publish", b"a/cid"), (2, "publish", b"a/cid"), (1, "publish", b"a/%c"),
                   (0, "subscribe", b"a/%c"), (1, "subscribe", b"a/%c"), (2, "subscribe", b"a/%c")}


def test_max_shape_and_wave_cases():
    terms, clients, requests = K.max_shape_case()
    assert {len(q[2]) for q in requests} == {4095, 4096}
    assert max(len(t) for rule in terms for t in (x[1] if isinstance(x, tuple) else x for x in rule[3])) == 4096
    assert {len(c["clientid"]) for c in clients if c["clientid"] is not None} >= {0, 1, 2, 3, 4097}
    _v, r, _k = K.mirror_batch(terms, clients, requests)
    assert set(r) == {0, 1, 2, 3, 4, N.TM_NONE}
    for n in (1, 63, 64, 65, 255, 256, 257, 511, 513):
        for final in (True, False):
            terms, clients, requests = K.wave_case(n, final)
            v, r, _k = K.mirror_batch(terms, clients, requests)
            assert (v[-1], r[-1]) == ((N.TM_ACL_DENY, 48) if final else (N.TM_ACL_NOMATCH, N.TM_NONE))
            for w in range(0, n - 62, 64):
                assert len(set(r[w:w + 64])) >= 49 - (w + 64 == n), (n, w)
    assert 64 % 5 != 0 and len(clients) == 49
    terms, clients, requests, period = K.slice_case(70000)
    assert period == 1213 and 35000 % period == 1036
    assert sum(len(q[2]) for q in requests[:35000]) % 16 != 0


# ---- C ABI on a host-only engine ------------------------------------------------------
def _create(e, arr, n):
    h = C.c_void_p()
    rc = e.L.tm_acl_create(e.h, arr, n, C.byref(h))
    if rc == 0:
        e.L.tm_acl_free(e.h, h)
    return rc, (e.L.tm_last_error() or b"").decode()


def _one_rule(who_nodes, topics=(b"t",), allow=1, access=3, eq=0):
    keep = []
    arr = (N.AclRule * 1)()
    wa = (N.AclWho * max(len(who_nodes), 1))(*who_nodes)
    ta = (N.AclTopic * max(len(topics), 1))()
    for i, t in enumerate(topics):
        ta[i].filter, ta[i].len, ta[i].eq = A._buf(t, keep), len(t), eq
    arr[0].allow, arr[0].access = allow, access
    arr[0].who, arr[0].n_who, arr[0].topics, arr[0].n_topics = wa, len(who_nodes), ta, len(topics)
    keep += [wa, ta]
    return arr, keep


def _node(kind, n_children=0, family=0):
    n = N.AclWho()
    n.kind, n.n_children, n.family = kind, n_children, family
    return n


def test_acl_create_validates_on_a_host_only_engine():
    e = Engine(device=-1)
    ok = [_node(N.TM_WHO_ALL)]
    arr, keep = _one_rule(ok)
    assert _create(e, arr, 1)[0] == N.TM_OK
    assert _create(e, None, 0)[0] == N.TM_OK                     # zero rules
    bad = {
        "allow": _one_rule(ok, allow=2),
        "access": _one_rule(ok, access=4),
        "two trees": _one_rule([_node(N.TM_WHO_ALL), _node(N.TM_WHO_ALL)]),
        "ends inside": _one_rule([_node(N.TM_WHO_AND, 2), _node(N.TM_WHO_ALL)]),
        "family": _one_rule([_node(N.TM_WHO_IPADDR, family=5)]),
        "kind": _one_rule([_node(99)]),
        "long": _one_rule(ok, topics=(b"a" * (N.TM_MAX_TOPIC_LEN + 1),)),
        "deep": _one_rule([_node(N.TM_WHO_AND, 1)] * N.TM_ACL_MAX_WHO_DEPTH + [_node(N.TM_WHO_ALL)]),
    }
    for what, (arr, keep) in bad.items():
        rc, text = _create(e, arr, 1)
        assert rc == N.TM_EINVAL, what
        assert text.startswith("rule 0:"), (what, text)
    # the documented limit itself is accepted: 31 nested 'and' + a leaf = depth 32
    arr, keep = _one_rule([_node(N.TM_WHO_OR, 1)] * (N.TM_ACL_MAX_WHO_DEPTH - 1) + [_node(N.TM_WHO_ALL)])
    assert _create(e, arr, 1)[0] == N.TM_OK
    arr, keep = _one_rule(ok, topics=(b"a" * N.TM_MAX_TOPIC_LEN,))
    assert _create(e, arr, 1)[0] == N.TM_OK
    arr, keep = _one_rule(ok, topics=())                        # [] topics: a rule that never matches
    assert _create(e, arr, 1)[0] == N.TM_OK


def test_acl_check_without_a_device_is_refused():
    e = Engine(device=-1)
    acl = e.acl_create([("allow", R.ALL)])
    with pytest.raises(N.TmError) as ei:
        e.acl_check(acl, [{"clientid": b"c", "username": None, "peerhost": None}], [(0, "publish", b"t")])
    assert ei.value.rc == N.TM_ENODEV
    with pytest.raises(R.RuleError):
        e.acl_create([("allow", b"client1", "pubsub", ["t"])])
    acl.close()
    with pytest.raises(RuntimeError):
        acl.h


def test_encoder_writes_who_trees_in_pre_order():
    who = R.compile_who(("and", [("or", [("client", "a"), ("user", R.ALL)]), ("ipaddr", "192.168.0.1/24")]))
    nodes = A.who_nodes(who, [])
    assert [(n.kind, n.n_children) for n in nodes] == [
        (N.TM_WHO_AND, 2), (N.TM_WHO_OR, 2), (N.TM_WHO_CLIENT, 0), (N.TM_WHO_USER_ALL, 0), (N.TM_WHO_IPADDR, 0)]
    assert nodes[4].family == 4 and bytes(nodes[4].lo)[:4] == bytes([192, 168, 0, 0])
    assert bytes(nodes[4].hi)[:4] == bytes([192, 168, 0, 255])
    six = A.who_nodes(R.compile_who(("ipaddr", "2001:db8::/32")), [])[0]
    assert six.family == 6 and bytes(six.lo) == bytes([0x20, 0x01, 0x0d, 0xb8]) + bytes(12)
    assert bytes(six.hi) == bytes([0x20, 0x01, 0x0d, 0xb8]) + b"\xff" * 12


ACL_PAIRS = [("tm_acl_who", N.AclWho), ("tm_acl_topic", N.AclTopic), ("tm_acl_rule", N.AclRule),
             ("tm_acl_clients", N.AclClients)]


@pytest.mark.skipif(not shutil.which("gcc"), reason="needs gcc")
def test_acl_ctypes_mirrors_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "emqx_tm.h"', "int main(void) {"]
    for cname, py in ACL_PAIRS:
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    for name in ("TM_ACL_DENY", "TM_ACL_ALLOW", "TM_ACL_NOMATCH", "TM_ACL_PUBLISH", "TM_ACL_SUBSCRIBE", "TM_ACL_PUBSUB",
                 "TM_WHO_ALL", "TM_WHO_CLIENT_ALL", "TM_WHO_USER_ALL", "TM_WHO_CLIENT", "TM_WHO_USER",
                 "TM_WHO_IPADDR", "TM_WHO_AND", "TM_WHO_OR", "TM_ACL_MAX_WHO_DEPTH"):
        lines.append(f'printf("const {name} %u\\n", (unsigned){name});')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        k1, k2, v = ln.split()
        got[(k1, k2)] = int(v)
    for cname, py in ACL_PAIRS:
        assert got[(cname, "size")] == C.sizeof(py), cname
        for f in py._fields_:
            assert got[(cname, f[0])] == getattr(py, f[0]).offset, (cname, f[0])
    for (k1, k2), v in got.items():
        if k1 == "const":
            assert getattr(N, k2) == v, k2


# ---- the NIF boundary (host-only engine) -------------------------------------------------
@pytest.fixture(scope="module")
def nif():
    from nif_harness import Nif
    return Nif()


def test_nif_scheduler_classes(nif):
    assert nif.flags("acl_new", 2) == 2           # ERL_NIF_DIRTY_JOB_IO_BOUND: compiles and uploads
    assert nif.flags("acl_check", 4) == 2         # waits for the device


def test_nif_acl_terms(nif):
    e = nif.new(-1)
    before = nif.live_resources()
    terms = [K.dec_rule(r) for r in K.kat()["acl_conf"]["rules"]]
    terms.append(("deny", ("or", [("client", R.ALL), ("and", [("user", "u"), ("ipaddr", "2001:db8::/32")])]),
                  "publish", ["a/%c/#", ("eq", "x/+")]))
    t = nif.call_raw("acl_new", e, K.nif_rules(terms))
    assert nif.decode(t)[0] == "ok"
    from nif_harness import Raw
    acl = Raw(nif.L.mock_tuple_elem(t, 1))
    assert nif.live_resources() == before + 1
    clients = K.nif_clients([{"clientid": b"c", "username": None, "peerhost": "::1"}])
    # a host-only engine refuses the check itself, after the terms were accepted
    assert nif.call("acl_check", e, acl, clients, [(0, "publish", b"t")]) == ("error", "enodev")
    assert nif.call("acl_check", e, acl, [], []) == ("error", "enodev")
    bad_rules = [
        [("allow", b"client1", "pubsub", [b"t"])],                 # a bare binary who
        [("permit", "all")], [("allow", "everyone")], [("allow", "all", "connect", [b"t"])],
        [("allow", "all", "pubsub", b"t")], [("allow", "all", "pubsub", ["t"])],
        [("allow", ("client", 7), "pubsub", [b"t"])], [("allow", ("ipaddr", b"127.0.0.1"), "pubsub", [b"t"])],
        [("allow", ("ipaddr", ((1, 2, 3, 4), (0, 0, 0, 0, 0, 0, 0, 1), 32)), "pubsub", [b"t"])],
        [("allow", ("ipaddr", ((1, 2, 3, 256), (1, 2, 3, 4), 32)), "pubsub", [b"t"])],
        [("allow", ("and", ("client", "all")), "pubsub", [b"t"])],
        [("allow", "all", "pubsub", [("ne", b"t")])], [("allow", "all", "pubsub")], "rules",
    ]
    for bad in bad_rules:
        assert nif.call("acl_new", e, bad) == ("#badarg",), bad
    for cl, rq in [([("c", b"u", "undefined")], [(0, "publish", b"t")]),            # an atom clientid
                   ([(b"c", b"u", (1, 2, 3))], [(0, "publish", b"t")]),             # not an inet tuple
                   ([(b"c", b"u")], [(0, "publish", b"t")]),
                   (clients, [(1, "publish", b"t")]),                                # no such client
                   (clients, [(0, "pubsub", b"t")]), (clients, [(0, "publish", "t")]), (clients, [(0, "publish")]),
                   (clients, "requests")]:
        assert nif.call("acl_check", e, acl, cl, rq) == ("#badarg",), (cl, rq)
    assert nif.call("acl_check", e, e, clients, []) == ("#badarg",)                 # not a rule set
    e2 = nif.new(-1)
    assert nif.call("acl_check", e2, acl, clients, []) == ("#badarg",)              # another engine's rule set
    nif.drop(e2)
    # too deep for the device's who stack: the engine refuses it, not the term parser
    deep = "all"
    for _ in range(N.TM_ACL_MAX_WHO_DEPTH):
        deep = ("and", [deep])
    assert nif.call("acl_new", e, [("allow", deep, "pubsub", [b"t"])]) == ("error", "einval")
    # the rule set keeps its engine alive; both go with their last terms
    eng_alive = nif.live_resources()
    nif.drop(e)
    assert nif.live_resources() == eng_alive
    nif.drop(acl)
    assert nif.live_resources() == eng_alive - 2
