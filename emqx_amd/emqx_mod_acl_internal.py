"""emqx_mod_acl_internal mirror (src/emqx_mod_acl_internal.erl) plus the default
fold of emqx_access_control:do_check_acl/3 (src/emqx_access_control.erl:62-67).

The batched device form is Engine.acl_check; emqx_acl_cache and the
file:consult parsing of acl.conf are not mirrored.
"""

from __future__ import annotations

from . import emqx_access_rule as R


def filter_(pubsub, rule) -> bool:
    """filter/2, src/emqx_mod_acl_internal.erl:110-121 (rule compiled)."""
    if len(rule) == 2:                                   # :110-113
        return True
    access = rule[2]
    if pubsub == "publish" and access == "publish":      # :114-115
        return True
    if access == "pubsub":                               # :116-117
        return True
    if pubsub == "subscribe" and access == "subscribe":  # :118-119
        return True
    return False                                         # :120-121


def rules(terms):
    """rules_from_file/1 after file:consult, src/emqx_mod_acl_internal.erl:96-98."""
    rs = [R.compile(t) for t in terms]
    return {"publish": [r for r in rs if filter_("publish", r)],
            "subscribe": [r for r in rs if filter_("subscribe", r)]}


def match(client, topic, rule_list):
    """match/3, src/emqx_mod_acl_internal.erl:82-90: the first matching rule wins."""
    for rule in rule_list:
        m = R.match(client, topic, rule)
        if m != "nomatch":
            return m
    return "nomatch"


def check_acl(client, pubsub, topic, rules):   # noqa: A002
    """check_acl/5, src/emqx_mod_acl_internal.erl:69-74 -> ("ok", A) | "ok"."""
    m = match(client, topic, rules.get(pubsub, []))      # lookup/2, :79-80
    return "ok" if m == "nomatch" else ("ok", m[1])


def check_acl_default(client, pubsub, topic, rules, acl_nomatch="deny"):   # noqa: A002
    """emqx_access_control:do_check_acl/3 with this module as the only
    'client.check_acl' hook (src/emqx_access_control.erl:62-67): the hook's
    {ok, A} replaces the zone's acl_nomatch default; anything but allow denies."""
    r = check_acl(client, pubsub, topic, rules)
    acc = acl_nomatch if r == "ok" else r[1]
    return "allow" if acc == "allow" else "deny"
