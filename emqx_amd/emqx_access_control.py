"""emqx_access_control:check_acl/3 mirror (src/emqx_access_control.erl:47-67),
with emqx_mod_acl_internal as the only 'client.check_acl' hook and no ACL cache."""

from __future__ import annotations

from . import emqx_mod_acl_internal as M


def check_acl(client, pubsub, topic, rules, acl_nomatch="deny"):
    """do_check_acl/3, :62-67 -> "allow" | "deny"."""
    return M.check_acl_default(client, pubsub, topic, rules, acl_nomatch)
