"""emqx_pqueue restated clause by clause (src/emqx_pqueue.erl): the priority
queue under emqx_mqueue, used by the tests as the reference of
tm_batch_window_prio.  Pure host code, written from the Erlang.

Erlang terms as Python values, so that every clause reads as its original:
  []            None
  [H | T]       (H, T)             a cons cell; cons/1 and uncons by index
  {queue, In, Out, Len}            ("queue", In, Out, Len)
  {pqueue, [{P, Q}]}               ("pqueue", [(P, Q), ...])  (a short Python list)
  infinity      "infinity"
Inside a pqueue the priorities are negated (maybe_negate_priority/1 :267-268)
so that lists:keysort/2 puts the highest first; `infinity` stays and is kept
in front by hand (:137-146).  All values are immutable: every function returns
the new queue.
"""

from __future__ import annotations

INFINITY = "infinity"
NIL = None


def _list(*xs):
    out = NIL
    for x in reversed(xs):
        out = (x, out)
    return out


def _reverse(lst, tail=NIL):
    """lists:reverse/2."""
    while lst is not NIL:
        tail = (lst[0], tail)
        lst = lst[1]
    return tail


def _is_one(lst) -> bool:
    """the pattern [_]"""
    return lst is not NIL and lst[1] is NIL


def new():
    """new/0 (:71-73)."""
    return ("queue", NIL, NIL, 0)                                       # :73


def is_empty(q) -> bool:
    """is_empty/1 (:85-89)."""
    return q == ("queue", NIL, NIL, 0)                                  # :86-87, else :88-89


def len_(q) -> int:
    """len/1 (:91-95)."""
    if q[0] == "queue":                                                 # :92-93
        return q[3]
    return sum(len_(sq) for _, sq in q[1])                              # :94-95


def maybe_negate_priority(p):
    """maybe_negate_priority/1 (:267-268)."""
    return INFINITY if p == INFINITY else -p


def _keysearch(p, queues):
    for k, sq in queues:
        if k == p:
            return sq
    return None


def _keysort(queues):
    """lists:keysort(1, _) over integer keys (the callers keep infinity out)."""
    return sorted(queues, key=lambda e: e[0])


def plen(p, q) -> int:
    """plen/2 (:97-106)."""
    if q[0] == "queue":
        return q[3] if p == 0 else 0                                    # :98-99, :100-101
    sq = _keysearch(maybe_negate_priority(p), q[1])                     # :103
    return len_(sq) if sq is not None else 0                            # :104-105


def in_(x, *args):
    """in/2 (:119-121) and in/3 (:123-147): in_(X, Q) or in_(X, Priority, Q)."""
    if len(args) == 1:
        return in_(x, 0, args[0])                                       # :120-121
    priority, q = args
    if q[0] == "queue":
        _, in_l, out_l, n = q
        if priority == 0:
            if _is_one(in_l) and out_l is NIL and n == 1:               # :124-125
                return ("queue", _list(x), in_l, 2)
            return ("queue", (x, in_l), out_l, n + 1)                   # :126-127
        if in_l is NIL and out_l is NIL and n == 0:                     # :128-129
            return in_(x, priority, ("pqueue", []))
        return in_(x, priority, ("pqueue", [(0, q)]))                   # :130-131
    queues = q[1]                                                       # :132
    p = maybe_negate_priority(priority)                                 # :133
    sq = _keysearch(p, queues)                                          # :134
    if sq is not None:
        return ("pqueue", [(k, in_(x, s)) if k == p else (k, s) for k, s in queues])   # :135-136 keyreplace
    one = ("queue", _list(x), NIL, 1)
    if p == INFINITY:                                                   # :137-138
        return ("pqueue", [(p, one)] + queues)
    if queues and queues[0][0] == INFINITY:                             # :141-143
        return ("pqueue", [queues[0]] + _keysort([(p, one)] + queues[1:]))
    return ("pqueue", _keysort([(p, one)] + queues))                    # :144-145


def r2f(r, n):
    """r2f/2 (:262-265)."""
    if r is NIL and n == 0:                                             # :262
        return ("queue", NIL, NIL, 0)
    if _is_one(r) and n == 1:                                           # :263
        return ("queue", NIL, r, 1)
    if n == 2:                                                          # :264  [X, Y]
        return ("queue", _list(r[0]), _list(r[1][0]), 2)
    x, (y, rest) = r                                                    # :265
    return ("queue", _list(x, y), _reverse(rest), n)


def out(*args):
    """out/1 (:149-171) and out/2 (:177-197): out(Q) or out(Priority, Q)
    -> ("empty" | ("value", V), Q1)."""
    if len(args) == 2:
        priority, q = args
        if q[0] == "queue":
            if priority == 0:                                           # :177-178
                return out(q)
            raise ValueError(f"badarg {priority!r}")                    # :179-180
        queues = q[1]
        p = maybe_negate_priority(priority)                             # :182
        sq = _keysearch(p, queues)                                      # :183
        if sq is None:                                                  # :195-196
            return "empty", q
        r, q1 = out(sq)                                                 # :185
        if is_empty(q1):                                                # :186-187 keydelete
            queues1 = [(k, s) for k, s in queues if k != p]
        else:                                                           # :188 keyreplace
            queues1 = [(k, q1) if k == p else (k, s) for k, s in queues]
        return r, _collapse(queues1)                                    # :190-194
    (q,) = args
    if q[0] == "queue":
        _, in_l, out_l, n = q
        if in_l is NIL and out_l is NIL and n == 0:                     # :150-151
            return "empty", q
        if _is_one(in_l) and out_l is NIL and n == 1:                   # :152-153
            return ("value", in_l[0]), ("queue", NIL, NIL, 0)
        if out_l is NIL:                                                # :154-156  [Y | In]
            y, rest = in_l
            v, o = _reverse(rest)
            return ("value", v), ("queue", _list(y), o, n - 1)
        if _is_one(out_l):                                              # :157-158
            return ("value", out_l[0]), r2f(in_l, n - 1)
        return ("value", out_l[0]), ("queue", in_l, out_l[1], n - 1)    # :159-160
    (p, sq), queues = q[1][0], q[1][1:]                                 # :161
    r, q1 = out(sq)                                                     # :162
    if is_empty(q1):                                                    # :163-168
        return r, _collapse(queues)
    return r, ("pqueue", [(p, q1)] + queues)                            # :169


def _collapse(queues):
    """the case of :164-168 and :190-194: no queue left, only priority 0 left, or a pqueue."""
    if not queues:
        return ("queue", NIL, NIL, 0)
    if len(queues) == 1 and queues[0][0] == 0:
        return queues[0][1]
    return ("pqueue", queues)
