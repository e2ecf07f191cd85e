"""The expiry clauses of emqx_message restated one by one (src/emqx_message.erl),
with the clock passed in: the tests' reference of tm_sessions_drain's expiry.
Pure host code, written from the Erlang.

  is_expired/1     src/emqx_message.erl:224-228
  update_expiry/1  src/emqx_message.erl:230-239
  elapsed/1        src/emqx_message.erl:296-297

A message is a dict; `timestamp` is #message.timestamp in milliseconds and
`headers` #message.headers, a dict that may hold `properties`, a dict that may
hold 'Message-Expiry-Interval' in seconds.  `now` stands for
erlang:system_time(millisecond).  Nothing changes in place.
"""

from __future__ import annotations

EXPIRY = "Message-Expiry-Interval"


def timer_seconds(s: int) -> int:
    """timer:seconds/1."""
    return 1000 * s


def elapsed(since: int, now: int) -> int:
    """elapsed/1 (:296-297), milliseconds."""
    return max(0, now - since)                                          # :297


def _interval(msg):
    """The Interval of the pattern #message{headers = #{properties :=
    #{'Message-Expiry-Interval' := Interval}}}, or None when it does not match."""
    props = msg.get("headers", {}).get("properties")
    if isinstance(props, dict) and EXPIRY in props:
        return props[EXPIRY]
    return None


def is_expired(msg, now: int) -> bool:
    """is_expired/1 (:224-228)."""
    interval = _interval(msg)
    if interval is not None:                                            # :225-226
        return elapsed(msg["timestamp"], now) > timer_seconds(interval)   # :227
    return False                                                        # :228


def update_expiry(msg, now: int):
    """update_expiry/1 (:230-239) -> the message (a new dict when it changes)."""
    interval = _interval(msg)
    if interval is not None:                                            # :231-232
        e = elapsed(msg["timestamp"], now)                              # :233
        if e > 0:                                                       # :234
            interval1 = max(1, interval - e // 1000)                    # :235
            props = dict(msg["headers"]["properties"], **{EXPIRY: interval1})
            return dict(msg, headers=dict(msg["headers"], properties=props))   # :236 set_header/3
        return msg                                                      # :237
    return msg                                                          # :239
