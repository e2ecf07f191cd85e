"""Pythonic wrapper of one tm_engine (one host trie mirrored into an HBM
replica on each of its MI355X devices).

    eng = Engine(device=0)                       # one GPU
    eng = Engine(devices=[0, 1, 2, 3])           # one engine over four GPUs
    eng.insert(b"sensor/+/#")
    eng.match(b"sensor/1/temp")                  # -> [b"sensor/+/#"]
    offs, ids = eng.match_batch(topics)          # CSR over a whole batch
"""

from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _native as N
from .gen import Strings


def _pack(topics) -> Strings:
    if isinstance(topics, Strings):
        return topics
    return Strings.from_list(list(topics))


class Tokens:
    """Tokenised publishes (tm_tokenize layout): words u32 = class << 29 | word id,
    toff u32[n+1], tflags u8[n]."""

    def __init__(self, words: np.ndarray, toff: np.ndarray, tflags: np.ndarray):
        self.words, self.toff, self.tflags = words, toff, tflags

    def __len__(self):
        return len(self.toff) - 1

    @property
    def nwords(self) -> int:
        return int(self.toff[-1])


class Batch:
    """A device-resident publish batch (tm_batch_prepare / launch / wait / result)."""

    def __init__(self, eng: "Engine", topics=None, handle=None, n=0, dedup=False, stream=False, replica=None):
        self.eng = eng
        if handle is not None:          # built by Engine.prepare_tokens
            self.h = handle
            self.n = n
            return
        s = _pack(topics)
        self.n = len(s)
        buf = s.buf if s.buf.size else np.zeros(1, np.uint8)
        self._buf = np.ascontiguousarray(buf)
        self._offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        h = C.c_void_p()
        flags = (N.TM_BATCH_DEDUP if dedup else 0) | (N.TM_BATCH_STREAM if stream else 0)
        if replica is None:
            N.check(eng.L.tm_batch_prepare_ex(eng.h, self._buf.ctypes.data, self._offs.ctypes.data, self.n,
                                              flags, C.byref(h)), "tm_batch_prepare_ex")
        else:
            N.check(eng.L.tm_batch_prepare_on(eng.h, replica, self._buf.ctypes.data, self._offs.ctypes.data,
                                              self.n, flags, C.byref(h)), "tm_batch_prepare_on")
        self.h = h

    def reprepare(self, topics, dedup=False):
        """tm_batch_prepare_ex in place: new publishes in the same handle (its
        replica, stream and buffers are kept)."""
        s = _pack(topics)
        self.n = len(s)
        buf = s.buf if s.buf.size else np.zeros(1, np.uint8)
        self._buf = np.ascontiguousarray(buf)
        self._offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        N.check(self.eng.L.tm_batch_prepare_ex(self.eng.h, self._buf.ctypes.data, self._offs.ctypes.data, self.n,
                                               N.TM_BATCH_DEDUP if dedup else 0, C.byref(self.h)),
                "tm_batch_prepare_ex")
        return self

    @property
    def replica(self) -> int:
        return int(self.eng.L.tm_batch_replica(self.eng.h, self.h))

    @property
    def slow_info(self) -> dict:
        """tm_debug_batch_slow: the generic path's restarts in the last launch
        and its scratch sizes (entries per wave) and waves."""
        out = (C.c_uint32 * 4)()
        N.check(self.eng.L.tm_debug_batch_slow(self.h, out), "tm_debug_batch_slow")
        return dict(zip(("restarts", "s_qcap", "s_ocap", "s_waves"), map(int, out)))

    def row_map(self):
        """-> (row_of uint32[n publishes], n_rows): result row of every publish."""
        p = C.POINTER(C.c_uint32)()
        nr = C.c_uint32()
        N.check(self.eng.L.tm_batch_row_map(self.eng.h, self.h, C.byref(p), C.byref(nr)), "tm_batch_row_map")
        return (np.ctypeslib.as_array(p, shape=(self.n,)).copy() if self.n else np.zeros(0, np.uint32)), nr.value

    def export(self, d_counts: int, d_ids: int, mul: int = 1, add: int = 0):
        """Per-topic counts and ids*mul+add into caller device buffers (tm_batch_export)."""
        N.check(self.eng.L.tm_batch_export(self.eng.h, self.h, d_counts, d_ids, mul, add), "tm_batch_export")

    def launch(self):
        N.check(self.eng.L.tm_batch_launch(self.eng.h, self.h), "tm_batch_launch")
        return self

    def wait(self):
        N.check(self.eng.L.tm_batch_wait(self.eng.h, self.h), "tm_batch_wait")
        return self

    def retokenize(self):
        """tm_batch_retokenize: the next launch tokenises the resident bytes again."""
        N.check(self.eng.L.tm_batch_retokenize(self.eng.h, self.h), "tm_batch_retokenize")
        return self

    def result(self):
        r = N.Result()
        N.check(self.eng.L.tm_batch_result(self.eng.h, self.h, C.byref(r)), "tm_batch_result")
        return _result_arrays(r)

    def result_packed(self):
        """tm_batch_result_packed -> (row_offsets u32[n+1], packed ids u8, id_bytes)."""
        r = N.ResultPacked()
        N.check(self.eng.L.tm_batch_result_packed(self.eng.h, self.h, C.byref(r)), "tm_batch_result_packed")
        n, m, ib = r.n_topics, int(r.n_matches), int(r.id_bytes)
        ro = np.ctypeslib.as_array(r.row_offsets, shape=(n + 1,)).copy()
        ids = np.ctypeslib.as_array(r.ids, shape=(m * ib,)).copy() if m else np.zeros(0, np.uint8)
        return ro, ids, ib

    def sample(self, rows):
        """tm_batch_sample: rows `rows` (row indices) of the waited batch,
        gathered on the device -> (offsets u32[k+1], ids) in that order."""
        idx = np.ascontiguousarray(np.asarray(rows, dtype=np.uint32))
        r = N.Result()
        N.check(self.eng.L.tm_batch_sample(self.eng.h, self.h, idx.ctypes.data, len(idx), C.byref(r)),
                "tm_batch_sample")
        return _result_arrays(r)

    def routes(self):
        """Device route resolution (tm_batch_routes) -> (row_offsets, filter_ids, dests)."""
        r = N.Routes()
        N.check(self.eng.L.tm_batch_routes(self.eng.h, self.h, C.byref(r)), "tm_batch_routes")
        return _routes_arrays(r)

    def dispatch(self, match_offsets: bool = False, counts_only: bool = False):
        """Device fan-out (tm_batch_dispatch): emqx_broker:dispatch/2 for every
        matched filter of every publish -> (row_offsets u64[n+1], match_offsets
        u64[m+1] or None, subscribers u32[deliveries] or None)."""
        d = self._dispatch((N.TM_DISPATCH_MATCH_OFFSETS if match_offsets else 0)
                           | (N.TM_DISPATCH_COUNT_ONLY if counts_only else 0))
        n, m, t = d.n_topics, int(d.n_matches), int(d.n_deliveries)
        offs = np.ctypeslib.as_array(d.row_offsets, shape=(n + 1,)).copy()
        moff = np.ctypeslib.as_array(d.match_offsets, shape=(m + 1,)).copy() if match_offsets else None
        if counts_only:
            subs = None
        else:
            subs = np.ctypeslib.as_array(d.subscribers, shape=(t,)).copy() if t else np.zeros(0, np.uint32)
        return offs, moff, subs

    def dispatch_device(self, match_offsets: bool = False):
        """Device-resident fan-out: -> (n_deliveries, fill kernel ms, device ptrs row/moff/subs);
        the moff pointer is None unless match_offsets."""
        d = self._dispatch(N.TM_DISPATCH_DEVICE | (N.TM_DISPATCH_MATCH_OFFSETS if match_offsets else 0))
        ptr = lambda p: C.cast(p, C.c_void_p).value  # noqa: E731
        return int(d.n_deliveries), float(d.fill_ms), ptr(d.row_offsets), ptr(d.match_offsets), ptr(d.subscribers)

    def dispatch_rows(self):
        """Fan-out over the walk's rows as it left them (TM_DISPATCH_ROWS), copied
        to the host for checking: (first delivery u64[n], deliveries u32[n],
        subscribers u32[total]); row i's deliveries are
        subscribers[first[i] : first[i] + count[i]]."""
        d = self._dispatch(N.TM_DISPATCH_ROWS)
        n, t = d.n_topics, int(d.n_deliveries)
        first = np.zeros(n, np.uint64)
        cnt = np.zeros(n, np.uint32)
        subs = np.zeros(t, np.uint32)
        ptr = lambda p: C.cast(p, C.c_void_p).value  # noqa: E731
        _d2h(first, ptr(d.row_offsets))
        _d2h(cnt, ptr(d.row_counts))
        _d2h(subs, ptr(d.subscribers))
        return first, cnt, subs

    def dispatch_rows_device(self):
        """TM_DISPATCH_ROWS kept in HBM: -> (n_deliveries, fill kernel ms)."""
        d = self._dispatch(N.TM_DISPATCH_ROWS)
        return int(d.n_deliveries), float(d.fill_ms)

    def dispatch_shared(self, strategy, keys=None, seed: int = 0, counts_only: bool = False):
        """Shared-subscription dispatch (tm_batch_dispatch_shared):
        emqx_shared_sub:dispatch/3 for every {To, Group} route of every publish
        -> (row_offsets u32[n+1], filter_ids, groups, subscribers), the three
        None with counts_only.  strategy: N.TM_SHARED_* or "random" /
        "round_robin" / "hash"; keys = one u32 per publish (hash:
        erlang:phash2(ClientId)); seed for random."""
        d = self._dispatch_shared(strategy, keys, seed, N.TM_SHARED_COUNT_ONLY if counts_only else 0)
        n, t = d.n_topics, int(d.n_deliveries)
        offs = np.ctypeslib.as_array(d.row_offsets, shape=(n + 1,)).copy()
        if counts_only:
            return offs, None, None, None
        cp = lambda p: np.ctypeslib.as_array(p, shape=(t,)).copy() if t else np.zeros(0, np.uint32)  # noqa: E731
        return offs, cp(d.filter_ids), cp(d.groups), cp(d.subscribers)

    def dispatch_shared_device(self, strategy, keys=None, seed: int = 0):
        """TM_SHARED_DEVICE: -> (n_deliveries, kernel ms, device ptrs
        row_offsets / filter_ids / groups / subscribers)."""
        d = self._dispatch_shared(strategy, keys, seed, N.TM_SHARED_DEVICE)
        ptr = lambda p: C.cast(p, C.c_void_p).value  # noqa: E731
        return (int(d.n_deliveries), float(d.kernel_ms), ptr(d.row_offsets), ptr(d.filter_ids), ptr(d.groups),
                ptr(d.subscribers))

    def shared_mode(self, strategy, keys=None, seed: int = 0):
        """Arms the batch (tm_batch_shared_mode): inboxes() / deliver() /
        window() then work on the merged list of ordinary and shared
        deliveries; strategy / keys / seed as dispatch_shared (the keys are
        copied).  shared_mode(None) disarms."""
        if strategy is None:
            N.check(self.eng.L.tm_batch_shared_mode(self.eng.h, self.h, None), "tm_batch_shared_mode")
            return
        o, _keep = self._shared_opts(strategy, keys, seed, 0)
        N.check(self.eng.L.tm_batch_shared_mode(self.eng.h, self.h, C.byref(o)), "tm_batch_shared_mode")

    def inbox_groups(self):
        """tm_batch_inbox_groups: u32[D'] parallel to publishes / filter_ids
        of the last inboxes() / deliver() / window() call on the armed batch:
        the group id of a shared delivery, TM_NONE for an ordinary one."""
        count = getattr(self, "_last_deliveries", 0)
        p = C.POINTER(C.c_uint32)()
        N.check(self.eng.L.tm_batch_inbox_groups(self.eng.h, self.h, 0, C.byref(p)), "tm_batch_inbox_groups")
        return np.ctypeslib.as_array(p, shape=(count,)).copy() if count else np.zeros(0, np.uint32)

    def inbox_groups_device(self) -> int:
        """TM_INBOX_DEVICE: the device pointer of the groups."""
        p = C.POINTER(C.c_uint32)()
        N.check(self.eng.L.tm_batch_inbox_groups(self.eng.h, self.h, N.TM_INBOX_DEVICE, C.byref(p)),
                "tm_batch_inbox_groups")
        return C.cast(p, C.c_void_p).value

    def inboxes(self):
        """Per-subscriber inboxes (tm_batch_inboxes): the deliveries of
        dispatch() grouped by subscriber, each inbox in mailbox order ->
        (subscribers u32[R] ascending, offsets u32[R+1], publishes u32[D],
        filter_ids u32[D]); inbox r is entries offsets[r] .. offsets[r+1]."""
        d = self._inboxes(0)
        r, t = int(d.n_subscribers), int(d.n_deliveries)
        cp = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy() if k else np.zeros(0, np.uint32)  # noqa: E731
        self.inbox_info = {"kernel_ms": float(d.kernel_ms), "passes": int(d.passes)}
        return cp(d.subscribers, r), cp(d.inbox_offsets, r + 1), cp(d.publishes, t), cp(d.filter_ids, t)

    def inboxes_device(self):
        """TM_INBOX_DEVICE: -> (n_subscribers, n_deliveries, kernel ms, passes,
        device ptrs subscribers / offsets / publishes / filter_ids)."""
        d = self._inboxes(N.TM_INBOX_DEVICE)
        ptr = lambda p: C.cast(p, C.c_void_p).value  # noqa: E731
        return (int(d.n_subscribers), int(d.n_deliveries), float(d.kernel_ms), int(d.passes), ptr(d.subscribers),
                ptr(d.inbox_offsets), ptr(d.publishes), ptr(d.filter_ids))

    def deliver(self, from_=None, msg=None, upgrade_qos: bool = False, nl_all: bool = False, subids: bool = False):
        """What the session sends (tm_batch_deliver): inboxes() after
        ignore_local/3 and enrich_subopts/3.  from_: u32[n] publisher of every
        publish (TM_NONE = none; None = nobody), msg: u8[n] QoS | TM_MSG_RETAIN
        | TM_MSG_RETAINED -> (subscribers u32[R'], offsets u32[R'+1], publishes
        u32[D'], filter_ids u32[D'], msg u8[D'], subids u32[D'] or None);
        deliver_info holds n_dropped_no_local and kernel_ms."""
        d, _keep = self._deliver(from_, msg, self._deliver_flags(upgrade_qos, nl_all, subids))
        r, t = int(d.n_subscribers), int(d.n_deliveries)
        cp = lambda p, k, ty=np.uint32: (np.ctypeslib.as_array(p, shape=(k,)).copy() if k  # noqa: E731
                                         else np.zeros(0, ty))
        self.deliver_info = {"kernel_ms": float(d.kernel_ms), "n_dropped_no_local": int(d.n_dropped_no_local)}
        return (cp(d.subscribers, r), cp(d.inbox_offsets, r + 1), cp(d.publishes, t), cp(d.filter_ids, t),
                cp(d.msg, t, np.uint8), cp(d.subids, t) if subids else None)

    def deliver_device(self, from_=None, msg=None, upgrade_qos: bool = False, nl_all: bool = False,
                       subids: bool = False):
        """TM_DELIVER_DEVICE: -> (n_subscribers, n_deliveries, n_dropped_no_local,
        kernel ms, device ptrs subscribers / offsets / publishes / filter_ids /
        msg / subids (None without subids))."""
        d, _keep = self._deliver(from_, msg, self._deliver_flags(upgrade_qos, nl_all, subids) | N.TM_DELIVER_DEVICE)
        ptr = lambda p: C.cast(p, C.c_void_p).value  # noqa: E731
        return (int(d.n_subscribers), int(d.n_deliveries), int(d.n_dropped_no_local), float(d.kernel_ms),
                ptr(d.subscribers), ptr(d.inbox_offsets), ptr(d.publishes), ptr(d.filter_ids), ptr(d.msg),
                ptr(d.subids) if subids else None)

    @staticmethod
    def _deliver_flags(upgrade_qos: bool, nl_all: bool, subids: bool) -> int:
        return ((N.TM_DELIVER_UPGRADE_QOS if upgrade_qos else 0) | (N.TM_DELIVER_NL_ALL if nl_all else 0)
                | (N.TM_DELIVER_SUBIDS if subids else 0))

    def window(self, sessions=None, defaults=None, from_=None, msg=None, upgrade_qos: bool = False,
               nl_all: bool = False, subids: bool = False):
        """The session's send window (tm_batch_window): deliver() of the same
        options, then every delivery's disposition and packet id.  sessions:
        iterable of dicts {subscriber, next_pkt_id, flags, inflight_free,
        mqueue_len, mqueue_max} (missing keys as in defaults), ascending by
        subscriber; defaults: one such dict for subscribers not listed
        (missing: next_pkt_id 1, connected, unbounded window, empty unbounded
        queue) -> (deliver()'s 6-tuple, disp u8[D'], packet_ids u16[D'],
        records u32[R', 4] = next_pkt_id / n_inflight / n_queued /
        n_dropped_old); window_info holds totals[TM_DISP_*], kernel_ms,
        deliver_kernel_ms and n_dropped_no_local."""
        w, _keep = self._window(sessions, defaults, from_, msg, self._deliver_flags(upgrade_qos, nl_all, subids), 0)
        d = w.inboxes
        r, t = int(d.n_subscribers), int(d.n_deliveries)
        cp = lambda p, k, ty=np.uint32: (np.ctypeslib.as_array(p, shape=(k,)).copy() if k  # noqa: E731
                                         else np.zeros(0, ty))
        self._window_info(w)
        rec = (np.ctypeslib.as_array(C.cast(w.records, C.POINTER(C.c_uint32)), shape=(r, 4)).copy() if r
               else np.zeros((0, 4), np.uint32))
        return ((cp(d.subscribers, r), cp(d.inbox_offsets, r + 1), cp(d.publishes, t), cp(d.filter_ids, t),
                 cp(d.msg, t, np.uint8), cp(d.subids, t) if subids else None),
                cp(w.disp, t, np.uint8), cp(w.packet_ids, t, np.uint16), rec)

    def window_device(self, sessions=None, defaults=None, from_=None, msg=None, upgrade_qos: bool = False,
                      nl_all: bool = False, subids: bool = False):
        """TM_WINDOW_DEVICE: -> (n_subscribers, n_deliveries, device ptrs
        subscribers / offsets / publishes / filter_ids / msg / subids (None
        without subids) / disp / packet_ids / records); window_info as window()."""
        w, _keep = self._window(sessions, defaults, from_, msg, self._deliver_flags(upgrade_qos, nl_all, subids),
                                N.TM_WINDOW_DEVICE)
        d = w.inboxes
        ptr = lambda p: C.cast(p, C.c_void_p).value  # noqa: E731
        self._window_info(w)
        return (int(d.n_subscribers), int(d.n_deliveries), ptr(d.subscribers), ptr(d.inbox_offsets),
                ptr(d.publishes), ptr(d.filter_ids), ptr(d.msg), ptr(d.subids) if subids else None,
                ptr(w.disp), ptr(w.packet_ids), ptr(w.records))

    def _window_info(self, w):
        self.window_info = {"totals": [int(x) for x in w.totals], "kernel_ms": float(w.kernel_ms),
                            "deliver_kernel_ms": float(w.inboxes.kernel_ms),
                            "n_dropped_no_local": int(w.inboxes.n_dropped_no_local)}

    SESSION_DEFAULTS = {"subscriber": 0, "next_pkt_id": 1, "flags": 0, "inflight_free": N.TM_SESS_UNBOUNDED,
                        "mqueue_len": 0, "mqueue_max": 0}

    @classmethod
    def _session(cls, s, base) -> "N.SessionState":
        vals = dict(base)
        unknown = set(s or {}) - set(cls.SESSION_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown session fields {sorted(unknown)}")
        vals.update({k: int(v) for k, v in (s or {}).items()})
        for k, v in vals.items():   # ctypes would wrap a value past the field's width before the C range check
            if not 0 <= v <= 0xFFFFFFFF:
                raise ValueError(f"session field {k} = {v} out of range")
        return N.SessionState(**vals)

    def window_prio(self, sessions=None, defaults=None, tables=(), prio=None, default_table=None, from_=None, msg=None,
                    upgrade_qos: bool = False, nl_all: bool = False, subids: bool = False):
        """window() over mqueues with priority tables (tm_batch_window_prio).
        tables: PTable handles (Engine.ptable); prio: iterable of dicts
        {subscriber, table (index into tables, None = no table), plen (messages
        per class in the queue now, at most 8)} ascending by subscriber, each
        also listed in sessions; default_table: the table index of subscribers
        not in prio (None = no table) -> window()'s tuple plus pclass u8[D']
        (TM_PRIO_NOCLASS without a table) and precords u32[R', 8, 2] =
        n_queued / n_dropped_old per class; window_info also holds
        lookup_kernel_ms."""
        w, pw, _keep = self._window_prio(sessions, defaults, tables, prio, default_table, from_, msg,
                                         self._deliver_flags(upgrade_qos, nl_all, subids), 0)
        d = w.inboxes
        r, t = int(d.n_subscribers), int(d.n_deliveries)
        cp = lambda p, k, ty=np.uint32: (np.ctypeslib.as_array(p, shape=(k,)).copy() if k  # noqa: E731
                                         else np.zeros(0, ty))
        rec = (np.ctypeslib.as_array(C.cast(w.records, C.POINTER(C.c_uint32)), shape=(r, 4)).copy() if r
               else np.zeros((0, 4), np.uint32))
        prec = (np.ctypeslib.as_array(C.cast(pw.precords, C.POINTER(C.c_uint32)),
                                      shape=(r, N.TM_PRIO_MAX_CLASSES, 2)).copy() if r
                else np.zeros((0, N.TM_PRIO_MAX_CLASSES, 2), np.uint32))
        return ((cp(d.subscribers, r), cp(d.inbox_offsets, r + 1), cp(d.publishes, t), cp(d.filter_ids, t),
                 cp(d.msg, t, np.uint8), cp(d.subids, t) if subids else None),
                cp(w.disp, t, np.uint8), cp(w.packet_ids, t, np.uint16), rec, cp(pw.pclass, t, np.uint8), prec)

    def window_prio_device(self, sessions=None, defaults=None, tables=(), prio=None, default_table=None, from_=None,
                           msg=None, upgrade_qos: bool = False, nl_all: bool = False, subids: bool = False):
        """TM_WINDOW_DEVICE: window_device()'s tuple plus the device pointers
        of pclass and precords; window_info as window_prio()."""
        w, pw, _keep = self._window_prio(sessions, defaults, tables, prio, default_table, from_, msg,
                                         self._deliver_flags(upgrade_qos, nl_all, subids), N.TM_WINDOW_DEVICE)
        d = w.inboxes
        ptr = lambda p: C.cast(p, C.c_void_p).value  # noqa: E731
        return (int(d.n_subscribers), int(d.n_deliveries), ptr(d.subscribers), ptr(d.inbox_offsets),
                ptr(d.publishes), ptr(d.filter_ids), ptr(d.msg), ptr(d.subids) if subids else None,
                ptr(w.disp), ptr(w.packet_ids), ptr(w.records), ptr(pw.pclass), ptr(pw.precords))

    def _window_prio(self, sessions, defaults, tables, prio, default_table, from_, msg, dflags: int, wflags: int):
        o, keep = self._deliver_opts(from_, msg, dflags)
        wo = self._window_opts(sessions, defaults, wflags, keep)
        po = N.WindowPrioOpts()
        tables = list(tables or ())
        po.n_tables = len(tables)
        if tables:
            arr = (C.c_void_p * len(tables))(*[t.h.value for t in tables])
            keep.append(arr)
            po.tables = C.cast(arr, C.POINTER(C.c_void_p))
        idx = lambda t: N.TM_NONE if t is None else int(t)  # noqa: E731
        po.default_table = idx(default_table)
        ents = []
        for e in (prio or []):
            plen = [int(x) for x in e.get("plen", ())]
            if len(plen) > N.TM_PRIO_MAX_CLASSES or any(not 0 <= x <= 0xFFFFFFFF for x in plen):
                raise ValueError(f"plen of subscriber {e['subscriber']}: at most {N.TM_PRIO_MAX_CLASSES} u32 counts")
            plen += [0] * (N.TM_PRIO_MAX_CLASSES - len(plen))
            ents.append(N.SessionPrio(int(e["subscriber"]), idx(e.get("table")), (C.c_uint32 * N.TM_PRIO_MAX_CLASSES)(*plen)))
        po.n_prio = len(ents)
        if ents:
            arr = (N.SessionPrio * len(ents))(*ents)
            keep.append(arr)
            po.prio = C.cast(arr, C.POINTER(N.SessionPrio))
        w, pw = N.SessionWindow(), N.WindowPrio()
        N.check(self.eng.L.tm_batch_window_prio(self.eng.h, self.h, C.byref(o), C.byref(wo), C.byref(po), C.byref(w),
                                                C.byref(pw)), "tm_batch_window_prio")
        self._last_deliveries = int(w.inboxes.n_deliveries)
        self._window_info(w)
        self.window_info["lookup_kernel_ms"] = float(pw.lookup_kernel_ms)
        return w, pw, keep

    def _window(self, sessions, defaults, from_, msg, dflags: int, wflags: int):
        o, keep = self._deliver_opts(from_, msg, dflags)
        wo = self._window_opts(sessions, defaults, wflags, keep)
        w = N.SessionWindow()
        N.check(self.eng.L.tm_batch_window(self.eng.h, self.h, C.byref(o), C.byref(wo), C.byref(w)), "tm_batch_window")
        self._last_deliveries = int(w.inboxes.n_deliveries)
        return w, keep

    def _window_opts(self, sessions, defaults, wflags: int, keep):
        wo = N.WindowOpts()
        wo.flags = wflags
        wo.defaults = self._session(defaults, self.SESSION_DEFAULTS)
        base = {k: int(getattr(wo.defaults, k)) for k in self.SESSION_DEFAULTS}
        if isinstance(sessions, np.ndarray):   # u32[n, 6], the struct's words
            tab = np.ascontiguousarray(sessions, dtype=np.uint32).reshape(-1, 6)
            wo.n_sessions = len(tab)
            if len(tab):
                keep.append(tab)
                wo.sessions = C.cast(tab.ctypes.data, C.POINTER(N.SessionState))
        else:
            ss = [self._session(s, base) for s in (sessions or [])]
            wo.n_sessions = len(ss)
            if ss:
                arr = (N.SessionState * len(ss))(*ss)
                keep.append(arr)
                wo.sessions = C.cast(arr, C.POINTER(N.SessionState))
        return wo

    def _deliver(self, from_, msg, flags: int):
        o, keep = self._deliver_opts(from_, msg, flags)
        d = N.SessionInboxes()
        N.check(self.eng.L.tm_batch_deliver(self.eng.h, self.h, C.byref(o), C.byref(d)), "tm_batch_deliver")
        self._last_deliveries = int(d.n_deliveries)
        return d, keep

    def _deliver_opts(self, from_, msg, flags: int):
        o = N.DeliverOpts()
        o.flags = flags
        keep = []
        for name, val, ty in (("from_", from_, np.uint32), ("msg", msg, np.uint8)):
            if val is None:
                continue
            a = np.ascontiguousarray(np.asarray(val, dtype=ty))
            if len(a) != self.n:
                raise ValueError(f"{len(a)} {name.rstrip('_')} entries for {self.n} publishes")
            if not len(a):
                a = np.zeros(1, ty)
            keep.append(a)
            setattr(o, name, a.ctypes.data)
        return o, keep

    def _inboxes(self, flags: int) -> "N.Inboxes":
        d = N.Inboxes()
        N.check(self.eng.L.tm_batch_inboxes(self.eng.h, self.h, flags, C.byref(d)), "tm_batch_inboxes")
        self._last_deliveries = int(d.n_deliveries)
        return d

    def _shared_opts(self, strategy, keys, seed: int, flags: int):
        o = N.SharedOpts()
        o.strategy = N.SHARED_STRATEGIES.get(strategy, strategy) if isinstance(strategy, str) else int(strategy)
        o.flags = flags
        o.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        keep = []
        if keys is not None:
            k = np.ascontiguousarray(np.asarray(keys, dtype=np.uint32))
            if len(k) != self.n:
                raise ValueError(f"{len(k)} keys for {self.n} publishes")
            if not len(k):
                k = np.zeros(1, np.uint32)
            o.keys = k.ctypes.data
            keep.append(k)
        return o, keep

    def _dispatch_shared(self, strategy, keys, seed: int, flags: int) -> "N.SharedDeliveries":
        o, _keep = self._shared_opts(strategy, keys, seed, flags)
        d = N.SharedDeliveries()
        N.check(self.eng.L.tm_batch_dispatch_shared(self.eng.h, self.h, C.byref(o), C.byref(d)),
                "tm_batch_dispatch_shared")
        return d

    def _dispatch(self, flags: int) -> "N.Deliveries":
        d = N.Deliveries()
        N.check(self.eng.L.tm_batch_dispatch(self.eng.h, self.h, flags, C.byref(d)), "tm_batch_dispatch")
        return d

    def stats(self) -> dict:
        st = N.BatchStats()
        N.check(self.eng.L.tm_batch_stats_get(self.eng.h, self.h, C.byref(st)), "tm_batch_stats_get")
        return st.asdict()

    def device_csr(self):
        row, ids, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        N.check(self.eng.L.tm_batch_device_csr(self.eng.h, self.h, C.byref(row), C.byref(ids), C.byref(n)),
                "tm_batch_device_csr")
        return row.value, ids.value, n.value

    def device_rows(self):
        """Device pointers of the result as the walk left it (tm_batch_rows):
        (count u32[n], start u64[n], ids u32[...], n_matches); no CSR pass."""
        cnt, start, ids, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        N.check(self.eng.L.tm_batch_rows(self.eng.h, self.h, C.byref(cnt), C.byref(start), C.byref(ids),
                                         C.byref(n)), "tm_batch_rows")
        return cnt.value, start.value, ids.value, n.value

    def publish_rows_device(self):
        """tm_batch_publish_rows: device pointers of every PUBLISH's row
        (count u32[publishes], start u64[publishes], ids) and the delivered
        (publish, filter) matches; for a device-deduplicated batch the rows
        expanded behind the walk."""
        cnt, start, ids, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        N.check(self.eng.L.tm_batch_publish_rows(self.eng.h, self.h, C.byref(cnt), C.byref(start), C.byref(ids),
                                                 C.byref(n)), "tm_batch_publish_rows")
        return cnt.value, start.value, ids.value, n.value

    def rows(self, n_rows: int):
        """Host copy of the walk's rows (tm_batch_rows + hipMemcpy, for tests):
        (count u32[n_rows], start u64[n_rows], staging u32[max end])."""
        cnt, start, ids, _ = self.device_rows()
        c = np.zeros(n_rows, np.uint32)
        s = np.zeros(n_rows, np.uint64)
        _d2h(c, cnt)
        _d2h(s, start)
        end = int((s + c).max()) if n_rows else 0
        stg = np.zeros(max(end, 1), np.uint32)
        if end:
            _d2h(stg, ids)
        return c, s, stg[:end]

    def free(self):
        if self.h:
            self.eng.L.tm_batch_free(self.eng.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


_hip = None


def _d2h(dst: np.ndarray, src_ptr: int):
    """hipMemcpy device -> host through the HIP runtime the engine already
    loaded (same soname, so the same copy): test/diagnostic use only."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so.7")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    if dst.nbytes:
        rc = _hip.hipMemcpy(dst.ctypes.data, src_ptr, dst.nbytes, 2)   # hipMemcpyDeviceToHost
        if rc:
            raise RuntimeError(f"hipMemcpy D2H failed: {rc}")


def _result_arrays(r: N.Result):
    n = r.n_topics
    offs = np.ctypeslib.as_array(r.row_offsets, shape=(n + 1,)).copy()
    m = int(r.n_matches)
    ids = np.ctypeslib.as_array(r.filter_ids, shape=(max(m, 1),))[:m].copy() if m else np.zeros(0, np.uint32)
    return offs, ids


def _routes_arrays(r: N.Routes):
    n, m = r.n_topics, int(r.n_routes)
    offs = np.ctypeslib.as_array(r.row_offsets, shape=(n + 1,)).copy()
    if not m:
        return offs, np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    fids = np.ctypeslib.as_array(r.filter_ids, shape=(m,)).copy()
    dests = np.ctypeslib.as_array(r.dests, shape=(m,)).copy()
    return offs, fids, dests


def _invalidate(owner):
    """Borrowed Engine views of an owner that is being closed lose their handle."""
    for e in list(getattr(owner, "_borrowed", ())):
        e._h = None


class GroupBatch:
    """A publish batch split over a Group's replicas (tm_group_prepare ...)."""

    def __init__(self, grp: "Group", topics):
        self.grp = grp
        s = _pack(topics)
        self.n = len(s)
        self._buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        self._offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        h = C.c_void_p()
        N.check(grp.L.tm_group_prepare(grp.h, self._buf.ctypes.data, self._offs.ctypes.data, self.n, C.byref(h)),
                "tm_group_prepare")
        self.h = h

    def launch(self):
        N.check(self.grp.L.tm_group_launch(self.grp.h, self.h), "tm_group_launch")
        return self

    def wait(self):
        N.check(self.grp.L.tm_group_wait(self.grp.h, self.h), "tm_group_wait")
        return self

    def result(self):
        r = N.Result()
        N.check(self.grp.L.tm_group_result(self.grp.h, self.h, C.byref(r)), "tm_group_result")
        return _result_arrays(r)

    def sample(self, publishes):
        """tm_group_sample: the rows of `publishes` (indices into the whole
        batch), each gathered on its slice's device -> (offsets u32[k+1], ids)."""
        idx = np.ascontiguousarray(np.asarray(publishes, dtype=np.uint32))
        r = N.Result()
        N.check(self.grp.L.tm_group_sample(self.grp.h, self.h, idx.ctypes.data, len(idx), C.byref(r)),
                "tm_group_sample")
        return _result_arrays(r)

    def dispatch(self):
        """tm_group_dispatch -> (row_offsets u64[n+1], subscribers u32[deliveries])."""
        d = N.Deliveries()
        N.check(self.grp.L.tm_group_dispatch(self.grp.h, self.h, C.byref(d)), "tm_group_dispatch")
        n, t = d.n_topics, int(d.n_deliveries)
        offs = np.ctypeslib.as_array(d.row_offsets, shape=(n + 1,)).copy()
        subs = np.ctypeslib.as_array(d.subscribers, shape=(t,)).copy() if t else np.zeros(0, np.uint32)
        return offs, subs

    def stats(self) -> dict:
        st = N.BatchStats()
        N.check(self.grp.L.tm_group_batch_stats(self.grp.h, self.h, C.byref(st)), "tm_group_batch_stats")
        return st.asdict()

    def free(self):
        if self.h:
            self.grp.L.tm_group_batch_free(self.grp.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Group:
    """Replicated multi-device matching in one process (tm_group_*, config C3):
    a view of one replicated engine -- one host trie, one HBM replica per
    listed device, a mutation made once and uploaded to every replica, batches
    split into one contiguous slice per replica."""

    def __init__(self, devices, host_threads: int = 0):
        self.L = N.lib()
        devs = (C.c_int32 * len(devices))(*devices)
        cfg = N.Config(0, 0, host_threads, 0)
        h = C.c_void_p()
        N.check(self.L.tm_group_create(devs, len(devices), C.byref(cfg), C.byref(h)), "tm_group_create")
        self.h = h
        self.devices = list(devices)
        self._borrowed = weakref.WeakSet()

    def close(self):
        if getattr(self, "h", None):
            _invalidate(self)
            self.L.tm_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self.L.tm_group_size(self.h))

    def insert(self, f: bytes):
        N.check(self.L.tm_group_trie_insert(self.h, f, len(f)), "tm_group_trie_insert")

    def delete(self, f: bytes):
        N.check(self.L.tm_group_trie_delete(self.h, f, len(f)), "tm_group_trie_delete")

    def insert_many(self, filters) -> int:
        s = _pack(filters)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        done = C.c_uint64()
        N.check(self.L.tm_group_insert_many(self.h, buf.ctypes.data, offs.ctypes.data, len(s), C.byref(done)),
                "tm_group_insert_many")
        return int(done.value)

    def route_apply(self, events) -> int:
        s = _pack([t for _, t, _ in events])
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        dests = np.ascontiguousarray(np.array([d for _, _, d in events] or [0], np.uint32))
        ops = np.ascontiguousarray(np.array([o for o, _, _ in events] or [0], np.uint8))
        done = C.c_uint64()
        N.check(self.L.tm_group_route_apply(self.h, buf.ctypes.data, offs.ctypes.data, dests.ctypes.data,
                                            ops.ctypes.data, len(events), C.byref(done)), "tm_group_route_apply")
        return int(done.value)

    def sync(self):
        N.check(self.L.tm_group_sync(self.h), "tm_group_sync")

    def prepare(self, topics) -> GroupBatch:
        return GroupBatch(self, topics)

    def engine(self) -> "Engine":
        """The group's engine (every tm_* call on it spans the replicas); the
        Group keeps ownership."""
        return Engine._borrow(self.L.tm_group_engine(self.h, 0), self.devices, owner=self)

    def match_batch(self, topics):
        s = _pack(topics)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        r = N.Result()
        N.check(self.L.tm_group_match_batch(self.h, buf.ctypes.data, offs.ctypes.data, len(s), C.byref(r)),
                "tm_group_match_batch")
        return _result_arrays(r)

    def filter_bytes(self, fid: int, replica: int = 0) -> bytes:
        e = self.L.tm_group_engine(self.h, replica)
        n = C.c_size_t()
        p = self.L.tm_filter_bytes(e, fid, C.byref(n))
        if not p:
            raise KeyError(fid)
        return C.string_at(p, n.value)


def _acl_check(L, rc, what):
    if rc == N.TM_EINVAL:   # the ACL calls say which rule / request was refused
        raise N.TmError(rc, what + " [" + (L.tm_last_error() or b"").decode(errors="replace") + "]")
    return N.check(rc, what)


class Acl:
    """A compiled, immutable rule set on the engine's devices (tm_acl)."""

    def __init__(self, engine: "Engine", h, n_rules: int):
        self.engine, self._h, self.n_rules = engine, h, n_rules

    @property
    def h(self):
        if self._h is None:
            raise RuntimeError("rule set is closed (or its engine was)")
        return self._h

    @property
    def kernel_ms(self) -> float:
        """Device time of the last acl_check's kernel."""
        return float(self.engine.L.tm_acl_kernel_ms(self.engine.h, self.h))

    def close(self):
        if self._h is not None:
            self.engine.L.tm_acl_free(self.engine.h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PTable:
    """A priority table of an mqueue (tm_ptable)."""

    def __init__(self, engine: "Engine", h):
        self.engine, self._h = engine, h
        out = (C.c_uint16 * N.TM_PRIO_MAX_CLASSES)()
        k = engine.L.tm_ptable_classes(h, out)
        self.classes = ["infinity" if out[i] == N.TM_PRIO_INFINITY else int(out[i]) for i in range(k)]

    @property
    def h(self):
        if self._h is None:
            raise RuntimeError("priority table is freed (or its engine was closed)")
        return self._h

    def free(self):
        if self._h is not None:
            self.engine.L.tm_ptable_free(self.engine.h, self._h)
            self._h = None

    close = free

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    def __init__(self, device: int = 0, init_slots: int = 0, host_threads: int = 0, frozen_dict: bool = False,
                 host_tokenize: bool = False, devices=None):
        self.L = N.lib()
        flags = (N.TM_CFG_FROZEN_DICT if frozen_dict else 0) | (N.TM_CFG_HOST_TOKENIZE if host_tokenize else 0)
        cfg = N.Config(device, init_slots, host_threads, flags)
        h = C.c_void_p()
        self._owned = True
        if devices is None:
            N.check(self.L.tm_create(C.byref(cfg), C.byref(h)), "tm_create")
            self.devices = [device] if device >= 0 else []
        else:
            devs = (C.c_int32 * max(len(devices), 1))(*devices)
            N.check(self.L.tm_create_replicated(C.byref(cfg), devs, len(devices), C.byref(h)), "tm_create_replicated")
            self.devices = list(devices)
        self._h = h
        self.device = self.devices[0] if self.devices else -1

    @classmethod
    def _borrow(cls, handle, devices, owner=None) -> "Engine":
        """A view of an engine another object owns: it keeps the owner alive,
        and the owner's close() invalidates it (calls then raise instead of
        reaching freed native memory)."""
        if not handle:
            raise ValueError("no such engine")
        e = cls.__new__(cls)
        e.L, e._h, e._owned = N.lib(), C.c_void_p(handle), False
        e.devices, e.device = list(devices), devices[0]
        e._owner = owner
        if owner is not None:
            owner._borrowed.add(e)
        return e

    @property
    def h(self):
        h = getattr(self, "_h", None)
        if h is None:
            raise RuntimeError("engine is closed (or its owner was)")
        return h

    @property
    def replicas(self) -> int:
        return int(self.L.tm_replica_count(self.h))

    def async_start(self):
        N.check(self.L.tm_async_start(self.h), "tm_async_start")

    def close(self):
        if getattr(self, "_h", None):
            for a in list(getattr(self, "_acls", ())):   # rule sets hold device memory of this engine
                a.close()
            if getattr(self, "_owned", True):
                self.L.tm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- emqx_trie ---------------------------------------------------------
    def insert(self, f: bytes):
        N.check(self.L.tm_trie_insert(self.h, f, len(f)), "tm_trie_insert")

    def delete(self, f: bytes):
        N.check(self.L.tm_trie_delete(self.h, f, len(f)), "tm_trie_delete")

    def lookup(self, node_id):
        """-> None or (edge_count, topic_bytes_or_None)"""
        out = N.TrieNode()
        is_root = node_id is None
        nid = b"" if is_root else node_id
        rc = N.check(self.L.tm_trie_lookup(self.h, nid, len(nid), int(is_root), C.byref(out)), "tm_trie_lookup")
        if rc == 0:
            return None
        return out.edge_count, (self.filter_bytes(out.filter_id) if out.has_topic else None)

    def empty(self) -> bool:
        return bool(self.L.tm_trie_empty(self.h))

    def match_ids(self, topic: bytes):
        cap = 1024
        while True:
            ids = (C.c_uint32 * cap)()
            n = C.c_uint32()
            N.check(self.L.tm_trie_match(self.h, topic, len(topic), ids, cap, C.byref(n)), "tm_trie_match")
            if n.value <= cap:
                return list(ids[:n.value])
            cap = n.value

    def match(self, topic: bytes):
        return [self.filter_bytes(i) for i in self.match_ids(topic)]

    def match_coalesced(self, topic: bytes):
        """emqx_trie:match/1 ids through tm_match_coalesced: concurrent callers
        (threads; ctypes drops the GIL) share device batches."""
        cap = 1024
        while True:
            ids = (C.c_uint32 * cap)()
            n = C.c_uint32()
            N.check(self.L.tm_match_coalesced(self.h, topic, len(topic), ids, cap, C.byref(n)), "tm_match_coalesced")
            if n.value <= cap:
                return list(ids[:n.value])
            cap = n.value

    def match_async(self, topic: bytes, done):
        """tm_match_async: done(rc, ids list) runs on the engine's completion
        thread.  The ctypes callback object is kept alive until it has run."""
        keep = getattr(self, "_async_keep", None)
        if keep is None:
            keep = self._async_keep = {}

        def cb(ctx, rc, ids, n, _key=[None]):
            try:
                done(rc, [ids[i] for i in range(n)] if rc == 0 else None)
            finally:
                keep.pop(_key[0], None)
        c = N.MATCH_CB(cb)
        key = id(c)
        cb.__defaults__[0][0] = key
        keep[key] = c
        rc = self.L.tm_match_async(self.h, topic, len(topic), c, None)
        if rc:
            keep.pop(key, None)
        N.check(rc, "tm_match_async")

    def async_stats(self) -> dict:
        st = N.AsyncStats()
        N.check(self.L.tm_async_stats_get(self.h, C.byref(st)), "tm_async_stats_get")
        return st.asdict()

    def coalesce_config(self, max_batch: int = 0, linger_us: int = N.TM_NONE):
        """-> (batches, requests) served by tm_match_coalesced so far."""
        b, r = C.c_uint64(), C.c_uint64()
        N.check(self.L.tm_coalesce_config(self.h, max_batch, linger_us, C.byref(b), C.byref(r)), "tm_coalesce_config")
        return int(b.value), int(r.value)

    # ---- batches -----------------------------------------------------------
    def match_batch(self, topics):
        """-> (row_offsets uint32[n+1], filter_ids uint32[total]); rows sorted by filter bytes."""
        s = _pack(topics)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        r = N.Result()
        N.check(self.L.tm_match_batch(self.h, buf.ctypes.data, offs.ctypes.data, len(s), C.byref(r)),
                "tm_match_batch")
        return _result_arrays(r)

    def match_batch_packed(self, topics):
        """tm_match_batch_packed -> (row_offsets uint32[n+1], packed ids uint8[total * id_bytes],
        id_bytes); id j = ids[j*id_bytes ...] little-endian."""
        s = _pack(topics)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        r = N.ResultPacked()
        N.check(self.L.tm_match_batch_packed(self.h, buf.ctypes.data, offs.ctypes.data, len(s), C.byref(r)),
                "tm_match_batch_packed")
        n, m, ib = r.n_topics, int(r.n_matches), int(r.id_bytes)
        ro = np.ctypeslib.as_array(r.row_offsets, shape=(n + 1,)).copy()
        ids = np.ctypeslib.as_array(r.ids, shape=(max(m * ib, 1),))[:m * ib].copy() if m else np.zeros(0, np.uint8)
        return ro, ids, ib

    def filters_copy_packed(self, ids, id_bytes: int) -> list:
        """tm_filters_copy_packed over packed ids: [(index, filter bytes)]."""
        a = np.ascontiguousarray(ids, dtype=np.uint8)
        n = len(a) // id_bytes
        offs = np.zeros(n + 1, np.uint64)
        keep = np.zeros(max(n, 1), np.uint32)
        k, need = C.c_uint32(), C.c_uint64()
        cap = 64 * max(n, 1)
        while True:
            buf = np.zeros(max(cap, 1), np.uint8)
            N.check(self.L.tm_filters_copy_packed(self.h, a.ctypes.data if n else None, id_bytes, n, buf.ctypes.data,
                                                  cap, offs.ctypes.data, keep.ctypes.data, C.byref(k),
                                                  C.byref(need)), "tm_filters_copy_packed")
            if need.value <= cap:
                break
            cap = need.value
        raw = buf.tobytes()
        return [(int(keep[j]), raw[int(offs[j]):int(offs[j + 1])]) for j in range(k.value)]

    def prepare(self, topics, dedup: bool = False, stream: bool = False, replica=None) -> Batch:
        """Device-resident batch; dedup=True matches identical topics once (TM_BATCH_DEDUP);
        stream=True gives it a HIP stream of its own, so launches of several
        batches overlap on the device (TM_BATCH_STREAM); replica = the device
        replica it runs on (default: the next one, round-robin)."""
        return Batch(self, topics, dedup=dedup, stream=stream, replica=replica)

    # ---- routes (emqx_router + emqx_broker:aggre/1) -------------------------
    def route_add(self, topic: bytes, dest: int):
        N.check(self.L.tm_route_add(self.h, topic, len(topic), dest), "tm_route_add")

    def route_delete(self, topic: bytes, dest: int) -> bool:
        rc = self.L.tm_route_delete(self.h, topic, len(topic), dest)
        if rc == N.TM_ENOENT:
            return False
        N.check(rc, "tm_route_delete")
        return True

    def route_apply(self, events) -> int:
        """tm_route_apply: [(op, topic, dest)] in order, op 1 = write (add), 0 =
        delete_object (absent = no-op).  Returns how many changed the table."""
        n = len(events)
        s = _pack([t for _, t, _ in events])
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        dests = np.ascontiguousarray(np.array([d for _, _, d in events] or [0], np.uint32))
        ops = np.ascontiguousarray(np.array([o for o, _, _ in events] or [0], np.uint8))
        done = C.c_uint64()
        N.check(self.L.tm_route_apply(self.h, buf.ctypes.data, offs.ctypes.data, dests.ctypes.data,
                                      ops.ctypes.data, n, C.byref(done)), "tm_route_apply")
        return int(done.value)

    # ---- subscribers (emqx_broker subscribe/unsubscribe/subscriber_down) ------
    def subscribe(self, topic: bytes, sub: int, node_dest: int = 0):
        N.check(self.L.tm_subscribe(self.h, topic, len(topic), sub, node_dest), "tm_subscribe")

    # ---- the ?SUBOPTION table (emqx_broker subscribe/3, set_subopts/2, get_subopts/2) --
    @staticmethod
    def _subopts(opts) -> "N.SubOpts":
        opts = opts or {}
        unknown = set(opts) - set(N.SUBOPT_MASKS)
        if unknown:
            raise ValueError(f"unknown subscription options {sorted(unknown)}")
        vals = {k: int(v) for k, v in opts.items()}
        for k, v in vals.items():   # ctypes would wrap a value past the field's width before the C range check
            if not 0 <= v <= (N.TM_SUBID_MAX if k == "subid" else 255):
                raise ValueError(f"subscription option {k} = {v} out of range")
        return N.SubOpts(**vals)

    def subscribe_opts(self, topic: bytes, sub: int, opts=None, node_dest: int = 0):
        """subscribe/3: opts = {qos, nl, rap, rh, subid} (missing = default;
        None = all defaults).  An existing subscription merges: the four flags
        are replaced, the subid only when non-zero."""
        o = self._subopts(opts)
        N.check(self.L.tm_subscribe_opts(self.h, topic, len(topic), sub, node_dest, C.byref(o) if opts is not None
                                         else None), "tm_subscribe_opts")

    def set_subopts(self, topic: bytes, sub: int, opts: dict) -> bool:
        """set_subopts/2 for a partial map: only the keys of opts change.
        False when not subscribed."""
        o = self._subopts(opts)
        mask = 0
        for k in opts:
            mask |= N.SUBOPT_MASKS[k]
        rc = self.L.tm_set_subopts(self.h, topic, len(topic), sub, mask, C.byref(o))
        if rc == N.TM_ENOENT:
            return False
        N.check(rc, "tm_set_subopts")
        return True

    def get_subopts(self, topic: bytes, sub: int):
        """get_subopts/2: {qos, nl, rap, rh, subid}, or None when not subscribed."""
        o = N.SubOpts()
        rc = self.L.tm_get_subopts(self.h, topic, len(topic), sub, C.byref(o))
        if rc == N.TM_ENOENT:
            return None
        N.check(rc, "tm_get_subopts")
        return o.asdict()

    def unsubscribe(self, topic: bytes, sub: int, node_dest: int = 0) -> bool:
        rc = self.L.tm_unsubscribe(self.h, topic, len(topic), sub, node_dest)
        if rc == N.TM_ENOENT:
            return False
        N.check(rc, "tm_unsubscribe")
        return True

    def subscriber_down(self, sub: int, node_dest: int = 0) -> int:
        n = C.c_uint64()
        N.check(self.L.tm_subscriber_down(self.h, sub, node_dest, C.byref(n)), "tm_subscriber_down")
        return n.value

    # ---- shared subscriptions (emqx_shared_sub subscribe/unsubscribe/cleanup_down) --
    def shared_subscribe(self, topic: bytes, group_dest: int, sub: int):
        N.check(self.L.tm_shared_subscribe(self.h, topic, len(topic), group_dest, sub), "tm_shared_subscribe")

    def shared_subscribe_opts(self, topic: bytes, group_dest: int, sub: int, opts=None):
        """subscribe/3 with share => Group (tm_shared_subscribe_opts): the
        options go under (sub, topic), owned by the membership.  If (sub,
        topic) has options already, of either kind, only they merge and no
        membership changes."""
        o = self._subopts(opts)
        N.check(self.L.tm_shared_subscribe_opts(self.h, topic, len(topic), group_dest, sub,
                                                C.byref(o) if opts is not None else None), "tm_shared_subscribe_opts")

    def shared_unsubscribe(self, topic: bytes, group_dest: int, sub: int) -> bool:
        rc = self.L.tm_shared_unsubscribe(self.h, topic, len(topic), group_dest, sub)
        if rc == N.TM_ENOENT:
            return False
        N.check(rc, "tm_shared_unsubscribe")
        return True

    def shared_member_down(self, sub: int) -> int:
        n = C.c_uint64()
        N.check(self.L.tm_shared_member_down(self.h, sub, C.byref(n)), "tm_shared_member_down")
        return n.value

    def shared_members(self, topic: bytes, group_dest: int) -> list:
        """subscribers/2: the members of (group, topic) in insertion order."""
        n = C.c_uint32()
        buf = np.zeros(64, np.uint32)
        while True:
            N.check(self.L.tm_shared_members(self.h, topic, len(topic), group_dest, buf.ctypes.data, len(buf),
                                             C.byref(n)), "tm_shared_members")
            if n.value <= len(buf):
                return buf[:n.value].tolist()
            buf = np.zeros(n.value, np.uint32)

    def match_routes_batch(self, topics):
        """-> (row_offsets, filter_ids, dests): aggre(match_routes(T)) per topic."""
        s = _pack(topics)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        r = N.Routes()
        N.check(self.L.tm_match_routes_batch(self.h, buf.ctypes.data, offs.ctypes.data, len(s), C.byref(r)),
                "tm_match_routes_batch")
        return _routes_arrays(r)

    # ---- batched emqx_topic:match/2 (ACL / rewrite / tracer rules) -----------
    def rules_match(self, names, rules, dollar_rule: bool = True) -> np.ndarray:
        """-> bool[n, r]: emqx_topic:match(names[i], rules[j]) computed on the device
        (dollar_rule: the binary form's '$' rule; False = word-list form, as ACL)."""
        sn, sr = _pack(names), _pack(rules)
        n, r = len(sn), len(sr)
        if not n or not r:
            return np.zeros((n, r), bool)
        nb = np.ascontiguousarray(sn.buf if sn.buf.size else np.zeros(1, np.uint8))
        no = np.ascontiguousarray(sn.offs, dtype=np.uint64)
        rb = np.ascontiguousarray(sr.buf if sr.buf.size else np.zeros(1, np.uint8))
        ro = np.ascontiguousarray(sr.offs, dtype=np.uint64)
        wpr = (r + 31) // 32
        bits = np.zeros(n * wpr, np.uint32)
        N.check(self.L.tm_rules_match(self.h, nb.ctypes.data, no.ctypes.data, n, rb.ctypes.data, ro.ctypes.data, r,
                                      int(dollar_rule), bits.ctypes.data), "tm_rules_match")
        b = np.unpackbits(bits.view(np.uint8).reshape(n, wpr * 4), axis=1, bitorder="little")
        return b[:, :r].astype(bool)

    # ---- mqueue priority tables ------------------------------------------------
    def ptable(self, entries, default="lowest") -> "PTable":
        """A priority table (tm_ptable_create; #mqueue.p_table and default_p,
        src/emqx_mqueue.erl:94-116): entries {topic bytes: 0..255 or
        "infinity"}, default "lowest" | "highest" | int -> a handle with
        .classes (the priorities highest first, "infinity" for infinity) and
        .free().  Works on a host-only engine."""
        enc = lambda p: N.TM_PRIO_INFINITY if p == "infinity" else int(p)  # noqa: E731
        dflt = 0 if default == "lowest" else N.TM_PRIO_INFINITY if default in ("highest", "infinity") else int(default)
        keys = list(entries)
        pr = [enc(entries[k]) for k in keys]
        if not (0 <= dflt <= 0xFFFFFFFF) or any(not 0 <= p <= 0xFFFF for p in pr):   # (ctypes would wrap them)
            raise ValueError("priority out of range")
        s = _pack(keys)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        prio = np.ascontiguousarray(np.asarray(pr if pr else [0], dtype=np.uint16))
        h = C.c_void_p()
        _acl_check(self.L, self.L.tm_ptable_create(self.h, buf.ctypes.data, offs.ctypes.data, prio.ctypes.data, len(keys),
                                                   dflt, C.byref(h)), "tm_ptable_create")
        t = PTable(self, h)
        self.__dict__.setdefault("_acls", weakref.WeakSet()).add(t)   # freed with the engine, as the rule sets
        return t

    # ---- batched emqx_access_control:check_acl/3 -----------------------------
    def acl_create(self, rules) -> "Acl":
        """Compiles an ordered rule list (emqx_access_rule terms, as
        emqx_mod_acl_internal.rules takes them) into a device rule set."""
        from . import acl as A
        from . import emqx_access_rule as AR
        arr, keep = A.encode_rules([AR.compile(r) for r in rules])
        h = C.c_void_p()
        _acl_check(self.L, self.L.tm_acl_create(self.h, arr, len(rules), C.byref(h)), "tm_acl_create")
        del keep
        a = Acl(self, h, len(rules))
        self.__dict__.setdefault("_acls", weakref.WeakSet()).add(a)
        return a

    def acl_check(self, acl: "Acl", clients, requests, nomatch=None):
        """requests = [(client index, "publish" | "subscribe", topic)] against the
        rule set -> (verdict u8[n], rule u32[n]): TM_ACL_ALLOW / _DENY /
        _NOMATCH and the index of the deciding rule (TM_NONE on nomatch).
        nomatch = "allow" | "deny" folds the zone's acl_nomatch default into
        the verdicts (emqx_access_control:do_check_acl/3)."""
        from . import acl as A
        n = len(requests)
        verdict = np.full(n, N.TM_ACL_NOMATCH, np.uint8)
        rule = np.full(n, N.TM_NONE, np.uint32)
        cs, keep = A.encode_clients(clients)
        buf, offs, cof, acc = A.encode_requests(requests)
        _acl_check(self.L, self.L.tm_acl_check(self.h, acl.h, C.byref(cs), buf.ctypes.data, offs.ctypes.data,
                                               cof.ctypes.data, acc.ctypes.data, n, verdict.ctypes.data,
                                               rule.ctypes.data), "tm_acl_check")
        del keep
        if nomatch is not None:
            verdict[verdict == N.TM_ACL_NOMATCH] = N.TM_ACL_ALLOW if nomatch == "allow" else N.TM_ACL_DENY
        return verdict, rule

    # ---- emqx_session:dequeue/1 with message expiry -----------------------------
    def drain(self, sessions, queues, now_ms: int, expiry_out: bool = True):
        """tm_sessions_drain: the dequeue after acks over a batch of sessions.

        sessions  [(next_pkt_id, inflight_free)] (or an (n, 2) array);
                  inflight_free TM_SESS_UNBOUNDED for a window of max size 0
        queues    {"q_off": u64[n + 1], "qmsg": u8[Q], "created_ms": i64[Q] or
                  None, "expiry_s": u32[Q] or None}: every session's messages
                  in arrival order (see include/emqx_tm.h for qmsg's bits)
        -> {"disp": u8[Q], "packet_ids": u16[Q], "order": u32[Q], "expiry_out":
            u32[Q] or None, "records": u32[n, 4] (next_pkt_id, n_send, n_send0,
            n_expired), "popped": u32[n, TM_PRIO_MAX_CLASSES]}
        self.drain_info holds the totals per disposition and kernel_ms."""
        sess = np.ascontiguousarray(np.asarray(sessions, dtype=np.uint32).reshape(-1, 2))
        n = len(sess)
        q_off = np.ascontiguousarray(queues["q_off"], dtype=np.uint64)
        if len(q_off) != n + 1:
            raise ValueError("q_off holds one offset more than there are sessions")
        qmsg = np.ascontiguousarray(queues["qmsg"], dtype=np.uint8)
        Q = len(qmsg)
        if int(q_off[n]) != Q:
            raise ValueError("q_off does not end at the number of messages")
        created, expiry = queues.get("created_ms"), queues.get("expiry_s")
        created = None if created is None else np.ascontiguousarray(created, dtype=np.int64)
        expiry = None if expiry is None else np.ascontiguousarray(expiry, dtype=np.uint32)
        if any(x is not None and len(x) != Q for x in (created, expiry)):
            raise ValueError("created_ms / expiry_s hold one value per message")
        res = {"disp": np.zeros(Q, np.uint8), "packet_ids": np.zeros(Q, np.uint16), "order": np.zeros(Q, np.uint32),
               "expiry_out": np.zeros(Q, np.uint32) if expiry_out else None,
               "records": np.zeros((n, 4), np.uint32), "popped": np.zeros((n, N.TM_PRIO_MAX_CLASSES), np.uint32)}
        di, do = N.DrainIn(), N.DrainOut()
        di.sessions = C.cast(sess.ctypes.data, C.POINTER(N.DrainSession))
        di.q_off, di.qmsg = q_off.ctypes.data, qmsg.ctypes.data
        di.created_ms = None if created is None else created.ctypes.data
        di.expiry_s = None if expiry is None else expiry.ctypes.data
        di.now_ms, di.n_sessions = int(now_ms), n
        do.disp, do.packet_ids, do.order = res["disp"].ctypes.data, res["packet_ids"].ctypes.data, res["order"].ctypes.data
        do.expiry_out = res["expiry_out"].ctypes.data if expiry_out else None
        do.records = C.cast(res["records"].ctypes.data, C.POINTER(N.DrainRecord))
        do.popped = res["popped"].ctypes.data
        _acl_check(self.L, self.L.tm_sessions_drain(self.h, C.byref(di), C.byref(do)), "tm_sessions_drain")
        self.drain_info = {"totals": dict(zip(("send0", "send", "kept", "expired"), (int(x) for x in do.totals))),
                           "kernel_ms": float(do.kernel_ms)}
        return res

    # ---- bulk load / filter-sharded mode -----------------------------------
    def insert_many(self, filters, shard: int = 0, nshards: int = 1) -> int:
        """emqx_trie:insert/1 over a filter list; with nshards > 1 only this
        shard's filters and the replicated ones.  Returns how many were inserted."""
        s = _pack(filters)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        done = C.c_uint64()
        N.check(self.L.tm_trie_insert_many(self.h, buf.ctypes.data, offs.ctypes.data, len(s), shard, nshards,
                                           C.byref(done)), "tm_trie_insert_many")
        return int(done.value)

    def delete_many(self, filters) -> int:
        """emqx_trie:delete/1 over a filter list (one C call)."""
        s = _pack(filters)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        done = C.c_uint64()
        N.check(self.L.tm_trie_delete_many(self.h, buf.ctypes.data, offs.ctypes.data, len(s), C.byref(done)),
                "tm_trie_delete_many")
        return int(done.value)

    def apply_many(self, dels, adds) -> tuple:
        """One subscription delta: delete_many(dels) then insert_many(adds),
        planned together (tm_trie_apply_many).  Returns (deleted, inserted)."""
        d, a = _pack(dels), _pack(adds)
        db = np.ascontiguousarray(d.buf if d.buf.size else np.zeros(1, np.uint8))
        do = np.ascontiguousarray(d.offs, dtype=np.uint64)
        ab = np.ascontiguousarray(a.buf if a.buf.size else np.zeros(1, np.uint8))
        ao = np.ascontiguousarray(a.offs, dtype=np.uint64)
        nd, ni = C.c_uint64(), C.c_uint64()
        N.check(self.L.tm_trie_apply_many(self.h, db.ctypes.data, do.ctypes.data, len(d), ab.ctypes.data,
                                          ao.ctypes.data, len(a), C.byref(nd), C.byref(ni)), "tm_trie_apply_many")
        return int(nd.value), int(ni.value)

    def dict_load(self, words):
        s = _pack(words)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        N.check(self.L.tm_dict_load(self.h, buf.ctypes.data, offs.ctypes.data, len(s)), "tm_dict_load")

    def filter_shard(self, f: bytes, nshards: int) -> int:
        return N.check(self.L.tm_filter_shard(self.h, f, len(f), nshards), "tm_filter_shard")

    def tokenize(self, topics) -> Tokens:
        s = _pack(topics)
        n = len(s)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        cap = int(n + np.count_nonzero(s.buf == ord("/"))) if n else 0
        words = np.zeros(max(cap, 1), np.uint32)
        toff = np.zeros(n + 1, np.uint32)
        tflags = np.zeros(max(n, 1), np.uint8)
        nw = C.c_uint64()
        N.check(self.L.tm_tokenize(self.h, buf.ctypes.data, offs.ctypes.data, n, words.ctypes.data, cap,
                                   toff.ctypes.data, tflags.ctypes.data, C.byref(nw)), "tm_tokenize")
        return Tokens(words[:nw.value], toff, tflags[:n])

    def tokenize_device(self, topics, words_cap: int = None):
        """tm_tokenize_device -> (words, toff, tflags) as torch tensors on this
        engine's GPU (the device tokeniser tm_match_batch uses)."""
        import torch
        s = _pack(topics)
        n = len(s)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        if words_cap is None:
            words_cap = int(n + np.count_nonzero(s.buf == ord("/"))) if n else 0
        dev = torch.device("cuda", self.device)
        words = torch.zeros(max(words_cap, 1), dtype=torch.int32, device=dev)
        toff = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        tflags = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        nw = C.c_uint64()
        N.check(self.L.tm_tokenize_device(self.h, buf.ctypes.data, offs.ctypes.data, n, words.data_ptr(), words_cap,
                                          toff.data_ptr(), tflags.data_ptr(), C.byref(nw)), "tm_tokenize_device")
        return words[:nw.value], toff, tflags[:n]

    def prepare_tokens(self, words: int, toff: int, tflags: int, n: int, nwords: int, on_device: bool,
                       batch: Batch = None) -> Batch:
        """A batch from tokenised arrays given as raw pointers (device pointers when
        on_device, e.g. torch tensors' data_ptr()); `batch` is re-prepared in place."""
        h = C.c_void_p(batch.h.value if batch is not None else None)
        N.check(self.L.tm_batch_prepare_tokens(self.h, words, toff, tflags, n, nwords, int(on_device), C.byref(h)),
                "tm_batch_prepare_tokens")
        if batch is not None:
            batch.n = n
            return batch
        return Batch(self, handle=h, n=n)

    def prepare_tokens_host(self, tok: Tokens, batch: Batch = None) -> Batch:
        w = np.ascontiguousarray(tok.words if len(tok.words) else np.zeros(1, np.uint32))
        t = np.ascontiguousarray(tok.toff)
        f = np.ascontiguousarray(tok.tflags if len(tok.tflags) else np.zeros(1, np.uint8))
        return self.prepare_tokens(w.ctypes.data, t.ctypes.data, f.ctypes.data, len(tok), tok.nwords, False, batch)

    def gather_rows(self, d_src: int, d_src_off: int, d_idx: int, n: int, d_dst_off: int, d_dst: int):
        N.check(self.L.tm_gather_rows(self.h, d_src, d_src_off, d_idx, n, d_dst_off, d_dst), "tm_gather_rows")

    def tokens_shard(self, d_words: int, d_toff: int, n: int, nshards: int, d_shard: int):
        N.check(self.L.tm_tokens_shard(self.h, d_words, d_toff, n, nshards, d_shard), "tm_tokens_shard")

    # ---- filters -----------------------------------------------------------
    def filter_bytes(self, fid: int) -> bytes:
        n = C.c_size_t()
        p = self.L.tm_filter_bytes(self.h, fid, C.byref(n))
        if not p:
            raise KeyError(fid)
        return C.string_at(p, n.value)

    def filter_copy(self, fid: int) -> bytes:
        """tm_filter_copy: the filter's bytes copied under the engine lock."""
        n = C.c_size_t()
        buf = C.create_string_buffer(N.TM_MAX_TOPIC_LEN + 1)
        rc = self.L.tm_filter_copy(self.h, fid, buf, len(buf), C.byref(n))
        if rc == N.TM_ENOENT:
            raise KeyError(fid)
        N.check(rc, "tm_filter_copy")
        return buf.raw[:n.value]

    def filters_copy(self, ids) -> list:
        """tm_filters_copy: [(index in ids, filter bytes)] for the ids that
        still name a filter, copied under one acquisition of the engine lock."""
        a = np.ascontiguousarray(ids, dtype=np.uint32)
        n = len(a)
        offs = np.zeros(n + 1, np.uint64)
        keep = np.zeros(max(n, 1), np.uint32)
        k, need = C.c_uint32(), C.c_uint64()
        cap = 64 * max(n, 1)
        while True:
            buf = np.zeros(max(cap, 1), np.uint8)
            N.check(self.L.tm_filters_copy(self.h, a.ctypes.data, n, buf.ctypes.data, cap, offs.ctypes.data,
                                           keep.ctypes.data, C.byref(k), C.byref(need)), "tm_filters_copy")
            if need.value <= cap:
                break
            cap = need.value
        raw = buf.tobytes()
        return [(int(keep[j]), raw[int(offs[j]):int(offs[j + 1])]) for j in range(k.value)]

    def filter_id(self, f: bytes) -> int:
        out = C.c_uint32()
        rc = self.L.tm_filter_id(self.h, f, len(f), C.byref(out))
        if rc == N.TM_ENOENT:
            raise KeyError(f)
        N.check(rc, "tm_filter_id")
        return out.value

    # ---- engine ------------------------------------------------------------
    @property
    def version(self) -> int:
        return int(self.L.tm_version(self.h))

    def stats(self) -> dict:
        st = N.EngineStats()
        N.check(self.L.tm_stats(self.h, C.byref(st)), "tm_stats")
        return st.asdict()

    def sync(self):
        N.check(self.L.tm_sync(self.h), "tm_sync")

    def sync_async(self):
        """Queue the pending deltas' upload now, without waiting (tm_sync_async)."""
        N.check(self.L.tm_sync_async(self.h), "tm_sync_async")

    def debug_check(self) -> int:
        """tm_debug_check: edge-hash invariants; -> largest displacement."""
        md = C.c_uint64()
        N.check(self.L.tm_debug_check(self.h, C.byref(md)), "tm_debug_check")
        return int(md.value)

    def debug_slots(self):
        """tm_debug_slots: the host edge hash as stored -> (nslots x 4 u32
        array of parent, word, child, hash; bucket count).  Read-only; works
        on a host-only engine."""
        nb = C.c_uint64()
        rc = self.L.tm_debug_slots(self.h, None, 0, C.byref(nb))
        if rc != N.TM_EOVERFLOW:
            N.check(rc, "tm_debug_slots")
        out = np.empty((int(nb.value) * 4, 4), np.uint32)
        N.check(self.L.tm_debug_slots(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.shape[0], C.byref(nb)),
                "tm_debug_slots")
        return out, int(nb.value)

    def upload_info(self) -> dict:
        """tm_debug_upload_info: what the delta-upload path has pending and
        what it has done so far, by name (N.UPLOAD_INFO); uploads nothing."""
        out = (C.c_uint64 * len(N.UPLOAD_INFO))()
        N.check(self.L.tm_debug_upload_info(self.h, out), "tm_debug_upload_info")
        return dict(zip(N.UPLOAD_INFO, (int(x) for x in out)))

    @staticmethod
    def _diff(out) -> dict:
        return {t: (int(out[2 * i]), None if out[2 * i + 1] == 2 ** 64 - 1 else int(out[2 * i + 1]))
                for i, t in enumerate(N.DIFF_TABLES)}

    def shadow_sync(self, apply: bool = True) -> dict:
        """tm_debug_shadow_sync: bring the engine's host-memory stand-in for a
        replica up to date the way an upload would (apply), then compare it
        with the host tables -> {table: (differing elements, first index)}."""
        out = (C.c_uint64 * (2 * len(N.DIFF_TABLES)))()
        N.check(self.L.tm_debug_shadow_sync(self.h, int(bool(apply)), out), "tm_debug_shadow_sync")
        return self._diff(out)

    def replica_diff(self, replica: int = 0, sync: bool = True) -> dict:
        """tm_debug_replica_diff: (after a tm_sync, if sync) the replica's tables
        read back and compared with the host's, as shadow_sync reports."""
        out = (C.c_uint64 * (2 * len(N.DIFF_TABLES)))()
        N.check(self.L.tm_debug_replica_diff(self.h, replica, int(bool(sync)), out), "tm_debug_replica_diff")
        return self._diff(out)

    @property
    def fan_big_limit(self) -> int:
        """tm_debug_fan_big_limit: deliveries of a fan-out scan block above which
        its match offsets are u64 (TM_FAN_BIG at creation, else 2^32 - 1)."""
        return int(self.L.tm_debug_fan_big_limit(self.h))


class ShardedBatch:
    """A publish batch of a ShardedGroup (tm_sharded_prepare / run / result)."""

    def __init__(self, grp: "ShardedGroup", topics):
        self.grp = grp
        s = _pack(topics)
        self.n = len(s)
        self._buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        self._offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        h = C.c_void_p()
        N.check(grp.L.tm_sharded_prepare(grp.h, self._buf.ctypes.data, self._offs.ctypes.data, self.n, C.byref(h)),
                "tm_sharded_prepare")
        self.h = h

    def run(self):
        N.check(self.grp.L.tm_sharded_run(self.grp.h, self.h), "tm_sharded_run")
        return self

    def reprepare(self, topics):
        """tm_sharded_prepare in place: new publishes (or the same ones again)."""
        s = _pack(topics)
        self.n = len(s)
        self._buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        self._offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        N.check(self.grp.L.tm_sharded_prepare(self.grp.h, self._buf.ctypes.data, self._offs.ctypes.data, self.n,
                                              C.byref(self.h)), "tm_sharded_prepare")
        return self

    def result(self):
        r = N.Result()
        N.check(self.grp.L.tm_sharded_result(self.grp.h, self.h, C.byref(r)), "tm_sharded_result")
        return _result_arrays(r)

    def stats(self) -> dict:
        st = N.ShardedStats()
        N.check(self.grp.L.tm_sharded_batch_stats(self.grp.h, self.h, C.byref(st)), "tm_sharded_batch_stats")
        out = st.match.asdict()
        out.update(ms_partition=st.ms_partition, ms_exchange=st.ms_exchange, ms_step=st.ms_step,
                   ms_unpartition=st.ms_unpartition, host_waits=st.host_waits,
                   part_topics=list(st.part_topics)[:len(self.grp)], ms_stage=st.ms_stage, ms_plan=st.ms_plan)
        return out

    def free(self):
        if self.h:
            self.grp.L.tm_sharded_batch_free(self.grp.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ShardedGroup:
    """Filter-sharded matching in one process (tm_sharded_*, config C4 without
    torch or a collective): G shard engines, filters partitioned by their
    literal (w0, w1) prefix, publishes matched by their owner shard, rows in
    publish order with global ids (local id * G + shard)."""

    def __init__(self, devices, host_threads: int = 0):
        self.L = N.lib()
        devs = (C.c_int32 * len(devices))(*devices)
        cfg = N.Config(0, 0, host_threads, 0)
        h = C.c_void_p()
        N.check(self.L.tm_sharded_create(devs, len(devices), C.byref(cfg), C.byref(h)), "tm_sharded_create")
        self.h = h
        self.devices = list(devices)
        self._borrowed = weakref.WeakSet()

    def close(self):
        if getattr(self, "h", None):
            _invalidate(self)
            self.L.tm_sharded_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self.L.tm_sharded_size(self.h))

    def link(self, i: int, j: int) -> str:
        """How shard i's memory reaches shard j's device: same / peer / staged."""
        return {N.TM_LINK_SAME: "same", N.TM_LINK_PEER: "peer", N.TM_LINK_STAGED: "staged"}[
            N.check(self.L.tm_sharded_link(self.h, i, j), "tm_sharded_link")]

    def dict_load(self, words):
        s = _pack(words)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        N.check(self.L.tm_sharded_dict_load(self.h, buf.ctypes.data, offs.ctypes.data, len(s)), "tm_sharded_dict_load")

    def insert_many(self, filters) -> int:
        s = _pack(filters)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        done = C.c_uint64()
        N.check(self.L.tm_sharded_insert_many(self.h, buf.ctypes.data, offs.ctypes.data, len(s), C.byref(done)),
                "tm_sharded_insert_many")
        return int(done.value)

    def delete_many(self, filters) -> int:
        s = _pack(filters)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        done = C.c_uint64()
        N.check(self.L.tm_sharded_delete_many(self.h, buf.ctypes.data, offs.ctypes.data, len(s), C.byref(done)),
                "tm_sharded_delete_many")
        return int(done.value)

    def prepare(self, topics) -> ShardedBatch:
        return ShardedBatch(self, topics)

    def match_batch(self, topics):
        s = _pack(topics)
        buf = np.ascontiguousarray(s.buf if s.buf.size else np.zeros(1, np.uint8))
        offs = np.ascontiguousarray(s.offs, dtype=np.uint64)
        r = N.Result()
        N.check(self.L.tm_sharded_match_batch(self.h, buf.ctypes.data, offs.ctypes.data, len(s), C.byref(r)),
                "tm_sharded_match_batch")
        return _result_arrays(r)

    def filter_bytes(self, gid: int) -> bytes:
        cap = 4096
        buf = C.create_string_buffer(cap)
        n = C.c_size_t()
        N.check(self.L.tm_sharded_filter_copy(self.h, gid, buf, cap, C.byref(n)), "tm_sharded_filter_copy")
        return buf.raw[:n.value]

    def engine(self, shard: int) -> "Engine":
        return Engine._borrow(self.L.tm_sharded_engine(self.h, shard), [self.devices[shard]], owner=self)
