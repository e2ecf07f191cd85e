"""Executable model of the generic match path (tm_match_slow in tm_kernels.hip)
-- test infrastructure.

One wave walks one topic: a LIFO probe stack (SLOW_SQ entries of LDS, or the
first TM_SLOW_LDS of them), up to 64 probes popped from the top per iteration,
pushes and emissions appended in lane order.  A frontier that outgrows the LDS
stack abandons the walk and starts it again with the stack in the wave's
global scratch (S_QCAP entries); a frontier or a row that outgrows the scratch
is an error the host answers with four times the scratch and another launch.
The finished row is then sorted in one of the regimes named by regime().

The trie and the expansion rules are kernel_model.Model's.  What this adds is
the single-topic loop with its capacities, the literal probe of a word the
dictionary does not know (never pushed), the sort regimes, the rank merge of
the two-run sort, and builders for topics with a chosen number of matches.
"""

from __future__ import annotations

import itertools
import os
import random
import re

from kernel_model import C_EMPTY, DIG_H, DIG_L, DIG_P, FAST_MAX_DEPTH, Model, word_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SLOW_SQ = 512               # probe stack entries in LDS
SORT_LDS = 2 * SLOW_SQ      # u64 entries of the same LDS as the sort area
S_QCAP = 1 << 13            # probe stack entries of a wave's global scratch, first launch
S_OCAP = 1 << 14            # row entries of a wave's global scratch, first launch
SLOW_WAVES_SMALL = 64       # waves of the generic path below 65,536 topics
ROW_CAP = 128               # default K: a longer row leaves the tile walk for the generic path


def source_constants():
    """The same constants as the sources spell them."""
    def src(*p):
        with open(os.path.join(ROOT, "emqx_amd", "csrc", *p)) as f:
            return f.read()
    kern, impl, batch = src("tm_kernels.hip"), src("tm_engine_impl.hpp"), src("tm_batch.cpp")
    sq = int(re.search(r"#define TM_SLOW_SQ (\d+)", kern).group(1))
    mul = int(re.search(r"constexpr uint32_t SORT_LDS = SLOW_SQ \* (\d+);", kern).group(1))
    caps = re.search(r"s_qcap = 1u << (\d+), s_ocap = 1u << (\d+);", impl)
    waves = re.search(r"b->n < 65536 \? (\d+)u :", batch)
    return {"SLOW_SQ": sq, "SORT_LDS": sq * mul, "S_QCAP": 1 << int(caps.group(1)), "S_OCAP": 1 << int(caps.group(2)),
            "SLOW_WAVES_SMALL": int(waves.group(1)),
            "ROW_CAP": int(re.search(r"uint32_t row_cap = (\d+);", impl).group(1))}


class Walk:
    """What walk() returns: the emissions in emission order as (key, filter),
    the largest stack the finished walk held, whether it started again in
    global scratch, and whether it ran out of scratch (the emissions are then
    the ones made before it did)."""

    def __init__(self, emissions, peak, restarted, error):
        self.emissions, self.peak, self.restarted, self.error = emissions, peak, restarted, error


class SlowModel:
    def __init__(self, filters):
        self.m = Model(filters)
        self.known = {w for f in filters for w in f.split(b"/")}    # the dictionary

    def insert(self, f):
        self.m._insert(f)
        self.known.update(f.split(b"/"))

    def _literal(self, w):
        """The literal probe of topic word w is pushed: not for '+', nor for a word no filter holds."""
        return w != b"+" and (w == b"" or w in self.known)

    def _attempt(self, topic, cap, ocap):
        """One walk with a stack of cap entries -> (emissions, peak, overflowed the stack, overflowed the row)."""
        m = self.m
        ws = topic.split(b"/")
        d = len(ws)
        dollar = topic[:1] == b"$"

        def put(key, lvl, dig):   # (deeper levels have no digit: their rows are ordered by bytes)
            return key | (dig << (61 - 3 * lvl)) if lvl <= FAST_MAX_DEPTH else key

        cls, _ = word_class(ws[0])
        stack, out = [], []
        if not dollar and m.hterm(0) is not None:
            out.append((DIG_H[cls] << 61, m.hterm(0)))
        if ws[0] == b"#":
            if not dollar and m.probe(0, b"#") is not None:
                stack.append((0, b"#", DIG_L[cls] << 61, 1, d == 1))
        elif self._literal(ws[0]):
            stack.append((0, ws[0], DIG_L[cls] << 61, 1, False))
        if not dollar and m.probe(0, b"+") is not None:
            stack.append((0, b"+", DIG_P[cls] << 61, 1, False))
        peak = len(stack)
        while stack:
            k = min(len(stack), 64)
            popped = stack[len(stack) - k:]
            del stack[len(stack) - k:]
            pushes, emits = [], []
            for (parent, w, key, lc, skipe) in popped:     # lane order
                c = m.probe(parent, w)
                if c is None:
                    continue
                if lc == d:
                    if not skipe and c in m.topic:
                        kk = key
                        sp = 61 - 3 * (lc - 1)
                        if word_class(ws[lc - 1])[0] == C_EMPTY and lc - 1 <= FAST_MAX_DEPTH and ((kk >> sp) & 7) == 4:
                            kk = (kk & ~(7 << sp)) | (1 << sp)
                        emits.append((kk, m.topic[c]))
                    if m.hterm(c) is not None:
                        emits.append((put(key, lc, 2), m.hterm(c)))
                    continue
                wh = ws[lc]
                cls, _ = word_class(wh)
                if m.hterm(c) is not None:
                    emits.append((put(key, lc, DIG_H[cls]), m.hterm(c)))
                if wh == b"#":
                    if m.probe(c, b"#") is not None:
                        pushes.append((c, b"#", put(key, lc, DIG_L[cls]), lc + 1, lc + 1 == d))
                elif self._literal(wh):
                    pushes.append((c, wh, put(key, lc, DIG_L[cls]), lc + 1, False))
                if m.probe(c, b"+") is not None:
                    pushes.append((c, b"+", put(key, lc, DIG_P[cls]), lc + 1, False))
            if len(stack) + len(pushes) > cap:
                return out, peak, True, False
            if len(out) + len(emits) > ocap:
                return out, peak, False, True
            stack.extend(pushes)
            out.extend(emits)
            peak = max(peak, len(stack))
        return out, peak, False, False

    def walk(self, topic, lcap=SLOW_SQ, qcap=S_QCAP, ocap=S_OCAP):
        """The kernel's loop for one topic: in LDS (lcap entries, at most
        SLOW_SQ), and again in global scratch (qcap) when qn + ptot > lcap."""
        lcap = min(lcap, SLOW_SQ) if lcap else SLOW_SQ
        assert lcap <= qcap
        out, peak, spill, err = self._attempt(topic, lcap, ocap)
        if spill:
            out, peak, full, err = self._attempt(topic, qcap, ocap)
            return Walk(out, peak, True, err or full)
        return Walk(out, peak, False, err)


def regime(on, by_bytes, ocap=S_OCAP):
    """Where the kernel sorts a row of on entries (by_bytes: a deep or irregular topic's)."""
    np2 = 1
    while np2 < on:
        np2 <<= 1
    if not on > 1:
        return "none"
    if not by_bytes and np2 > SORT_LDS and on <= 2 * SORT_LDS:
        return "two_runs"
    if not by_bytes and np2 <= SORT_LDS:
        return "lds64"
    if by_bytes and np2 <= 2 * SORT_LDS:
        return "lds_bytes"
    if np2 <= ocap:
        return "global"
    return "scratch_error"


def lower_bound(run, x):
    lo, hi = 0, len(run)
    while lo < hi:
        mid = (lo + hi) >> 1
        if run[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return lo


def merge_runs(a_sorted, b_sorted):
    """merge_runs_out: every entry goes to its index in its own run plus its
    rank (a lower-bound search) in the other; the keys are distinct."""
    out = [None] * (len(a_sorted) + len(b_sorted))
    for i, x in enumerate(a_sorted):
        out[i + lower_bound(b_sorted, x)] = x
    for j, x in enumerate(b_sorted):
        out[j + lower_bound(a_sorted, x)] = x
    return out


# ---- layouts ---------------------------------------------------------------------------------

def words_of(depth, n, hashes, seed):
    tag = b"L%d%s%dn%d" % (depth, b"h" if hashes else b"p", seed, n)
    return [tag + b"w%d" % i for i in range(depth)]


def candidates(ws, hashes, own=True):
    """All literal / '+' masks of the words; with hashes also every mask with
    a '#' after it and with '#' for its last level.  own: without the filters
    made of wildcards alone, which would match other layouts' topics too."""
    full, tail, last = [], [], set()
    for mask in itertools.product((0, 1), repeat=len(ws)):
        lv = [b"+" if m else w for m, w in zip(mask, ws)]
        full.append(b"/".join(lv))
        if hashes:
            tail.append(b"/".join(lv + [b"#"]))
            last.add(b"/".join(lv[:-1] + [b"#"]))
    c = full + tail + sorted(last)
    if own:
        c = [f for f in c if any(w not in (b"+", b"#") for w in f.split(b"/"))]
    return c


def layout(depth, n, hashes, seed, own=True):
    """-> (topic, filters): a topic of depth words of its own and exactly n
    filters that match it, a seeded sample of candidates() (a prefix of them
    would leave the halves of a row barely interleaved).  Up to 10 levels the
    row is path-coded, deeper it is ordered by bytes."""
    ws = words_of(depth, n, hashes, seed)
    c = candidates(ws, hashes, own)
    assert n <= len(c), (n, len(c))
    return b"/".join(ws), random.Random(seed).sample(c, n)


def brim_layout(depth):
    """The full mask product: 2^depth filters.  From 64 probes on, a full
    iteration pops 64 and pushes 128, so the stack peaks at 128 + 64 * (depth -
    7) when the last level is pushed: 512 = SLOW_SQ at depth 13."""
    ws = words_of(depth, 1 << depth, False, 0)
    return b"/".join(ws), candidates(ws, False, own=False)


def past_brim_layout(depth, plus_under):
    """The full product of the first depth - 1 levels, each followed by the
    literal last word, and one more filter that ends in '+' under each of the
    product's prefixes named by plus_under (indices in candidates() order).
    The push of the last level is then one literal probe per popped node and
    a '+' probe for each that has the child."""
    ws = words_of(depth, 0, False, 1)
    heads = candidates(ws[:-1], False, own=False)
    return b"/".join(ws), [h + b"/" + ws[-1] for h in heads] + [heads[i] + b"/+" for i in plus_under]


def find_past_brim(depth, peak):
    """Searches, last prefix first, for the one prefix whose '+' child makes
    the stack of past_brim_layout peak at `peak` -> (plus_under, peaks tried)."""
    topic, base = past_brim_layout(depth, [])
    heads = 1 << (depth - 1)
    sm = SlowModel(base)
    tried = []
    for i in range(heads - 2, -1, -1):      # (heads - 1 is the prefix of '+' alone)
        f = past_brim_layout(depth, [i])[1][-1]
        n_edges, nid = len(sm.m.edges), sm.m.nid
        sm.insert(f)
        assert len(sm.m.edges) == n_edges + 1
        got = sm.walk(topic, lcap=SLOW_SQ, qcap=1 << 30, ocap=1 << 30).peak
        edge = next(reversed(sm.m.edges))   # (the edge and the node just added)
        del sm.m.topic[sm.m.edges.pop(edge)]
        sm.m.nid = nid
        tried.append(got)
        if got == peak:
            return [i], tried
        if len(tried) >= 64:
            break
    return None, tried
