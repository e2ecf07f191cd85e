"""Probe runs of the edge hash, restated in plain Python (no device).

The edge hash is open addressing over 64-byte buckets of four 16-byte slots,
keyed (parent, word); a key that did not fit its home bucket sits up to
max_disp buckets further on, the run wrapping from the last bucket to bucket
0.  Slots of a bucket fill in order, so a bucket whose last slot is free ends
every run through it.  Both device walks follow such a run for at most
max_probe + 1 buckets, max_probe being max_disp stepped up to 4, 8, 16 or 48.

Two references live here:

    Table(dump)   a run read off the table Engine.debug_slots() copied out,
                  with no model of how the table came to be: found or absent,
                  the displacement, and the number of bucket reads.  walk()
                  adds up the reads of every probe the tile walk issues for
                  one topic -- what stats()["probes"] must equal for a batch
                  that stays on the tile path.
    simulate()    the placement of an insert-only key list (slots fill in
                  order, next bucket when full).  Only used to choose inputs
                  and to cross-check the engine.

The world builders below make small tables (256 buckets) whose runs have a
known shape; test_probe_model.py checks from the dump alone that every world
has the shape it claims, test_gpu_probe_edges.py walks them on the device.
"""

import numpy as np

MASK64 = (1 << 64) - 1
NB = 256                    # buckets of a fresh table; it stays there while used slots <= 768
BUCKET = 4
EMPTY = 0xFFFFFFFF
ID_MASK = (1 << 30) - 1
WID_BITS = 29
WID_MASK = (1 << WID_BITS) - 1
ROOT, W_UNKNOWN, W_EMPTY, W_PLUS, W_HASH = 0, 0, 1, 2, 3
B_TOPIC, B_PLUS = 1 << 30, 1 << 31      # child field
B_HTERM, B_HASH = 1 << 30, 1 << 31      # hash field
MAX_PROBE_DISP = 48
POOL_N = 60000


def edge_hash(parent, word):
    k = ((parent << 32) | word) & MASK64
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & MASK64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & MASK64
    k ^= k >> 33
    return k & 0xFFFFFFFF


def home_bucket(parent, word, nb=NB):
    return (edge_hash(parent, word) * nb) >> 32


def lsig_pos(w):
    return (((w * 0x9E3779B1) & 0xFFFFFFFF) * 5) >> 32


def lext_pos(w):
    return (((w * 0x85EBCA6B) & 0xFFFFFFFF) * 30) >> 32


def stepped(max_disp):
    """The launch's max_probe for a table whose largest displacement is max_disp."""
    assert max_disp <= MAX_PROBE_DISP
    return 4 if max_disp <= 4 else 8 if max_disp <= 8 else 16 if max_disp <= 16 else MAX_PROBE_DISP


# ---- the word pool ---------------------------------------------------------------------------

def pool_words(dollar=False):
    return [(b"$k%05d" if dollar else b"k%05d") % i for i in range(POOL_N)]


def pool_ids(eng, dollar=False):
    """The pool's words (loaded into eng's dictionary on first use) and their ids."""
    pools = eng.__dict__.setdefault("_probe_pools", {})
    if dollar not in pools:
        words = pool_words(dollar)
        eng.dict_load(words)
        tok = eng.tokenize(words)
        assert tok.words.size == len(words)
        ids = (tok.words & WID_MASK).astype(np.int64)
        assert (ids >= 4).all() and np.unique(ids).size == ids.size
        pools[dollar] = (words, ids)
    return pools[dollar]


def word_id(eng, w):
    tok = eng.tokenize([w])
    return int(tok.words[0]) & WID_MASK


def pick(eng, parent_id, bucket, count, nb=NB, dollar=False, skip=0):
    """count pool words whose key (parent_id, id) is homed in bucket (after the first skip such)."""
    words, ids = pool_ids(eng, dollar)
    out = []
    for w, i in zip(words, ids.tolist()):
        if home_bucket(parent_id, i, nb) == bucket:
            if skip:
                skip -= 1
                continue
            out.append(w)
            if len(out) == count:
                return out
    raise AssertionError("the pool has only %d words homed in bucket %d" % (len(out), bucket))


# ---- a run read off the dump -----------------------------------------------------------------

class Run:
    def __init__(self, found, disp, reads, slot):
        self.found, self.disp, self.reads, self.slot = found, disp, reads, slot

    def __repr__(self):
        return "Run(found=%s, disp=%d, reads=%d)" % (self.found, self.disp, self.reads)


class Table:
    def __init__(self, dump):
        slots, nb = dump
        self.nb = nb
        self.s = np.asarray(slots, dtype=np.uint32).reshape(nb, BUCKET, 4).astype(np.int64)

    def run(self, parent, word, max_probe):
        """The probe run of key (parent, word): buckets from home, with wrap,
        until the key is found, a bucket's last slot is free, or max_probe + 1
        buckets were read."""
        b = home_bucket(parent, word, self.nb)
        reads = 0
        for disp in range(max_probe + 1):
            reads += 1
            for k in range(BUCKET):
                p, w = int(self.s[b, k, 0]), int(self.s[b, k, 1])
                if p != EMPTY and (p & ID_MASK) == parent and (w & WID_MASK) == word:
                    return Run(True, disp, reads, self.s[b, k])
            if int(self.s[b, BUCKET - 1, 0]) == EMPTY:
                return Run(False, disp, reads, None)
            b = 0 if b + 1 == self.nb else b + 1
        return Run(False, max_probe, reads, None)

    def where(self, parent, word):
        """(home bucket, stored bucket) of a live key, by a scan of the whole table."""
        for b in range(self.nb):
            for k in range(BUCKET):
                p, w = int(self.s[b, k, 0]), int(self.s[b, k, 1])
                if p != EMPTY and (p & ID_MASK) == parent and (w & WID_MASK) == word:
                    return home_bucket(parent, word, self.nb), b
        return None

    def keys(self):
        """Per bucket, the set of (parent, word) stored there."""
        out = []
        for b in range(self.nb):
            out.append({(int(p) & ID_MASK, int(w) & WID_MASK) for p, w in self.s[b, :, :2] if int(p) != EMPTY})
        return out

    def max_disp(self):
        md = 0
        for b, ks in enumerate(self.keys()):
            for p, w in ks:
                md = max(md, (b - home_bucket(p, w, self.nb)) % self.nb)
        return md

    def full(self, b):
        return int(self.s[b % self.nb, BUCKET - 1, 0]) != EMPTY

    def child(self, parent, word):
        r = self.run(parent, word, MAX_PROBE_DISP)
        return int(r.slot[2]) & ID_MASK if r.found else None

    def node(self, eng, path):
        """Node id of the filter prefix path (a list of words), followed through the dump."""
        n = ROOT
        for w in path:
            n = self.child(n, W_PLUS if w == b"+" else W_HASH if w == b"#" else word_id(eng, w))
            assert n is not None, path
        return n

    def walk(self, ids, dollar, max_probe):
        """Bucket reads of the tile walk for one topic (ids: its word ids, 0 =
        not in the dictionary; at most 10 regular words), and the probes
        as (parent, word, Run).  Mirrors the walk's choice of probes: the root
        probes every known first word and its '+' child; below the root a
        literal is probed only when the found slot's signatures allow it."""
        d = len(ids)
        probes, stack = [], []
        if d == 0:
            return 0, probes
        root_plus = self.run(ROOT, W_PLUS, max_probe).found
        root_hash = self.run(ROOT, W_HASH, max_probe).found
        w0 = ids[0]
        if w0 == W_HASH:
            if not dollar and root_hash:
                stack.append((ROOT, W_HASH, 1))
        elif w0 not in (W_UNKNOWN, W_PLUS):
            stack.append((ROOT, w0, 1))
        if not dollar and root_plus:
            stack.append((ROOT, W_PLUS, 1))
        reads = 0
        while stack:
            p, w, lc = stack.pop()
            r = self.run(p, w, max_probe)
            probes.append((p, w, r))
            reads += r.reads
            if not r.found or lc == d:
                continue
            pf, wf, cf, hf = (int(x) for x in r.slot)
            child, wid = cf & ID_MASK, ids[lc]
            n_hash, n_plus = bool(hf & B_HASH), bool(cf & B_PLUS)
            sig = (wf >> WID_BITS) | ((pf >> 30) << 3)
            lit = wid not in (W_UNKNOWN, W_PLUS) and (sig >> lsig_pos(wid)) & 1 and (n_hash or (hf >> lext_pos(wid)) & 1)
            if n_hash if wid == W_HASH else lit:
                stack.append((child, wid, lc + 1))
            if n_plus:
                stack.append((child, W_PLUS, lc + 1))
        return reads, probes


def topic_ids(eng, topics):
    """Per topic: (word ids, starts with '$'), by the host tokeniser."""
    tok = eng.tokenize(topics)
    out = []
    for i, t in enumerate(topics):
        ws = tok.words[tok.toff[i]:tok.toff[i + 1]]
        out.append(([int(w) & WID_MASK for w in ws], t[:1] == b"$"))
    return out


def batch_reads(eng, table, topics, max_probe):
    """Sum of the tile walk's bucket reads over a batch (distinct topics walked once)."""
    cache = {}
    for t, (ids, dollar) in zip(topics, topic_ids(eng, topics)):
        if t not in cache:
            cache[t] = table.walk(ids, dollar, max_probe)[0]
    return sum(cache[t] for t in topics)


# ---- placement simulation --------------------------------------------------------------------

def simulate(keys, nb=NB):
    """Insert-only placement of (parent, word) keys, in order: -> (per-bucket
    key lists, {key: displacement})."""
    buckets = [[] for _ in range(nb)]
    disp = {}
    for p, w in keys:
        b = home_bucket(p, w, nb)
        d = 0
        while len(buckets[b]) == BUCKET:
            b = 0 if b + 1 == nb else b + 1
            d += 1
            assert d < nb
        buckets[b].append((p, w))
        disp[(p, w)] = d
    return buckets, disp


# ---- worlds ----------------------------------------------------------------------------------
# A world is a dict: filters (in insert order), topics, max_probe (the stepped
# bound it means to run under), found = [(topic, parent path, word, displacement)]
# and absent = [(topic, home bucket, reads)] for root keys, wrap = [topics whose
# key is homed at the table's end and stored at its start].

STEP_CASES = [(4, 100), (5, 100), (8, 250), (9, 250), (16, 100), (17, 255), (48, 255)]   # (D, home bucket)


def build(eng, world):
    """Insert a world's filters one by one (placement follows the list's order)."""
    for f in world["filters"]:
        eng.insert(f)
    return world


def step_world(eng, D, bucket):
    """4 D + 1 one-word filters homed in one bucket: the last sits D buckets
    from home, filter i at i // 4.  Absent words homed in the cluster's
    buckets end at its tail bucket after 1, 2, ... reads.  'w/#' filters on the
    deepest and two nearer keys give the generic path's topics their rows."""
    pool_ids(eng)
    cluster = pick(eng, ROOT, bucket, 4 * D + 1)
    found = [(w, [], w, i // 4) for i, w in enumerate(cluster)]
    absent = []
    tail = (bucket + D) % NB                      # the bucket holding the last key: its last slot is free
    for reads in sorted({1, 2, stepped(D), D + 1}):
        if reads > D + 1:
            continue
        b = (tail - (reads - 1)) % NB
        absent.append((pick(eng, ROOT, b, 1, skip=4 * D + 1 if b == bucket else 0)[0], b, reads))
    deep = [cluster[-1], cluster[len(cluster) // 2], cluster[0]]
    filters = cluster + [w + b"/#" for w in deep]
    wrap = [w for i, w in enumerate(cluster) if bucket + i // 4 >= NB]
    return dict(filters=filters, topics=cluster + [a[0] for a in absent], max_probe=stepped(D), found=found,
                absent=absent, wrap=wrap, deep=deep, D=D, bucket=bucket)


def absent_world(eng, max_probe, first):
    """max_probe + 1 neighbouring buckets from `first` (wrapping if it is near
    the end), each filled by four keys of its own: no key is displaced, yet an
    absent key homed in the first reads max_probe + 1 full buckets and is cut
    by the bound; absent keys homed further on reach the free bucket behind
    the run after max_probe, 2 and 1 reads.  A cluster elsewhere sets the step
    when max_probe > 4."""
    pool_ids(eng)
    L = max_probe + 1
    filters, found = [], []
    if max_probe > 4:
        D = {8: 5, 16: 9}[max_probe]
        cl = pick(eng, ROOT, 30, 4 * D + 1)
        filters += cl
        found += [(w, [], w, i // 4) for i, w in enumerate(cl)]
    for j in range(L):
        own = pick(eng, ROOT, (first + j) % NB, 4)
        filters += own
        found += [(w, [], w, 0) for w in own]
    absent = []
    for home_off, reads in [(0, max_probe + 1), (2, max_probe), (L - 1, 2), (L, 1)]:
        b = (first + home_off) % NB
        absent.append((pick(eng, ROOT, b, 1, skip=4)[0], b, reads))
    return dict(filters=filters, topics=[f[0] for f in found] + [a[0] for a in absent], max_probe=max_probe,
                found=found, absent=absent, wrap=[], first=first, L=L)


def wrap_world(eng):
    """Nine keys homed in the last bucket but one, then 21 homed in the last:
    30 keys from bucket 254 on fill 254, 255, 0 .. 4 and half of 5."""
    pool_ids(eng)
    a = pick(eng, ROOT, NB - 2, 9)
    b = pick(eng, ROOT, NB - 1, 21)
    _, disp = simulate([(ROOT, word_id(eng, w)) for w in a + b])
    found = [(w, [], w, disp[(ROOT, word_id(eng, w))]) for w in a + b]
    absent = [(pick(eng, ROOT, NB - 1, 1, skip=21)[0], NB - 1, 7), (pick(eng, ROOT, 1, 1)[0], 1, 5)]
    wrap = [w for w, _, _, d in found if home_bucket(ROOT, word_id(eng, w)) + d >= NB]
    return dict(filters=a + b, topics=a + b + [x[0] for x in absent], max_probe=8, found=found, absent=absent,
                wrap=wrap)


KIND_D = 5


def kinds_world(eng, twin=None):
    """Continued probes of every kind, each key D = 5 buckets from home because
    20 one-word filters homed in its home bucket went in first:

        root '+'            (ROOT, '+')
        literal '#' last    (ROOT, '#'): the topic '#' probes it with M_SKIPE
        $-start             21 clustered '$' words (the last one at 5)
        under a parent      (P, x) and (P, '+') for P = node of 'par'
        level 10            the last edge of a 10-word filter

    Node ids are read from the dump as the world is built (eng is filled here;
    a twin engine, if given, gets the same inserts)."""
    pool_ids(eng)
    pool_ids(eng, dollar=True)
    engines = [eng] + ([twin] if twin is not None else [])
    if twin is not None:
        pool_ids(twin)
        pool_ids(twin, dollar=True)
    filters, found, used = [], [], {}

    def put(fs):
        for f in fs:
            for e in engines:
                e.insert(f)
        filters.extend(fs)

    def fill(parent, word):
        """20 root words homed where (parent, word) is homed, skipping words already used there."""
        b = home_bucket(parent, word)
        ws = pick(eng, ROOT, b, 4 * KIND_D, skip=used.get(b, 0))
        used[b] = used.get(b, 0) + len(ws)
        put(ws)
        return ws

    fill(ROOT, W_PLUS)
    put([b"+", b"+/t"])
    found.append((b"k00000", [], b"+", KIND_D))
    fill(ROOT, W_HASH)
    put([b"#"])
    found.append((b"#", [], b"#", KIND_D))
    dl = pick(eng, ROOT, 60, 4 * KIND_D + 1, dollar=True)
    put(dl + [dl[-1] + b"/x", dl[-1] + b"/+"])
    found += [(w, [], w, i // 4) for i, w in enumerate(dl)]
    put([b"par"])
    P = Table(eng.debug_slots()).node(eng, [b"par"])
    pool = pool_words()
    x = pool[7]
    fill(P, word_id(eng, x))
    put([b"par/" + x])
    fill(P, W_PLUS)
    put([b"par/+"])
    found += [(b"par/" + x, [b"par"], x, KIND_D), (b"par/" + x, [b"par"], b"+", KIND_D)]
    lv = [b"l%d" % i for i in range(1, 11)]
    put([b"/".join(lv[:9])])
    N9 = Table(eng.debug_slots()).node(eng, lv[:9])
    eng.dict_load([lv[9]])
    if twin is not None:
        twin.dict_load([lv[9]])
    fill(N9, word_id(eng, lv[9]))
    put([b"/".join(lv)])
    found.append((b"/".join(lv), lv[:9], lv[9], KIND_D))
    topics = [b"k00000", b"k00001/t", b"#", b"zz/#", dl[-1], dl[-1] + b"/x", dl[-1] + b"/y", dl[0], dl[8],
              b"$k59999", b"par/" + x, b"par/" + pool[8], b"par", b"/".join(lv), b"/".join(lv[:9] + [pool[9]]),
              b"/".join(lv[:9])]
    return dict(filters=filters, topics=topics, max_probe=8, found=found, absent=[], wrap=[], dollar_last=dl[-1])


def change_world(eng):
    """The step change: 17 keys homed in bucket 100 (displacement 4, max_probe
    4), then four more (the last at 5, max_probe 8), then the first four are
    deleted, which pulls keys of every later bucket one bucket towards home."""
    pool_ids(eng)
    ws = pick(eng, ROOT, 100, 21)
    return dict(first=ws[:17], more=ws[17:], gone=ws[:4], topics=ws + pick(eng, ROOT, 100, 2, skip=21))


def check_world(eng, world):
    """Every property a world claims, read from the dump alone; -> its Table."""
    t = Table(eng.debug_slots())
    assert t.nb == NB, t.nb
    md = t.max_disp()
    assert md == eng.debug_check() and stepped(md) == world["max_probe"], (md, world["max_probe"])
    for topic, path, w, disp in world["found"]:
        parent = t.node(eng, path)
        wid = W_PLUS if w == b"+" else W_HASH if w == b"#" else word_id(eng, w)
        r = t.run(parent, wid, world["max_probe"])
        assert r.found and r.disp == disp and r.reads == disp + 1, (topic, w, disp, r)
        home, at = t.where(parent, wid)
        assert (at - home) % NB == disp
    for w, home, reads in world["absent"]:
        wid = word_id(eng, w)
        assert wid >= 4 and home_bucket(ROOT, wid) == home, w
        r = t.run(ROOT, wid, world["max_probe"])
        assert not r.found and r.reads == reads, (w, reads, r)
    for w in world["wrap"]:
        home, at = t.where(ROOT, word_id(eng, w))
        assert at < home and home >= NB - MAX_PROBE_DISP, (w, home, at)
    return t
