"""Shared inputs of the long-word tests (test_long_words.py on the host engine,
test_gpu_long_words.py on the device): words of 9 to 1,000 bytes, most of them
in families of equal length that share their first 8, 12, 16, 24 or 36 bytes,
so that the dictionary mirror's second and third comparison stages (bytes 8-15
in the tail record, bytes 16 and up in the arena) decide lookups; a plain
Python model of the mirror (the word hash with both seeds, the host table, the
cuckoo table and its rebuilds) that counts how often they do; and the
tokeniser's tile rule, to build batches whose tiles take the path a test means
them to take."""

import numpy as np

from emqx_amd import emqx_topic as T
from kernel_model import FAST_MAX_DEPTH, word_class

# ---- words -------------------------------------------------------------------
N_FAMILY = 1500
FAMILIES = [(8, 4), (12, 4), (16, 4), (24, 5), (36, 4)]   # (prefix bytes, digits)
LADDER = range(1, 41)
VERY_LONG = (100, 255, 1000)


def family(plen, width):
    prefix = (b"p%02d-" % plen + b"abcdefghijklmnopqrstuvwxyz0123456789")[:plen]
    return [prefix + b"%0*d" % (width, i) for i in range(N_FAMILY)]


FAMILY_WORDS = [family(p, w) for p, w in FAMILIES]


def ladder_word(n, known):
    return ((b"K" if known else b"U") + b"lenword-" * 6)[:n]


def very_long_word(n, known):
    return (b"verylong-" * 112)[:n - 1] + (b"k" if known else b"u")


def known_words():
    """Every subscribed word, in the order the dictionary is filled: the
    families side by side (even members), the ladder, the very long words."""
    out = [fam[i] for i in range(0, N_FAMILY, 2) for fam in FAMILY_WORDS]
    out += [ladder_word(n, True) for n in LADDER]
    out += [very_long_word(n, True) for n in VERY_LONG]
    return out


def unknown_words():
    out = [fam[i] for i in range(1, N_FAMILY, 2) for fam in FAMILY_WORDS]
    out += [ladder_word(n, False) for n in LADDER]
    out += [very_long_word(n, False) for n in VERY_LONG]
    return out


def filters_of(words):
    return [f for w in words for f in (b"f/" + w + b"/#", b"+/" + w)]


def all_filters():
    return filters_of(known_words()) + [b"#"]


# ---- topics ------------------------------------------------------------------
class Probes:
    """An ordered batch of probe topics: topics[i] ends in the probed word
    word[i] (None for a b"" topic), which is subscribed iff known[i]."""

    def __init__(self):
        self.topics, self.word, self.known = [], [], []
        self.nbytes = 0

    def add(self, topic, word, known):
        self.topics.append(topic)
        self.word.append(word)
        self.known.append(known)
        self.nbytes += len(topic)

    def offsets(self):
        return np.concatenate([[0], np.cumsum([len(t) for t in self.topics], dtype=np.int64)])

    def word_starts(self):
        """[(word, byte offset of the word in the packed batch)]"""
        o = self.offsets()
        return [(w, int(o[i + 1]) - len(w)) for i, w in enumerate(self.word) if w is not None]

    def assert_every_alignment(self):
        """Every start offset mod 16 occurs for every family and for every
        ladder length from 9 up (the tokeniser reads words from a 16-byte
        aligned window in 4- and 8-byte pieces)."""
        seen = {}
        for w, s in self.word_starts():
            seen.setdefault(len(w), set()).add(s % 16)
        lengths = [p + w for p, w in FAMILIES] + [n for n in LADDER if n >= 9]
        short = {n: sorted(set(range(16)) - seen.get(n, set())) for n in lengths}
        assert not any(short.values()), {n: r for n, r in short.items() if r}


def base_probes():
    """f/<W> and <filler>/<W> for every known and unknown word, filler =
    b"x" * k with k cycling through 1..16.  The families are dealt side by
    side so that any 64 consecutive topics have about the average length; one
    ladder topic follows every ten family topics, each ladder word under
    all 16 fillers, taken in the order that puts its start on each offset
    mod 16 in turn; the very long words stand far apart."""
    P = Probes()
    kw, uw = set(known_words()), unknown_words()
    ladder = []   # (word, residue of its start, or None for f/<W>)
    for j in range(len(LADDER)):
        n = j // 2 + 1 if j % 2 == 0 else len(LADDER) - j // 2   # 1, 40, 2, 39, ...: long beside short
        for known in (True, False):
            w = ladder_word(n, known)
            ladder += [(w, None)] + [(w, r) for r in range(16)]
    far = {100 + 50 * j: (very_long_word(n, known), form)   # (no two of them in one tile's window)
           for j, (n, known, form) in enumerate((n, k, f) for n in VERY_LONG for k in (True, False) for f in (0, 1))}
    k = 0
    for i in range(N_FAMILY):
        for fam in FAMILY_WORDS:
            w = fam[i]
            k = k % 16 + 1
            P.add(b"f/" + w, w, w in kw)
            P.add(b"x" * k + b"/" + w, w, w in kw)
        if i < len(ladder):
            w, r = ladder[i]
            if r is None:
                P.add(b"f/" + w, w, w in kw)
            else:
                fill = (r - P.nbytes - 1) % 16 or 16   # start = nbytes + fill + 1 = r (mod 16)
                P.add(b"x" * fill + b"/" + w, w, w in kw)
        if i in far:
            w, form = far[i]
            k = k % 16 + 1
            P.add(b"x" * k + b"/" + w if form else b"f/" + w, w, w in kw)
    assert len(ladder) <= N_FAMILY and {w for w in P.word} == kw | set(uw)
    return P


def with_empties(P, pick=lambda chunk: True, chunk=192):
    """The same probes with one b"" opening every aligned group of four
    topics, in the chunks (of `chunk` probes: 3 tiles of 64 as they are, 4
    with the empties) that `pick` selects.  Empty topics have no bytes: every
    word keeps its offset."""
    Q = Probes()
    for c in range(0, len(P.topics), chunk):
        hole = pick(c // chunk)
        for i in range(c, min(c + chunk, len(P.topics))):
            if hole and len(Q.topics) % 4 == 0:
                Q.add(b"", None, False)
            Q.add(P.topics[i], P.word[i], P.known[i])
    return Q


# ---- the tokeniser's tile rule -------------------------------------------------
TILE = 64
TOK_BYTES = 64 * 48     # LDS window of a tile, from its 16-byte aligned start
TOK_WORDS = 512         # words of a tile on the LDS path


def tok_tile_topics(n, nbytes):
    tt = TILE
    while tt > 1 and tt * nbytes > (TOK_BYTES * 3 // 4) * (n or 1):
        tt >>= 1
    while tt > 4 and (n + tt - 1) // tt < 32:
        tt >>= 1
    return tt


def tile_paths(topics):
    """-> (topics per tile, [the tile takes the LDS path])"""
    n = len(topics)
    offs = np.concatenate([[0], np.cumsum([len(t) for t in topics], dtype=np.int64)])
    tt = tok_tile_topics(n, int(offs[-1]))
    lds = []
    for t0 in range(0, n, tt):
        t1 = min(t0 + tt, n)
        window = int(offs[t1]) - (int(offs[t0]) & ~15)
        words = sum(t.count(b"/") + 1 for t in topics[t0:t1])
        lds.append(window <= TOK_BYTES and all(topics[t0:t1]) and words <= TOK_WORDS)
    return tt, lds


def lds_batch():
    P = base_probes()
    tt, lds = tile_paths(P.topics)
    assert tt == TILE and all(lds), (tt, [i for i, x in enumerate(lds) if not x][:5])
    return P


def global_batch():
    P = with_empties(base_probes())
    tt, lds = tile_paths(P.topics)
    assert tt == TILE and not any(lds)
    return P


def mixed_batch():
    P = with_empties(base_probes(), pick=lambda c: c % 2 == 1)
    tt, lds = tile_paths(P.topics)
    # three tiles on the LDS path, then four on the other one, and so on: a
    # tile leaves the LDS path for its empty topics only
    assert tt == TILE and lds[:14] == ([True] * 3 + [False] * 4) * 2
    assert lds == [all(P.topics[t:t + TILE]) for t in range(0, len(P.topics), TILE)]
    assert 3 * sum(lds) > len(lds) and 3 * (len(lds) - sum(lds)) > len(lds)
    return P


# ---- expected tokens -----------------------------------------------------------
W_UNKNOWN, W_EMPTY, W_PLUS, W_HASH, W_FIRST = 0, 1, 2, 3, 4
WID_BITS = 29
WID_MASK = (1 << WID_BITS) - 1
TF_DOLLAR, TF_SLOW = 1, 2


def expected_layout(topics):
    """emqx_topic:words/1 plus the class rule -> (words of every topic as
    [(class, word or atom)], toff, tflags)"""
    rows, toff, flags = [], [0], []
    for t in topics:
        ws = T.words(t)
        irregular = False
        row = []
        for w in ws:
            cls, irr = word_class(b"" if w is T.EMPTY else b"+" if w is T.PLUS else b"#" if w is T.HASH else w)
            irregular |= irr
            row.append((cls, w))
        rows.append(row)
        toff.append(toff[-1] + len(ws))
        flags.append((TF_DOLLAR if t[:1] == b"$" else 0) | (TF_SLOW if irregular or len(ws) > FAST_MAX_DEPTH else 0))
    return rows, np.array(toff, np.uint32), np.array(flags, np.uint8)


def check_tokens(tok, topics, known):
    """The host tokeniser's output on `topics`: layout as expected_layout, atoms
    their reserved ids, every word of `known` one id of its own (>= W_FIRST),
    every other word W_UNKNOWN.  -> {word: id}"""
    rows, toff, flags = expected_layout(topics)
    assert np.array_equal(tok.toff, toff) and np.array_equal(tok.tflags, flags)
    assert len(tok.words) == int(toff[-1])
    ids = {}
    flat = [e for row in rows for e in row]
    for (cls, w), e in zip(flat, tok.words.tolist()):
        assert e >> WID_BITS == cls, (w, e)
        wid = e & WID_MASK
        if w is T.EMPTY or w is T.PLUS or w is T.HASH:
            assert wid == {T.EMPTY: W_EMPTY, T.PLUS: W_PLUS, T.HASH: W_HASH}[w]
        elif w in known:
            assert wid >= W_FIRST and ids.setdefault(w, wid) == wid, (w, wid)
        else:
            assert wid == W_UNKNOWN, (w, wid)
    assert len(set(ids.values())) == len(ids)
    return ids


# ---- model of the dictionary mirror --------------------------------------------
M32 = 0xFFFFFFFF
HW_SEED, HW_SEED2 = 0x9E3779B9, 0x7F4A7C15


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def mix_chunk(d):
    return (_rotl((d * 0xCC9E2D51) & M32, 15) * 0x1B873593) & M32


def hw_acc(h, mixed):
    return (_rotl(h ^ mixed, 13) * 5 + 0xE6546B64) & M32


def hw_final(h, n):
    h ^= n
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return (h ^ (h >> 16)) | 1


def hash_word(w, seed):
    h = seed
    for i in range(0, len(w), 4):
        h = hw_acc(h, mix_chunk(int.from_bytes(w[i:i + 4], "little")))
    return hw_final(h, len(w))


class DictModel:
    """WordDict restated: the host's open-addressed table (its slot order is
    the order a cuckoo rebuild reinserts in), the 2-choice cuckoo table at load
    <= 1/4 with its random walk of evictions, the arena's size."""

    def __init__(self):
        self.tab = [None] * 1024
        self.ck = [None] * 1024
        self.ids, self.h = {}, {}
        self.arena = 0
        self.rebuilds = 0          # after the constructor's

    def hashes(self, w):
        if w not in self.h:
            self.h[w] = (hash_word(w, HW_SEED), hash_word(w, HW_SEED2))
        return self.h[w]

    def _tab_put(self, w):
        m = len(self.tab) - 1
        i = self.hashes(w)[0] & m
        while self.tab[i] is not None:
            i = (i + 1) & m
        self.tab[i] = w

    def _ck_put(self, k):
        m = len(self.ck) - 1
        frm = None
        for _ in range(512):
            h1, h2 = self.hashes(k)
            a, b = h1 & m, h2 & m
            i = a if self.ck[a] is None else b if self.ck[b] is None else (a if a != frm else b)
            k, self.ck[i] = self.ck[i], k
            if k is None:
                return True
            frm = i
        return False

    def _ck_rebuild(self, cap):
        while True:
            self.ck = [None] * cap
            if all(self._ck_put(w) for w in self.tab if w is not None):
                break
            cap *= 2
        self.rebuilds += 1

    def intern(self, w):
        if w in self.ids:
            return self.ids[w]
        if (len(self.ids) + 1) * 2 > len(self.tab):
            old, self.tab = self.tab, [None] * (2 * len(self.tab))
            for o in old:
                if o is not None:
                    self._tab_put(o)
        self._tab_put(w)
        self.ids[w] = W_FIRST + len(self.ids)
        self.arena += len(w)
        if len(self.ids) * 4 > len(self.ck) or not self._ck_put(w):
            self._ck_rebuild(2 * len(self.ck))
        return self.ids[w]

    def insert(self, flt):
        for w in flt.split(b"/"):
            if w not in (b"", b"+", b"#"):
                self.intern(w)

    def probed(self, w):
        """the occupants of the slots the device's lookup of w reads: the
        primary slot, and the alternate one unless the primary is empty or
        holds w"""
        m = len(self.ck) - 1
        h1, h2 = self.hashes(w)
        o = self.ck[h1 & m]
        if o is None or o == w:
            return [o]
        return [o, self.ck[h2 & m]]


def near_misses(known_in_order, probes):
    """Over the lookups of `probes` in a dictionary filled with the words of
    known_in_order: how often a probed slot holds a DIFFERENT word of equal
    length and equal first 8 bytes (head_eq: only bytes 8 and up can reject
    it), and how often that word also agrees on bytes 8-15 (head2_eq: only
    the arena can)."""
    d = DictModel()
    for w in known_in_order:
        d.intern(w)
    head_eq = head2_eq = 0
    for w in probes:
        for o in d.probed(w):
            if o is not None and o != w and len(o) == len(w) and o[:8] == w[:8]:
                head_eq += 1
                head2_eq += o[8:16] == w[8:16]
    return {"head_eq": head_eq, "head2_eq": head2_eq, "words": len(d.ids), "slots": len(d.ck)}


def dictionary_order():
    """the words of all_filters() in interning order"""
    return [b"f"] + known_words()


def assert_floors():
    """From the model alone: the probes meet enough near misses for a lookup
    that skipped the second or the third comparison stage to show.  (Of a
    family's 750 subscribed words, the one in a probed slot is another member
    about as often as the table's load, 1/4, times the family's share, 1/5.)"""
    P = base_probes()
    kn = [w for w, k in zip(P.word, P.known) if k]
    un = [w for w, k in zip(P.word, P.known) if not k]
    u, k = near_misses(dictionary_order(), un), near_misses(dictionary_order(), kn)
    assert u["head_eq"] >= 200 and u["head2_eq"] >= 100, u
    assert k["head_eq"] >= 100 and k["head2_eq"] >= 50, k
    return u, k


# ---- subscribing in steps --------------------------------------------------------
STEPS = 12


def step_bounds(n, ratio=1.5):
    """Ends of 12 steps over n words, each step half again as many words as
    all before it: the arena outgrows a block sized need * 1.25 at nearly
    every step, the cuckoo table (which doubles) at every other one -- so
    steps with a rebuilt table and steps with a delta of dirty slots both
    occur."""
    return [max(j + 1, round(n / ratio ** (STEPS - 1 - j))) for j in range(STEPS)]


def step_model(words, bounds):
    """-> (cuckoo rebuilds, [arena bytes after each step]) of a dictionary
    that interns the filters of words[: bounds[j]] step by step"""
    d = DictModel()
    arena = []
    for lo, hi in zip([0] + bounds, bounds):
        for f in filters_of(words[lo:hi]):
            d.insert(f)
        arena.append(d.arena)
    return d.rebuilds, arena


# ---- DevBuf::reserve restated ----------------------------------------------------
def regrowths(sizes, min_cap=1024):
    """How often a device buffer that must hold size + 1 elements at each of
    `sizes` in turn is allocated anew: a block too small is replaced by one of
    need + need / 4 elements (min_cap at least) and filled again from 0."""
    cap = count = 0
    for s in sizes:
        if cap < s + 1:
            cap = max((s + 1) + (s + 1) // 4, min_cap)
            count += 1
    return count
