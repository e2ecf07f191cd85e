"""Long and prefix-sharing words through the host interner and tokeniser
(tm_tokenize on a host-only engine): words of 1 to 1,000 bytes, families of
equal-length words that share their first 8 to 36 bytes, subscribed and not.
Every subscribed word keeps one id of its own, every other word is unknown,
and the layout follows emqx_topic:words/1 (src/emqx_topic.erl:150-164) --
also while the host table rehashes with long words in it.  The model of the
device's dictionary mirror (long_words.py) is held to its floors here too, so
that the device tests' inputs are known to bite before a GPU is involved."""

import long_words as LW
from emqx_amd.engine import Engine


def test_model_floors_and_probe_alignments():
    u, k = LW.assert_floors()
    assert u["words"] == k["words"] == len(LW.known_words()) + 1 and u["slots"] == 16384
    for batch in (LW.lds_batch(), LW.global_batch(), LW.mixed_batch()):
        batch.assert_every_alignment()


def test_model_hash_is_the_murmur3_32_of_the_padded_word():
    """hash_word restated from its definition (murmur3's 32-bit steps over the
    zero-padded little-endian dwords, the length mixed in last, | 1): the
    empty string's murmur3_32 with seed 0 is 0, so only the | 1 is left; a
    word and the same word zero-padded to the next dword differ in the length
    alone."""
    assert LW.hash_word(b"", 0) == 1
    h, n = LW.HW_SEED, 5
    for d in (int.from_bytes(b"abcd", "little"), ord("e")):
        h = LW.hw_acc(h, LW.mix_chunk(d))
    assert LW.hash_word(b"abcde", LW.HW_SEED) == LW.hw_final(h, n)
    assert LW.hash_word(b"abcde\0\0\0", LW.HW_SEED) == LW.hw_final(h, 8)
    assert LW.hash_word(b"abcde", LW.HW_SEED) != LW.hash_word(b"abcde", LW.HW_SEED2)


def test_host_tokens_of_long_and_prefix_sharing_words():
    eng = Engine(device=-1)
    for f in LW.all_filters():
        eng.insert(f)
    known = set(LW.dictionary_order())
    P = LW.mixed_batch()                      # (with b"" topics among the probes)
    ids = LW.check_tokens(eng.tokenize(P.topics), P.topics, known)
    assert set(ids) == known
    # the ids are the interning order's (the model's ids name the device's tails)
    d = LW.DictModel()
    for f in LW.all_filters():
        d.insert(f)
    assert ids == d.ids


def test_host_tokens_while_the_table_rehashes():
    eng = Engine(device=-1)
    eng.insert(b"#")
    words = LW.known_words()
    P = LW.lds_batch()
    steps = LW.step_bounds(len(words))
    for lo, hi in zip([0] + steps, steps):
        for f in LW.filters_of(words[lo:hi]):
            eng.insert(f)
        known = set(words[:hi]) | {b"f"}
        ids = LW.check_tokens(eng.tokenize(P.topics), P.topics, known)
        assert set(ids) == known
    # (the host table of 1,024 entries doubled at 512, 1,024 and 2,048 words)
    assert len(words) > 2048
