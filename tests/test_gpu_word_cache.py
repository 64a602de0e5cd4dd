"""The learned table of multi-token words (csrc/hutk_wcache.h; k_tiles reads it, k_finish's d_learn fills it): every batch
here is encoded by a context with the table, by one created under HUTK_WORD_CACHE=0, and by the oracle, and the three
must agree id for id -- on the first encode, which learns, and on the later ones, which hit.  The shapes are the smallest
at which each path can go wrong: a batch of more than 32 tiles (30720 bytes) is the smallest that learns.  GPU only."""
import random

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

RARE = b"qxzjkvwy"      # letters whose strings are hardly ever vocabulary keys: every such word goes through the merge loop
LARGE = 32 * 960 + 1    # bytes from which a batch takes the large path (k_finish, which learns)


def rare_word(rng, lo, hi):
    return bytes(rng.choice(RARE) for _ in range(rng.randint(lo, hi)))


def filler(rng, n_bytes, lo=3, hi=12):
    """Distinct-ish merge-loop words, space separated, at least n_bytes of them."""
    out, size = [], 0
    while size < n_bytes:
        out.append(rare_word(rng, lo, hi))
        size += len(out[-1]) + 1
    return b" ".join(out)


def make(vocab="VG", prefix="file", **env):
    """-> a context of `vocab` created under the environment switches `env`."""
    from hutoken_amd import _capi, data
    vp, sp, kw = data.vocab_files(vocab)
    with H.env_switches(**env):
        return _capi.Context(vp, sp, kw["prefix"] if prefix == "file" else prefix, kw["is_byte_encoder"], device=0)


def oracle_for(vocab="VG", prefix="file", pattern=None):
    from hutoken_amd import data
    from oracle import oracle as O
    vp, sp, kw = data.vocab_files(vocab)
    return O.Oracle(vp, sp, kw["prefix"] if prefix == "file" else prefix, kw["is_byte_encoder"], pattern=pattern)


@pytest.fixture(scope="module")
def vg():
    """One context with the table (tests that read its statistics make their own), one without, the oracle."""
    on, off, orc = make(), make(HUTK_WORD_CACHE="0"), oracle_for()
    assert on.word_cache_stats()["capacity"] == 2 << 19 and on.word_cache_stats()["open"]
    assert off.word_cache_stats() == {"entries": 0, "capacity": 0, "appended": 0, "open": False}
    yield on, off, orc
    on.close(), off.close(), orc.close()


def check(ctxs, orc, docs, times=2, tag="", want=None):
    """Every context encodes the batch `times` times; ids and offsets equal the oracle's each time."""
    from oracle import oracle as O
    data, offs = O.pack(docs)
    ids_o, oo_o = want if want is not None else orc.encode_packed(data, offs, 4)[:2]
    for c, ctx in enumerate(ctxs):
        for t in range(times):
            ids, oo, st, rc = ctx.encode_packed(data, offs)
            assert rc == 0, (tag, c, t, rc)
            assert np.array_equal(oo, oo_o), (tag, "offsets", c, t)
            if not np.array_equal(ids, ids_o):
                k = int(np.nonzero(ids != ids_o)[0][0])
                d = int(np.searchsorted(oo_o, k, side="right") - 1)
                raise AssertionError((tag, "ids", c, t, d, docs[d][:120], ids[oo_o[d]:oo_o[d + 1]].tolist()[:40],
                                      ids_o[oo_o[d]:oo_o[d + 1]].tolist()[:40]))
    return ids_o, oo_o


def split_word(w):
    """The word the splitter makes of `w` between two other words: its bytes (a leading space may belong to it)."""
    from oracle import oracle as O
    doc = b"ab " + w + b" ab"
    starts = O.split_words(doc) + [len(doc)]
    for i in range(len(starts) - 1):
        if starts[i] <= 3 < starts[i + 1]:
            assert starts[i + 1] == 3 + len(w), "the splitter cuts the word"
            return doc[starts[i]:starts[i + 1]]
    raise AssertionError("no word")


COMMON = b"etaoinshr"  # letters whose strings merge well: long words of few ids


def word_with(orc, n_bytes=None, n_ids=None, seed=0):
    """A word whose split form has n_bytes bytes and 2 .. 16 ids (common letters: the byte limit alone decides whether it is
    cached), or one of rare letters, at most 30 bytes, whose encoding has n_ids ids.  Both counts by the oracle."""
    from oracle import oracle as O
    rng = random.Random(1000 + seed)
    for _ in range(20000):
        if n_bytes is None:
            w = rare_word(rng, 1, 31)
        else:
            w = bytes(rng.choice(COMMON) for _ in range(rng.randint(max(n_bytes - 1, 1), n_bytes)))
        s = split_word(w)
        if n_bytes is not None and len(s) != n_bytes:
            continue
        if O.split_words(s) != [0]:
            continue
        n = len(orc.encode(s))
        if n < 2 or (n_ids is None and n > 16) or (n_ids is not None and (n != n_ids or len(s) > 30)):
            continue
        return w
    raise AssertionError("no such word: n_bytes=%s n_ids=%s" % (n_bytes, n_ids))


def test_learning_and_hitting():
    from hutoken_amd import synth
    from oracle import oracle as O
    d, o = synth.corpus("C3", 150)
    assert int(o[-1]) >= 40000
    docs = [bytes(d[o[i]:o[i + 1]]) for i in range(len(o) - 1)]
    on, off, orc = make(), make(HUTK_WORD_CACHE="0"), oracle_for()
    assert on.word_cache_stats()["entries"] == 0
    want = check([on], orc, docs, times=1, tag="call 1")
    s1 = on.word_cache_stats()
    assert s1["entries"] > 0 and s1["appended"] >= s1["entries"] and s1["open"], s1
    check([on], orc, docs, times=1, tag="call 2", want=want)
    s2 = on.word_cache_stats()
    assert s2["appended"] == 0, s2       # every cacheable merge-loop word of the batch hit
    assert s2["entries"] == s1["entries"]
    check([on, off], orc, docs, times=1, tag="call 3", want=want)
    assert off.word_cache_stats()["capacity"] == 0
    on.close(), off.close(), orc.close()


def two_byte_word(orc):
    """Two bytes that the splitter takes as a word of their own behind a letter and that are two ids (a two-letter word
    behind a space is three bytes with it, and nearly always one token)."""
    from oracle import oracle as O
    marks = b"!#$%&*+/<=>?@^_`{|}~"
    for a in marks:
        for b in marks:
            s = bytes([a, b])
            doc = b"ab" + s + b" ab"
            starts = O.split_words(doc) + [len(doc)]
            if 2 in starts and 4 in starts and 3 not in starts and O.split_words(s) == [0] and len(orc.encode(s)) == 2:
                return s
    raise AssertionError("no two-byte merge-loop word")


def test_limits_of_key_and_result(vg):
    on, off, orc = vg
    rng = random.Random(5)
    words = [word_with(orc, n_bytes=n, seed=n) for n in (14, 15, 30, 31)]
    words += [word_with(orc, n_ids=n, seed=100 + n) for n in (16, 17)]  # (of at most 30 bytes: the id limit alone decides)
    assert [len(split_word(w)) for w in words[:4]] == [14, 15, 30, 31]
    assert [len(orc.encode(split_word(w))) for w in words[4:]] == [16, 17]
    assert all(len(split_word(w)) <= 30 for w in words[4:])
    words.append(b"a")  # one byte: never a merge-loop word
    body = []
    for w in words:
        body += [w, rare_word(rng, 3, 9), w]
    two = two_byte_word(orc)
    docs = [b" ".join(body), filler(rng, LARGE), b" ".join(reversed(body)), b"ab" + two + b" ab" + two + b" a", two]
    check([on, off], orc, docs, times=2, tag="limits")


def test_position_in_the_tile(vg):
    on, off, orc = vg
    rng = random.Random(6)
    w = word_with(orc, n_bytes=24, seed=24)
    pre = bytearray(filler(rng, 2 * 960)[:2 * 960 - 11])
    pre[-1:] = b"q"
    first = bytes(pre) + b" " + w + b" " + filler(rng, 400)   # w starts 10 bytes in front of a tile's end and ends in its halo
    assert first[2 * 960 - 10:2 * 960 - 10 + len(w)] == w
    docs = [first,
            w,                                       # a document's first and only word
            w + b" " + rare_word(rng, 5, 9) + b" " + w,  # the same bytes at a document start and mid-document
            filler(rng, LARGE),
            rare_word(rng, 4, 8) + b" " + w]         # ... ending at the batch's last byte
    check([on, off], orc, docs, times=2, tag="positions")
    # a byte-mode vocabulary with a prefix: the first word of a document is an exception word, cached bytes or not
    pon, poff, porc = make(prefix="qx"), make(prefix="qx", HUTK_WORD_CACHE="0"), oracle_for(prefix="qx")
    check([pon, poff], porc, docs, times=2, tag="positions, prefix")
    assert pon.word_cache_stats()["entries"] > 0
    pon.close(), poff.close(), porc.close()


def test_tiny_table_fills_closes_and_clears():
    rng = random.Random(7)
    words = list({rare_word(rng, 5, 12) for _ in range(2200)})
    assert len(words) >= 2000
    docs = [b" ".join(words[i:i + 50] * 2) for i in range(0, len(words), 50)]
    assert sum(map(len, docs)) >= LARGE
    tiny, orc = make(HUTK_WORD_CACHE_LOG2="2"), oracle_for()
    assert tiny.word_cache_stats() == {"entries": 0, "capacity": 8, "appended": 0, "open": True}
    want = check([tiny], orc, docs, times=1, tag="tiny 1")
    s = tiny.word_cache_stats()
    assert 0 < s["entries"] <= s["capacity"] == 8 and not s["open"], s
    check([tiny], orc, docs, times=2, tag="tiny 2", want=want)
    s2 = tiny.word_cache_stats()
    assert s2["entries"] == s["entries"] and not s2["open"], s2
    tiny.word_cache_clear()
    assert tiny.word_cache_stats() == {"entries": 0, "capacity": 8, "appended": 0, "open": True}
    check([tiny], orc, docs, times=2, tag="tiny 3", want=want)
    s3 = tiny.word_cache_stats()
    assert 0 < s3["entries"] <= 8, s3
    tiny.close(), orc.close()


def test_two_contexts_keep_their_tables_apart():
    rng = random.Random(8)
    docs = [filler(rng, 700) for _ in range(48)]
    assert sum(map(len, docs)) >= LARGE
    ctxs = {v: (make(v), oracle_for(v)) for v in ("VG", "VC")}
    want = {}
    for turn in range(2):
        for v, (ctx, orc) in ctxs.items():
            want[v] = check([ctx], orc, docs, times=1, tag=v + " turn %d" % turn, want=want.get(v))
    assert not np.array_equal(want["VG"][0], want["VC"][0])  # (the two vocabularies do encode these words differently)
    for v, (ctx, orc) in ctxs.items():
        assert ctx.word_cache_stats()["entries"] > 0
        ctx.close(), orc.close()


def test_small_paths_read_and_do_not_learn():
    rng = random.Random(9)
    words = [rare_word(rng, 4, 14) for _ in range(300)]
    ctx, orc = make(), oracle_for()
    large = [b" ".join(rng.choice(words) for _ in range(60)) for _ in range(70)]
    assert sum(map(len, large)) >= LARGE
    check([ctx], orc, large, times=1, tag="large")
    entries = ctx.word_cache_stats()["entries"]
    assert entries > 0
    sentence = b" ".join(words[:40])                     # one launch (at most four tiles)
    assert len(sentence) <= 4 * 960
    assert ctx.encode_one(sentence)[0] == orc.encode(sentence)
    small = [b" ".join(rng.choice(words) for _ in range(40)) for _ in range(40)]
    assert 4 * 960 < sum(map(len, small)) <= 32 * 960    # k_tail_small
    check([ctx], orc, small, times=2, tag="small")
    assert ctx.exc_counts()["tail"] == 1
    fresh = [b" ".join(rare_word(rng, 4, 14) for _ in range(40)) for _ in range(40)]  # words the table has not seen
    assert sum(map(len, fresh)) <= 32 * 960
    check([ctx], orc, fresh, times=2, tag="small, new words")
    assert ctx.word_cache_stats()["entries"] == entries
    ctx.close(), orc.close()


def test_regex_path_split_preset_and_a_context_without_the_table():
    import importlib
    import presplit_ref as R
    PT = importlib.import_module("hutoken_amd.pretokenize")
    from oracle import oracle as O
    rng = random.Random(10)
    words = [rare_word(rng, 4, 14) for _ in range(400)]
    docs = [b" ".join(rng.choice(words) for _ in range(60)) + b" 12 !" for _ in range(70)]
    assert sum(map(len, docs)) >= LARGE
    # regex pre-token path
    ctx, orc = make(), oracle_for(pattern="[a-z]+")
    ctx.set_pattern("[a-z]+")
    check([ctx], orc, docs, times=2, tag="regex")
    assert ctx.word_cache_stats()["entries"] > 0
    ctx.set_pattern(None)
    orc.close()
    # a split preset: the oracle's ids of the restatement's words, each as a document of its own
    ctx.set_pretokenizer(PT.preset_index("gpt2"), PT.table_blob())
    whole = oracle_for(pattern="(.|\n)+")
    ws = [[w.encode("utf-8") for w in R.words(d.decode("ascii"), "gpt2")] for d in docs]
    flat = [w for row in ws for w in row]
    fd, fo = O.pack(flat)
    fids, foo, _ = whole.encode_packed(fd, fo, 4)
    bounds = np.cumsum([0] + [len(row) for row in ws])
    want = (fids, foo[bounds].astype(np.int64))
    check([ctx], None, docs, times=2, tag="preset", want=want)
    ctx.close(), whole.close()
    # VL (not a byte encoder): no table, and the batch as before
    vl, vorc = make("VL"), oracle_for("VL")
    assert vl.word_cache_stats() == {"entries": 0, "capacity": 0, "appended": 0, "open": False}
    vl.word_cache_clear()
    check([vl], vorc, docs, times=2, tag="VL")
    assert vl.word_cache_stats()["capacity"] == 0
    vl.close(), vorc.close()
