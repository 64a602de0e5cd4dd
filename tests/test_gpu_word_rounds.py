"""k_tiles' word rounds (csrc/hutk_kernels.hip, phase 5) on the automaton path: one-byte words are resolved by the lane that
owns the byte, words of 2 .. 14 bytes go through rounds of their own, everything else through the general rounds.  Every
batch is encoded by a context with the word cache, by one created under HUTK_WORD_CACHE=0, and by the oracle; every id
and every offset must be equal (integer work: no tolerance), on the first encode and on the second, which hits the cache.

Batches have 40 tiles of 960 bytes: more than the 32 of the small-batch tail, far fewer than the persistent kernel asks
for, so the default kernel runs (asserted through hutk_debug_tile_kernel).  The shapes sit in the first tiles, where their
byte positions are known: a lane owns 16 positions, a round takes 64 words, the whole-word table's key is 14 bytes and
the companion table's 28.  What the splitter makes of each batch is asserted on the host first (oracle.split_words), so
that a shape which the splitter cuts differently cannot pass for the shape it was meant to be.  GPU only."""
import random

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

TILE = 960
N_TILES = 40
COMMON = b"etaoinshr"  # letters whose strings are often vocabulary keys: table hits and merge-loop words mixed
NL = b"\n"             # a word of its own wherever it stands (asserted in layout())


def make(vocab="VG", **env):
    from hutoken_amd import _capi, data
    vp, sp, kw = data.vocab_files(vocab)
    with H.env_switches(**env):
        return _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=0)


def oracle_for(vocab="VG", pattern=None):
    from hutoken_amd import data
    from oracle import oracle as O
    vp, sp, kw = data.vocab_files(vocab)
    return O.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"], pattern=pattern)


@pytest.fixture(scope="module")
def vg():
    on, off, orc = make(), make(HUTK_WORD_CACHE="0"), oracle_for()
    assert on.word_cache_stats()["capacity"] > 0 and off.word_cache_stats()["capacity"] == 0
    yield on, off, orc
    on.close(), off.close(), orc.close()


@pytest.fixture(scope="module")
def vl():
    ctx, orc = make("VL"), oracle_for("VL")
    yield ctx, orc
    ctx.close(), orc.close()


@pytest.fixture(scope="module")
def vg_regex():
    ctx, orc = make(), oracle_for(pattern="[a-z]+")
    ctx.set_pattern("[a-z]+")
    yield ctx, orc
    ctx.close(), orc.close()


# ---- inputs -------------------------------------------------------------------------------------------------

def word(rng, n):
    """A word of n >= 2 bytes as the splitter sees it between others: a space and n - 1 letters."""
    return b" " + bytes(rng.choice(COMMON) for _ in range(n - 1))


def join(rng, lengths):
    """Words of exactly these lengths back to back; 1 = a newline."""
    return b"".join(NL if n == 1 else word(rng, n) for n in lengths)


def filler(rng, n_bytes):
    """Exactly n_bytes of ordinary words (2 .. 12 bytes, now and then a newline or a longer one)."""
    lengths, left = [], n_bytes
    while left:
        n = rng.choice([1, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 8, 9, 10, 12, 17])
        if n > left or left - n == 1:  # (a word has a space and a letter: never leave one byte over)
            n = left if left <= 17 else 2
        lengths.append(n)
        left -= n
    return join(rng, lengths)


def batch(rng, head, total=N_TILES * TILE):
    """head, then filler up to `total` bytes, as one blob."""
    assert len(head) <= total
    return head + filler(rng, total - len(head))


def cut(blob):
    """The blob as documents of 2000 bytes (the cuts fall anywhere: a document's end ends a word)."""
    return [blob[a:a + 2000] for a in range(0, len(blob), 2000)]


def layout(docs):
    """-> (batch positions of the word starts, length of the word at each): what the splitter makes of the documents."""
    from oracle import oracle as O
    starts, base = [], 0
    for d in docs:
        starts += [base + s for s in O.split_words(d)] if d else []
        base += len(d)
    ends = starts[1:] + [base]
    bounds = set(np.cumsum([len(d) for d in docs]).tolist())
    lens = {}
    for s, e in zip(starts, ends):
        nxt = min([b for b in bounds if s < b <= e] + [e])  # (a word ends with its document)
        lens[s] = nxt - s
    return lens


def check(ctxs, orc, docs, tag, times=2):
    from oracle import oracle as O
    data, offs = O.pack(docs)
    nb = int(offs[-1])
    assert nb > 32 * TILE, "the small-batch tail would take it"
    ids_o, oo_o = orc.encode_packed(data, offs, 4)[:2]
    for c, ctx in enumerate(ctxs):
        assert ctx.tile_kernel(nb) == 0, "not k_tiles"
        for t in range(times):
            ids, oo, st, rc = ctx.encode_packed(data, offs)
            assert rc == 0, (tag, c, t, rc)
            assert np.array_equal(oo, oo_o), (tag, "offsets", c, t)
            if not np.array_equal(ids, ids_o):
                k = int(np.nonzero(ids != ids_o)[0][0])
                d = int(np.searchsorted(oo_o, k, side="right") - 1)
                raise AssertionError((tag, "ids", c, t, d, docs[d][:120], ids[oo_o[d]:oo_o[d + 1]].tolist()[:40],
                                      ids_o[oo_o[d]:oo_o[d + 1]].tolist()[:40]))


def plant(blob, positions):
    """Newlines at the given positions of the blob."""
    b = bytearray(blob)
    for p in positions:
        b[p] = NL[0]
    return bytes(b)


def in_tile(lens, t):
    """Lengths of the words that start in tile t."""
    return [n for s, n in lens.items() if t * TILE <= s < (t + 1) * TILE]


def round_tile(rng, n_short, n_one):
    """960 bytes: exactly n_short words of 2 .. 14 bytes, n_one one-byte words, and words of 20 .. 27 bytes for the rest."""
    lengths = [rng.randint(2, 5 if n_short > 100 else 12) for _ in range(n_short)] + [1] * n_one
    left = TILE - sum(lengths)
    assert left >= 0
    while left >= 40:
        lengths.append(20)
        left -= 20
    if left >= 20:
        lengths.append(left)  # 20 .. 39: beyond the table key
        left = 0
    i = 0
    while left:  # a few bytes over: lengthen short words that stay short
        if 2 <= lengths[i] < 14:
            lengths[i] += 1
            left -= 1
        i = (i + 1) % n_short
    rng.shuffle(lengths)
    assert sum(lengths) == TILE
    return join(rng, lengths)


# ---- the shapes ---------------------------------------------------------------------------------------------

def shapes():
    """name -> documents.  Made once; the oracle's view of each is asserted here."""
    from oracle import oracle as O
    rng = random.Random(20)
    out = {}

    singles = [b for b in range(1, 128) if O.split_words(bytes([b]) * 4) == [0, 1, 2, 3]]
    assert NL[0] in singles and len(singles) >= 3
    run = bytes(rng.choice(singles) for _ in range(2 * TILE + 7))
    docs = cut(batch(rng, run))
    lens = layout(docs)
    assert all(lens.get(p) == 1 for p in range(2 * TILE + 7)), "every byte of the first two tiles is a word"
    out["nothing but one-byte words"] = docs

    edge = [16 * l + 15 for l in (0, 1, 7, 30, 58, 59)] + [16 * l for l in (1, 2, 8, 31, 59)]
    edge += [TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, TILE + 16 * 20 + 15, TILE + 16 * 21]
    docs = cut(plant(batch(rng, b""), edge))
    lens = layout(docs)
    assert all(lens.get(p) == 1 for p in edge), "one-byte words at lane and tile edges"
    out["one-byte words at lane and tile edges"] = docs

    blob = batch(rng, b"")
    starts = sorted(layout([blob]))
    at = [s for s in starts if 100 < s < 3 * TILE][::9]
    cuts = []
    blob = bytearray(blob)
    for s in at[:12]:  # a one-byte document, then an empty one
        blob[s] = ord("a")
        cuts += [s, s + 1]
    marks = [0] + sorted(set(cuts)) + [len(blob)]
    full = []
    for a, b in zip(marks[:-1], marks[1:]):
        full.append(bytes(blob[a:b]))
        if b - a == 1:
            full.append(b"")
    assert sum(len(d) == 1 for d in full) == 12 and sum(len(d) == 0 for d in full) == 12
    out["one-byte document followed by an empty one"] = full

    for n_short in (64, 65, 128, 129):
        for n_one in (0, 1):
            head = filler(rng, TILE) + round_tile(rng, n_short, n_one)
            docs = cut(batch(rng, head))
            got = in_tile(layout(docs), 1)
            assert sum(2 <= n <= 14 for n in got) == n_short and sum(n == 1 for n in got) == n_one, (n_short, n_one)
            out["%d short words and %d one-byte words in a tile" % (n_short, n_one)] = docs

    real = [b" international", b" administration", b" responsibility", b" representatives", b" recommendations",
            b" telecommunications", b" characteristics", b" congratulations"]
    head = b"".join(real) + join(rng, [14, 15, 14, 15, 13, 16, 28, 29, 28, 29, 27, 30, 14, 15, 28, 29]) + b"".join(real)
    docs = cut(batch(rng, head))
    got = in_tile(layout(docs), 0)
    assert all(got.count(n) >= 2 for n in (14, 15, 28, 29))
    out["words of 14, 15, 28 and 29 bytes"] = docs

    head = filler(rng, TILE - 5) + join(rng, [12]) + filler(rng, TILE - 7 - 3) + join(rng, [70]) + filler(rng, 100)
    docs = cut(batch(rng, head, total=N_TILES * TILE - 7) + join(rng, [7]))
    lens = layout(docs)
    assert lens[TILE - 5] == 12, "a short word runs into the halo"
    assert lens[2 * TILE - 3] == 70, "a word of 70 bytes starts in the tile"
    assert lens[N_TILES * TILE - 7] == 7, "a short word starts in the last 16 bytes of the batch"
    out["short word into the halo, 70-byte word, short word at the end of the batch"] = docs

    docs = []
    for i in range(40):  # 17 = 1 (mod 16): the documents start at every offset of a lane
        docs.append(join(rng, [5, 6, 6]) if i % 2 else join(rng, [5, 6, 6])[1:] + b"e")
        assert len(docs[-1]) == 17
    docs += cut(filler(rng, N_TILES * TILE - 17 * 40))
    assert {sum(map(len, docs[:i])) % 16 for i in range(40)} == set(range(16))
    out["documents at every offset of a lane, with and without a leading space"] = docs

    docs = cut(batch(rng, b"", total=N_TILES * TILE) + b"e")
    assert sum(map(len, docs)) % TILE == 1
    out["last tile of one byte"] = docs
    return out


_shapes = None


def shape(name):
    global _shapes
    if _shapes is None:
        _shapes = shapes()
    return _shapes[name]


NAMES = ["nothing but one-byte words", "one-byte words at lane and tile edges",
         "one-byte document followed by an empty one"] + \
        ["%d short words and %d one-byte words in a tile" % (s, o) for s in (64, 65, 128, 129) for o in (0, 1)] + \
        ["words of 14, 15, 28 and 29 bytes", "short word into the halo, 70-byte word, short word at the end of the batch",
         "documents at every offset of a lane, with and without a leading space", "last tile of one byte"]


@pytest.mark.parametrize("name", NAMES)
def test_byte_mode_with_and_without_the_word_cache(vg, name):
    on, off, orc = vg
    check([on, off], orc, shape(name), name)


@pytest.mark.parametrize("name", ["one-byte words at lane and tile edges",
                                  "documents at every offset of a lane, with and without a leading space"])
def test_non_byte_mode_with_a_prefix_keeps_the_general_rounds(vl, name):
    ctx, orc = vl
    check([ctx], orc, shape(name), "VL: " + name)


@pytest.mark.parametrize("name", ["one-byte words at lane and tile edges", "65 short words and 1 one-byte words in a tile"])
def test_regex_path_keeps_the_general_rounds(vg_regex, name):
    ctx, orc = vg_regex
    check([ctx], orc, shape(name), "regex: " + name)


def test_every_shape_is_named():
    assert sorted(NAMES) == sorted(shapes())
