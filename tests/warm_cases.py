"""Inputs of tests/test_gpu_warm_context.py (checked without a GPU by tests/test_warm_cases_cpu.py), seeded.

A byte-encoder context keeps a learned table of multi-token words (csrc/hutk_wcache.h): the first batch of more than 32
tiles lists the words its merge loop finished, k_finish's d_learn puts them into the table, and every later call reads
it.  The builders here make the batches that meet a WARM table on every encode path, and the one batch large enough to
overflow the candidate list.  Every planted word is a string of letters with a leading space (what the splitter makes
of a word between others), so that the same bytes are the same key wherever they stand.

The restatements are plain Python and numpy: which sub-list a word's workgroup appends to (k_tiles: the XCD-aware block
order and `blockIdx.x & (LIST_SHARDS - 1)`), a tile's pending words (the merge-loop words phase 6a deals to the lanes),
and a word's place relative to a tile edge.  Constants restated from the headers are named with their header;
tests/test_warm_cases_cpu.py reads the headers and compares."""
import random

import numpy as np

TILE = 960                      # csrc/hutk_device.h TILE_BYTES
TILE_WAVES = 4                  # csrc/hutk_kernels.hip: tiles (= wavefronts) per workgroup of k_tiles
GROUP = TILE * TILE_WAVES       # bytes of one workgroup
SMALL_TILES, ONE_TILES = 32, 4  # up to 32 tiles: k_tail_small (reads the table, never learns); up to 4: the one-launch form
LARGE = SMALL_TILES * TILE + 1  # bytes from which a batch takes k_finish, which learns
LANE_MAX_BYTES = 63             # csrc/hutk_device.h: longer words are exception words
# csrc/hutk_wcache.h
KEY_BYTES, MIN_BYTES, MAX_IDS = 30, 2, 16
LIST_CAP, LIST_SHARDS = 1 << 20, 256
SHARD_CAP = LIST_CAP // LIST_SHARDS
ROUND = 64                      # words phase 6a probes per trip of its r0 loop (a lane each)

RARE = b"qxzjkvwy"    # letters whose strings are hardly ever vocabulary keys: merge-loop words of about an id per byte
COMMON = b"etaoinshr"  # letters whose strings merge well: long words of few ids
EOT, EOT_ID = b"<|endoftext|>", 50256  # GPT-2's marker and its id (the VG vocabulary)

_made = {}


def _once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def pack(docs):
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(d) for d in docs], out=offs[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), offs


# ---- words --------------------------------------------------------------------------------------------------------------
def pool_words(seed, n, lo, hi, letters=RARE):
    """n distinct words of lo .. hi bytes: a space and letters."""
    rng = random.Random(seed)
    seen, out = set(), []
    while len(out) < n:
        w = b" " + bytes(rng.choice(letters) for _ in range(rng.randint(lo, hi) - 1))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def id_counts(orc, words):
    """The oracle's number of ids of every word, each as a document of its own (a word's ids do not depend on where it
    stands, except for a prefix).  One id: the word is in the whole-word table's domain (build_word_table keeps the
    vocabulary keys that encode to themselves); two or more: it needs the merge loop."""
    data, offs = pack(list(words))
    _ids, oo, _st = orc.encode_packed(data, offs, 4)
    return np.diff(np.asarray(oo)).tolist()


def is_one_word(w):
    """Is `w` exactly one word for the splitter between two other words?"""
    from oracle import oracle as O
    doc = b"ab" + w + b" ab"
    starts = O.split_words(doc) + [len(doc)]
    lo, hi = 2, 2 + len(w)
    return lo in starts and hi in starts and not any(lo < s < hi for s in starts)


def cacheable(n_bytes, n_ids):
    """wc::cacheable for a merge-loop word (two ids or more)"""
    return MIN_BYTES <= n_bytes <= KEY_BYTES and 2 <= n_ids <= MAX_IDS


def find_words(orc, seed, n, n_bytes, ids_lo, ids_hi, letters):
    """n distinct words of exactly n_bytes bytes (n_bytes: an int, or (lo, hi) for a length drawn per word) whose id count
    by the oracle is in ids_lo .. ids_hi, each one word for the splitter."""
    rng = random.Random(seed)
    out, seen = [], set()
    for _ in range(400):
        cands = []
        for _ in range(128):
            nb = n_bytes if isinstance(n_bytes, int) else rng.randint(*n_bytes)
            cands.append(b" " + bytes(rng.choice(letters) for _ in range(nb - 1)))
        for w, c in zip(cands, id_counts(orc, cands)):
            if ids_lo <= c <= ids_hi and w not in seen and is_one_word(w):
                seen.add(w)
                out.append(w)
                if len(out) == n:
                    return out
    raise AssertionError("no such words: %r bytes, %d .. %d ids" % (n_bytes, ids_lo, ids_hi))


def two_byte_word(orc):
    """Two bytes that are a word of their own behind a letter, in front of a space and alone, and two ids (a two-letter
    word behind a space is three bytes with it)."""
    from oracle import oracle as O
    marks = b"!#$%&*+/<=>?@^_`{|}~"
    for a in marks:
        for b in marks:
            s = bytes([a, b])
            doc = b"ab" + s + b" ab"
            starts = O.split_words(doc) + [len(doc)]
            if 2 in starts and 4 in starts and 3 not in starts and O.split_words(s) == [0] and id_counts(orc, [s]) == [2]:
                return s
    raise AssertionError("no two-byte merge-loop word")


def exact(rng, pool, n):
    """Exactly n bytes of whole words of the pool (its lengths lo .. hi without a gap, hi >= 2 lo; n == 0 or n >= lo)."""
    by_len = {}
    for w in pool:
        by_len.setdefault(len(w), []).append(w)
    lo, hi = min(by_len), max(by_len)
    assert sorted(by_len) == list(range(lo, hi + 1)) and hi >= 2 * lo and (n == 0 or n >= lo), (lo, hi, n)
    out, left = [], n
    while left:
        if left <= hi:
            w = rng.choice(by_len[left])
        else:
            w = rng.choice(pool)
            if 0 < left - len(w) < lo:
                continue
        out.append(w)
        left -= len(w)
    return b"".join(out)


def filler_docs(seed, n_bytes=LARGE, n_words=300, lo=5, hi=12, doc_bytes=700):
    """Documents of words drawn from a pool of n_words merge-loop words, n_bytes and a little more in all."""
    rng = random.Random(seed)
    pool = pool_words(seed, n_words, lo, hi)
    docs, size = [], 0
    while size < n_bytes:
        doc = bytearray()
        while len(doc) < doc_bytes:
            doc += rng.choice(pool)
        docs.append(bytes(doc))
        size += len(doc)
    return docs


def word_spans(docs):
    """[(document, start, end, batch position of the start)] of every word the splitter makes"""
    from oracle import oracle as O
    out, base = [], 0
    for d, doc in enumerate(docs):
        starts = (O.split_words(doc) if doc else []) + [len(doc)]
        out += [(d, a, b, base + a) for a, b in zip(starts, starts[1:])]
        base += len(doc)
    return out


class Builder:
    """Documents written one after another; `pos` is the batch position of the next byte."""

    def __init__(self, seed, pool):
        self.rng, self.pool, self.docs, self.cur, self.pos, self.marks = random.Random(seed), pool, [], bytearray(), 0, {}

    def put(self, piece, name=None):
        if name:
            self.marks[name] = self.pos
        self.cur += piece
        self.pos += len(piece)

    def pad_to(self, pos):
        """whole words of the pool up to batch position `pos`"""
        self.put(exact(self.rng, self.pool, pos - self.pos))

    def fill(self, n):
        self.put(exact(self.rng, self.pool, n))

    def end_doc(self):
        self.docs.append(bytes(self.cur))
        self.cur = bytearray()


# ---- a, b: the batch that overflows every sub-list -----------------------------------------------------------------------
OVER_MAX_WORD = 9   # a space and 6, 7 or 8 rare letters: words of 7 to 9 bytes
OVER_DOC_WORDS = 512
OVER_SAMPLE = 16    # the CPU test runs the splitter over the first, the last and every 16th document


def overflow_size():
    """Bytes of the overflow batch.  A workgroup of k_tiles takes TILE_WAVES tiles (GROUP = 3840 bytes) and appends the
    words its merge loop finished to the sub-list `blockIdx.x & (LIST_SHARDS - 1)`, SHARD_CAP places each.  No word of
    the batch is longer than OVER_MAX_WORD bytes, so any GROUP consecutive bytes hold at least GROUP // OVER_MAX_WORD = 426
    word starts, and each is a candidate: the words are pairwise distinct (no hit in a table that was empty when the
    batch began, and none in the whole-word table: two ids or more each), and cacheable.  The grid is the number of
    groups rounded up to a multiple of 8; block order is a bijection onto the groups, so a sub-list gets at least
    groups // LIST_SHARDS workgroups, of which at most one is not full (the batch's last group and the padding: at most
    eight, on block indices 8 apart).  For a sub-list to receive more than SHARD_CAP candidates with a factor of two
    to spare, 2 * SHARD_CAP / 426 = 20 full workgroups are needed, 21 with the one that may not be full:
    21 * LIST_SHARDS groups = 20.6 MB, about 2.4 * LIST_CAP words.  Word lengths (the bound takes the longest) and hits
    (none in a cold table) are the only slack; tests/test_warm_cases_cpu.py counts the word starts of every sub-list by
    the kernel's own block order."""
    per_group = GROUP // OVER_MAX_WORD
    groups_per_shard = -(-2 * SHARD_CAP // per_group) + 1
    return GROUP * LIST_SHARDS * groups_per_shard


def overflow_batch():
    """-> (data uint8, document offsets, batch positions of the word starts).  Word k is a space and 6 letters (one in
    16), 7 (eight in 16) or 8 (seven in 16); the letters are the base-8 digits of the word's index within its length,
    multiplied by an odd constant modulo 8^letters (a bijection, so words of one length differ; words of different
    lengths differ anyway).  A document is OVER_DOC_WORDS words."""
    def make():
        target = overflow_size()
        n = target // 8 + 16  # (the mean length is 8.4 bytes: more than enough words)
        k = np.arange(n, dtype=np.int64)
        cls, turn = k % 16, k // 16
        letters = np.where(cls == 0, 6, np.where(cls % 2 == 1, 7, 8))
        idx = np.where(cls == 0, turn, np.where(cls % 2 == 1, turn * 8 + cls // 2, turn * 7 + cls // 2 - 1))
        assert int(idx[letters == 6].max()) < 8 ** 6 and int(idx[letters == 7].max()) < 8 ** 7 and int(idx[letters == 8].max()) < 8 ** 8
        code = (idx * 0x9E3779B1) % (8 ** letters)
        starts = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(letters + 1, out=starts[1:])
        n_words = int(np.searchsorted(starts, target, side="left"))  # the first word boundary at or behind the target
        assert n_words < n
        total = int(starts[n_words])
        buf = np.full(total, 0x20, dtype=np.uint8)
        rare = np.frombuffer(RARE, dtype=np.uint8)
        letters, code, starts = letters[:n_words], code[:n_words], starts[:n_words]
        for d in range(8):
            m = letters > d
            buf[starts[m] + 1 + d] = rare[(code[m] >> (3 * d)) & 7]
        offs = np.concatenate((starts[::OVER_DOC_WORDS], [total])).astype(np.int64)
        return buf, offs, starts
    return _once("overflow", make)


def overflow_sample(n_docs):
    """the documents whose words the CPU test checks one by one: the first, the last and every OVER_SAMPLE-th"""
    return sorted(set(range(0, n_docs, OVER_SAMPLE)) | {0, n_docs - 1})


def shard_of_group(group, n_bytes):
    """The sub-list of tile group `group` (numpy array or int) of a batch of n_bytes: k_tiles' block b works on group
    (b % 8) * (grid / 8) + b / 8 and lists on b & (LIST_SHARDS - 1)."""
    n_tiles = -(-n_bytes // TILE)
    grid = (-(-n_tiles // TILE_WAVES) + 7) // 8 * 8
    per = grid // 8
    block = (group % per) * 8 + group // per
    return block & (LIST_SHARDS - 1)


def fresh_docs(seed):
    """A learning batch of words no other batch here holds: 13 to 16 bytes, where the overflow batch's have 7 to 9."""
    return filler_docs(seed, LARGE, n_words=2000, lo=13, hi=16, doc_bytes=704)


# ---- c: special tokens ---------------------------------------------------------------------------------------------------
def special_case(orc):
    """-> dict: `warm`, a plain learning batch with every planted word; `docs`, the batch with markers; `marks`, batch
    positions by name.  Words A .. D and S are cached after `warm`; S = left + right, two words of their own once a
    marker stands between them.  Markers: behind a cached word, in front of one, between two, inside S, and at a tile
    edge three ways (across it, beginning on it, ending on it)."""
    def make():
        pool = pool_words(31, 300, 5, 12)
        A, B, C, D = pool[:4]
        S = next(w for w in pool[4:] if len(w) == 10)
        left, right = S[:5], S[5:]
        b = Builder(32, pool)
        b.fill(400)
        b.put(A, "A")
        b.put(EOT, "behind A")      # ... A<EOT> B ...: directly behind a cached word and directly in front of one
        b.put(B, "B")
        b.put(EOT, "between")       # B<EOT>C
        b.put(C, "C")
        b.fill(200)
        b.put(left, "left")
        b.put(EOT, "inside S")
        b.put(right, "right")
        b.put(D, "D")
        b.pad_to(2 * TILE - 5)
        b.put(EOT, "across an edge")
        b.put(A)
        b.pad_to(4 * TILE)
        b.put(EOT, "begins on an edge")
        b.put(B)
        b.end_doc()
        b.put(EOT, "first in its document")
        b.put(C)
        b.pad_to(7 * TILE - len(EOT) - len(D))
        b.put(D)
        b.put(EOT, "ends on an edge")
        b.end_doc()
        while b.pos < LARGE + 2000:
            b.fill(600)
            b.put(EOT)
            b.end_doc()
        warm = filler_docs(31, LARGE)  # (the same pool)
        warm[0] = A + B + C + D + S + warm[0]
        return {"warm": warm, "docs": b.docs, "marks": b.marks, "words": (A, B, C, D), "S": S, "halves": (left, right)}
    return _once("special", make)


# ---- d: split presets ----------------------------------------------------------------------------------------------------
PRESETS = ("gpt2", "cl100k", "qwen2")


def preset_docs():
    """ASCII documents on which the three presets differ: a word behind a tab or a full stop (cl100k and qwen2 take the
    one character into the word, gpt2 does not), digit runs (one word, groups of three, single digits), contractions in
    both cases (cl100k and qwen2 fold the case), a leading space -- all on stems that need the merge loop."""
    def make():
        rng = random.Random(41)
        pool = pool_words(41, 200, 5, 12)
        docs, size = [], 0
        while size < LARGE + 1000:
            parts = []
            for _ in range(50):
                w = rng.choice(pool)
                r = rng.random()
                if r < 0.5:
                    parts.append(w)
                elif r < 0.6:
                    parts.append(b"\t" + w[1:])
                elif r < 0.7:
                    parts.append(b"." + w[1:])
                elif r < 0.8:
                    parts.append(w + rng.choice([b"'s", b"'ll", b"'S", b"'LL", b"'re", b"'T"]))
                elif r < 0.9:
                    parts.append(b" " + bytes(rng.choice(b"0123456789") for _ in range(rng.choice([2, 3, 4, 7]))))
                else:
                    parts.append(b" " + w)  # two spaces in front
            docs.append(b"".join(parts))
            size += len(docs[-1])
        return docs
    return _once("presets", make)


def preset_expected(docs, preset, whole):
    """(ids, out_offsets): the ids of the whole-pattern oracle `whole` over the restatement's words of every document"""
    import presplit_ref as R
    ws = [[w.encode("utf-8") for w in R.words(d.decode("ascii"), preset)] for d in docs]
    flat = [w for row in ws for w in row]
    fd, fo = pack(flat)
    fids, foo, _ = whole.encode_packed(fd, fo, 4)
    bounds = np.cumsum([0] + [len(row) for row in ws])
    return np.asarray(fids, dtype=np.int32), np.asarray(foo)[bounds].astype(np.int64), ws


# ---- e: exception words beside hits --------------------------------------------------------------------------------------
PREFIX = "qx"  # a byte-mode context with a prefix: every document's first word is an exception word


def exception_case(orc):
    """-> dict for a context with PREFIX: documents of about two tiles that begin with a letter (their first word gets the
    prefix: an exception word) and go on with three kinds of words side by side -- `cached` (24 to 30 bytes of common
    letters, 2 to 16 ids), `long` (31 to 45 bytes: beyond the key) and `many` (22 to 30 bytes of rare letters, more than
    16 ids: beyond the result) -- and one tile, `dense_tile`, that holds nothing but words of 8 and 9 bytes."""
    def make():
        cached = find_words(orc, 51, 40, (24, 30), 2, MAX_IDS, COMMON)
        long_ = find_words(orc, 52, 20, (KEY_BYTES + 1, 45), 2, 99, COMMON + RARE)
        many = find_words(orc, 53, 20, (22, KEY_BYTES), MAX_IDS + 1, 99, RARE)
        short = find_words(orc, 54, 150, (8, 9), 2, MAX_IDS, RARE)
        rng = random.Random(55)
        docs, pos = [], 0

        def body(n):
            out, size = [], 0
            while size < n:
                out.append(rng.choice(cached if rng.random() < 0.5 else long_ if rng.random() < 0.5 else many))
                size += len(out[-1])
            return b"".join(out)
        for _ in range(6):
            docs.append(rng.choice(cached)[1:] + body(2 * TILE - 100))
            pos += len(docs[-1])
        # the dense tile: its document is padded with words of 5 .. 12 bytes up to the tile's start
        dense_tile = pos // TILE + 2
        head = rng.choice(cached)[1:]
        pad = exact(rng, pool_words(56, 100, 5, 12), dense_tile * TILE - pos - len(head))
        dense, k = [], 0
        while sum(map(len, dense)) + 9 <= TILE:
            dense.append(short[k])
            k += 1
        dense_doc = len(docs)
        docs.append(head + pad + b"".join(dense) + body(300))
        pos += len(docs[-1])
        while pos < LARGE + 1000:
            docs.append(rng.choice(cached)[1:] + body(2 * TILE - 100))
            pos += len(docs[-1])
        return {"docs": docs, "cached": cached, "long": long_, "many": many, "short": short, "dense_tile": dense_tile,
                "dense_doc": dense_doc}
    return _once("exceptions", make)


def pending_per_tile(orc, docs):
    """-> ({tile: [(word bytes, ids)]} of the words phase 6a deals to the lanes on a context with a prefix, n_tiles): the
    words that start in the tile, are not their document's first word (an exception word), have at most
    LANE_MAX_BYTES bytes and need the merge loop (two ids or more by the oracle without a prefix)."""
    spans = word_spans(docs)
    uniq = sorted({docs[d][a:b] for d, a, b, _p in spans})
    n_ids = dict(zip(uniq, id_counts(orc, uniq)))
    tiles = {}
    for d, a, b, p in spans:
        w = docs[d][a:b]
        if a > 0 and b - a <= LANE_MAX_BYTES and n_ids[w] >= 2:
            tiles.setdefault(p // TILE, []).append((w, n_ids[w]))
    return tiles, -(-sum(map(len, docs)) // TILE)


# ---- g: views ------------------------------------------------------------------------------------------------------------
def view_docs():
    """A learning batch whose first and last word (the first and last ids of the output) are words the batch holds
    elsewhere too: cached from the second encode on whatever came before."""
    def make():
        docs = filler_docs(71, LARGE)
        pool = pool_words(71, 300, 5, 12)
        docs[0] = pool[0] + docs[0]
        docs[-1] = docs[-1] + pool[1]
        docs[3] = pool[0] + pool[1] + docs[3]
        return docs, pool[0], pool[1]
    return _once("views", make)


# ---- h: kernel choice ----------------------------------------------------------------------------------------------------
def cjk_docs(n_tiles=40):
    """CJK paragraphs (hutoken_amd.synth), cut to n_tiles tiles less 400 bytes: dense for k_pre's sample, learning size"""
    from hutoken_amd import synth
    d, o = synth.cjk_paragraphs(8 + n_tiles * 3)
    nb = n_tiles * TILE - 400
    assert nb <= int(o[-1])
    raw = d.tobytes()[:nb]
    cuts = [int(x) for x in o if x < nb] + [nb]
    return [raw[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


# ---- i: the one-launch form ----------------------------------------------------------------------------------------------
def one_launch_case(orc):
    """-> dict: `warm`, a learning batch that holds every planted word between other words; `inputs`, name -> (text for
    encode_one, [(start, end)] of the planted words in it).  K is a 12-byte word, W30 / W31 have 30 / 31 bytes (the
    longest key, and one byte more: never cached), W2 and W3 two and three."""
    def make():
        pool = pool_words(91, 300, 5, 12)
        rng = random.Random(92)
        K = next(w for w in pool if len(w) == 12)
        W30 = find_words(orc, 93, 1, KEY_BYTES, 2, MAX_IDS, COMMON)[0]
        W31 = find_words(orc, 94, 1, KEY_BYTES + 1, 2, 99, COMMON)[0]
        W3 = find_words(orc, 95, 1, 3, 2, 3, RARE)[0]
        W2 = two_byte_word(orc)
        warm = filler_docs(91, LARGE)
        warm[0] = K + W30 + W31 + W3 + b" ab" + W2 + warm[0]
        full = ONE_TILES * TILE
        inputs = {}

        def add(name, front, word, behind=b""):
            inputs[name] = (front + word + behind, [(len(front), len(front) + len(word))])
        add("at byte 0", b"", K, exact(rng, pool, 1000))
        add("ends at the last byte of four tiles", exact(rng, pool, full - len(K)), K)
        add("30 bytes, ends at the last byte of four tiles", exact(rng, pool, full - len(W30)), W30)
        for e in (1, 2, 3):
            add("across the edge of tile %d" % e, exact(rng, pool, e * TILE - 5), K, exact(rng, pool, 500))
        add("the only word", b"", K)
        for tail in (b"", b" a", b" ab", b" qxzj"):  # fewer than 6 bytes behind the 30: the key's nine dwords pass the text's end
            add("30 bytes and %d behind" % len(tail), b"", W30, tail)
        add("30 bytes at the end of a tile and a half", exact(rng, pool, TILE + 500), W30, b" ab")
        for w in (W2, W3, W30, W31):
            add("exactly %d bytes" % len(w), b"", w)
        return {"warm": warm, "inputs": inputs, "K": K, "W30": W30, "W31": W31, "W3": W3, "W2": W2}
    return _once("one launch", make)
