"""Batches past 2^31 and 2^32 bytes as R copies of one block of documents: what tests/test_gpu_wide_batches.py runs on the
GPU and tests/test_wide_cases_cpu.py holds to its claims without one.

Every operation of the library is per document, so a batch of R copies of a block has R times the block's result: the
CPU references run on the block once (seconds) and the GPU's result for the batch is compared, on the device, with the
block's row.  The block's length L is odd, so every copy starts at another phase of the 960-byte tile, of the 16-byte
load and of the normaliser's chunk.

A block is laid out for two boundaries lo < hi (2^31 and 2^32 on the GPU, 2^20 and 2^21 in the CPU test).  With
p_lo = lo mod L and p_hi = hi mod L -- the place inside a copy where the batch's byte position crosses the boundary --

    at p_hi  a word of more than 2046 units begins 1500 bytes in front of p_hi; a word of 513..1024 units lies inside
             the 4 KiB behind it; a three-byte character has its first byte at p_hi - 1 + 1920 (it straddles a tile edge
             of a copy that begins on one)
    at p_lo  the other order: a word of 513..1024 units from 400 bytes in front of p_lo to 400 behind, a word of more
             than 2046 units inside the 4 KiB behind it
    both     a document boundary falls exactly at p + 960

Kinds: "text" (mixed text, every exception list, edge documents, one over-long word), "chars" (the same with every
document valid UTF-8, for character-mode vocabularies, which refuse anything else), "cjk" (paragraphs of CJK: a word
each), "dense" (nearly every byte a word) and "norm" (the normaliser's interesting code points; runs of combining marks
across p_lo and p_hi in place of the words).

A document boundary ends a word, so the long word at p_hi cannot both reach 1500 bytes past p_hi and leave a boundary at
p_hi + 960: the boundary is kept where it is and the word runs from p_hi - 1500 to it (2460 units); the 540 letters from
there to p_hi + 1500 are the first word of the next document (a prefix case in character mode).

marked() and with_unknowns() write special-token markers and characters no vocabulary here knows OVER a block's text
(lengths and offsets stay): one across p_lo and one across p_hi, and into every third document that has room.
with_split_piece() does the same with a piece of text on which the split presets differ (a digit run, contractions, a
whitespace run); preset_words() and preset_ids() are the references of the split and of the encode under a preset.

check_layout() asserts all of this from the block's bytes alone.  Row is the memory rule and the table line of a wide
case, shared with tests/test_gpu_wide_rows.py.  Nothing here touches the package under test except for
hutoken_amd.synth's frozen corpora."""
import gc
import random
import time

import numpy as np
import pytest

import helpers as H

TILE = 960
B31, B32 = 2 ** 31, 2 ** 32
LETTERS = b"etaoinshrdlu"
MARKS = ["\u0301", "\u0323", "\u0327", "\u0308", "\u05ae", "\u0315", "\u031b", "\u0345", "\u0334", "\u0e38", "\u302a"]
LONG_SHARE = 0.03  # long and over-long words: at most this share of a text block's bytes
OVERLONG = 262145  # one byte more than the longest word the encoders take
KINDS = ("text", "cjk", "dense", "norm", "chars")
WS = b" \t\n\r"
EOT, EOT_ID = b"<|endoftext|>", 50256  # GPT-2's marker and its id (the VG vocabulary)
UNKNOWN = "\u6f22".encode("utf-8")      # a character the character-mode vocabulary (VL) has no key for


class Block:
    """docs: the documents; data, offs: packed; L = len(data); p_lo, p_hi: where lo and hi fall inside a copy"""

    def __init__(self, kind, docs, lo, hi):
        self.kind, self.docs, self.lo, self.hi = kind, docs, lo, hi
        self.offs = np.zeros(len(docs) + 1, dtype=np.int64)
        np.cumsum(np.fromiter(map(len, docs), dtype=np.int64, count=len(docs)), out=self.offs[1:])
        self.data = np.frombuffer(b"".join(docs), dtype=np.uint8)
        self.L = len(self.data)
        self.p_lo, self.p_hi = lo % self.L, hi % self.L


def copies_cross(per_copy, boundary, extra=2 ** 26):
    """R: the fewest copies of `per_copy` bytes (or elements) each whose total is boundary + extra or more"""
    return -(-(boundary + extra) // int(per_copy))


def choose_length(around, lo, hi, front=8192, back=8192):
    """The first odd L >= around for which p_lo and p_hi leave `front` bytes in front of them and `back` behind, inside
    the block and between the two."""
    L = around | 1
    while True:
        a, b = sorted((lo % L, hi % L))
        if a >= front and b + back <= L and b - a >= front + back:
            return L
        L += 2


# ---- pieces -------------------------------------------------------------------------------------------------------------
def _letters(rng, n):
    return bytes(rng.choice(LETTERS) for _ in range(n))


def _cjk(rng, n):
    assert n % 3 == 0
    return "".join(chr(0x4E00 + rng.randrange(3000)) for _ in range(n // 3)).encode("utf-8")


def _short_words(rng, n):
    """exactly n bytes of words of 1..8 letters with one space behind each (n >= 1; the last byte is a space)"""
    out = bytearray()
    while len(out) < n:
        out += _letters(rng, rng.randint(1, 8)) + b" "
    out = out[:n]
    out[-1:] = b" "
    return bytes(out)


def _marks(rng, n):
    """exactly n bytes: combining marks of mixed classes, then letters where no mark fits any more"""
    out = bytearray()
    while True:
        m = rng.choice(MARKS).encode("utf-8")
        if len(out) + len(m) > n:
            break
        out += m
    return bytes(out) + b"x" * (n - len(out))


def zone(kind, which, rng):
    """-> (front, documents): the documents that cover [p - front, p + back) of a block, p = p_hi (which == "hi") or p_lo.
    The first begins and the last ends on a document boundary; one boundary lies at p + 960."""
    if kind == "norm":  # a run of marks across p (behind a base letter), the boundary, a run behind it
        lead = b"norm a"
        run = 1500 if which == "hi" else 402
        return len(lead) + run, [lead + _marks(rng, run + TILE), b"o" + _marks(rng, 1201) + " é end".encode("utf-8")]
    word = _cjk if kind == "cjk" else _letters
    mid = 801 if kind == "cjk" else 800  # (whole characters)
    lead = b"straddle "
    if which == "hi":
        d1 = lead + word(rng, 1500 + TILE)                   # the long word: p - 1500 .. p + 960
        d2 = word(rng, 540) + b" "                           # p + 960 .. p + 1500, a space
        d2 += _short_words(rng, 1919 - 1501)                 # .. p + 1919
        d2 += "漢".encode("utf-8") + b" "               # the three-byte character at p - 1 + 1920
        d2 += word(rng, mid) + b" end"
        return len(lead) + 1500, [d1, d2]
    half = 399 if kind == "cjk" else 400
    d1 = lead + word(rng, mid) + b" "                        # p - half .. p - half + mid
    d1 += _short_words(rng, TILE - (mid - half) - 1)         # .. p + 960
    d2 = word(rng, 2100) + b" end"
    return len(lead) + half, [d1, d2]


def overlong_doc(rng):
    """ONE document with a word of OVERLONG bytes that really merges: the encoders cut the document in front of it"""
    pieces = [b"international", b"szolg", "árvíztűrő".encode("utf-8"), b"xq", b"the", b"ation"]
    parts, size = [], 0
    while size < OVERLONG:
        parts.append(rng.choice(pieces))
        size += len(parts[-1])
    blob = b"".join(parts)[:OVERLONG]
    while (blob[-1] & 0xC0) == 0x80 or blob[-1] >= 0xC0:  # (no character cut at the word's end)
        blob = blob[:-1] + b"e"
    return b"kept words, then " + blob + b" dropped words"


def edge_docs():
    """empty and one-byte documents, documents that end inside a character of two, three and four bytes"""
    hu, han, emo = "ő".encode("utf-8"), "漢".encode("utf-8"), "\U0001f602".encode("utf-8")
    return [b"", b"a", b"", b"", b" ", b"\n", b"7", hu[:1], b"sz" + hu[:1], b"k " + han[:1], b"kanji " + han[:2], han[:2],
            b"ha " + emo[:1], emo[:2], b"haha " + emo[:3], b"", b"."]


def _text_pool(rng, n_bytes, rich):
    from hutoken_amd import synth
    if rich:
        yield from edge_docs()
        yield from H.ragged_docs()
        yield from H.long_word_docs()                  # every exception list: 49 .. 9000 units
        yield from H.later_tile_word_docs()[0][::12]   # words that end one to three tiles on
        yield H.merge_loop_words(rng, 1500, 2, 14)
        yield H.merge_loop_words(rng, 300, 20, 47)
        d, o = synth.cjk_paragraphs(12)
        raw = d.tobytes()
        yield from (raw[int(o[i]):int(o[i + 1])] for i in range(12))
        yield overlong_doc(rng)
        yield from edge_docs()
    else:
        yield from edge_docs()
        yield _letters(rng, 70) + b" " + _letters(rng, 300) + b"\n" + _letters(rng, 1100)
    for _ in range(300 if rich else 20):
        yield H.random_text(rng, max_words=40).encode("utf-8")
    d, o = synth.corpus("C3", max(64, n_bytes // 150))  # (documents of 16 bytes and more: enough for n_bytes)
    raw = d.tobytes()
    for i in range(len(o) - 1):
        yield raw[int(o[i]):int(o[i + 1])]
        if i % 97 == 0:
            yield b"" if i % 2 else b"e"
    raise AssertionError("the text pool ran dry")


def _cjk_pool(rng, n_bytes, rich):
    from hutoken_amd import synth
    yield from edge_docs()
    # (paragraphs of 30 .. 120 characters, a word each: the exception kernels' time grows with the square of a word's length,
    # and the 300 .. 1200 bytes of the default paragraphs cost ten seconds per encode of 2 GiB)
    d, o = synth.cjk_paragraphs(max(16, n_bytes // 180), lo=30, hi=120)
    raw = d.tobytes()
    for i in range(len(o) - 1):
        yield raw[int(o[i]):int(o[i + 1])]
        if i % 53 == 0:
            yield raw[int(o[i]):int(o[i]) + 3 * (i % 40) + i % 3]  # a short document, two in three end inside a character
    raise AssertionError("the CJK pool ran dry")


def _dense_pool(rng, n_bytes, rich):
    docs = [d[:1 + len(d) // 4] for d in H.dense_word_docs()]
    while True:
        yield from docs
        yield b""


def _norm_pool(rng, n_bytes, rich):
    import norm_ref as NR
    import view_cases as V
    hot = NR.interesting_code_points()
    plain = [ord(x) for x in "aeouAEOU xyz019"] + [0x4E00, 0x3042, 0x0915, 0x09C7, 0x1100, 0xAC00, 0x1F600, 0x00DF]
    yield from edge_docs()

    def doc(k):
        if k % 7 == 0:    # ASCII: no form changes it
            return _short_words(rng, rng.randint(1, 3000))
        if k % 7 == 1:    # precomposed Hungarian: its own NFC form, NFD and NFKD lengthen it
            return V.hungarian(rng.randint(10, 2000)).encode("utf-8")
        if k % 400 == 2 and rich:  # (few: reordering a run costs the normaliser far more than anything else here)
            return b"a" + _marks(rng, rng.randint(100, 3000))
        n = rng.randint(1, 60)
        return "".join(chr(rng.choice(hot) if rng.random() < 0.5 else rng.choice(plain)) for _ in range(n)).encode("utf-8")
    docs = [doc(k) for k in range(4100 if rich else 300)]
    while True:  # (the same documents again and again, at other places: a block has room for some tens of thousands)
        yield from docs
        yield b""


def _chars_pool(rng, n_bytes, rich):
    """the text pool as valid UTF-8: a character-mode context refuses text that is not (HUTK_E_INVALID_UTF8), so the
    documents that end inside a character end in front of it here"""
    for d in _text_pool(rng, n_bytes, rich):
        yield d.decode("utf-8", "ignore").encode("utf-8")


_POOLS = {"text": _text_pool, "cjk": _cjk_pool, "dense": _dense_pool, "norm": _norm_pool, "chars": _chars_pool}


def _fill(docs, pool, deferred, size, target):
    """documents of the pool up to byte `target` exactly: one that does not fit waits in `deferred` for a later call, and
    the last stretch (below 4 KiB) is a padding document.  -> target"""
    for d in list(deferred):
        if size + len(d) <= target:
            deferred.remove(d)
            docs.append(d)
            size += len(d)
    while target - size >= 4096:
        d = next(pool)
        if size + len(d) > target:
            deferred.append(d)
            continue
        docs.append(d)
        size += len(d)
    if size < target:
        docs.append((b" pad" * ((target - size) // 4 + 1))[:target - size])
    return target


def build(kind, L, lo, hi, seed=1, rich=True):
    """The block of `kind` (KINDS): exactly L bytes, the zones of p_lo and p_hi laid out as the module's header says.
    rich: with the rare and expensive documents (the over-long word, every exception list), for blocks of 1 MiB and more."""
    assert kind in KINDS and L % 2 == 1
    rng = random.Random(seed * 1000 + KINDS.index(kind))
    pool = _POOLS[kind](rng, L, rich)
    docs, size, deferred = [], 0, []
    for p, which in sorted(((lo % L, "lo"), (hi % L, "hi"))):
        front, zdocs = zone(kind, which, rng)
        assert p - front >= size, "the zones overlap, or one begins in front of the block: choose_length()"
        size = _fill(docs, pool, deferred, size, p - front)
        docs += zdocs
        size += sum(map(len, zdocs))
    assert size <= L
    _fill(docs, pool, deferred, size, L)
    assert not (rich and deferred), "a document of the pool found no room in the block"
    b = Block(kind, docs, lo, hi)
    assert b.L == L
    check_layout(b)
    return b


# ---- what a block claims ------------------------------------------------------------------------------------------------
def runs(block, least):
    """[(start, end)] of the stretches of `least` bytes and more without whitespace or a document boundary"""
    a = block.data
    brk = (a == 0x20) | (a == 0x09) | (a == 0x0A) | (a == 0x0D)
    cut = np.zeros(block.L + 1, dtype=bool)
    cut[block.offs] = True
    starts = np.nonzero(~brk & (np.concatenate(([True], brk[:-1])) | cut[:-1]))[0]
    ends = np.nonzero(~brk & (np.concatenate((brk[1:], [True])) | cut[1:]))[0] + 1
    assert len(starts) == len(ends)
    keep = ends - starts >= least
    return list(zip(starts[keep].tolist(), ends[keep].tolist()))


def run_at(block, pos):
    """(start, end) of the stretch without whitespace or a document boundary that holds byte `pos`"""
    a, offs = block.data, block.offs
    d = int(np.searchsorted(offs, pos, side="right")) - 1
    s = e = pos
    assert a[pos] not in WS
    while s > offs[d] and a[s - 1] not in WS:
        s -= 1
    while e < offs[d + 1] and a[e] not in WS:
        e += 1
    return s, e


def long_share(block):
    """share of the block's bytes in words of 49 bytes and more (what leaves the tile kernel for the exception kernels)"""
    return sum(e - s for s, e in runs(block, 49)) / block.L


def check_layout(block):
    """The straddler rule of the module's header, from the block's bytes and offsets alone."""
    b, offs = block, set(block.offs.tolist())
    assert b.L % 2 == 1
    for p in (b.p_lo, b.p_hi):
        assert p + TILE in offs, "no document boundary at p + 960"
        assert p - 1600 > 0 and p + 4096 < b.L
    if b.kind == "chars":
        for d in b.docs:
            d.decode("utf-8")  # (raises on a document that is not valid UTF-8)
    if b.kind == "norm":
        for p in (b.p_lo, b.p_hi):
            text = b.data[p - 300:p + 300].tobytes().decode("utf-8", "ignore")
            assert sum(1 for c in text if c in MARKS) >= 150, "no run of marks across p"
        return
    s, e = run_at(b, b.p_hi)
    assert s == b.p_hi - 1500 and e == b.p_hi + TILE and e - s > 2046, (s - b.p_hi, e - b.p_hi)
    mids = [(s, e) for s, e in runs(b, 513) if e - s <= 1024 and b.p_hi <= s and e <= b.p_hi + 4096]
    assert mids and mids[0][0] == b.p_hi + TILE, "the first word of the document behind p_hi + 960 is not there"
    # (that one is the cut-off rest of the long word; the word laid down for the rule lies behind the three-byte character)
    assert [1 for s, e in mids if s == b.p_hi + 2 * TILE + 3 and e - s >= 800], "no word of 513..1024 units in the 4 KiB behind p_hi"
    c = b.data[b.p_hi - 1 + 2 * TILE:b.p_hi + 2 + 2 * TILE]
    assert 0xE0 <= c[0] <= 0xEF and (c[1] & 0xC0) == 0x80 and (c[2] & 0xC0) == 0x80, "no three-byte character at p_hi - 1 + 1920"
    s, e = run_at(b, b.p_lo)
    assert s < b.p_lo - 390 and e > b.p_lo + 390 and 513 <= e - s <= 1024, (s - b.p_lo, e - b.p_lo)
    longs = [(s, e) for s, e in runs(b, 2047) if b.p_lo <= s and e <= b.p_lo + 4096]
    assert longs and longs[0][0] == b.p_lo + TILE, "no word of more than 2046 units behind p_lo"


# ---- markers and unknown characters written over a block ----------------------------------------------------------------
def _overwritten(block, piece, every, begin_before, ascii_only):
    """The block's bytes with `piece` written over them (the offsets stay): beginning `begin_before` bytes in front of
    p_lo and of p_hi, so that it lies across the place where each boundary falls, and at the front, in the middle or at
    the end of every `every`-th document that has room for it.  ascii_only: only over ASCII bytes, so that valid UTF-8
    stays valid.  -> (uint8 array, [start of every piece])"""
    a, n, at = block.data.copy(), len(piece), []

    def put(s):
        if ascii_only and (a[s:s + n] >= 0x80).any():
            return
        a[s:s + n] = np.frombuffer(piece, dtype=np.uint8)
        at.append(s)
    zone_docs = set()
    for p in (block.p_lo, block.p_hi):
        d = int(np.searchsorted(block.offs, p, side="right")) - 1
        assert block.offs[d] <= p - begin_before and p - begin_before + n <= block.offs[d + 1]
        zone_docs.add(d)
        put(p - begin_before)
    assert len(at) == 2, "the bytes across p_lo and p_hi do not take the piece"
    for d in range(0, len(block.docs), every):
        s, e = int(block.offs[d]), int(block.offs[d + 1])
        if e - s >= n and d not in zone_docs:
            put((s, (s + e - n) // 2, e - n)[(d // every) % 3])
    return a, sorted(at)


def marked(block, marker=EOT, every=3):
    """Special-token markers over the text: one from p - 8 to p + 5 at both boundaries, one in every third document."""
    return _overwritten(block, marker, every, 8, False)


def with_unknowns(block, ch=UNKNOWN, every=3):
    """An unknown character over ASCII text (a "chars" block stays valid UTF-8): its first byte at p - 1 at both
    boundaries, so that its bytes lie on either side, and one in every third document."""
    assert block.kind == "chars"
    return _overwritten(block, ch, every, 1, True)


SPLIT_PIECE = b"x's 1234567 \n\n  we'll"  # a contraction, a digit run that cl100k groups in threes, a whitespace run, a contraction
SPLIT_DIGITS = (4, 11)                    # where the digits lie in it


def with_split_piece(block, every=3):
    """What the split presets treat differently over the text: the piece begins 9 bytes in front of p_lo and of p_hi, so
    that the place where the boundary falls lies inside the digit run, between its fifth and sixth digit, with the
    contractions and the whitespace run within a dozen bytes either side; and in every third document."""
    return _overwritten(block, SPLIT_PIECE, every, 9, False)


WHOLE = "(.|\n)+"  # the whole-document pattern of test_regex_path.py: the oracle then encodes a document as ONE word


def preset_words(data, offs, preset):
    """presplit_ref over every document -> (starts: int64, the word starts as positions in data; start_offs: int64[n + 1])"""
    import presplit_ref as PR
    raw, starts, so = np.asarray(data).tobytes(), [], [0]
    for d in range(len(offs) - 1):
        a, b = int(offs[d]), int(offs[d + 1])
        starts += [a + p for p in PR.word_starts(raw[a:b], preset)]
        so.append(len(starts))
    return np.array(starts, dtype=np.int64), np.array(so, dtype=np.int64)


def preset_ids(oracle_mod, files, data, offs, starts, start_offs):
    """What tests/test_gpu_presplit.py::expected_ids builds, for documents of bytes: the oracle's ids under the
    whole-document pattern of every word of preset_words as a document of its own -> (ids int32, out_offsets int64[n + 1]
    per DOCUMENT).  POSIX's `.` passes over a byte that is no character of the locale, so the words that are not valid
    UTF-8 (documents that end inside a character, a piece written over one) are encoded under LC_CTYPE "C", where every
    byte is one; the others under the process's own, as expected_ids does."""
    import locale
    vp, sp, kw = files
    raw = np.asarray(data).tobytes()
    edges = np.concatenate((starts, [len(raw)])).tolist()
    assert len(raw) == int(offs[-1])  # (a word ends where the next starts: the documents tile the block)
    words = [raw[a:b] for a, b in zip(edges, edges[1:])]
    ill = []
    for i, w in enumerate(words):
        try:
            w.decode("utf-8")
        except UnicodeDecodeError:
            ill.append(i)
    orc = oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"], pattern=WHOLE)
    try:
        d, o = oracle_mod.pack(words)
        ids, oo, _st = orc.encode_packed(d, o, 8)
        ids, oo = np.asarray(ids, dtype=np.int32), np.asarray(oo, dtype=np.int64)
        if ill:
            keep = locale.setlocale(locale.LC_CTYPE, None)
            locale.setlocale(locale.LC_CTYPE, "C")
            try:
                d, o = oracle_mod.pack([words[i] for i in ill])
                ids_c, oo_c, _st = orc.encode_packed(d, o, 8)
            finally:
                locale.setlocale(locale.LC_CTYPE, keep)
            ids_c = np.asarray(ids_c, dtype=np.int32)
            parts, at = [], 0
            for n, i in enumerate(ill):
                parts += [ids[oo[at]:oo[i]], ids_c[oo_c[n]:oo_c[n + 1]]]
                at = i + 1
            parts.append(ids[oo[at]:])
            lens = np.diff(oo)
            lens[ill] = np.diff(np.asarray(oo_c, dtype=np.int64))
            ids = np.concatenate(parts)
            oo = np.concatenate(([0], np.cumsum(lens)))
    finally:
        orc.close()
    return ids, oo[start_offs]


def byte_table(vocab_path):
    """int32[256]: the ids of the keys "<0x00>" .. "<0xFF>" of a vocabulary file, read from its text"""
    keys = {}
    with open(vocab_path, "r", encoding="ascii") as f:
        for line in f:
            key, _eq, idx = line.partition(" == ")
            keys[bytes.fromhex(key.replace("0x", ""))] = int(idx)
    return np.array([keys[b"<0x%02X>" % v] for v in range(256)], dtype=np.int32), len(keys)


class RefTokenText:
    """spans_ref.TokenText's two questions answered from a decode_ref.DecodeRef (its tables hold every token's bytes at
    the front of a document and elsewhere), for the shipped vocabularies' tens of thousands of ids"""

    def __init__(self, ref):
        self.ref, self.blob = ref, ref.blob.tobytes()

    def _text(self, i, off, ln):
        if i < 0 or i >= self.ref.n or self.ref.bad[i]:
            return None
        return self.blob[int(off[i]):int(off[i]) + int(ln[i])]

    def first(self, i):
        return self._text(i, self.ref.soff, self.ref.slen)

    def rest(self, i):
        return self._text(i, self.ref.off, self.ref.len)


# ---- the batch of R copies and what is expected of it -------------------------------------------------------------------
def repeated_offsets(offs, per_copy, R):
    """numpy: offs[:-1] + r * per_copy for r < R, then R * per_copy"""
    offs = np.asarray(offs, dtype=np.int64)
    body = (offs[None, :-1] + np.arange(R, dtype=np.int64)[:, None] * int(per_copy)).reshape(-1)
    return np.concatenate((body, [R * int(per_copy)]))


def side(pos):
    """which side of which boundary an absolute byte (or element) position is on"""
    return "below 2^31" if pos < B31 else "in [2^31, 2^32): negative as int32" if pos < B32 else "at or above 2^32: wraps as uint32"


def encode_workspace(n_bytes, n_docs, units_per_item):
    """Device workspace of an encode, from include/hutoken_amd.h (hutk_ids_capacity): about 18 bytes per input byte for
    ordinary vocabulary files, about 60 + 12 x (units per item) where an item can become several units."""
    per = 18 if units_per_item <= 1 else 60 + 12 * units_per_item
    return per * n_bytes + 64 * n_docs


class Row:
    """One case at one boundary: the memory rule in front of it, one line of the table behind it."""

    def __init__(self, name, boundary, need):
        self.name, self.boundary, self.need = name, "2^31" if boundary == B31 else "2^32", int(need)

    def __enter__(self):
        import torch
        gc.collect()
        torch.cuda.empty_cache()
        self.free = torch.cuda.mem_get_info()[0]
        if self.free < 1.25 * self.need:
            print("WIDE | %s | %s | skipped | %d | %d | -" % (self.name, self.boundary, self.need, self.free))
            pytest.skip("%s at %s needs 1.25 x %d bytes of device memory, %d are free" % (self.name, self.boundary, self.need, self.free))
        self.t0 = time.time()
        return self

    def __exit__(self, kind, exc, tb):
        import torch
        torch.cuda.synchronize()
        took = time.time() - self.t0
        gc.collect()
        torch.cuda.empty_cache()
        print("WIDE | %s | %s | %s | %d | %d | %.1f" % (self.name, self.boundary, "ran" if kind is None else "ran, FAILED", self.need,
                                                      self.free, took))


def assert_rows(got, row, R, what, where, L, slice_elems=2 ** 28):
    """got: a torch tensor of R * T elements (on the device), row: the T the reference gives for one copy.  Compared
    slice_elems at a time, so no temporary is larger than that.  where(r, j) -> the byte position in the batch that
    element j of copy r belongs to; the message names it, the copy and the side of the boundaries it is on."""
    import torch
    row = row.reshape(-1)
    T = row.numel()
    assert got.numel() == R * T, "%s: %d elements, %d copies of %d expected" % (what, got.numel(), R, T)
    if T == 0:
        return
    step = max(1, slice_elems // T)
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        ne = got[r0 * T:r1 * T].view(r1 - r0, T) != row
        if bool(ne.any()):
            k = int(ne.view(-1).to(torch.uint8).argmax())  # (the first of the largest)
            r, j = r0 + k // T, k % T
            pos = int(where(r, j))
            raise AssertionError("%s: the first difference is element %d of copy %d (element %d of the batch): %d, the "
                                 "reference has %d; byte position %d = %d * %d + %d of the batch, %s"
                                 % (what, j, r, r * T + j, int(got[r * T + j]), int(row[j]), pos, r, L, pos - r * L, side(pos)))
        del ne


def assert_offsets(got, oo_block, R, what, where, L, slice_elems=2 ** 28):
    """got[r * n + d] == r * T + oo_block[d] for every document d of every copy r, got[R * n] == R * T (T = oo_block[n])"""
    import torch
    n, T = len(oo_block) - 1, int(oo_block[-1])
    assert got.numel() == R * n + 1
    assert int(got[R * n]) == R * T, "%s: the total is %d, %d copies of %d expected" % (what, int(got[R * n]), R, T)
    rel = got[:R * n].view(R, n) - torch.arange(R, dtype=torch.int64, device=got.device)[:, None] * T
    row = torch.from_numpy(np.ascontiguousarray(oo_block[:-1])).to(got.device)
    assert_rows(rel.reshape(-1), row, R, what, where, L, slice_elems)
